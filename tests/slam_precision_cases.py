"""The cases, derived rounding bounds and plain float64 models of the SLAM landmark update's precision tests
(tests/test_slam_precision_gpu.py on the device, tests/test_slam_precision_cpu.py for the bounds themselves): ovp_slam_update and
ovp_slam_update_general, stage by stage, every stage fed with the device's own output of the stage before.  The truth is
tests/slam_ref.py (rows) and oracle/ld_ref.py (everything behind them) in long double; the metric is cov_bookkeeping_cases.ratio,
element by element, a case passes at ratio <= 1, an element with a zero bound must be exact.

The bounds.  u = 2^-53; every count is of roundings of the device's arithmetic, fused or not, in any order; + 2 on every count
covers gamma_K versus K u and the truth's own rounding, as in cov_bookkeeping_cases.py and zupt_cases.py.  rows / cols are those of
the system a stage solves: a landmark's block at the gate, the stack (m_total x gcols) at the tail.  Nothing is taken from a run of
the code under test.

  rows   slam_ref.E carries with every element the first-order bound e of one rounding per operation of the restated expression,
         any order of association in a sum.  The device (ovp_feat_model.h) and np_ref evaluate the same expressions up to where a
         product is distributed over a sum (dz_dzn dzn_dpfc formed first or folded into one row, the whitening factor applied to
         the row or to its factors, R_ItoC R_GtoI formed or applied one after the other): the operands' magnitudes, hence the
         companion, are the same, and such a variant adds along a path at most the roundings the path already has.  So the count
         is doubled:                                                                 |d H_ij| <= (2 e_ij + 2 |H_ij|) u
         A column the landmark does not touch, a row of a rejected landmark and a plane row the fallback dropped have e = 0.
  gate   S = H P_marg H^T + I from the rows the device stacked (exact inputs): two nested sums over cols and the two additions,
         (2 cols + 2) u comp.S with comp.S = |H| |P_marg| |H|^T + I.  An unpivoted elimination of `rows` steps has the backward error
         gamma_(rows + 1) |L| |U|, of norm <= (rows + 1) trace(S) u <= (rows + 1) rows lam_max u.  The eigenvalues of S are >= 1:
         kappa = lam_max / lam_min <= lam_max.
             |d S|_2 <= eps_S lam_max,  eps_S = ((2 cols + 2) |comp.S|_F / lam_max + (rows + 1) rows) u
         z = L^-1 r, chi2 = |z|^2 (the device's sum of y_c^2 / pivot_c is this sum).  As zupt_cases.py derives it for its 6 x 6:
             |d z|_2 <= (sqrt(rows) eps_S + rows^2 u) kappa |z|_2 =: dz;      |d chi2| <= 2 |z| dz + dz^2 + (rows + 2) u chi2
         The fallback's statistic is the same on the leading nb x nb block (the partial sum over the first nb pivots IS the
         elimination of that block).  Where the stack does not hold a landmark's rows (status 0; the plane rows behind status 2) the
         gate's input is the truth's rows, and their own bound enters to first order with w = S^-1 r:
             |d chi2| += 2 |w|^T |d r| + 2 |w|^T |d H| |P_marg H^T w|
  M      M = P[:, ids] H_l^T: a dot product over the block's columns, (cols + 2) u |P[:, ids]| |H_l|^T.  Rows of a rejected or dropped
         block: 0.
  tail   (S-form, up to 80 stacked rows that fit one workgroup) dx and P+ against ld_ref.ekf_update_dense on the device's stack, in
         the shape of the zero-velocity bound: Y = M L^-T, a_i = |Y_i|_2, c_i = sqrt(rows) |comp.M_i|_2 / sqrt(lam_min),
             d_i = phi a_i + (cols + rows + 2) u c_i,  phi = (sqrt(rows) eps_S + 6 rows^2 u) kappa
             |d dx_i| <= d_i |z| + a_i dz + d_i dz + (rows + 2) u a_i |z|
             |d P+_ij| <= (rows + 3) u (|P| + |Y| |Y|^T)_ij + d_i a_j + a_i d_j + d_i d_j
         With nothing accepted P is the input bit for bit and dx = 0.
         The information form (more than 80 stacked rows, or a stack that fails ovp_init_fits by LDS) goes through a factor of P
         itself: its bound is derived at info_tail_truth, from the steps of ekf_from_gram; M_all is not formed there.  With
         nothing accepted the call must not update at all, in either form.

The gate margin: every truth chi2 lies outside thr (1 -+ MARGIN) for each threshold it is compared with (test_slam_precision_cpu).

The covariance: the scene's own (so that the statistics mean what the scene intends), scaled by D P D with D = 1 on the columns the
call touches and 10^U(-4, 4) elsewhere: positive definite, the touched columns at the scene's scales, the others spread over
eight decades as precision_helpers.spd_with spreads them.

Not here yet: delayed initialisation."""
import numpy as np

import cov_bookkeeping_cases as B
import slam_ref as R
from precision_helpers import capacities  # noqa: F401
from oracle import ld_ref, np_ref

LD = ld_ref.LD
U = B.U
MARGIN = 1e-9


def _header_constants():
    """(S-form row limit, k_init_core's LDS limit, the gate's LDS limit, chunk width) read from csrc/ovp_lds_sizes.h, so that a limit
    that moves there moves here; the two size formulas below restate ovp_slam_gate_lds / ovp_init_core_lds, and the device's own
    decisions are read back on the GPU (ovp_debug_read "slam_dims")"""
    import os
    import re

    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ov_plane_amd", "csrc", "ovp_lds_sizes.h")).read()
    rows = int(re.search(r"ovp_init_max_rows\(\)\s*\{\s*return\s+(\d+)\s*;", src).group(1))
    init = int(re.search(r"ovp_init_max_lds\(\)\s*\{\s*return\s+(\d+)\s*\*\s*1024\s*;", src).group(1)) * 1024
    gate = int(re.search(r"OVP_SLAM_GATE_MAX_LDS\s*=\s*(\d+)\s*\*\s*1024\s*;", src).group(1)) * 1024
    cw = int(re.search(r"#define\s+SL_CW\s+(\d+)", src).group(1))
    return rows, init, gate, cw


SFORM_ROWS, INIT_LDS, GATE_LDS, CW = _header_constants()


def gate_lds(rows, cols, with_h):
    d = rows * (rows + 2) + rows + rows * CW + cols * CW + ((cols + 1) // 2 + 1) + (rows * cols if with_h else 0)
    return 8 * d


def init_fits(rup, cols):
    return rup <= SFORM_ROWS and 8 * (cols * rup + rup * (2 * rup + 2)) <= INIT_LDS


def cases():
    """dict(name, kind mono | stereo, scene keywords, ms (observations per landmark), plane (landmarks that carry their plane),
    outlier (landmarks whose pixels get gross noise), pre (landmarks whose block the host builds), expect (statuses), form)"""
    cs = [
        # 9 / 15 / 21 columns: either side of one 16-column chunk, odd totals, no calibration; m = 1 is a two-row block
        dict(name="m123_nocal", kw=dict(C=4, n_slam=3, seed=21, calib=False), ms=[1, 2, 3], expect=[1, 1, 1], form="s"),
        # 29 / 35 / 47 columns: either side of two chunks, 14 calibration columns
        dict(name="m235_cal", kw=dict(C=6, n_slam=3, seed=22), ms=[2, 3, 5], expect=[1, 1, 1], form="s"),
        # even totals (the plane's three columns): plane accepted, wrong plane (keep 6 of 9 rows), an outlier between accepted ones
        dict(name="planes_outlier_between", kw=dict(C=5, n_slam=5, seed=23, n_planes=2, wrong_plane=1), ms=[3, 2, 3, 4, 2],
             plane=[0, 1, 2, 3, 4], outlier=[2], expect=[2, 1, 0, 1, 1], form="s"),
        dict(name="fisheye", kw=dict(C=4, n_slam=3, seed=24, fisheye=True), ms=[2, 3, 4], expect=[1, 1, 1], form="s"),
        dict(name="nofej", kw=dict(C=4, n_slam=3, seed=25, do_fej=False), ms=[3, 2, 4], expect=[1, 1, 1], form="s"),
        # 14 calibration columns, no plane: m = 29 is the largest block with H in LDS, m = 30 the smallest with H in scratch
        dict(name="m29_h_in_lds", kw=dict(C=32, n_slam=1, seed=26), ms=[29], expect=[1], form="s", h_in_lds=1),
        # ... with a two-row landmark beside it (the switch is per call); 62 rows whose 206 columns fail ovp_init_fits by LDS
        dict(name="m30_h_in_scratch", kw=dict(C=32, n_slam=2, seed=27), ms=[30, 1], expect=[1, 1], form="info", h_in_lds=0),
        dict(name="m32_plane_96rows", kw=dict(C=32, n_slam=1, seed=28, n_planes=1), ms=[32], plane=[0], expect=[1], form="info"),
        dict(name="rows80", kw=dict(C=6, n_slam=8, seed=29), ms=[5] * 8, expect=[1] * 7 + [0], form="s"),
        dict(name="rows81", kw=dict(C=6, n_slam=7, seed=30, n_planes=1), ms=[3] + [6] * 6, plane=[0], expect=[1] * 7, form="info"),
        dict(name="pre_mixed", kw=dict(C=5, n_slam=3, seed=31), ms=[2, 3, 2], pre=[1], expect=[1, 1, 1], form="s"),
        # two cameras: landmark 0 stereo, landmark 1 by camera 1 alone, landmarks 2 and 3 by camera 0
        dict(name="stereo", kind="stereo", kw=dict(C=5, n_slam=4, seed=32, stereo_frac=0.5, cam1_only=1), ms=None,
             expect=[1, 1, 1, 1], form="s"),
        # two cameras with different lens models: camera 0 radtan, camera 1 equidistant (tests/multicam.add_cameras); landmark 0 by
        # both, landmark 1 by camera 1 alone, landmark 2 by camera 0
        dict(name="lens_mix", kind="cams", kw=dict(C=5, n_slam=3, seed=33), ms=[3, 2, 3], cam_of=[[0, 1, 0], [1, 1], [0, 0, 0]],
             expect=[1, 1, 1], form="s"),
        # more than 80 stacked rows, every landmark an outlier: the information form with nothing accepted
        dict(name="info_none_accepted", kw=dict(C=6, n_slam=7, seed=34), ms=[6] * 7, outlier=list(range(7)), expect=[0] * 7, form="info"),
    ]
    for c in cs:
        c.setdefault("kind", "mono")
        for k in ("plane", "outlier", "pre"):
            c.setdefault(k, [])
    return cs


_SC = {}


def scene(c):
    """the case's scene: the observations cut to ms, the outliers' pixels disturbed, the covariance rescaled (module docstring)"""
    if c["name"] in _SC:
        return _SC[c["name"]]
    from ov_plane_amd.synth import make_slam_scene, make_stereo_slam_scene

    kw = dict(c["kw"])
    sc = (make_stereo_slam_scene if c["kind"] == "stereo" else make_slam_scene)(ragged=False, **kw)
    if c["ms"] is not None:
        assert (np.asarray(sc.n_meas) >= np.asarray(c["ms"])).all()
        sc["n_meas"] = np.asarray(c["ms"], dtype=np.int32)
    rng = np.random.default_rng(5000 + kw["seed"])
    if c["kind"] == "cams":
        sc = _with_fisheye_camera_1(c, sc, rng)
    for f in c["outlier"]:
        m = int(sc.n_meas[f])
        sc.uv[f, :m] += (25.0 * rng.standard_normal((m, 2))).astype(np.float32)
    touched = np.zeros(sc.N, dtype=bool)
    for blk in layout(c, sc):
        touched[blk["ids"]] = True
    d = 10.0 ** rng.uniform(-4.0, 4.0, sc.N)
    d[touched] = 1.0
    sc["P"] = np.outer(d, d) * sc.P
    assert np.array_equal(sc.P, sc.P.T) and (~touched).any()
    _SC[c["name"]] = sc
    return sc


def _with_fisheye_camera_1(c, sc, rng):
    """the scene with an equidistant camera 1 (its 14 columns behind the state's, correlated with the window) and the observations
    c["cam_of"] names as camera 1's: the truth projected through camera 1's true tables, plus pixel noise"""
    import multicam
    from ov_plane_amd.synth import project_all

    out = multicam.add_cameras(sc, 2, fisheye=(False, True), seed=c["kw"]["seed"])
    R_t, p_t, intr_t, fish = out.truth["cams"][1]
    tr = out.truth
    uv1, _ = project_all(tr["p_f"], tr["R"], tr["p"], R_t, p_t, intr_t, fish)
    uv = np.array(out.uv, dtype=np.float32)
    cam_idx = np.zeros(np.asarray(out.clone_idx).shape, dtype=np.int32)
    for f, cams in enumerate(c["cam_of"]):
        for a, cam in enumerate(cams):
            if cam == 1:
                ci = int(out.clone_idx[f, a])
                uv[f, a] = (uv1[f, ci] + out.opts["sigma_px"] * rng.standard_normal(2)).astype(np.float32)
                cam_idx[f, a] = 1
    out.update(uv=uv, cam_idx=cam_idx)
    return out


def plane_args(c, sc):
    """(plane_state_id [L], cp [L, 3], cp_fej [L, 3]) of the call, or three None"""
    if not c["plane"]:
        return None, None, None
    pid = np.maximum(np.asarray(sc.plane_id, dtype=np.int64), 1) - 1
    sid = np.full(sc.F, -1, dtype=np.int32)
    sid[c["plane"]] = np.asarray(sc.plane_state_id)[pid][c["plane"]]
    return sid, np.asarray(sc.cp)[pid], np.asarray(sc.cp_fej)[pid]


def layout(c, sc):
    """per landmark dict(row0, rows, nb, cols, ids (its local column list, the kernel's order), plane)"""
    o = sc.opts
    mask = [k for k in range(14) if (o["do_calib_pose"] if k < 6 else o["do_calib_intr"])]
    sid, _, _ = plane_args(c, sc)
    out, row0 = [], 0
    for f in range(sc.F):
        m = int(sc.n_meas[f])
        ids = [int(sc.ids["clones"][int(sc.clone_idx[f, a])]) + k for a in range(m) for k in range(6)]
        cams = sorted(set(int(x) for x in sc.cam_idx[f, :m])) if "cam_idx" in sc else [0]
        for cam in cams:
            if "cams" in sc:
                cid, iid = sc.cams[cam]["calib_id"], sc.cams[cam]["intr_id"]
            else:
                cid, iid = (sc.ids["calib"], sc.ids["intr"]) if cam == 0 else (sc.ids["calib1"], sc.ids["intr1"])
            ids += [int(cid) + k if k < 6 else int(iid) + k - 6 for k in mask]
        ids += [int(sc.lm_id[f]) + k for k in range(3)]
        plane = sid is not None and sid[f] >= 0
        if plane:
            ids += [int(sid[f]) + k for k in range(3)]
        rows = 3 * m if plane else 2 * m
        # cols: the kernel's count (a clone two cameras see has a block per observation); ids: each state column once
        out.append(dict(row0=row0, rows=rows, nb=2 * m, cols=len(ids), ids=np.array(list(dict.fromkeys(ids)), dtype=np.int64), plane=plane))
        row0 += rows
    return out


def geometry(c, sc):
    """(m_total, gcols, h_in_lds, S-form) as ovp_slam_plan.h decides them"""
    lay = layout(c, sc)
    m_total = sum(b["rows"] for b in lay)
    gcols = len(set(int(i) for b in lay for i in b["ids"]))
    rmax, cmax = max(b["rows"] for b in lay), max(b["cols"] for b in lay)
    assert gate_lds(rmax, cmax, 0) <= GATE_LDS
    return m_total, gcols, int(gate_lds(rmax, cmax, 1) <= GATE_LDS), init_fits(m_total, gcols)


def thresholds(sc, blk):
    """(thr of all rows, thr of the bearing rows)"""
    return sc.opts["chi2_mult"] * np_ref.chi2_095(blk["rows"]), sc.opts["chi2_mult"] * np_ref.chi2_095(blk["nb"])


# ---- stage 1: rows ------------------------------------------------------------------------------------------------------------
def rows_of(c, sc, num, p_fej_at_value=False, drop_plane_cols=False):
    """every landmark's rows over the state's columns, ungated: list of (H [rows, N], res [rows]) arrays of num"""
    sid, cp, cpf = plane_args(c, sc)
    out = []
    for f, blk in enumerate(layout(c, sc)):
        plane = (int(sid[f]), cp[f], cpf[f]) if blk["plane"] else None
        H, res = R.landmark_rows(sc, f, plane, num, p_fej=sc.p_FinG[f] if p_fej_at_value else None)
        if drop_plane_cols and plane is not None:
            H[:, plane[0]:plane[0] + 3] = num(0.0)
        out.append((H, res))
    return out


_ROWS = {}


def truth_rows(c):
    """per landmark (H, res, bound of H, bound of res) in long double, bounds in units of u (module docstring: 2 e + 2 |v|); a
    host-built block is its own truth with bound 0"""
    if c["name"] not in _ROWS:
        sc = scene(c)
        out = []
        pre = pre_blocks(c, sc)
        for f, (H, res) in enumerate(rows_of(c, sc, R.E)):
            Hv, He = R.split(H)
            rv, re = R.split(res)
            if pre[f] is not None:
                Hd = np.zeros(Hv.shape)
                Hd[:, pre[f][1]] = pre[f][0]
                out.append((ld_ref.ld(Hd), ld_ref.ld(pre[f][2]), np.zeros_like(He), np.zeros_like(re)))
            else:
                out.append((Hv, rv, np.where(He > 0, 2 * He + 2 * np.abs(Hv), 0), 2 * re + 2 * np.abs(rv)))
        _ROWS[c["name"]] = out
    return _ROWS[c["name"]]


def pre_blocks(c, sc):
    """per landmark None or (H [rows, cols], ids, res): the float64 model's rows of the landmarks the host builds"""
    out = [None] * sc.F
    if c["pre"]:
        lay = layout(c, sc)
        rows = rows_of(c, sc, float)
        for f in c["pre"]:
            H, _ = R.split(rows[f][0])
            r, _ = R.split(rows[f][1])
            out[f] = (np.ascontiguousarray(H[:, lay[f]["ids"]]), lay[f]["ids"], r)
    return out


def stack(c, sc, blocks, status):
    """(H [m_total, N], res [m_total]) of per-landmark (H, res) under the statuses: 1 all rows, 2 the bearing rows, 0 none"""
    lay = layout(c, sc)
    m_total = sum(b["rows"] for b in lay)
    H = np.zeros((m_total, sc.N), dtype=blocks[0][0].dtype)
    res = np.zeros(m_total, dtype=blocks[0][0].dtype)
    for blk, (Hl, rl), st in zip(lay, blocks, status):
        keep = blk["rows"] if st == 1 else (blk["nb"] if st == 2 else 0)
        H[blk["row0"]:blk["row0"] + keep] = Hl[:keep]
        res[blk["row0"]:blk["row0"] + keep] = rl[:keep]
    return H, res


# ---- stage 2: gate ------------------------------------------------------------------------------------------------------------
def chi2_with_bound(Hl, rl, P, ids, dH=None, dr=None):
    """(chi2, bound in units of u, kappa) of rows Hl [rows, N] (doubles, exact) on the marginal of `ids`; dH / dr: bounds (units of
    u) of rows that are themselves only known to a bound (module docstring)"""
    u = LD(U)
    rows, cols = Hl.shape[0], len(ids)
    H = ld_ref.ld(Hl)[:, ids]
    r = ld_ref.ld(rl)
    Pm = ld_ref.ld(P)[np.ix_(ids, ids)]
    S = ld_ref.sym(H @ Pm @ H.T + np.eye(rows, dtype=LD))
    compS = np.abs(H) @ np.abs(Pm) @ np.abs(H).T + np.eye(rows, dtype=LD)
    L = ld_ref.chol(S)
    z = ld_ref.solve_lower(L, r)
    chi2 = z @ z
    w = np.linalg.eigvalsh(np.array(S, dtype=np.float64)).astype(LD)  # (kappa enters the bound only; double's digits do)
    lam_min, lam_max = w[0], w[-1]
    kappa = lam_max / lam_min
    eps_S = ((2 * cols + 2 + 2) * np.sqrt((compS ** 2).sum()) / lam_max + (rows + 1) * rows) * u
    nz = np.sqrt(chi2)
    dz = (np.sqrt(LD(rows)) * eps_S + rows * rows * u) * kappa * nz
    b = 2 * nz * dz + dz * dz + (rows + 2 + 2) * u * chi2
    if dH is not None:
        wv = np.abs(ld_ref.solve_upper(L.T, z))
        b = b + 2 * u * (wv @ dr + wv @ (dH[:, ids] @ np.abs(Pm @ (H.T @ ld_ref.solve_upper(L.T, z)))))
    return chi2, b / u, kappa


def decide(sc, blk, chi2_f, chi2_b):
    """(status, the statistic that decided) as k_slam_body.h / UpdaterSLAM.cpp:541-620"""
    thr_f, thr_b = thresholds(sc, blk)
    if blk["rows"] > blk["nb"] and not chi2_f > thr_f:
        return 1, chi2_f
    if blk["rows"] > blk["nb"]:
        return (0 if chi2_b > thr_b else 2), chi2_b
    return (0 if chi2_b > thr_b else 1), chi2_b


def gate_truth(c, blocks):
    """per landmark dict(status, chi2, bound, compared [(chi2, thr)]) from `blocks` = per landmark (H, res, dH or None, dr or None)"""
    sc = scene(c)
    out = []
    for blk, (Hl, rl, dH, dr) in zip(layout(c, sc), blocks):
        nb = blk["nb"]
        cf, bf, _ = chi2_with_bound(Hl, rl, sc.P, blk["ids"], dH, dr)
        cb, bb, _ = (cf, bf, 0) if nb == blk["rows"] else chi2_with_bound(Hl[:nb], rl[:nb], sc.P, blk["ids"], None if dH is None else dH[:nb],
                                                                         None if dr is None else dr[:nb])
        st, chi2 = decide(sc, blk, cf, cb)
        thr_f, thr_b = thresholds(sc, blk)
        cmp_ = [(cf, thr_f)] + ([(cb, thr_b)] if (blk["rows"] > nb and st != 1) else []) if blk["rows"] > nb else [(cb, thr_b)]
        out.append(dict(status=st, chi2=chi2, bound=bf if (st == 1 and blk["rows"] > nb) else bb, compared=cmp_))
    return out


def gate_inputs(c, H_stack, res_stack, status):
    """the gate's input per landmark from a stack: the stack's own rows where it holds them all, the truth's (with their bounds)
    for the rows it does not hold"""
    sc = scene(c)
    out = []
    for blk, st, (Hv, rv, bH, br) in zip(layout(c, sc), status, truth_rows(c)):
        s = slice(blk["row0"], blk["row0"] + blk["rows"])
        if st == 1:
            out.append((H_stack[s], res_stack[s], None, None))
            continue
        keep = blk["nb"] if st == 2 else 0
        Hl = np.array(Hv, dtype=np.float64)
        rl = np.array(rv, dtype=np.float64)
        # (the truth rounded to double: one more rounding on top of its bound)
        dH = np.where(bH > 0, bH + np.abs(Hv), 0)
        dr = br + np.abs(rv)
        Hl[:keep], rl[:keep] = H_stack[s][:keep], res_stack[s][:keep]
        dH[:keep], dr[:keep] = 0, 0
        out.append((Hl, rl, dH, dr))
    return out


# ---- stage 3: M ---------------------------------------------------------------------------------------------------------------
def m_truth(c, H_stack):
    """(M [n, m_total], companion, K [m_total]) of M = P[:, ids] H_l^T per landmark block, from the stack's rows"""
    sc = scene(c)
    P = ld_ref.ld(sc.P)
    H = ld_ref.ld(H_stack)
    M = np.zeros((sc.N, H.shape[0]), dtype=LD)
    comp = np.zeros_like(M)
    K = np.zeros(H.shape[0])
    for blk in layout(c, sc):
        s = slice(blk["row0"], blk["row0"] + blk["rows"])
        ids = blk["ids"]
        M[:, s] = P[:, ids] @ H[s][:, ids].T
        comp[:, s] = np.abs(P[:, ids]) @ np.abs(H[s][:, ids]).T
        K[s] = blk["cols"] + 2
    return M, comp, K


# ---- stage 4: tail (S-form) ---------------------------------------------------------------------------------------------------
def tail_truth(c, H_stack, res_stack, gids):
    """dict(dx, P, b_dx, b_P) of ld_ref.ekf_update_dense on the stack (columns gids), bounds in units of u"""
    sc = scene(c)
    u = LD(U)
    g = np.asarray(gids, dtype=np.int64)
    H = ld_ref.ld(H_stack)[:, g]
    r = ld_ref.ld(res_stack)
    rows, cols = H.shape
    P = ld_ref.ld(sc.P)
    Pn, dx = ld_ref.ekf_update_dense(P, g, H, r)
    Pm = P[np.ix_(g, g)]
    S = ld_ref.sym(H @ Pm @ H.T + np.eye(rows, dtype=LD))
    compS = np.abs(H) @ np.abs(Pm) @ np.abs(H).T + np.eye(rows, dtype=LD)
    compM = np.abs(P[:, g]) @ np.abs(H).T
    L = ld_ref.chol(S)
    z = ld_ref.solve_lower(L, r)
    Y = ld_ref.solve_lower(L, (P[:, g] @ H.T).T).T
    w = np.linalg.eigvalsh(np.array(S, dtype=np.float64)).astype(LD)  # (kappa enters the bound only; double's digits do)
    lam_min, lam_max = w[0], w[-1]
    kappa = lam_max / lam_min
    eps_S = ((2 * cols + 2 + 2) * np.sqrt((compS ** 2).sum()) / lam_max + (rows + 1) * rows) * u
    nz = np.sqrt(z @ z)
    sr = np.sqrt(LD(rows))
    dz = (sr * eps_S + rows * rows * u) * kappa * nz
    phi = (sr * eps_S + 6 * rows * rows * u) * kappa
    a = np.sqrt((Y ** 2).sum(axis=1))
    cn = sr * np.sqrt((compM ** 2).sum(axis=1)) / np.sqrt(lam_min)
    d = phi * a + (cols + rows + 2 + 2) * u * cn
    b_dx = d * nz + a * dz + d * dz + (rows + 2 + 2) * u * a * nz
    b_P = (rows + 3 + 2) * u * (np.abs(P) + np.abs(Y) @ np.abs(Y).T) + np.outer(d, a) + np.outer(a, d) + np.outer(d, d)
    return dict(dx=dx, P=Pn, b_dx=b_dx / u, b_P=b_P / u, kappa=float(kappa))


class StatusDiffers(AssertionError):
    """a status of the result is not the truth's"""


# ---- stage 4: tail (information form) -----------------------------------------------------------------------------------------
def info_tail_truth(c, H_stack, res_stack, gids):
    """dict(dx, P, b_dx, b_P) of ld_ref.ekf_update_dense on the stack for a call the device solves in the information form
    (ekf_from_gram: L = chol(P), T = I + L^T A L, Lt = chol(T), V = Lt^-1 L^T, P+ = V^T V, dx = P+ b with A = H^T H, b = H^T r).
    n = state size, m = stacked rows, s_i = sqrt(P_ii) = |row i of L|_2, C = P / (s s^T) the correlation matrix; the eigenvalues
    of T are >= 1, so |T^-1| <= 1 and kappa_T = lam_max(T); |V_i|_2 <= s_i.  Every part is a bound on |d P+_ij| / (s_i s_j):
      chol(P)     L L^T = P + dP with |dP_ij| <= (n + 1) u s_i s_j; d P+ = L T^-1 (L^-1 dP L^-T) T^-1 L^T and |L^-1 dP L^-T|_2 <=
                  n (n + 1) u / lam_min(C): the one place the conditioning of P enters, through its correlation matrix alone
                  (a factorization does not see the scales)                                      n (n + 1) u / lam_min(C)
      T           the Gram sums of A (m) and the two nested products over n, + I: (m + 2 n + 3) u comp.T with comp.T = |L|^T |H|^T
                  |H| |L| + I; its factorization gamma_(n + 1) |Lt| |Lt|^T <= (n + 1) n lam_max u;  d P+ = L T^-1 dT T^-1 L^T:
                  eps_T kappa_T,  eps_T = ((m + 2 n + 3) |comp.T|_F / lam_max + (n + 1) n) u
      V, V^T V    the substitution per column, n^2 u kappa_T twice (as zupt_cases.py bounds |L^-1| |L|), the product's n + 2
    dx = P+ b:    sum_j |d P+_ij| |b_j| + (m + 2 + n + 2) u sum_j |P+_ij| (|H|^T |r|)_j
    Nothing here is a chosen factor; the float64 model of the same steps is held inside it on the CPU."""
    sc = scene(c)
    u = LD(U)
    g = np.asarray(gids, dtype=np.int64)
    H = ld_ref.ld(H_stack)[:, g]
    r = ld_ref.ld(res_stack)
    m = H.shape[0]
    n = sc.N
    P = ld_ref.ld(sc.P)
    Pn, dx = ld_ref.ekf_update_dense(P, g, H, r)
    s = np.sqrt(np.diag(P))
    lamC = LD(np.linalg.eigvalsh(sc.P / np.outer(np.sqrt(np.diag(sc.P)), np.sqrt(np.diag(sc.P))))[0])
    assert lamC > 0
    L = ld_ref.chol(P)
    HL = np.zeros((m, n), dtype=LD)
    HL = H @ L[g, :]
    T = ld_ref.sym(HL.T @ HL + np.eye(n, dtype=LD))
    aHL = np.abs(H) @ np.abs(L[g, :])
    compT = aHL.T @ aHL + np.eye(n, dtype=LD)
    lam_max = LD(np.linalg.eigvalsh(np.array(T, dtype=np.float64))[-1])  # (kappa enters the bound only; double's digits do)
    eps_T = ((m + 2 * n + 3 + 2) * np.sqrt((compT ** 2).sum()) / lam_max + (n + 1) * n) * u
    rel = n * (n + 1) * u / lamC + eps_T * lam_max + 2 * n * n * u * lam_max + (n + 2 + 2) * u
    b_P = rel * np.outer(s, s)
    bv = np.zeros(n, dtype=LD)
    bv[g] = H.T @ r
    ab = np.zeros(n, dtype=LD)
    ab[g] = np.abs(H).T @ np.abs(r)
    b_dx = b_P @ np.abs(bv) + (m + n + 4 + 2) * u * (np.abs(Pn) @ ab)
    return dict(dx=dx, P=Pn, b_dx=b_dx / u, b_P=b_P / u)


def info_form_f64(P, g, H, r, fault=None):
    """the device's information form in plain float64 (numpy's Cholesky and solves); fault "info_last_row_lost": the Gram pair
    without the last stacked row that is not zero"""
    n = P.shape[0]
    if fault == "info_last_row_lost":
        last = int(np.nonzero(np.abs(H).sum(axis=1))[0][-1])
        H, r = np.delete(H, last, axis=0), np.delete(r, last)
    A = np.zeros((n, n))
    A[np.ix_(g, g)] = H.T @ H
    b = np.zeros(n)
    b[g] = H.T @ r
    L = np.linalg.cholesky(P)
    T = np.eye(n) + L.T @ (A @ L)
    T = (T + T.T) / 2
    V = np.linalg.solve(np.linalg.cholesky(T), L.T)
    Pn = V.T @ V
    return Pn, Pn @ b


# ---- all four stages of one result --------------------------------------------------------------------------------------------
def ratios(c, got):
    """got = dict(Ht [gcols, m_total], res, cols (the call's column list), M or None, chi2, status, dx, P): the worst ratio of
    every stage, dict(rows, gate, M, tail); a stage that does not apply is missing.  Raises AssertionError where a status differs
    from the truth's."""
    sc = scene(c)
    lay = layout(c, sc)
    tr = truth_rows(c)
    g = np.asarray(got["cols"], dtype=np.int64)
    H = np.zeros((got["Ht"].shape[1], sc.N))
    H[:, g] = np.asarray(got["Ht"]).T
    res = np.asarray(got["res"], dtype=np.float64)
    status = [int(s) for s in got["status"]]
    out = {}
    # rows: against the truth's rows under the truth's statuses
    gt0 = gate_truth(c, [(np.array(Hv, dtype=np.float64), np.array(rv, dtype=np.float64), np.where(bH > 0, bH + np.abs(Hv), 0), br + np.abs(rv))
                         for Hv, rv, bH, br in tr])
    st0 = [t["status"] for t in gt0]
    if status != st0:
        raise StatusDiffers((c["name"], status, st0))
    Ht, rt = stack(c, sc, [(Hv, rv) for Hv, rv, _, _ in tr], st0)
    Hb, rb = stack(c, sc, [(bH, br) for _, _, bH, br in tr], st0)
    out["rows"] = max(B.ratio(H, Ht, Hb, -1), B.ratio(res, rt, rb, -1))
    # gate: from the rows the device stacked
    gt = gate_truth(c, gate_inputs(c, H, res, status))
    if status != [t["status"] for t in gt]:
        raise StatusDiffers((c["name"], status, [t["status"] for t in gt]))
    out["gate"] = max(B.ratio(np.array([x]), np.array([t["chi2"]]), np.array([t["bound"]]), -1) for x, t in zip(got["chi2"], gt))
    if got.get("M") is not None:
        M, comp, K = m_truth(c, H)
        out["M"] = B.ratio(got["M"], M, comp, K[None, :])
    if not any(status):
        out["tail"] = 0.0 if (np.array_equal(got["P"], sc.P) and not np.any(got["dx"])) else np.inf
    else:
        if True:
            t = (tail_truth if geometry(c, sc)[3] else info_tail_truth)(c, H, res, g)
            out["tail"] = max(B.ratio(got["dx"], t["dx"], t["b_dx"], -1), B.ratio(got["P"], t["P"], t["b_P"], -1))
    return out


# ---- the plain float64 model and its faults ------------------------------------------------------------------------------------
FAULTS = ("info_last_row_lost", "rows_f32", "lm_jac_at_value", "plane_cols_lost", "no_identity_row", "fallback_all_rows", "chunk_last_col", "odd_last_col",
          "m_not_zeroed", "row0_plus_1")


def model(c, fault=None):
    """The update in plain float64 as the device splits it - rows (slam_ref on floats), per-landmark gate (numpy), M, the S-form
    tail (np_ref.ekf_update) - every stage from the stage before, with one fault:
      rows_f32           the rows rounded to float32
      lm_jac_at_value    the landmark's Jacobians at its value instead of its first estimate
      plane_cols_lost    the plane's three columns missing from the point-on-plane rows
      no_identity_row    + I missing on the last row of the first landmark's S
      fallback_all_rows  the fallback's chi2 summed over every pivot instead of the first nb
      chunk_last_col     S without the last column of a partial 16-column chunk of the marginal
      odd_last_col       S without the odd last column
      m_not_zeroed       M keeps the dropped plane rows' products
      row0_plus_1        the second landmark's rows stacked one row down
      info_last_row_lost the information form's Gram pair without the last accepted row
    Returns the dict ratios() takes."""
    sc = scene(c)
    lay = layout(c, sc)
    pre = pre_blocks(c, sc)
    blocks = []
    for f, (H, r) in enumerate(rows_of(c, sc, float, p_fej_at_value=fault == "lm_jac_at_value", drop_plane_cols=fault == "plane_cols_lost")):
        Hv, rv = R.split(H)[0], R.split(r)[0]
        if pre[f] is not None:
            Hv = np.zeros_like(Hv)
            Hv[:, pre[f][1]] = pre[f][0]
            rv = pre[f][2]
        if fault == "rows_f32":
            Hv, rv = Hv.astype(np.float32).astype(np.float64), rv.astype(np.float32).astype(np.float64)
        blocks.append((Hv, rv))
    status, chi2 = [], []
    for f, (blk, (Hv, rv)) in enumerate(zip(lay, blocks)):
        ids = blk["ids"]
        Hl = Hv[:, ids]
        if fault == "chunk_last_col" and blk["cols"] % CW:
            Hl = Hl.copy()
            Pm = sc.P[np.ix_(ids, ids)].copy()
            Pm[:, -1] = 0.0
            S = Hl @ Pm @ Hl.T + np.eye(blk["rows"])
        elif fault == "odd_last_col" and blk["cols"] % 2:
            S = Hl[:, :-1] @ sc.P[np.ix_(ids, ids)][:-1] @ Hl.T + np.eye(blk["rows"])
        else:
            S = Hl @ sc.P[np.ix_(ids, ids)] @ Hl.T + np.eye(blk["rows"])
        if fault == "no_identity_row" and f == 0:
            S[-1, -1] -= 1.0
        nb = blk["nb"]
        cf = float(rv @ np.linalg.solve(S, rv))
        cb = cf if (nb == blk["rows"] or fault == "fallback_all_rows") else float(rv[:nb] @ np.linalg.solve(S[:nb, :nb], rv[:nb]))
        st, x = decide(sc, blk, cf, cb)
        status.append(st)
        chi2.append(x)
    H, res = stack(c, sc, blocks, status)
    if fault == "row0_plus_1" and len(lay) > 1 and status[1]:
        b = lay[1]
        keep = b["rows"] if status[1] == 1 else b["nb"]
        s0 = b["row0"]
        H[s0 + 1:s0 + keep] = H[s0:s0 + keep - 1].copy()
        H[s0] = 0.0
        res[s0 + 1:s0 + keep] = res[s0:s0 + keep - 1].copy()
        res[s0] = 0.0
    m_total, gcols, _, sform = geometry(c, sc)
    g = []
    for blk in lay:
        g += [int(i) for i in blk["ids"] if int(i) not in g]
    g = np.array(g, dtype=np.int64)
    M = None
    if sform:
        M = np.zeros((sc.N, m_total))
        for blk, (Hv, _), st in zip(lay, blocks, status):
            s = slice(blk["row0"], blk["row0"] + blk["rows"])
            src = Hv if (fault == "m_not_zeroed" and st == 2) else H[s]
            M[:, s] = sc.P[:, blk["ids"]] @ src[:, blk["ids"]].T
    dx, Pn = np.zeros(sc.N), sc.P.copy()
    if sform and any(status):
        Pn, dx = np_ref.ekf_update(sc.P, [(int(i), 1) for i in g], H[:, g], res)
    elif any(status):
        Pn, dx = info_form_f64(sc.P, g, H[:, g], res, fault)
    return dict(Ht=np.ascontiguousarray(H[:, g].T), res=res, cols=g, M=M, chi2=np.array(chi2), status=np.array(status), dx=dx, P=Pn)
