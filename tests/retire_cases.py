"""The cases, derived rounding bounds and plain float64 models of the retire / merge precision tests
(tests/test_retire_precision_gpu.py on the device, tests/test_ld_ref_cpu.py for the bounds themselves).  The truth is
oracle/ld_ref.py::plane_merge, the compaction is numpy indexing (retire_ref.compact_ref); the metric is
cov_bookkeeping_cases.ratio, element by element, a case passes at ratio <= 1.

The bounds.  u = 2^-53; every count is of roundings of k_plane_merge_gate / k_plane_merge_apply (k_retire.hip), fused or not, in any
order; + 2 on every count as in cov_bookkeeping_cases.py.  A pair reads the P and the closest points the pairs before it left, so
the bound of a chain is carried along: EP (element by element) and Ecp (per plane) are the bounds on what the device holds when
the pair starts, zero for the first.  wc = 1 / sigma.  Nothing is taken from a run of the code under test.

  M         M_i = wc (P[i, new] - P[i, old]): a difference and a product relative to comp.M = wc (|P_i,new| + |P_i,old|), and the
            input's own error:                                              EM_i = 2 u comp.M_i + wc (EP[i, new] + EP[i, old])
  S         S_ab = wc (M[new + a][b] - M[old + a][b]) + delta_ab: the same once more, and the addition:
            ES = wc (EM[new rows] + EM[old rows]) + 3 u comp.S; in the 2-norm, with the 3 x 3 factorization's backward error
            gamma_4 |L| |L|^T (norm <= trace S <= 3 lam_max):                         eps_S = (|ES|_F / lam_max + 12 u)
  res       wc (0 - (c1 - c0)): two roundings, and the closest points' own error:      Eres = 2 u |res| + wc (Ecp_new + Ecp_old)
  y, chi2   y = L^-1 res, as z of zupt_cases.py with 3 in place of 6:
            dy = |Eres|_2 / sqrt(lam_min) + (sqrt(3) eps_S + 9 u) kappa |y|;     |d chi2| <= 2 |y| dy + dy^2 + 5 u chi2
  W         W = M Li^T with the explicit inverse Li = (I + F) L^-1, |F|_2 <= 3 u (3 sqrt(kappa))^2 = 27 u kappa (zupt_cases.py has
            the argument: a constant, not a second factor of kappa), three fused terms per element.  With a_i = |W_i|_2:
            d_i = |EM_i|_2 / sqrt(lam_min) + ((sqrt(3) eps_S + 27 u) kappa + 3 u) a_i
  dx        dx_i = W_i . y:                                                 Edx_i = d_i |y| + a_i dy + d_i dy + 4 u a_i |y|
  cp        cp += dx[c : c + 3] for every plane of the table:                  Ecp += Edx[c : c + 3] + u |cp|
  P         P_ij - W_i . W_j: 4 u comp.P with comp.P = |P| + |W| |W|^T, the errors of W norm-wise (so kappa multiplies
            a_i a_j >= (|W| |W|^T)_ij), on top of what P carried:   EP_ij += 4 u comp.P_ij + d_i a_j + a_i d_j + d_i d_j
  angle     the two norms (3 + 1 roundings each), the divisions, the three products and their sum leave the dot product
            within 10 u of its value (|dot| <= 1), the closest points' error moves it by at most 2 (|Ecp_new| / |cp_new| +
            |Ecp_old| / |cp_old|): delta.  acos has the derivative -1 / sin(theta), so
            |d angle| <= (180 / pi) delta / sin(theta) + 3 u angle   (valid while delta << 1 - dot, which the CPU test asserts).
            Exactly parallel closest points with components exact in binary give dot = 1 and the angle 0.0 exactly.
A rejected pair leaves P, the closest points and its row of dx (all zero) as they were: no error is added."""
import numpy as np

import cov_bookkeeping_cases as B
import retire_ref as R
from oracle import ld_ref
from precision_helpers import spd_with

LD = ld_ref.LD
U = B.U
MARGIN = 1e-9
PLANE_SCALE = 1.0e-2  # the standard deviation of a plane's closest point in ov_plane_amd.synth._cov


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def _perp(v):
    """a unit vector perpendicular to v"""
    a = np.cross(v, [0.3, -0.5, 0.8])
    return a / np.linalg.norm(a)


def _spec():
    """name -> dict(n, planes (first columns), pairs [(new, old, kind)], extra retired ranges, sigma, chi2_mult, deg_max).
    kind: accept | chi2 (rejected by chi2) | angle (rejected by the angle) | parallel (exactly parallel, exact in binary) | near
    (about 1e-3 degrees apart)"""
    base = dict(sigma=0.01, chi2_mult=1.0, deg_max=1.0, extra=[])
    s = {
        # survivor behind the old plane; planes at columns 0..2 and at the last three
        "n63_behind_first_last": dict(base, n=63, planes=[0, 60], pairs=[(60, 0, "accept")]),
        # survivor before the old plane, which holds the last three columns; one column of tiles, exactly
        "n64_before_last": dict(base, n=64, planes=[10, 61], pairs=[(10, 61, "accept")], extra=[(30, 6)]),
        # a plane across column 64: the second column of tiles of the downdate holds one column
        "n65_across64": dict(base, n=65, planes=[62, 20], pairs=[(62, 20, "accept")]),
        "n65_across64_rejected": dict(base, n=65, planes=[62, 20], pairs=[(62, 20, "chi2")]),
        "n65_parallel_exact": dict(base, n=65, planes=[62, 20], pairs=[(20, 62, "parallel")]),
        "n64_nearly_parallel": dict(base, n=64, planes=[3, 40], pairs=[(3, 40, "near")]),
        # accept, reject (chi2), accept: the rejected launch must leave the first pair's W unused
        "n129_chain_chi2": dict(base, n=129, planes=[62, 100, 126, 3], pairs=[(62, 100, "accept"), (62, 126, "chi2"), (62, 3, "accept")],
                                extra=[(15, 6)]),
        # the middle pair rejected by the angle; the survivor across row 256
        "n257_chain_angle": dict(base, n=257, planes=[254, 0, 128, 200], chi2_mult=40.0,
                                 pairs=[(254, 0, "accept"), (254, 128, "angle"), (254, 200, "accept")]),
        # merge and compaction in one call, 257 -> 254
        "n257_to_254": dict(base, n=257, planes=[254, 100], pairs=[(254, 100, "accept")]),
        # three strides of the gate's row loop, eleven columns of tiles, three workgroups of columns in the compaction
        "n700_two_survivors": dict(base, n=700, planes=[697, 0, 254, 62], pairs=[(697, 0, "accept"), (254, 62, "accept")],
                                   extra=[(300, 6), (512, 1)]),
    }
    # the limits in one call: 64 pairs over a table of 128 planes at n = 15 + 3 x 128, survivors alternately before and behind,
    # every fourth pair rejected by chi2, every old plane retired together with a clone and a single column
    cols = [15 + 3 * p for p in range(128)]
    pairs = []
    for k in range(64):
        a, b = cols[2 * k], cols[2 * k + 1]
        new, old = (a, b) if k % 2 == 0 else (b, a)
        pairs.append((new, old, "chi2" if k % 4 == 3 else "accept"))
    s["n399_limits"] = dict(base, n=399, planes=cols, pairs=pairs, extra=[(3, 6), (12, 1)])
    return s


def names():
    return list(_spec())


_CASES = {}


def case(name):
    """dict(n, P, pairs [(new, old)], kinds, plane_col, cp [n_planes, 3], sigma, chi2_mult, deg_max, retire_ids, retire_sizes).
    P: spd_with the planes' columns at plane scale.  The closest points are designed on the state the pairs before leave:
    the survivor's value as it will be when the pair runs, plus a step whose chi2 is 0.3 (accept, angle, near) or 3 (chi2) times the
    threshold - along the normal with a perpendicular part of a fifth for accept / chi2, a rotation of 2.5 degrees for angle."""
    if name in _CASES:
        return _CASES[name]
    sp = _spec()[name]
    n, planes = sp["n"], sp["planes"]
    seed = 900 + names().index(name)
    rng = np.random.default_rng(seed)
    pcols = np.concatenate([np.arange(c, c + 3) for c in planes])
    P = spd_with(n, seed, pcols, PLANE_SCALE)
    pairs = [(a, b) for a, b, _ in sp["pairs"]]
    kinds = [k for _, _, k in sp["pairs"]]
    cp = {c: np.array([2.0, 0.3, 0.1]) + 0.2 * rng.standard_normal(3) for c in planes}
    thr = sp["chi2_mult"] * R.CHI2_095_3
    wc = 1.0 / sp["sigma"]
    # the state the pair will find, carried along in double (the design needs the target's first digits only)
    Pk = P.copy()
    moved = {c: np.zeros(3) for c in planes}                             # what the accepted pairs so far added to a plane's value
    H = wc * np.hstack([np.eye(3), -np.eye(3)])
    for (cn, co), kind in zip(pairs, kinds):
        idx = np.r_[cn:cn + 3, co:co + 3]
        S = H @ Pk[np.ix_(idx, idx)] @ H.T + np.eye(3)
        c1 = cp[cn] + moved[cn]
        nrm = _unit(c1)
        if kind == "parallel":
            cp[cn], cp[co] = np.array([0.0, 0.0, 2.0 ** -6]), np.array([0.0, 0.0, 2.0 ** -7])
            want = cp[co] + moved[co]
            c1 = cp[cn] + moved[cn]
        elif kind in ("angle", "near"):
            a = np.deg2rad(2.5 if kind == "angle" else 1.0e-3)
            want = np.linalg.norm(c1) * (np.cos(a) * nrm + np.sin(a) * _perp(nrm))
        else:
            d = _unit(nrm + 0.2 * _perp(nrm))
            f = 3.0 if kind == "chi2" else 0.3
            want = c1 + np.sqrt(f * thr / (wc * wc * d @ np.linalg.solve(S, d))) * d
        cp[co] = want - moved[co]
        if kind in ("accept", "parallel", "near"):
            M = Pk[:, idx] @ H.T
            K = np.linalg.solve(S, M.T).T
            dx = K @ (wc * (want - c1))
            Pk = Pk - K @ M.T
            for c in planes:
                moved[c] = moved[c] + dx[c:c + 3]
    ids = [co for _, co in pairs] + [i for i, _ in sp["extra"]]
    sizes = [3] * len(pairs) + [s for _, s in sp["extra"]]
    _CASES[name] = dict(n=n, P=P, pairs=pairs, kinds=kinds, plane_col=list(planes), cp=np.array([cp[c] for c in planes]), sigma=sp["sigma"],
                        chi2_mult=sp["chi2_mult"], deg_max=sp["deg_max"], retire_ids=ids, retire_sizes=sizes)
    return _CASES[name]


def expected(c):
    return [k in ("accept", "parallel", "near") for k in c["kinds"]]


_TRUTH = {}


def truth(name):
    """(truth, companions, bounds) of a case, computed once"""
    if name not in _TRUTH:
        c = case(name)
        t, comps = ld_ref.plane_merge(c["P"], c["pairs"], c["plane_col"], c["cp"], c["sigma"], c["chi2_mult"], c["deg_max"])
        _TRUTH[name] = (t, comps, bounds(c, t, comps))
    return _TRUTH[name]


def bounds(c, t, comps):
    """dict(chi2 [np], angle [np], dx [np, n], P [n, n]) in units of u (ratio(got, truth, W, -1) <= 1 passes), carried through the
    chain as the module docstring derives it"""
    u = LD(U)
    n = c["n"]
    wc = 1 / LD(c["sigma"])
    EP = np.zeros((n, n), dtype=LD)
    Ecp = {int(col): np.zeros(3, dtype=LD) for col in c["plane_col"]}
    cur = {int(col): ld_ref.ld(v) for col, v in zip(c["plane_col"], c["cp"])}
    fro = lambda A: np.sqrt((A ** 2).sum())  # noqa: E731
    b_chi2, b_ang, b_dx = [], [], []
    steps = ld_ref.plane_merge_steps(c["P"], t)     # the n x n companion of every accepted pair, one at a time
    for k, (cn, co) in enumerate(c["pairs"]):
        comp = comps[k]
        kappa, lam_min, lam_max = LD(t["kappa"][k]), LD(t["lam_min"][k]), LD(t["lam_max"][k])
        sn, so = slice(cn, cn + 3), slice(co, co + 3)
        c1, c0 = t["cp_new"][k], t["cp_old"][k]
        # the angle
        delta = (10 + 2) * u + 2 * (fro(Ecp[cn]) / fro(c1) + fro(Ecp[co]) / fro(c0))
        dot = t["dot"][k]
        sin = np.sqrt(max(LD(0), (1 - dot) * (1 + dot)))
        b_ang.append((LD(180) / np.arccos(LD(-1))) * delta / sin + (3 + 2) * u * t["angle_deg"][k] if sin > 0 else LD(0))
        # the gate
        EM = (2 + 2) * u * comp["M"] + wc * (EP[:, sn] + EP[:, so])
        ES = wc * (EM[sn, :] + EM[so, :]) + (3 + 2) * u * comp["S"]
        eps_S = fro(ES) / lam_max + 12 * u
        y = t["y"][k]
        ny = fro(y)
        Eres = (2 + 2) * u * np.abs(t["res"][k]) + wc * (Ecp[cn] + Ecp[co])
        dy = fro(Eres) / np.sqrt(lam_min) + (np.sqrt(LD(3)) * eps_S + 9 * u) * kappa * ny
        b_chi2.append(2 * ny * dy + dy * dy + (5 + 2) * u * t["chi2"][k])
        if not t["accepted"][k]:
            b_dx.append(np.zeros(n, dtype=LD))
            continue
        a = np.sqrt((t["W"][k] ** 2).sum(axis=1))
        d = np.sqrt((EM ** 2).sum(axis=1)) / np.sqrt(lam_min) + ((np.sqrt(LD(3)) * eps_S + 27 * u) * kappa + (3 + 2) * u) * a
        Edx = d * ny + a * dy + d * dy + (4 + 2) * u * a * ny
        b_dx.append(Edx)
        for col in Ecp:
            cur[col] = cur[col] + t["dx"][k][col:col + 3]
            Ecp[col] = Ecp[col] + Edx[col:col + 3] + u * np.abs(cur[col])
        ks, _, comp_P = next(steps)
        assert ks == k
        EP = EP + (4 + 2) * u * comp_P + np.outer(d, a) + np.outer(a, d) + np.outer(d, d)
    return dict(chi2=np.array(b_chi2, dtype=LD) / u, angle=np.array(b_ang, dtype=LD) / u, dx=np.array(b_dx, dtype=LD).reshape(-1, n) / u,
                P=EP / u)


def keep_mask(c):
    keep = np.ones(c["n"], dtype=bool)
    for i, s in zip(c["retire_ids"], c["retire_sizes"]):
        keep[i:i + s] = False
    return keep


def ratios(name, chi2, angle, dx, P):
    """(chi2, angle, dx, P) error / bound of a result with the truth's decisions; P: the compacted covariance.  An element whose
    bound is zero (outside every accepted pair's reach there is none: W is dense) must be exact."""
    c = case(name)
    t, _, b = truth(name)
    keep = keep_mask(c)
    kk = np.ix_(keep, keep)
    return [B.ratio(chi2, t["chi2"], b["chi2"], -1), B.ratio(angle, t["angle_deg"], b["angle"], -1), B.ratio(dx, t["dx"], b["dx"], -1),
            B.ratio(P, t["P"][kk], b["P"][kk], -1)]


# ---- the plain float64 model and its faults ----------------------------------------------------------------------------------
FAULTS = ("stale_W", "stale_cp", "old_minus_new", "skip_cols_64")


def model(name, fault=None):
    """The merge in plain float64 as the kernels split it (W = M L^-T, P -= W W^T), with one fault:
    stale_W        a rejected pair applies the W the accepted pair before it left
    stale_cp       every pair reads the closest points as they were at entry
    old_minus_new  the residual from cp_old - cp_new in place of cp_new - cp_old
    skip_cols_64   the downdate leaves the columns >= 64 alone
    Returns dict(accepted, chi2, angle_deg, dx, P (compacted))."""
    c = case(name)
    P = np.array(c["P"])
    n = c["n"]
    wc = 1.0 / c["sigma"]
    thr = c["chi2_mult"] * R.CHI2_095_3
    cp0 = {int(col): np.array(v) for col, v in zip(c["plane_col"], c["cp"])}
    cur = {col: v.copy() for col, v in cp0.items()}
    sgn = -1.0 if fault == "old_minus_new" else 1.0
    W = None
    acc, chi2s, angles, dxs = [], [], [], []
    for cn, co in c["pairs"]:
        src = cp0 if fault == "stale_cp" else cur
        c1, c0 = src[cn], src[co]
        dot = float(np.dot(c1 / np.linalg.norm(c1), c0 / np.linalg.norm(c0)))
        with np.errstate(invalid="ignore"):
            angle = (180.0 / np.pi) * np.arccos(dot)
        M = wc * (P[:, cn:cn + 3] - P[:, co:co + 3])
        S = wc * (M[cn:cn + 3] - M[co:co + 3]) + np.eye(3)
        res = wc * (0.0 - sgn * (c1 - c0))
        L = np.linalg.cholesky(S)
        y = np.linalg.solve(L, res)
        chi2 = float(y @ y)
        ok = bool(chi2 < thr and angle < c["deg_max"])
        dx = np.zeros(n)
        if ok:
            W = np.linalg.solve(L, M.T).T
            dx = W @ y
            for col in cur:
                cur[col] = cur[col] + dx[col:col + 3]
        if ok or (fault == "stale_W" and W is not None):
            down = W @ W.T
            if fault == "skip_cols_64":
                down[:, 64:] = 0.0
            P = P - down
        acc.append(ok), chi2s.append(chi2), angles.append(angle), dxs.append(dx)
    return dict(accepted=np.array(acc, dtype=bool), chi2=np.array(chi2s), angle_deg=np.array(angles), dx=np.array(dxs).reshape(-1, n),
                P=R.compact_ref(P, c["retire_ids"], c["retire_sizes"]))


# ---- compaction --------------------------------------------------------------------------------------------------------------
def compact_cases():
    """name -> (n, ids, sizes): bit-equal to retire_ref.compact_ref.  k_cov_compact gives a workgroup 256 output columns and
    rebuilds the scan and the map in each: n_out > 256, ranges that end at, start at and straddle column 256, 1 / 255 / 256 / 257
    single-column ranges in shuffled order (257 needs the scan's second stride), all but one column, the first, the last."""
    rng = np.random.default_rng(77)
    cs = {
        "n300_to_257": (300, [20, 100, 280], [6, 30, 7]),
        "n700_minus_3": (700, [333], [3]),
        "n700_ends_at_256": (700, [250], [6]),
        "n700_starts_at_256": (700, [256], [6]),
        "n700_straddles_256": (700, [254], [6]),
        "n700_around_256_and_512": (700, [254, 510, 3], [3, 5, 1]),
        "n700_all_but_one": (700, [0, 400], [399, 300]),
        "n700_first": (700, [0], [1]),
        "n700_last": (700, [699], [1]),
    }
    for nr in (1, 255, 256, 257):
        cols = rng.permutation(700)[:nr]
        cs["n700_%d_single_columns" % nr] = (700, [int(x) for x in cols], [1] * nr)
    return cs


def compact_model(P, ids, sizes, restart=False):
    """compact_ref through an explicit map output column -> source column; restart: the map counts the removed columns from zero
    again at output column 256 (a workgroup that scanned only its own ranges)"""
    n = P.shape[0]
    keep = np.ones(n, dtype=bool)
    for i, s in zip(ids, sizes):
        keep[i:i + s] = False
    smap = np.nonzero(keep)[0]
    if restart and len(smap) > 256:
        removed_before = smap[255] + 1 - 256                      # what the first workgroup's columns skipped
        smap = np.concatenate([smap[:256], np.minimum(smap[256:] - removed_before, n - 1)])
    return np.ascontiguousarray(P[np.ix_(smap, smap)])
