"""General point features on the device (ovp_cameras_upload / ovp_msckf_general_features / ovp_triangulate_general): features the
batch format cannot carry - another camera's observations, tracks longer than OVP_MAX_MEAS - are linearised, projected and gated
against the resident covariance on the device, and their information pair joins the next point update.  References: the dense
numpy restatement (np_ref.msckf_point_update_dense, np_ref.feature_jacobian_full) and the host-gated dense blocks
(ovp_msckf_dense_blocks)."""
import os

import numpy as np
import pytest

from ov_plane_amd.synth import Scene, make_scene, make_stereo_scene, quat_boxplus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TOL_DX = 1e-6
TOL_P = 1e-4

SCENES = [
    ("stereo_c8", lambda: make_stereo_scene(C=8, F=60, seed=3, chi2_mult=1.0)),
    ("stereo_c11_reject", lambda: make_stereo_scene(C=11, F=80, seed=5, chi2_mult=0.75, stereo_frac=0.3)),
    ("stereo_c20", lambda: make_stereo_scene(C=20, F=40, seed=6, chi2_mult=1.0, stereo_frac=0.5)),
    ("mono_c40", lambda: make_scene(C=40, F=50, seed=41, chi2_mult=1.0, ragged=True)),
]


def relP(Pa, Pb):
    d = np.sqrt(np.abs(np.diag(Pb)))
    return float((np.abs(Pa - Pb) / np.outer(d, d)).max())


def chi2_table():
    return np.load(os.path.join(GOLD, "chi2_095_table.npy"))


def fits_batch(sc):
    cam0 = (sc.cam_idx == 0).all(axis=1) if "cam_idx" in sc else np.ones(sc.F, dtype=bool)
    return cam0 & (sc.n_meas <= 32)


def new_context(capi, sc):
    ctx = capi.Context(sc.N, sc.C, sc.F)
    ctx.cov_upload(sc.P)
    ctx.state_upload(sc)
    ctx.cameras_upload(sc)
    return ctx


def upload_batch(ctx, sc, feats):
    M = min(int(sc.uv.shape[1]), 32)
    ctx.batch_upload(sc.uv[feats, :M], sc.clone_idx[feats, :M], sc.n_meas[feats], sc.p_FinG[feats])


def dense_blocks(sc, feats):
    from oracle import np_ref as R

    blocks = []
    for f in feats:
        H_f, H_x, res, order = R.feature_jacobian_full(sc, int(f))
        Q, _ = np.linalg.qr(H_f, mode="complete")
        N = Q[:, H_f.shape[1]:]
        blocks.append((N.T @ H_x, R.order_cols(order), N.T @ res))
    return blocks


@pytest.mark.gpu
@pytest.mark.parametrize("name,make", SCENES, ids=[s[0] for s in SCENES])
def test_gate_matches_the_dense_path(hiplib, name, make):
    """Every feature of the scene through the new entry: accept decisions equal ovp_msckf_dense_blocks on the same features (rows
    from np_ref) and np_ref.msckf_point_update_dense; chi2 within 1e-8 of the largest."""
    from oracle import np_ref as R

    capi = hiplib
    sc = make()
    ref = R.msckf_point_update_dense(sc, chi2_table())
    if name.endswith("reject"):
        assert not ref["accepted"].all()
    if name == "mono_c40":
        assert int(sc.n_meas.max()) > 32
    ctx = new_context(capi, sc)
    acc, chi2, _ = ctx.msckf_general_features(capi.opts_from_scene(sc), sc)
    assert (acc == ref["accepted"]).all() and acc.sum() >= 0.5 * sc.F
    tol = 1e-8 * np.abs(ref["chi2"]).max()
    assert np.abs(chi2 - ref["chi2"]).max() <= tol
    two = np.where(sc.n_meas >= 2)[0]
    acc_d, chi2_d = ctx.msckf_dense_blocks(sc.opts["chi2_mult"], dense_blocks(sc, two))
    assert (acc_d == acc[two]).all() and np.abs(chi2_d - chi2[two]).max() <= tol
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,make", SCENES, ids=[s[0] for s in SCENES])
def test_one_update_with_the_batch(hiplib, name, make):
    """The features that fit take the batch, the others the new entry: ONE update equal to the dense restatement; the same through
    the sharded entry on a one-rank communicator, bit for bit; a covariance upload in between drops the pending pair; two runs on
    the same inputs are bit-identical."""
    from oracle import np_ref as R

    capi = hiplib
    sc = make()
    fit = fits_batch(sc)
    gen = np.where(~fit)[0]
    if len(gen) < 3:  # (a mono scene: the long tracks plus every third feature go through the new entry)
        gen = np.where(~fit | (np.arange(sc.F) % 3 == 1))[0]
    bat = np.setdiff1d(np.arange(sc.F), gen)
    ref = R.msckf_point_update_dense(sc, chi2_table())
    o = capi.opts_from_scene(sc)
    ctx = new_context(capi, sc)
    runs = []
    for _ in range(2):
        ctx.cov_upload(sc.P)
        acc_g, chi2_g, _ = ctx.msckf_general_features(o, sc, gen)
        upload_batch(ctx, sc, bat)
        out = ctx.msckf_update(o)
        runs.append((acc_g, chi2_g, out, ctx.cov_download()))
    (acc_g, chi2_g, out, P), (acc_2, chi2_2, out2, P2) = runs
    assert (acc_g == ref["accepted"][gen]).all() and (out["accepted"] == ref["accepted"][bat]).all()
    assert np.abs(out["dx"] - ref["dx"]).max() < TOL_DX and relP(P, ref["P"]) < TOL_P
    assert np.array_equal(out["dx"], out2["dx"]) and np.array_equal(P, P2) and np.array_equal(chi2_g, chi2_2)
    comm = capi.rccl_comm_create(capi.rccl_unique_id(), 0, 1, 0)
    try:
        ctx.cov_upload(sc.P)
        ctx.msckf_general_features(o, sc, gen)
        upload_batch(ctx, sc, bat)
        outs = ctx.msckf_update_sharded(o, comm, 0, 1)
        assert np.array_equal(outs["dx"], out["dx"]) and np.array_equal(ctx.cov_download(), P)
    finally:
        capi.rccl_comm_destroy(comm)
    ctx.cov_upload(sc.P)
    ctx.msckf_general_features(o, sc, gen)
    ctx.cov_upload(sc.P)
    upload_batch(ctx, sc, bat)
    out3 = ctx.msckf_update(o)
    sc_b = Scene(sc)
    keep = np.zeros(sc.F, dtype=bool)
    keep[bat] = True
    sc_b["n_meas"] = np.where(keep, sc.n_meas, 0)
    ref3 = R.msckf_point_update_dense(sc_b, chi2_table())
    assert np.abs(out3["dx"] - ref3["dx"]).max() < TOL_DX and relP(ctx.cov_download(), ref3["P"]) < TOL_P
    ctx.close()


# ---- triangulation over every camera: numpy restatement of single_triangulation + single_gaussnewton with per-camera poses ----
def _q2R(q):
    from ov_plane_amd.synth import quat_2_rot

    return quat_2_rot(np.asarray(q, dtype=np.float64))


def triangulate_general_np(sc, f, opts=None):
    """np_ref.triangulate_feature with each observation in its own camera's frame; anchor = last observation of the lowest camera."""
    o = dict(max_runs=5, init_lamda=1e-3, max_lamda=1e10, min_dx=1e-6, min_dcost=1e-6, lam_mult=10.0, min_dist=0.10,
             max_dist=60.0, max_baseline=40.0, max_cond_number=10000.0)
    if opts:
        o.update(opts)
    m = int(sc.n_meas[f])
    if m < 2:
        return False, np.zeros(3)
    camk = sc.cam_idx[f, :m] if "cam_idx" in sc else np.zeros(m, dtype=int)
    tabs = {0: (_q2R(sc.calib_q), np.asarray(sc.calib_p))}
    if "cams" in sc:
        tabs = {k: (_q2R(t["calib_q"]), np.asarray(t["calib_p"])) for k, t in enumerate(sc.cams)}
    elif "cam1" in sc:
        tabs[1] = (_q2R(sc.cam1["calib_q"]), np.asarray(sc.cam1["calib_p"]))
    cams = []
    for k in range(m):
        ci = int(sc.clone_idx[f, k])
        R_ItoC, p_IinC = tabs[int(camk[k])]
        R_GtoC = R_ItoC @ _q2R(sc.clone_q[ci])
        cams.append((R_GtoC, sc.clone_p[ci] - R_GtoC.T @ p_IinC))
    cmin = int(camk.min())
    anchor = max(k for k in range(m) if int(camk[k]) == cmin)
    R_GtoA, p_AinG = cams[anchor]
    uvn = sc.uv_norm[f, :m]
    A, b, rel = np.zeros((3, 3)), np.zeros(3), []
    for k in range(m):
        R_GtoCi, p_CiinG = cams[k]
        R_AtoCi = R_GtoCi @ R_GtoA.T
        p_CiinA = R_GtoA @ (p_CiinG - p_AinG)
        rel.append((R_AtoCi, p_CiinA, -R_AtoCi @ p_CiinA))
        bi = R_AtoCi.T @ np.array([float(uvn[k, 0]), float(uvn[k, 1]), 1.0])
        bi /= np.linalg.norm(bi)
        Sb = np.array([[0, -bi[2], bi[1]], [bi[2], 0, -bi[0]], [-bi[1], bi[0], 0]])
        Ai = Sb.T @ Sb
        A += Ai
        b += Ai @ p_CiinA
    pA = np.linalg.solve(A, b)
    sv = np.linalg.svd(A, compute_uv=False)
    if sv[0] / sv[-1] > o["max_cond_number"] or pA[2] < o["min_dist"] or pA[2] > o["max_dist"]:
        return False, np.zeros(3)

    def cost(al, be, rho):
        e = 0.0
        for k in range(m):
            R, _, pAC = rel[k]
            h = R @ np.array([al, be, 1.0]) + rho * pAC
            z = np.array([h[0] / h[2], h[1] / h[2]]).astype(np.float32)
            r = uvn[k] - z
            e += float(np.sqrt(r[0] * r[0] + r[1] * r[1])) ** 2
        return e

    rho, al, be = 1.0 / pA[2], pA[0] / pA[2], pA[1] / pA[2]
    lam, eps, runs, recompute = o["init_lamda"], 1e4, 0, True
    cost_old = cost(al, be, rho)
    Hess, grad = np.zeros((3, 3)), np.zeros(3)
    while runs < o["max_runs"] and lam < o["max_lamda"] and eps > o["min_dx"]:
        if recompute:
            Hess[:] = 0
            grad[:] = 0
            for k in range(m):
                R, _, pAC = rel[k]
                h = R @ np.array([al, be, 1.0]) + rho * pAC
                H = np.array([[(R[0, 0] * h[2] - h[0] * R[2, 0]), (R[0, 1] * h[2] - h[0] * R[2, 1]), (pAC[0] * h[2] - h[0] * pAC[2])],
                              [(R[1, 0] * h[2] - h[1] * R[2, 0]), (R[1, 1] * h[2] - h[1] * R[2, 1]), (pAC[1] * h[2] - h[1] * pAC[2])]]) / h[2]**2
                z = np.array([h[0] / h[2], h[1] / h[2]]).astype(np.float32)
                r = (uvn[k] - z).astype(np.float64)
                grad += H.T @ r
                Hess += H.T @ H
        Hl = Hess.copy()
        Hl[np.diag_indices(3)] *= (1.0 + lam)
        dx = np.linalg.solve(Hl, grad)
        c = cost(al + dx[0], be + dx[1], rho + dx[2])
        if c <= cost_old and (cost_old - c) / cost_old < o["min_dcost"]:
            al, be, rho = al + dx[0], be + dx[1], rho + dx[2]
            break
        if c <= cost_old:
            recompute, cost_old = True, c
            al, be, rho = al + dx[0], be + dx[1], rho + dx[2]
            runs += 1
            lam /= o["lam_mult"]
            eps = np.linalg.norm(dx)
        else:
            recompute = False
            lam *= o["lam_mult"]
    pA = np.array([al / rho, be / rho, 1.0 / rho])
    u = pA / np.linalg.norm(pA)
    base = max(np.linalg.norm(r[1] - (r[1] @ u) * u) for r in rel)
    if pA[2] < o["min_dist"] or pA[2] > o["max_dist"] or np.linalg.norm(pA) / base > o["max_baseline"]:
        return False, np.zeros(3)
    return True, R_GtoA.T @ pA + p_AinG


def with_camera1_only(sc, feats):
    """The stereo features `feats` keep only camera 1's observations (features no camera-0 triangulation can place)."""
    s = Scene(sc)
    uv, uvn, ci, cam, nm = sc.uv.copy(), sc.uv_norm.copy(), sc.clone_idx.copy(), sc.cam_idx.copy(), sc.n_meas.copy()
    for f in feats:
        m = int(nm[f]) // 2
        uv[f, :m], uvn[f, :m], ci[f, :m] = uv[f, m:2 * m], uvn[f, m:2 * m], ci[f, m:2 * m]
        uv[f, m:], uvn[f, m:], ci[f, m:] = 0, 0, -1
        cam[f, :m], cam[f, m:] = 1, 0
        nm[f] = m
    s.update(uv=uv, uv_norm=uvn, clone_idx=ci, cam_idx=cam, n_meas=nm)
    return s


@pytest.mark.gpu
def test_triangulation_over_every_camera(hiplib):
    capi = hiplib
    sc0 = make_stereo_scene(C=20, F=40, seed=6, chi2_mult=1.0, stereo_frac=0.5)
    sc = with_camera1_only(sc0, np.arange(0, sc0.n_stereo, 3))
    assert ((sc.cam_idx == 1) | (np.arange(sc.cam_idx.shape[1])[None] >= sc.n_meas[:, None])).all(axis=1).sum() >= 5
    ctx = new_context(capi, sc)
    out = ctx.triangulate_general(sc)
    ref = [triangulate_general_np(sc, f) for f in range(sc.F)]
    ok_ref = np.array([r[0] for r in ref])
    p_ref = np.array([r[1] for r in ref])
    assert (out["ok"] == ok_ref).all() and ok_ref.sum() >= 0.9 * sc.F
    assert np.abs(out["p_FinG"][ok_ref] - p_ref[ok_ref]).max() < 1e-6
    # 1-D triangulation along the anchor bearing runs as well (the anchor of a camera-1-only feature is camera 1's)
    out1 = ctx.triangulate_general(sc, opts=capi.triang_defaults(triangulate_1d=1, refine_features=0))
    assert out1["ok"].sum() >= 0.9 * sc.F
    assert np.abs(out1["p_FinG"][out1["ok"]] - sc.truth["p_f"][out1["ok"]]).max() < 0.5
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(C=8, F=60, seed=3, chi2_mult=1.0), dict(C=11, F=80, seed=5, chi2_mult=0.75, stereo_frac=0.3),
                                dict(C=20, F=40, seed=6, chi2_mult=1.0, stereo_frac=0.5)])
def test_updater_option_on(hiplib, kw):
    """UpdaterMSCKF::update with StateOptions::gpu_general_features: same state and covariance as the dense restatement; with the
    option off the outputs are those of the default path, bit for bit."""
    from ov_plane_amd.build import build_host
    from oracle import np_ref as R

    build_host()
    from ov_plane_amd import hostlib

    sc = make_stereo_scene(**kw)
    ref = R.msckf_point_update_dense(sc, chi2_table())
    out = hostlib.run_msckf_update(sc, general_features=True)
    assert (out["kept"] == ref["accepted"]).all()
    dx, ids = ref["dx"], sc.ids
    for i in range(sc.C):
        cid = ids["clones"][i]
        assert np.abs(out["clone_q"][i] - quat_boxplus(sc.clone_q[i], dx[cid:cid + 3])).max() < TOL_DX
        assert np.abs(out["clone_p"][i] - (sc.clone_p[i] + dx[cid + 3:cid + 6])).max() < TOL_DX
    assert np.abs(out["cam1"]["intr"] - (sc.cam1["intr"] + dx[ids["intr1"]:ids["intr1"] + 8])).max() < TOL_DX
    assert relP(out["P"], ref["P"]) < TOL_P
    a, b = hostlib.run_msckf_update(sc), hostlib.run_msckf_update(sc, general_features=False)
    for k in ("clone_q", "clone_p", "calib_q", "calib_p", "intr", "P", "kept"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["cam1"]["intr"], b["cam1"]["intr"])


@pytest.mark.gpu
def test_updater_option_on_keeps_camera1_only_features(hiplib):
    """With triangulation in the updater: features seen by camera 1 only are triangulated over camera 1 and updated (camera-0
    triangulation erases them); reference = the numpy triangulation over every camera, then the dense update."""
    from ov_plane_amd.build import build_host
    from oracle import np_ref as R

    build_host()
    from ov_plane_amd import hostlib

    sc0 = make_stereo_scene(C=20, F=40, seed=6, chi2_mult=1.0, stereo_frac=0.5)
    c1 = np.arange(0, sc0.n_stereo, 3)
    sc = with_camera1_only(sc0, c1)
    tri = [triangulate_general_np(sc, f) for f in range(sc.F)]
    assert all(t[0] for t in tri)
    sc2 = Scene(sc)
    sc2["p_FinG"] = np.array([t[1] for t in tri])
    ref = R.msckf_point_update_dense(sc2, chi2_table())
    off = hostlib.run_msckf_update(sc, triangulate=True)
    assert not off["kept"][c1].any()   # today's path: camera-0 triangulation fails on them, they are erased
    out = hostlib.run_msckf_update(sc, triangulate=True, general_features=True)
    assert (out["kept"] == ref["accepted"]).all() and out["kept"][c1].sum() >= len(c1) - 1
    dx, ids = ref["dx"], sc.ids
    for i in range(sc.C):
        cid = ids["clones"][i]
        assert np.abs(out["clone_p"][i] - (sc.clone_p[i] + dx[cid + 3:cid + 6])).max() < TOL_DX
    assert np.abs(out["cam1"]["intr"] - (sc.cam1["intr"] + dx[ids["intr1"]:ids["intr1"] + 8])).max() < TOL_DX
    assert relP(out["P"], ref["P"]) < TOL_P


@pytest.mark.gpu
def test_limits_are_argument_checks(hiplib):
    """OVP_E_CAPACITY above OVP_GEN_MAX_MEAS observations, OVP_E_ARG for a camera without tables: refused on the host, nothing runs."""
    capi = hiplib
    sc = make_stereo_scene(C=8, F=6, seed=3, chi2_mult=1.0)
    ctx = new_context(capi, sc)
    o = capi.opts_from_scene(sc)
    M = capi.OVP_GEN_MAX_MEAS + 1
    uv = np.zeros((1, M, 2), dtype=np.float32)
    ci = np.zeros((1, M), dtype=np.int32)
    cam = np.zeros((1, M), dtype=np.int32)
    _, _, rc = ctx.msckf_general_features(o, uv=uv, clone_idx=ci, cam_idx=cam, n_meas=[M], p_FinG=np.ones((1, 3)), raise_on_error=False)
    assert rc == capi.OVP_E_CAPACITY
    assert ctx.triangulate_general(uv_norm=uv, clone_idx=ci, cam_idx=cam, n_meas=[M], raise_on_error=False)["rc"] == capi.OVP_E_CAPACITY
    cam2 = sc.cam_idx[:2].copy()
    cam2[1, 0] = 2   # two cameras uploaded
    _, _, rc = ctx.msckf_general_features(o, uv=sc.uv[:2], clone_idx=sc.clone_idx[:2], cam_idx=cam2, n_meas=sc.n_meas[:2],
                                          p_FinG=sc.p_FinG[:2], raise_on_error=False)
    assert rc == capi.OVP_E_ARG
    assert ctx.triangulate_general(uv_norm=sc.uv_norm[:2], clone_idx=sc.clone_idx[:2], cam_idx=cam2, n_meas=sc.n_meas[:2],
                                   raise_on_error=False)["rc"] == capi.OVP_E_ARG
    # the context is untouched: a regular call still works
    acc, _, rc = ctx.msckf_general_features(o, sc)
    assert rc == 0 and acc.any()
    ctx.close()
