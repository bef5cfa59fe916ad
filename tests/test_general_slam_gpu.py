"""SLAM landmarks seen by any camera on the device (ovp_slam_update_general / ovp_slam_delayed_init_general, csrc/k_slam.hip
k_slam_gate_gen, csrc/k_dinit.hip k_dinit_rows_gen) and the host mirror's StateOptions::gpu_general_slam.  The reference is a dense
numpy restatement written here: np_ref.feature_jacobian_full (every camera's tables, plane rows), np_ref.get_marginal_covariance /
np_ref.ekf_update, the chi2 / no-plane fallback rule of UpdaterSLAM::update and a sequential StateHelper::initialize."""
import os

import numpy as np
import pytest

from ov_plane_amd.synth import Scene, make_slam_scene, make_stereo_scene, make_stereo_slam_scene, quat_2_rot, quat_boxplus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TOL_DX = 1e-6
TOL_P = 1e-4


def relP(Pa, Pb):
    d = np.sqrt(np.abs(np.diag(Pb)))
    return float((np.abs(Pa - Pb) / np.outer(d, d)).max())


def chi2_table():
    return np.load(os.path.join(GOLD, "chi2_095_table.npy"))


def plane_args(sc):
    pid = np.asarray(sc.plane_id, dtype=np.int64)
    if sc.cp.shape[0] == 0:
        return None, None, None
    sid = np.where(pid > 0, np.asarray(sc.plane_state_id)[np.maximum(pid, 1) - 1], -1).astype(np.int32)
    return sid, np.asarray(sc.cp)[np.maximum(pid, 1) - 1], np.asarray(sc.cp_fej)[np.maximum(pid, 1) - 1]


def new_context(capi, sc, cap=None):
    ctx = capi.Context(sc.N if cap is None else cap, sc.C, sc.F)
    ctx.cov_upload(sc.P)
    ctx.state_upload(sc)
    ctx.cameras_upload(sc)
    return ctx


def landmark_block(sc, l, with_plane):
    """[H_x | H_landmark], state columns, residual of landmark l (bearing rows of every camera, plus the plane rows)."""
    from oracle import np_ref as R

    sid, cp, cpf = plane_args(sc)
    plane = with_plane and sid is not None and sid[l] >= 0
    H_f, H_x, res, order = R.feature_jacobian_full(sc, l, p_FinG=sc.p_FinG[l], cp=cp[l] if plane else None,
                                                   cp_fej=cpf[l] if plane else None, plane_state_id=int(sid[l]) if plane else -1,
                                                   planeid=int(sc.plane_id[l]) if plane else 0)
    cols = np.r_[R.order_cols(order), int(sc.lm_id[l]) + np.arange(3)]
    return np.hstack([H_x, H_f[:, :3]]), cols, res


def slam_update_reference(sc, pre=()):
    """UpdaterSLAM::update (update/UpdaterSLAM.cpp:526-673) densely: each landmark gated against the prior (with its plane rows,
    then - if those fail - without them), the accepted blocks stacked, one EKF update.  Landmarks in `pre` carry no plane rows."""
    from oracle import np_ref as R

    tab, mult = chi2_table(), sc.opts["chi2_mult"]
    sid, _, _ = plane_args(sc)

    def chi2_of(H, cols, r):
        S = H @ R.get_marginal_covariance(sc.P, [(int(c), 1) for c in cols]) @ H.T + np.eye(len(r))
        return float(r @ np.linalg.solve(S, r))

    status, chi2, blocks = np.zeros(sc.F, np.uint8), np.zeros(sc.F), []
    for l in range(sc.F):
        plane = sid is not None and sid[l] >= 0 and l not in pre
        H, cols, r = landmark_block(sc, l, plane)
        x = chi2_of(H, cols, r)
        if x <= mult * tab[len(r)]:
            status[l], chi2[l] = 1, x
            blocks.append((H, cols, r))
            continue
        if plane:
            H, cols, r = landmark_block(sc, l, False)
            x = chi2_of(H, cols, r)
            if x <= mult * tab[len(r)]:
                status[l] = 2
                blocks.append((H, cols, r))
        chi2[l] = x
    allc = sorted(set(int(c) for _, cols, _ in blocks for c in cols))
    pos = {c: i for i, c in enumerate(allc)}
    Hb = np.zeros((sum(len(r) for _, _, r in blocks), len(allc)))
    rb = np.zeros(Hb.shape[0])
    row = 0
    for H, cols, r in blocks:
        for j, c in enumerate(cols):
            Hb[row:row + len(r), pos[int(c)]] += H[:, j]
        rb[row:row + len(r)] = r
        row += len(r)
    P, dx = R.ekf_update(sc.P, [(c, 1) for c in allc], Hb, rb)
    return dict(status=status, chi2=chi2, dx=dx, P=P)


def plane_slam(sc):
    sid, cp, cpf = plane_args(sc)
    return dict(plane_state_id=sid, cp=cp, cp_fej=cpf)


UPDATE_SCENES = [
    ("planes_fallback_outliers", lambda: make_stereo_slam_scene(C=11, n_slam=14, seed=4, n_planes=3, outliers=2, wrong_plane=3,
                                                                cam1_only=2, do_fej=False)),
    ("no_planes_calib_off", lambda: make_stereo_slam_scene(C=8, n_slam=10, seed=5, outliers=1, do_fej=False)),
    ("c20_planes", lambda: make_stereo_slam_scene(C=20, n_slam=12, seed=6, n_planes=2, wrong_plane=1, do_fej=False)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,make", UPDATE_SCENES, ids=[s[0] for s in UPDATE_SCENES])
def test_slam_update_general_matches_numpy(hiplib, name, make):
    """Statuses equal, chi2 within 1e-9 relative, dx within 1e-6, normalised dP within 1e-4 of the dense restatement; the first
    scene also carries a host-built block (pre_*) for one landmark in the same call."""
    capi = hiplib
    sc = make()
    if name == "no_planes_calib_off":
        sc["opts"] = dict(sc.opts, do_calib_pose=False, do_calib_intr=False)
    pre_l = (1,) if name.startswith("planes") else ()
    ref = slam_update_reference(sc, pre=pre_l)
    pre = None
    if pre_l:
        pre = [None] * sc.F
        for l in pre_l:
            H, cols, r = landmark_block(sc, l, False)
            pre[l] = (H, cols, r)
    ctx = new_context(capi, sc)
    kw = plane_slam(sc)
    out = ctx.slam_update_general(capi.opts_from_scene(sc), sc.uv, sc.clone_idx, sc.cam_idx, sc.n_meas, sc.p_FinG, sc.p_FinG_fej,
                                  sc.lm_id, kw["plane_state_id"], kw["cp"], kw["cp_fej"], pre=pre)
    assert (out["status"] == ref["status"]).all(), (out["status"], ref["status"])
    if name.startswith("planes"):
        assert (out["status"] == 2).any() and (out["status"] == 0).any()
    assert np.abs(out["chi2"] - ref["chi2"]).max() <= 1e-9 * max(1.0, np.abs(ref["chi2"]).max())
    assert np.abs(out["dx"] - ref["dx"]).max() < TOL_DX
    assert relP(ctx.cov_download(), ref["P"]) < TOL_P
    assert out["info"].n_accepted == int((ref["status"] > 0).sum())
    ctx.close()


@pytest.mark.gpu
def test_camera0_batch_through_the_general_entry_matches_the_mono_entry(hiplib):
    """A camera-0-only batch (planes, FEJ, the no-plane fallback) through ovp_slam_update_general equals ovp_slam_update to 1e-12."""
    capi = hiplib
    sc = make_slam_scene(C=11, n_slam=14, seed=4, n_planes=3, outliers=2, wrong_plane=3)
    o = capi.opts_from_scene(sc)
    sid, cp, cpf = plane_args(sc)
    ctx = capi.Context(sc.N, sc.C, sc.F)
    ctx.cov_upload(sc.P)
    ctx.state_upload(sc)
    ctx.cameras_upload(sc)
    a = ctx.slam_update(o, sc.uv, sc.clone_idx, sc.n_meas, sc.p_FinG, sc.p_FinG_fej, sc.lm_id, sid, cp, cpf)
    Pa = ctx.cov_download()
    ctx.cov_upload(sc.P)
    b = ctx.slam_update_general(o, sc.uv, sc.clone_idx, np.zeros(sc.clone_idx.shape, np.int32), sc.n_meas, sc.p_FinG, sc.p_FinG_fej,
                                sc.lm_id, sid, cp, cpf)
    Pb = ctx.cov_download()
    assert (a["status"] == b["status"]).all() and (a["status"] == 2).any()
    assert np.abs(a["chi2"] - b["chi2"]).max() <= 1e-12 * max(1.0, np.abs(a["chi2"]).max())
    assert np.abs(a["dx"] - b["dx"]).max() <= 1e-12 and relP(Pb, Pa) <= 1e-12
    ctx.close()


def stereo_candidates(C=16, F=10, seed=3, cam1_only=(1, 4, 7), chi2_mult=1.0):
    """make_stereo_scene candidates (every stereo track: camera 0's views, then camera 1's at the same clones, <= 2 C), some of
    them reduced to their camera-1 views."""
    sc = make_stereo_scene(C=C, F=F, seed=seed, stereo_frac=0.8, chi2_mult=chi2_mult)
    sc = Scene(sc)
    uv, uvn, ci, cam, nm = sc.uv.copy(), sc.uv_norm.copy(), sc.clone_idx.copy(), sc.cam_idx.copy(), sc.n_meas.copy()
    for f in cam1_only:
        m = int(nm[f])
        sel = np.where(cam[f, :m] == 1)[0]
        assert len(sel) >= 2
        k = len(sel)
        uv[f, :k], uvn[f, :k], ci[f, :k], cam[f, :k] = uv[f, sel], uvn[f, sel], ci[f, sel], 1
        uv[f, k:], uvn[f, k:], ci[f, k:], cam[f, k:] = 0, 0, -1, 0
        nm[f] = k
    sc.update(uv=uv, uv_norm=uvn, clone_idx=ci, cam_idx=cam, n_meas=nm)
    return sc


def delayed_init_reference(sc):
    """UpdaterSLAM::delayed_init downstream of triangulation, candidate after candidate: get_feature_jacobian_full at the state the
    previous candidate left, StateHelper::initialize (QR split, chi2 of the update rows with dof = all rows, initialize_invertible,
    EKF update with the update rows), Type::update of every variable."""
    from oracle import np_ref as R

    tab, mult = chi2_table(), sc.opts["chi2_mult"]
    st = dict(clone_q=sc.clone_q.copy(), clone_p=sc.clone_p.copy(), clone_q_fej=sc.clone_q_fej, clone_p_fej=sc.clone_p_fej,
              calib_q=sc.calib_q.copy(), calib_p=sc.calib_p.copy(), intr=sc.intr.copy(), cam1=dict(sc.cam1))
    P = sc.P.copy()
    n0 = P.shape[0]
    ids = sc.ids
    lm = []  # (id, value)
    ok, new_id, dinit, dxs = np.zeros(sc.F, bool), -np.ones(sc.F, int), np.zeros((sc.F, 3)), []
    for l in range(sc.F):
        H_f, H_x, res, order = R.feature_jacobian_full(sc, l, p_FinG=sc.p_FinG[l], state=st)
        cols = R.order_cols(order)
        Q, Rf = np.linalg.qr(H_f, mode="complete")
        Hi, Hu = Q[:, :3].T @ H_x, Q[:, 3:].T @ H_x
        ri, ru = Q[:, :3].T @ res, Q[:, 3:].T @ res
        RL = Rf[:3, :3]
        S = Hu @ P[np.ix_(cols, cols)] @ Hu.T + np.eye(len(ru))
        x = float(ru @ np.linalg.solve(S, ru))
        if not x <= mult * tab[len(res)]:
            dxs.append(None)
            continue
        n = P.shape[0]
        Li = np.linalg.inv(RL)
        cross = -P[:, cols] @ Hi.T @ Li.T
        blk = Li @ (Hi @ P[np.ix_(cols, cols)] @ Hi.T + np.eye(3)) @ Li.T
        Pn = np.zeros((n + 3, n + 3))
        Pn[:n, :n], Pn[:n, n:], Pn[n:, :n], Pn[n:, n:] = P, cross, cross.T, blk
        P, dx = R.ekf_update(Pn, [(int(c), 1) for c in cols], Hu, ru)
        ok[l], new_id[l], dinit[l] = True, n, Li @ ri
        lm.append([n, sc.p_FinG[l] + Li @ ri])
        for e in lm:
            e[1] = e[1] + dx[e[0]:e[0] + 3]
        for i in range(sc.C):
            cid = ids["clones"][i]
            st["clone_q"][i] = quat_boxplus(st["clone_q"][i], dx[cid:cid + 3])
            st["clone_p"][i] = st["clone_p"][i] + dx[cid + 3:cid + 6]
        st["calib_q"] = quat_boxplus(st["calib_q"], dx[ids["calib"]:ids["calib"] + 3])
        st["calib_p"] = st["calib_p"] + dx[ids["calib"] + 3:ids["calib"] + 6]
        st["intr"] = st["intr"] + dx[ids["intr"]:ids["intr"] + 8]
        c1 = st["cam1"]
        st["cam1"] = dict(c1, calib_q=quat_boxplus(c1["calib_q"], dx[ids["calib1"]:ids["calib1"] + 3]),
                          calib_p=c1["calib_p"] + dx[ids["calib1"] + 3:ids["calib1"] + 6], intr=c1["intr"] + dx[ids["intr1"]:ids["intr1"] + 8])
        dxs.append(dx)
    assert n0 + 3 * int(ok.sum()) == P.shape[0]
    return dict(ok=ok, new_id=new_id, delta_init=dinit, dx=dxs, P=P, state=st, lm=lm)


def cam_table(q, p, intr):
    return np.r_[quat_2_rot(q).ravel(), p, intr]


@pytest.mark.gpu
def test_slam_delayed_init_general_matches_sequential_initialize(hiplib):
    """Ten stereo candidates at C = 16 (tracks of up to 32 views), three of them seen by camera 1 alone, calibration estimated:
    decisions, ids, H_L^-1 res_init, every candidate's correction, the final covariance, and the device camera tables after the call
    against the host applying the returned corrections in order."""
    capi = hiplib
    sc = stereo_candidates()
    assert int(sc.n_meas.max()) > 16
    ref = delayed_init_reference(sc)
    assert ref["ok"].sum() >= 6
    ctx = new_context(capi, sc, cap=sc.N + 3 * sc.F)
    out = ctx.slam_delayed_init_general(capi.opts_from_scene(sc), sc.uv, sc.clone_idx, sc.cam_idx, sc.n_meas, sc.p_FinG)
    assert (out["ok"] == ref["ok"]).all() and (out["new_id"] == ref["new_id"]).all()
    acc = np.where(ref["ok"])[0]
    assert np.abs(out["delta_init"][acc] - ref["delta_init"][acc]).max() < TOL_DX
    for l in acc:
        n = len(ref["dx"][l])
        assert np.abs(out["dx"][l][:n] - ref["dx"][l]).max() < TOL_DX
    assert ctx.cov_size() == ref["P"].shape[0]
    assert relP(ctx.cov_download(), ref["P"]) < TOL_P
    # the device tables = the caller's Type::update of the returned corrections, in order
    cq, cpos, cal0q, cal0p, intr0 = sc.clone_q.copy(), sc.clone_p.copy(), sc.calib_q.copy(), sc.calib_p.copy(), sc.intr.copy()
    c1 = dict(sc.cam1)
    ids = sc.ids
    for l in acc:
        dx = out["dx"][l]
        for i in range(sc.C):
            cid = ids["clones"][i]
            cq[i] = quat_boxplus(cq[i], dx[cid:cid + 3])
            cpos[i] = cpos[i] + dx[cid + 3:cid + 6]
        cal0q = quat_boxplus(cal0q, dx[ids["calib"]:ids["calib"] + 3])
        cal0p = cal0p + dx[ids["calib"] + 3:ids["calib"] + 6]
        intr0 = intr0 + dx[ids["intr"]:ids["intr"] + 8]
        c1 = dict(c1, calib_q=quat_boxplus(c1["calib_q"], dx[ids["calib1"]:ids["calib1"] + 3]),
                  calib_p=c1["calib_p"] + dx[ids["calib1"] + 3:ids["calib1"] + 6], intr=c1["intr"] + dx[ids["intr1"]:ids["intr1"] + 8])
    cal, gen = ctx.camera_tables_download(2)
    t0, t1 = cam_table(cal0q, cal0p, intr0), cam_table(c1["calib_q"], c1["calib_p"], c1["intr"])
    assert np.abs(cal - t0).max() < 1e-9 and np.abs(gen[0] - t0).max() < 1e-9 and np.abs(gen[1] - t1).max() < 1e-9
    assert np.abs(t1 - cam_table(sc.cam1["calib_q"], sc.cam1["calib_p"], sc.cam1["intr"])).max() > 1e-9  # (camera 1 did move)
    assert np.abs(cpos - ref["state"]["clone_p"]).max() < TOL_DX and np.abs(c1["intr"] - ref["state"]["cam1"]["intr"]).max() < TOL_DX
    ctx.close()


@pytest.mark.gpu
def test_general_slam_runs_are_bit_identical_and_limits_touch_nothing(hiplib):
    """Two runs of each entry on the same inputs give identical bits; a candidate beyond the rows kernel (40 views) gives
    OVP_E_CAPACITY and a bad cam_idx OVP_E_ARG, both with the covariance and the camera tables byte-identical."""
    capi = hiplib
    sc = make_stereo_slam_scene(C=11, n_slam=12, seed=4, n_planes=2, outliers=1, wrong_plane=1)
    o = capi.opts_from_scene(sc)
    kw = plane_slam(sc)
    ctx = new_context(capi, sc)
    runs = []
    for _ in range(2):
        ctx.cov_upload(sc.P)
        r = ctx.slam_update_general(o, sc.uv, sc.clone_idx, sc.cam_idx, sc.n_meas, sc.p_FinG, sc.p_FinG_fej, sc.lm_id,
                                    kw["plane_state_id"], kw["cp"], kw["cp_fej"])
        runs.append((r, ctx.cov_download()))
    (a, Pa), (b, Pb) = runs
    assert np.array_equal(a["dx"], b["dx"]) and np.array_equal(Pa, Pb) and np.array_equal(a["chi2"], b["chi2"])
    # a bad camera index: OVP_E_ARG, nothing touched
    ctx.cov_upload(sc.P)
    bad = sc.cam_idx.copy()
    bad[0, 0] = 2
    r = ctx.slam_update_general(o, sc.uv, sc.clone_idx, bad, sc.n_meas, sc.p_FinG, sc.p_FinG_fej, sc.lm_id, raise_on_error=False)
    assert r["rc"] == capi.OVP_E_ARG and np.array_equal(ctx.cov_download(), sc.P)
    ctx.close()
    # delayed initialisation: determinism, then the limits
    dc = stereo_candidates(C=12, F=6, seed=5, cam1_only=(2,))
    od = capi.opts_from_scene(dc)
    outs = []
    for _ in range(2):
        ctx = new_context(capi, dc, cap=dc.N + 3 * dc.F)
        outs.append((ctx.slam_delayed_init_general(od, dc.uv, dc.clone_idx, dc.cam_idx, dc.n_meas, dc.p_FinG), ctx.cov_download(),
                     ctx.camera_tables_download(2)))
        ctx.close()
    (a, Pa, ta), (b, Pb, tb) = outs
    assert a["ok"].any() and np.array_equal(a["dx"], b["dx"]) and np.array_equal(Pa, Pb)
    assert np.array_equal(ta[0], tb[0]) and np.array_equal(ta[1], tb[1])
    ctx = new_context(capi, dc, cap=dc.N + 3 * dc.F)
    t0 = ctx.camera_tables_download(2)
    M = 40
    uv = np.zeros((dc.F, M, 2), np.float32)
    ci = -np.ones((dc.F, M), np.int32)
    cam = np.zeros((dc.F, M), np.int32)
    uv[:, :dc.uv.shape[1]], ci[:, :dc.uv.shape[1]], cam[:, :dc.uv.shape[1]] = dc.uv, dc.clone_idx, dc.cam_idx
    nm = dc.n_meas.copy()
    m0 = int(nm[0])
    uv[0, m0:M], ci[0, m0:M], cam[0, m0:M] = uv[0, 0], ci[0, 0], cam[0, 0]   # candidate 0: 40 views
    nm[0] = M
    r = ctx.slam_delayed_init_general(od, uv, ci, cam, nm, dc.p_FinG, raise_on_error=False)
    assert r["rc"] == capi.OVP_E_CAPACITY and ctx.cov_size() == dc.N and np.array_equal(ctx.cov_download(), dc.P)
    bad = dc.cam_idx.copy()
    bad[1, 0] = 3
    r = ctx.slam_delayed_init_general(od, dc.uv, dc.clone_idx, bad, dc.n_meas, dc.p_FinG, raise_on_error=False)
    assert r["rc"] == capi.OVP_E_ARG and ctx.cov_size() == dc.N and np.array_equal(ctx.cov_download(), dc.P)
    t1 = ctx.camera_tables_download(2)
    assert np.array_equal(t0[0], t1[0]) and np.array_equal(t0[1], t1[1])
    ctx.close()


@pytest.mark.gpu
def test_host_mirror_slam_update_general_route(hiplib):
    """UpdaterSLAM::update on a stereo SLAM state with gpu_general_slam on (device general entry) against off (update_dense on the
    host): decisions equal, state and covariance within tolerance."""
    from ov_plane_amd import hostlib

    sc = make_stereo_slam_scene(C=11, n_slam=12, seed=4, n_planes=2, outliers=1, wrong_plane=2, cam1_only=1)
    off = hostlib.run_updater(sc, "slam_update")
    assert off["route"] == 3
    on = hostlib.run_updater(sc, "slam_update", general_slam=True)
    assert on["route"] == 1
    for k in ("kept", "deleted", "should_marg", "slam_to_plane"):
        assert np.array_equal(on[k], off[k]), k
    assert on["should_marg"].any()
    assert np.abs(on["slam_p"] - off["slam_p"]).max() < TOL_DX and np.abs(on["clone_p"] - off["clone_p"]).max() < TOL_DX
    assert np.abs(on["cam1"] - off["cam1"]).max() < TOL_DX and np.abs(on["intr"] - off["intr"]).max() < TOL_DX
    assert relP(on["P"], off["P"]) < TOL_P


@pytest.mark.gpu
def test_host_mirror_slam_delayed_init_general_route(hiplib):
    """UpdaterSLAM::delayed_init on stereo candidates with gpu_general_slam on (one device loop) against off (the per-candidate host
    loop): the same landmarks join at the same ids with the same values; state and covariance within tolerance."""
    from ov_plane_amd import hostlib

    sc = stereo_candidates(C=12, F=8, seed=7, cam1_only=(3,))
    off = hostlib.run_updater(sc, "slam_delayed_init")
    assert off["route"] == 4
    on = hostlib.run_updater(sc, "slam_delayed_init", general_slam=True)
    assert on["route"] == 1
    assert np.array_equal(on["new_id"], off["new_id"]) and (on["new_id"][: sc.F] >= 0).sum() >= 5
    ok = on["new_id"][: sc.F] >= 0
    assert np.abs(on["new_p"][: sc.F][ok] - off["new_p"][: sc.F][ok]).max() < TOL_DX
    assert np.abs(on["clone_p"] - off["clone_p"]).max() < TOL_DX and np.abs(on["cam1"] - off["cam1"]).max() < TOL_DX
    assert on["n"] == off["n"] and relP(on["P"], off["P"]) < TOL_P


@pytest.mark.gpu
def test_camera1_only_feature_survives_triangulation_with_the_option(hiplib):
    """delayed_init with triangulation on the device: with gpu_general_slam on, features seen only by camera 1 are triangulated with
    camera 1's extrinsics (ovp_triangulate_general) and initialised by the device loop.  The mono kernel the option-off path uses
    places every view at camera 0's pose: its position of such a feature is off by about the stereo baseline."""
    from ov_plane_amd import hostlib

    capi = hiplib
    sc = stereo_candidates(C=12, F=8, seed=7, cam1_only=(3, 5))
    on = hostlib.run_updater(sc, "slam_delayed_init", general_slam=True, triangulate=True)
    assert on["route"] == 1
    assert (on["new_id"][[3, 5]] >= 0).all() and (on["new_id"][: sc.F] >= 0).sum() >= 6
    off = hostlib.run_updater(sc, "slam_delayed_init", triangulate=True)
    assert off["route"] == 4
    # the triangulation itself: general (every view at its own camera) against mono (camera 0's extrinsics for every view)
    feats = np.array([3, 5])
    ctx = new_context(capi, sc)
    ctx.batch_upload(sc.uv[feats], sc.clone_idx[feats], sc.n_meas[feats], sc.p_FinG[feats])
    mono = ctx.triangulate(sc.uv_norm[feats])
    gen = ctx.triangulate_general(sc, feats)
    ctx.close()
    assert gen["ok"].all()
    truth = sc.truth["p_f"][feats]
    err_g = np.linalg.norm(gen["p_FinG"] - truth, axis=1)
    err_m = np.linalg.norm(mono["p_FinG"] - truth, axis=1)
    assert (np.linalg.norm(gen["p_FinG"] - mono["p_FinG"], axis=1) > 0.05).all() and (err_g < err_m).all(), (err_g, err_m)
