"""GPU tests of ovp_plane_fit_refine: RANSAC fit and joint refinement of every plane of a frame in one device pass, over the
observations of two cameras.

References: numpy for the pose table; the device's own per-plane pair ovp_plane_fitting + ovp_plane_optimize, fed with the pose
table the fused entry returned and the inliers in order (bit for bit - the same kernels on the same lists); the oracle chain of
tests/plane_frontend_ref.py (flags, iteration counts and kept sets equal, values within 1e-9: the tolerance of
test_plane_optimize_matches_oracle in tests/test_gpu_parity.py)."""
import numpy as np
import pytest

from ov_plane_amd.synth import make_plane_frontend_scene
from tests import plane_frontend_ref as R

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
TOL = 1e-9  # tests/test_gpu_parity.py::test_plane_optimize_matches_oracle

# 8 planes in one call.  The scans of k_planefit_link run over 256 threads (4 waves) and its items in passes of 256: a plane whose
# outliers lie behind its second wave, one of exactly 256 features (8 views each: 2048 items), failed planes between good ones.
BIG = dict(C=8, seed=7, planes=[
    dict(n=130, outliers=20, stereo=10),               # 110 inliers, compaction across two wave boundaries
    dict(n=12, kind="scatter"),                        # RANSAC fails
    dict(n=256),                                       # the capacity limit; 2048 observation items
    dict(n=3),                                         # fewer than 4 features
    dict(n=10, kind="fixed", n_slam=2, stereo=3),      # in-state plane
    dict(n=20, n_slam=3, stereo=6),                    # SLAM constants on a free plane
    dict(n=12, kind="noisy"),                          # fits, does not converge
    dict(n=16, stereo=6, cam1only=2, short=4)])
# the generator's default planes seen from 20 clones: stereo tracks of 40 views
LONG = dict(C=20, seed=1)
# plane 2: four short camera-0 tracks (fewer than min_inlier_num = 5) and eight features only camera 1 saw
STEREO_ONLY = dict(C=12, seed=5, planes=[
    dict(n=14, outliers=2, stereo=5), dict(n=10, kind="fixed", n_slam=2, stereo=3), dict(n=12, cam1only=8, short=4),
    dict(n=12, kind="scatter"), dict(n=12, stereo=4), dict(n=3), dict(n=14, n_slam=2, stereo=4), dict(n=12, kind="noisy")])

_cache = {}


def _run(hiplib, name, kw, **over):
    """The scene, one context with its tables resident, and the fused call's result (computed once per scene)."""
    key = (name, tuple(sorted(over.items())))
    if name not in _cache:
        sc = make_plane_frontend_scene(**kw)
        ctx = hiplib.Context(sc.N, sc.C, 4)
        ctx.state_upload(sc)
        ctx.cameras_upload(sc)
        _cache[name] = (sc, ctx)
    sc, ctx = _cache[name]
    if key not in _cache:
        _cache[key] = ctx.plane_fit_refine(**R.fused_args(sc, **over))
    return sc, ctx, _cache[key]


def _device_pair(ctx):
    def fit(pts, min_inlier_num, max_cond, variant):
        o = ctx.plane_fitting([0, len(pts)], pts, min_inlier_num, max_cond, variant)
        return dict(ok=bool(o["ok"][0]), abcd=o["abcd"][0], inlier=o["inlier"])

    return fit, (lambda pb: ctx.plane_optimize([pb])[0])


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("kw", [BIG, STEREO_ONLY], ids=["c8", "c12"])
def test_pose_table_against_numpy(hiplib, kw):
    """Every entry is a three-term sum of products of factors bounded by 1 (rotations) or by |p| (positions): 16 eps."""
    sc, ctx, out = _run(hiplib, "c%d" % kw["C"], kw)
    ref = R.pose_table(sc)
    T = out["poses"]
    assert T.shape == (sc.C, 2, 12)
    eR = np.abs(T[:, :, :9] - ref[:, :, :9]).max()
    scale = np.maximum(1.0, np.abs(ref[:, :, 9:]))
    eP = (np.abs(T[:, :, 9:] - ref[:, :, 9:]) / scale).max()
    print("pose table: rotation err %.2e, position err %.2e (eps %.2e)" % (eR, eP, EPS))
    assert eR <= 16 * EPS and eP <= 16 * EPS


@pytest.mark.parametrize("refine", [True, False], ids=["refine", "fit_only"])
def test_bit_identical_to_the_per_plane_pair(hiplib, refine):
    sc, ctx, out = _run(hiplib, "c8", BIG, refine=refine)
    fit, opt = _device_pair(ctx)
    ref = R.chain(sc, out["poses"], fit, opt, refine=refine)
    fs = sc.feat_start
    # the scene does what it was built for
    assert list(ref["fit_ok"]) == [True, False, True, False, True, True, True, True]
    if refine:
        assert list(ref["ok"]) == [True, False, True, False, True, True, False, True] and ref["iterations"][6] == 12
    in0, in2 = ref["inlier"][fs[0]:fs[1]], ref["inlier"][fs[2]:fs[3]]
    assert 105 <= in0.sum() <= 110 and in0[:64].sum() > 60 and not in0[110:].any()  # (a noisy point or two beyond the 5 cm)
    assert len(in2) == 256 and in2.sum() >= 250 and sc.n_meas[fs[2]:fs[3]].sum() == 2048
    for k in ("fit_ok", "abcd", "inlier", "ok", "iterations", "kept", "cp", "p_FinG"):
        assert _bits(out[k], ref[k]), k
    if refine:
        moved = np.abs(out["p_FinG"] - sc.p_FinG).max(axis=1) > 0
        assert moved[fs[2]:fs[3]].sum() > 200 and not moved[fs[1]:fs[2]].any() and not moved[fs[6]:fs[7]].any()
    else:
        assert not out["iterations"].any() and _bits(out["p_FinG"], sc.p_FinG) and _bits(out["kept"], out["inlier"])


@pytest.mark.parametrize("name,kw", [("c12", STEREO_ONLY), ("c20", LONG)], ids=["c12", "c20_40_views"])
def test_parity_with_the_oracle_chain(hiplib, oracle, name, kw):
    """(Not on the 256-feature plane of BIG: the oracle's dense solve takes minutes there; the bit identity with the per-plane
    pair, which test_plane_optimize_matches_oracle holds to the oracle, covers it.)"""
    sc, ctx, out = _run(hiplib, name, kw)
    ref = R.chain(sc, out["poses"], oracle.plane_fitting, oracle.optimize_plane)
    assert ref["ok"].sum() >= 3 and (~ref["ok"]).sum() >= 3
    for k in ("fit_ok", "inlier", "ok", "iterations", "kept"):
        assert (out[k] == ref[k]).all(), k
    e = [float(np.abs(out[k] - ref[k]).max()) for k in ("abcd", "cp", "p_FinG")]
    print("abcd / cp / p_FinG err", e)
    assert max(e) < TOL
    if name == "c20":
        k5 = slice(int(sc.feat_start[5]), int(sc.feat_start[6]))
        assert sc.n_meas.max() == 40 and (out["kept"][k5] & (sc.n_meas[k5] > 32)).any()


def test_long_tracks_and_second_camera_take_part(hiplib, oracle):
    sc, ctx, out = _run(hiplib, "c12", STEREO_ONLY)
    lo, hi = int(sc.feat_start[2]), int(sc.feat_start[3])
    cam0_short = [f for f in range(lo, hi) if not sc.sees_cam1[f]]
    assert len(cam0_short) == 4 < sc.min_inlier_num and sc.sees_cam1[lo:hi].sum() == 8
    ref = R.chain(sc, out["poses"], oracle.plane_fitting, oracle.optimize_plane)
    assert out["ok"][2] and ref["ok"][2] and (out["kept"] == ref["kept"]).all() and (out["ok"] == ref["ok"]).all()
    assert out["kept"][lo:hi].sum() >= 8 and (out["kept"][lo:hi] & sc.sees_cam1[lo:hi]).sum() >= 6
    assert np.abs(out["cp"] - ref["cp"]).max() < TOL and np.abs(out["p_FinG"] - ref["p_FinG"]).max() < TOL
    # the per-plane route over what the camera-0 batch carries does not yield the plane
    fit, opt = _device_pair(ctx)
    mono = R.chain(sc, out["poses"], fit, opt, select=lambda f: not sc.sees_cam1[f])
    assert not mono["fit_ok"][2] and not mono["ok"][2]


def test_limits_are_checked_before_anything_is_enqueued(hiplib):
    sc, ctx, out = _run(hiplib, "c8", BIG)
    # 257 features on one plane
    F = 257
    z = np.zeros((F, 2), dtype=np.int32)
    big = dict(feat_start=[0, F], uv_norm=np.zeros((F, 2, 2), dtype=np.float32), clone_idx=z, cam_idx=z,
               n_meas=np.full(F, 2, dtype=np.int32), p_FinG=np.zeros((F, 3)), cp=[[0.0, 0.0, 3.0]], fix_plane=[0])
    r = ctx.plane_fit_refine(**R.fused_args(sc, **big), raise_on_error=False)
    assert r["rc"] == hiplib.OVP_E_CAPACITY
    # a camera without tables
    cam = sc.cam_idx.copy()
    cam[int(sc.feat_start[7]), 0] = 2
    r = ctx.plane_fit_refine(**R.fused_args(sc, cam_idx=cam), raise_on_error=False)
    assert r["rc"] == hiplib.OVP_E_ARG
    # a clone slot outside the tables, a track longer than the row pitch
    ci = sc.clone_idx.copy()
    ci[0, 0] = sc.C
    assert ctx.plane_fit_refine(**R.fused_args(sc, clone_idx=ci), raise_on_error=False)["rc"] == hiplib.OVP_E_ARG
    nm = sc.n_meas.copy()
    nm[0] = sc.clone_idx.shape[1] + 1
    assert ctx.plane_fit_refine(**R.fused_args(sc, n_meas=nm), raise_on_error=False)["rc"] == hiplib.OVP_E_ARG
    again = ctx.plane_fit_refine(**R.fused_args(sc))
    for k in ("fit_ok", "abcd", "inlier", "ok", "iterations", "kept", "cp", "p_FinG", "poses"):
        assert _bits(out[k], again[k]), k


def teardown_module(module):
    for v in _cache.values():
        if isinstance(v, tuple):
            v[1].close()
    _cache.clear()


# ------------------------------------------------------------------------------------------------------------------
# host mirror: StateOptions::gpu_fused_plane_fit
# ------------------------------------------------------------------------------------------------------------------
FIT = dict(min_feat=5, max_cond=200.0, variant=0)


def _same_bits(a, b, keys):
    for k in keys:
        assert _bits(np.asarray(a[k]), np.asarray(b[k])), k


def test_host_updater_msckf_fused_equals_per_plane_route(hiplib):
    """UpdaterMSCKF::update on the camera-0 scene of test_host_cpp_mirror_updater_msckf_fits_planes_first (which holds the
    per-plane route to the oracle composition within TOL_DX / TOL_P): with the option on, the single ovp_plane_fit_refine call
    gives the per-plane route's accepted planes, consumed features and state bit for bit - same kernels, same lists, and the
    pose table of the device equals the host's clonesCAM.  The option is consumed by the call: the run after it is the per-plane
    route again and repeats the first one."""
    from ov_plane_amd.build import build_host

    build_host()
    from ov_plane_amd import hostlib
    from ov_plane_amd.synth import make_scene

    sc = make_scene(C=10, F=150, seed=72, n_planes=4, feats_per_plane=20, chi2_mult=99999.0, px_noise=0.25, err_scale=0.05)
    keys = ("clone_q", "clone_p", "calib_q", "calib_p", "intr", "cp_state", "P", "kept", "used", "deleted")
    off = hostlib.run_msckf_update(sc, triangulate=True, fit_planes=FIT)
    on = hostlib.run_msckf_update(sc, triangulate=True, fit_planes=FIT, fused_plane_fit=True)
    off2 = hostlib.run_msckf_update(sc, triangulate=True, fit_planes=FIT)
    assert off["used"].sum() > 20
    _same_bits(on, off, keys)
    _same_bits(off2, off, keys)


def test_host_init_vio_plane_fused_equals_per_plane_route(hiplib):
    """UpdaterPlane::init_vio_plane on the camera-0 scene of test_host_cpp_mirror_plane_init_fits_planes_first: the same planes
    with the same ids and values, bit for bit, with the option on and off."""
    from ov_plane_amd.build import build_host

    build_host()
    from ov_plane_amd import hostlib
    from ov_plane_amd.synth import make_scene

    sc = make_scene(C=10, F=16, seed=34, n_planes=2, feats_per_plane=8, planes_in_state_frac=0.0, chi2_mult=1.0, px_noise=0.25,
                    err_scale=0.05)
    off = hostlib.run_updater(sc, "plane_init", 5.0, 1.0, fit_planes=FIT)
    on = hostlib.run_updater(sc, "plane_init", 5.0, 1.0, fit_planes=FIT, fused_plane_fit=True)
    assert off["n"] == on["n"] and (off["new_id"][:2] >= 0).all()
    _same_bits(on, off, ("new_id", "new_p", "deleted", "clone_q", "clone_p", "P"))


def _stereo_fit_scene():
    """Three planes of ten features (interleaved) seen by a stereo pair from 8 clones; the first 21 features are stereo, so every
    plane has seven stereo features and three camera-0 tracks.  On plane 1 the seven are seen by camera 1 ONLY: three features
    are all the camera-0 batch carries of it, and the per-plane route cannot fit it."""
    from ov_plane_amd.synth import make_stereo_plane_scene
    from tests.test_general_features_gpu import with_camera1_only

    sc = make_stereo_plane_scene(C=8, n_planes=3, feats_per_plane=10, n_free=0, seed=72, stereo_frac=0.7, planes_in_state_frac=0.0,
                                 chi2_mult=99999.0, px_noise=0.25, err_scale=0.05)
    p1 = np.where(sc.plane_id == 1)[0]
    st1 = p1[sc.cam_idx[p1].max(axis=1) == 1]
    assert len(st1) == 7 and len(p1) == 10
    # camera 1 as well tracked and calibrated as camera 0 is in this scene (the generator draws camera 1's pixels at the sigma the
    # filter assumes, and at residuals of the Cauchy scale optimize_plane does not converge within its 12 iterations): its
    # measurements again, 0.25 px around the projection through its calibration estimate
    from ov_plane_amd.synth import project_all, quat_2_rot, radtan_undistort

    rng = np.random.default_rng(5)
    c1, tr = sc.cam1, sc.truth
    uv1, _ = project_all(tr["p_f"], tr["R"], tr["p"], quat_2_rot(c1["calib_q"]), np.asarray(c1["calib_p"]), np.asarray(c1["intr"]), False)
    uv, uvn = sc.uv.copy(), sc.uv_norm.copy()
    for f in range(sc.F):
        for k in range(int(sc.n_meas[f])):
            if sc.cam_idx[f, k] == 1:
                uv[f, k] = (uv1[f, sc.clone_idx[f, k]] + 0.25 * rng.standard_normal(2)).astype(np.float32)
                xn, yn = radtan_undistort(np.float64(uv[f, k, 0]), np.float64(uv[f, k, 1]), c1["intr"])
                uvn[f, k] = (np.float32(xn), np.float32(yn))
    sc = type(sc)(sc)
    sc.update(uv=uv, uv_norm=uvn)
    return with_camera1_only(sc, st1)


def _stereo_fit_reference(sc, oracle):
    """update/UpdaterMSCKF.cpp:120-764 composed from the reference pieces, every camera taking part: triangulation over every
    camera, per plane (in id order) RANSAC fit + joint refinement of the triangulated on-plane features (the chain of
    tests/plane_frontend_ref.py), the plane loop on the kept features (tests/general_planes_ref.py), the point update on the rest
    at the state the loop left (oracle/np_ref.py).  Returns (state, cp, P, used, n_fitted, kept_by_plane)."""
    from oracle import np_ref
    from ov_plane_amd.synth import Scene, quat_2_rot
    from tests import general_planes_ref as GR
    from tests.test_general_features_gpu import chi2_table, triangulate_general_np

    tri = [triangulate_general_np(sc, f) for f in range(sc.F)]
    ok = np.array([t[0] for t in tri])
    sc2 = Scene(sc)
    sc2.update(p_FinG=np.where(ok[:, None], np.array([t[1] for t in tri]), sc.p_FinG), plane_id=sc.plane_id.copy(), cp=sc.cp.copy(),
               cp_fej=sc.cp_fej.copy(), sigma_px_norm=sc.opts["sigma_px"] / sc.intr[0], sigma_c=sc.opts["sigma_c"],
               R_GtoI=quat_2_rot(sc.clone_q[-1]), p_IinG=sc.clone_p[-1])
    poses = R.pose_table(sc)
    kept_by_plane = {}
    for k in range(sc.cp.shape[0]):
        feats = np.where((sc.plane_id == k + 1) & ok)[0]
        keep = None
        if sc.plane_in_state[k]:
            res = oracle.optimize_plane(R.plane_problem(sc2, feats, poses, sc.cp[k], True))
            if res["ok"]:
                keep, sel = feats[res["kept"]], feats
        elif len(feats) >= 4:
            fitr = oracle.plane_fitting(sc2["p_FinG"][feats], FIT["min_feat"], FIT["max_cond"], FIT["variant"])
            if fitr["ok"]:
                sel = feats[fitr["inlier"]]
                res = oracle.optimize_plane(R.plane_problem(sc2, sel, poses, -fitr["abcd"][:3] * fitr["abcd"][3], False))
                if res["ok"] and res["n_kept"] >= 4:
                    keep = sel[res["kept"]]
                    sc2["cp"][k] = sc2["cp_fej"][k] = res["cp"]
        sc2["plane_id"][np.where(sc.plane_id == k + 1)[0] if keep is None else np.setdiff1d(np.where(sc.plane_id == k + 1)[0], keep)] = 0
        if keep is not None:
            sc2["p_FinG"][keep] = res["p_FinG"][res["kept"]]
            kept_by_plane[k] = keep
    good = np.where(ok)[0]
    loop = GR.plane_loop_ref(sc2, feats=[f for f in good if sc2["plane_id"][f] > 0], use_qr=True)
    rest = np.array([f for f in good if not loop["used"][f]], dtype=int)
    st, cp, P = loop["state"], loop["cp"], loop["P"]
    if len(rest):
        view = Scene(sc2)
        view.update(P=P, clone_q=st["clone_q"], clone_p=st["clone_p"], calib_q=st["calib_q"], calib_p=st["calib_p"], intr=st["intr"],
                    cam1=dict(sc.cam1, **st["cam1"]), cp=cp, F=len(rest), plane_id=np.zeros(len(rest), dtype=sc.plane_id.dtype))
        for key in ("uv", "uv_norm", "clone_idx", "cam_idx", "n_meas", "p_FinG"):
            view[key] = sc2[key][rest]
        pt = np_ref.msckf_point_update_dense(view, chi2_table())
        st, cp = GR.apply_dx_state(sc, st, cp, pt["dx"])
        P = pt["P"]
    return st, cp, P, loop["used"], len(kept_by_plane), kept_by_plane


def test_host_updater_msckf_fits_planes_over_every_camera(hiplib, oracle):
    """UpdaterMSCKF::update with StateOptions::gpu_fused_plane_fit on a stereo scene: the same accepted planes, consumed features
    and state as the composition of the reference pieces, within TOL_DX / TOL_P of tests/test_gpu_parity.py.  Every plane has
    three features the camera-0 batch carries (plane 1's other seven are seen by camera 1 only): the planes are fitted, and their
    features consumed, only because the stereo and camera-1 tracks take part; with the option off none is."""
    from ov_plane_amd.build import build_host

    build_host()
    from ov_plane_amd import hostlib
    from tests import general_planes_ref as GR

    TOL_DX, TOL_P = 1e-6, 1e-4  # tests/test_gpu_parity.py
    sc = _stereo_fit_scene()
    p1 = sc.plane_id == 1
    st, cp, P, used, n_fit, kept = _stereo_fit_reference(sc, oracle)
    assert n_fit == 3 and used[p1].sum() >= 6 and (sc.cam_idx[used & p1].max(axis=1) == 1).sum() >= 4
    on = hostlib.run_msckf_update(sc, triangulate=True, fit_planes=FIT, general_features=True, general_planes=True,
                                  fused_plane_fit=True)
    err = max(np.abs(on["clone_p"] - st["clone_p"]).max(), np.abs(on["clone_q"] - st["clone_q"]).max(),
              np.abs(on["calib_p"] - st["calib_p"]).max(), np.abs(on["intr"] - st["intr"]).max(),
              np.abs(on["cam1"]["intr"] - st["cam1"]["intr"]).max(), np.abs(on["cam1"]["calib_p"] - st["cam1"]["calib_p"]).max())
    print("host route, stereo: used", int(on["used"].sum()), "state err", err, "relP", GR.relP(on["P"], P))
    assert (on["used"] == used).all()
    assert err < TOL_DX and GR.relP(on["P"], P) < TOL_P
    # without the fused fit no plane of this scene has enough to be fitted from: each has three tracks the camera-0 batch carries
    off = hostlib.run_msckf_update(sc, triangulate=True, fit_planes=FIT, general_features=True, general_planes=True)
    assert not off["used"].any() and on["used"].all()
    # the fit alone (its general features then go to the point update without their plane constraint): another result
    fit_only = hostlib.run_msckf_update(sc, triangulate=True, fit_planes=FIT, general_features=True, fused_plane_fit=True)
    assert not fit_only["used"][sc.cam_idx.max(axis=1) == 1].any()
