"""One call of every entry of the host mirror's harness (ov_plane_amd/hostlib.py) per option, on the small scenes the mirror tests
already use for that option.  cases() yields (name, thunk); a thunk returns the dict of arrays the call gave.  Shared by
tools/harness_digest.py (bits against another build) and tests/test_host_harness_gpu.py (bits against another call order)."""
import ctypes as C

import numpy as np

from ov_plane_amd.synth import (PROP_OPTS, make_imu_scenario, make_scene, make_slam_scene, make_stereo_plane_scene, make_stereo_slam_scene,
                                slam_rows_on_planes)

FIT = dict(min_feat=5, max_cond=200.0, variant=0)  # tests/test_plane_frontend_gpu.py

_SCENES = {}


def scene(name):
    """the scenes by name, each made once and never written to"""
    if name not in _SCENES:
        from tests import dinit_planes_ref, test_general_slam_gpu, test_plane_frontend_gpu

        make = dict(
            # tests/test_gpu_parity.py::test_host_cpp_mirror_updater_msckf
            mono=lambda: make_scene(C=8, F=90, seed=73, n_planes=3, feats_per_plane=15, chi2_mult=99999.0, ragged=True),
            fisheye=lambda: make_scene(C=9, F=80, seed=74, chi2_mult=1.0, fisheye=True),
            # tests/test_plane_frontend_gpu.py: triangulate + fit_planes, mono and stereo
            fit=lambda: make_scene(C=10, F=150, seed=72, n_planes=4, feats_per_plane=20, chi2_mult=99999.0, px_noise=0.25, err_scale=0.05),
            fit_slam=lambda: make_scene(C=10, F=150, seed=72, n_planes=4, feats_per_plane=20, n_slam=2, chi2_mult=99999.0,
                                        px_noise=0.25, err_scale=0.05),
            stereo_fit=test_plane_frontend_gpu._stereo_fit_scene,
            small=lambda: make_scene(C=6, F=4, seed=91),
            slam=lambda: make_slam_scene(C=8, n_slam=8, seed=6, outliers=1),
            candidates=lambda: make_scene(C=8, F=6, seed=6, ragged=True, chi2_mult=0.6),
            plane_init=lambda: make_scene(C=11, F=90, seed=33, n_planes=2, feats_per_plane=30, planes_in_state_frac=0.0, chi2_mult=1.0),
            plane_init_fit=lambda: make_scene(C=10, F=16, seed=34, n_planes=2, feats_per_plane=8, planes_in_state_frac=0.0,
                                              chi2_mult=1.0, px_noise=0.25, err_scale=0.05),
            # tests/test_general_slam_gpu.py
            stereo_slam=lambda: make_stereo_slam_scene(C=11, n_slam=12, seed=4, n_planes=2, outliers=1, wrong_plane=2, cam1_only=1),
            stereo_candidates=lambda: test_general_slam_gpu.stereo_candidates(C=12, F=8, seed=7, cam1_only=(3,)),
            # tests/test_dinit_planes_gpu.py
            dinit_mono=dinit_planes_ref.mono_scene, dinit_stereo=dinit_planes_ref.stereo_scene,
            maintenance=_maintenance_scene, anchors=lambda: make_scene(C=6, F=4, seed=5, n_slam=2, do_fej=True),
            jacobian=lambda: make_scene(C=7, F=4, seed=5, do_fej=True, ragged=True),
            files=lambda: make_scene(C=5, F=4, seed=9),
            # tests/test_plane_init_general_gpu.py: C = 34, the smallest window with tracks above the batch's 32 views; camera-1 views
            long_tracks=lambda: make_scene(C=34, F=4 + 2 * 8, seed=3, ragged=True, min_meas=28, n_planes=2, feats_per_plane=8, chi2_mult=1.0),
            stereo_plane=lambda: make_stereo_plane_scene(C=8, n_planes=2, feats_per_plane=10, planes_in_state_frac=0.0),
        )
        _SCENES[name] = make[name]()
    return _SCENES[name]


def _maintenance_scene():  # tests/test_gpu_parity.py: state maintenance with two nearly equal planes
    sc = make_slam_scene(C=6, n_slam=5, seed=8, n_planes=4)
    i1, i2 = int(sc.plane_state_id[0]), int(sc.plane_state_id[1])
    P = sc.P.copy()
    P[i2:i2 + 3, :] = P[i1:i1 + 3, :]
    P[:, i2:i2 + 3] = P[:, i1:i1 + 3]
    P[i2:i2 + 3, i2:i2 + 3] = P[i1:i1 + 3, i1:i1 + 3] + 1e-6 * np.eye(3)
    sc["P"] = P
    sc.cp[1] = sc.cp[0] + np.array([4e-4, -3e-4, 2e-4])
    return sc


def flat(out):
    """a result dict with its nested dicts (cam1 of run_msckf_update) spread out, every value an array"""
    res = {}
    for k, v in out.items():
        if isinstance(v, dict):
            res.update({k + "." + kk: np.asarray(vv) for kk, vv in v.items()})
        else:
            res[k] = np.asarray(v)
    return res


def _initialize(H):
    rng = np.random.default_rng(7)
    sc = scene("small")
    order = [(int(sc.ids["clones"][1]), 6), (int(sc.ids["calib"]), 6), (int(sc.ids["clones"][4]), 6)]
    rows, cols, k, r_iso = 30, 18, 3, 2.0
    H_R, H_L = rng.standard_normal((rows, cols)) * 20.0, rng.standard_normal((rows, k)) * 5.0
    res = rng.standard_normal(rows) * np.sqrt(r_iso)
    return H.run_initialize(sc, order, H_R, H_L, res, r_iso, 1.0, np.array([1.0, -2.0, 3.0]))


def _imu(seed, **kw):
    x, imu, _, _ = make_imu_scenario(seed, t_state=100.0, t_off=0.004, **kw)
    return x, imu


def _zupt(H):
    x, imu = _imu(5, stationary=True, n_cam=2)
    rng = np.random.default_rng(3)
    uv0 = rng.uniform(50, 700, (30, 2)).astype(np.float32)
    uv1 = (uv0 + 6.0 * np.array([0.6, 0.8])).astype(np.float32)
    return H.run_zupt(scene("small"), x, imu, 100.0, [100.1, 100.2], 0.004, dict(PROP_OPTS), uv0=uv0, uv1=uv1)


def _propagate(H):
    x, imu = _imu(7, dt_cam=0.1)
    return H.run_propagate(scene("small"), x, imu, 100.0, 100.1, 0.004, dict(PROP_OPTS))


def _change_anchors(H):
    from ov_plane_amd.synth import quat_2_rot

    sc = scene("anchors")
    p_A = quat_2_rot(sc.calib_q) @ quat_2_rot(sc.clone_q[0]) @ (sc.p_FinG[0] - sc.clone_p[0]) + sc.calib_p
    return H.run_change_anchors(sc, 2, p_A, p_A + np.array([2e-3, -1e-3, 3e-3]))


def _jacobian(H):
    sc, out = scene("jacobian"), {}
    for rep in (0, 2, 5):
        H_f, H_x, r, order = H.feature_jacobian_rep(sc, 1, rep, int(sc.clone_idx[1, 1]))
        out.update({"H_f%d" % rep: H_f, "H_x%d" % rep: H_x, "r%d" % rep: r, "order%d" % rep: np.array(order)})
    return out


def _state_files(H):
    sc = scene("files")
    f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    arrays = [f64(sc.clone_q), f64(sc.clone_p), f64(sc.calib_q), f64(sc.calib_p), f64(sc.intr)]
    P = np.asfortranarray(sc.P)
    out = {}
    for with_gt in (0, 1):
        est, sd, gt = (C.create_string_buffer(4096) for _ in range(3))
        rc = H.lib().ovph_format_state_files(C.c_int(sc.C), *(p(a) for a in arrays), C.c_int(sc.N), p(P), C.c_double(1403715273.262142),
                                             C.c_double(0.0041234567), C.c_int(with_gt), est, sd, gt, C.c_int(4096))
        assert rc == 0
        out.update({"est%d" % with_gt: np.frombuffer(est.value, dtype=np.uint8), "sd%d" % with_gt: np.frombuffer(sd.value, dtype=np.uint8),
                    "gt%d" % with_gt: np.frombuffer(gt.value, dtype=np.uint8)})
    return out


def _timing_file(H):
    v = np.arange(1.0, 10.0) * 0.0123
    buf = C.create_string_buffer(1024)
    n = H.lib().ovph_format_timing(1, 25, v.ctypes.data_as(C.c_void_p), buf, 1024)
    assert n > 0
    return dict(csv=np.frombuffer(buf.value, dtype=np.uint8))


def _simulator():
    from ov_plane_amd.sim import Simulator, synthetic_trajectory

    return Simulator(synthetic_trajectory(duration=12.0), num_pts=60, num_pts_plane=120)


def _sequence(H, planes):
    from ov_plane_amd import closed_loop

    r = closed_loop.run(_simulator(), n_frames=4, C=6, planes=planes, plane_min_feat=6)
    return dict(r["final"], kept_per_frame=r["kept_per_frame"])


def _session(H):
    from ov_plane_amd import closed_loop

    r = closed_loop.run_session(_simulator(), n_frames=10, C=8, planes=2, max_slam=5)
    return {k: r[k] for k in ("traj", "counts")}


def _slam_update_dense(H):
    H.set_slam_force_dense(True)
    try:
        return H.run_updater(scene("slam"), "slam_update")
    finally:
        H.set_slam_force_dense(False)


def cases(H):
    """H: ov_plane_amd.hostlib (of the checkout under test)"""
    S = scene
    yield "msckf_update", lambda: H.run_msckf_update(S("mono"))
    yield "msckf_update/fisheye", lambda: H.run_msckf_update(S("fisheye"))
    yield "msckf_update/triangulate", lambda: H.run_msckf_update(S("mono"), triangulate=True)
    yield "msckf_update/triangulate+fit_planes", lambda: H.run_msckf_update(S("fit"), triangulate=True, fit_planes=FIT)
    yield "msckf_update/fused_plane_fit", lambda: H.run_msckf_update(S("fit"), triangulate=True, fit_planes=FIT, fused_plane_fit=True)
    yield "msckf_update/stereo", lambda: H.run_msckf_update(S("stereo_fit"))
    yield "msckf_update/stereo+general", lambda: H.run_msckf_update(
        S("stereo_fit"), triangulate=True, fit_planes=FIT, general_features=True, general_planes=True, fused_plane_fit=True)
    # tracks above OVP_MAX_MEAS views: camera 0's first 32 views triangulate them and the host's dense blocks gate them, or
    # (general_features) both happen on the device
    yield "msckf_update/long_tracks", lambda: H.run_msckf_update(S("long_tracks"), triangulate=True)
    yield "msckf_update/long_tracks+general", lambda: H.run_msckf_update(S("long_tracks"), triangulate=True, general_features=True,
                                                                         general_planes=True)
    yield "initialize", lambda: _initialize(H)
    yield "updater/slam_update", lambda: H.run_updater(S("slam"), "slam_update")
    for rep in (1, 2, 3, 4):
        yield "updater/slam_update/slam_rep=%d" % rep, lambda rep=rep: H.run_updater(S("slam"), "slam_update", slam_rep=(rep, 2))
    yield "updater/slam_update/force_dense", lambda: _slam_update_dense(H)
    yield "updater/slam_update/stereo", lambda: H.run_updater(S("stereo_slam"), "slam_update")
    yield "updater/slam_update/general_slam", lambda: H.run_updater(S("stereo_slam"), "slam_update", general_slam=True)
    yield "updater/slam_delayed_init", lambda: H.run_updater(S("candidates"), "slam_delayed_init")
    for rep in (1, 2, 3, 4, 5):
        yield "updater/slam_delayed_init/feat_rep_slam=%d" % rep, lambda rep=rep: H.run_updater(S("candidates"), "slam_delayed_init",
                                                                                              feat_rep_slam=rep)
    yield "updater/slam_delayed_init/general_slam+triangulate", lambda: H.run_updater(S("stereo_candidates"), "slam_delayed_init",
                                                                                     general_slam=True, triangulate=True)
    for name in ("dinit_mono", "dinit_stereo"):
        for on in (False, True):
            yield "updater/slam_delayed_init/%s/dinit_planes=%d" % (name, on), lambda name=name, on=on: H.run_updater(
                S(name), "slam_delayed_init", state_planes=True, general_slam=name == "dinit_stereo", dinit_planes=on)
    yield "updater/plane_init", lambda: H.run_updater(S("plane_init"), "plane_init", 5.0, 1.0)
    yield "updater/plane_init/fit_planes", lambda: H.run_updater(S("plane_init_fit"), "plane_init", 5.0, 1.0, fit_planes=FIT)
    yield "updater/plane_init/fused+general", lambda: H.run_updater(S("plane_init_fit"), "plane_init", 5.0, 1.0, fit_planes=FIT,
                                                                    fused_plane_fit=True, general_plane_init=True)
    # camera-1 views on the planes: the general batch of ovp_plane_init_general is not empty, the triangulation takes its second pass
    yield "updater/plane_init/stereo+general", lambda: H.run_updater(S("stereo_plane"), "plane_init", 5.0, 1.0, general_plane_init=True)
    yield "updater/plane_init/stereo+fused+general", lambda: H.run_updater(S("stereo_plane"), "plane_init", 5.0, 1.0, fit_planes=FIT,
                                                                           fused_plane_fit=True, general_plane_init=True)
    yield "updater/msckf_fit", lambda: H.run_updater(S("fit_slam"), "msckf_fit", fit_planes=FIT, slam=slam_rows_on_planes(S("fit_slam"), 2))
    yield "propagate", lambda: _propagate(H)
    yield "zupt", lambda: _zupt(H)
    yield "state_maintenance", lambda: H.run_state_maintenance(S("maintenance"), np.array([0, 1, 0, 1, 0], dtype=np.uint8),
                                                               [(2, 1), (3, 9)], [1, 9])
    yield "change_anchors", lambda: _change_anchors(H)
    yield "feature_jacobian_rep", lambda: _jacobian(H)
    yield "format_state_files", lambda: _state_files(H)
    yield "format_timing", lambda: _timing_file(H)
    yield "sequence", lambda: _sequence(H, 0)
    yield "sequence/planes", lambda: _sequence(H, 2)
    yield "session", lambda: _session(H)
