"""CPU checks of the general SLAM boundary (ovp_slam_update_general / ovp_slam_delayed_init_general): the library exports the
entries and refuses calls without a context, the host mirror's C wrapper takes StateOptions::gpu_general_slam (off by default) and
reports its route, and synth.make_stereo_slam_scene lays out a two-camera SLAM state."""
import inspect

import numpy as np

from ov_plane_amd.synth import make_stereo_slam_scene


def test_library_exports_the_general_slam_entries(hiplib):
    L = hiplib.lib()
    for name in ("ovp_slam_update_general", "ovp_slam_delayed_init_general"):
        assert hasattr(L, name), name
        assert name in hiplib.EXPORTS
    for name in ("slam_update_general", "slam_delayed_init_general", "camera_tables_download"):
        assert callable(getattr(hiplib.Context, name))


def test_general_slam_entries_refuse_without_a_context(hiplib):
    L = hiplib.lib()
    assert L.ovp_slam_update_general(None, None, None, None, None, None, None, None) == hiplib.OVP_E_ARG
    assert L.ovp_slam_delayed_init_general(None, None, None, None, None, None, None, None, 0) == hiplib.OVP_E_ARG


def test_host_wrapper_takes_the_general_slam_option():
    from ov_plane_amd.build import build_host

    build_host()
    from ov_plane_amd import hostlib

    L = hostlib.lib()
    assert hostlib.carries_option("general_slam") and hasattr(L, "ovph_last_slam_route")
    assert hostlib.RunOpts().general_slam == 0 and hostlib.RunOpts(general_slam=True).general_slam == 1
    # a static of UpdaterSLAM: whatever the last SLAM call of this process took, any Route
    assert L.ovph_last_slam_route() in (hostlib.ROUTE_NONE, hostlib.ROUTE_DEVICE_GENERAL, hostlib.ROUTE_DEVICE_MONO,
                                        hostlib.ROUTE_DENSE_HOST, hostlib.ROUTE_HOST_LOOP, hostlib.ROUTE_DEVICE_PLANES)
    params = inspect.signature(hostlib.run_updater).parameters
    assert params["general_slam"].default is False
    assert params["triangulate"].default is False


def test_stereo_slam_scene_layout():
    sc = make_stereo_slam_scene(C=11, n_slam=12, seed=3, n_planes=3, outliers=2, wrong_plane=2, cam1_only=2)
    ids = sc.ids
    C, F = int(sc.C), int(sc.F)
    # [imu | dt | cam0 extrinsics, intrinsics | cam1 extrinsics, intrinsics | clones | landmarks | planes]
    assert (ids["calib"], ids["intr"], ids["calib1"], ids["intr1"]) == (16, 22, 30, 36)
    assert list(ids["clones"]) == [44 + 6 * i for i in range(C)]
    assert list(ids["slam"]) == [44 + 6 * C + 3 * k for k in range(F)]
    assert list(ids["planes"]) == [44 + 6 * C + 3 * F + 3 * k for k in range(3)]
    assert sc.N == 44 + 6 * C + 3 * F + 9
    assert list(sc.lm_id) == list(ids["slam"]) and list(sc.plane_state_id) == list(ids["planes"])
    assert (sc.cam1["calib_id"], sc.cam1["intr_id"]) == (30, 36)
    # P symmetric positive definite
    assert sc.P.shape == (sc.N, sc.N) and np.array_equal(sc.P, sc.P.T)
    assert np.linalg.eigvalsh(sc.P).min() > 0.0
    # measurements: at most 32 new observations per landmark; camera 1 on the stereo ones, alone on the cam1_only ones
    assert int(sc.n_meas.max()) <= 32 and sc.cam_idx.shape == sc.clone_idx.shape
    for f in range(F):
        cams = set(int(c) for c in sc.cam_idx[f, : int(sc.n_meas[f])])
        if f < sc.n_stereo - 2:
            assert cams == {0, 1}
        elif f < sc.n_stereo:
            assert cams == {1}
        else:
            assert cams == {0}
        assert (sc.clone_idx[f, : int(sc.n_meas[f])] >= 0).all()
    assert (sc.plane_id > 0).all()
