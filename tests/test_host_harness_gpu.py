"""The host mirror's harness keeps nothing between calls (csrc/host/host_capi.h): a call's result does not depend on the calls in
front of it, an error return leaves nothing behind, and per-call results (camera 1) come back in the caller's own options."""
import ctypes as C

import numpy as np
import pytest

from ov_plane_amd.synth import Scene
from tests import harness_calls as HC


@pytest.fixture(scope="module")
def hostlib(hiplib):
    from ov_plane_amd.build import build_host

    build_host()
    from ov_plane_amd import hostlib

    return hostlib


def _same_bits(a, b):
    a, b = HC.flat(a), HC.flat(b)
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


def _every_option(H):
    """run_msckf_update on a stereo scene with all its options on, then run_updater in each mode with its options on"""
    S = HC.scene
    H.run_msckf_update(S("stereo_fit"), triangulate=True, fit_planes=HC.FIT, general_features=True, general_planes=True,
                       fused_plane_fit=True)
    H.run_updater(S("stereo_slam"), "slam_update", general_slam=True)
    H.run_updater(S("slam"), "slam_update", slam_rep=(2, 2))
    H.run_updater(S("dinit_stereo"), "slam_delayed_init", state_planes=True, general_slam=True, dinit_planes=True)
    H.run_updater(S("candidates"), "slam_delayed_init", feat_rep_slam=2)
    H.run_updater(S("stereo_candidates"), "slam_delayed_init", general_slam=True, triangulate=True)
    H.run_updater(S("plane_init_fit"), "plane_init", 5.0, 1.0, fit_planes=HC.FIT, fused_plane_fit=True, general_plane_init=True)
    H.run_updater(S("fit_slam"), "msckf_fit", fit_planes=HC.FIT, slam=HC.slam_rows_on_planes(S("fit_slam"), 2))


@pytest.mark.gpu
@pytest.mark.parametrize("plain", ["msckf_update", "slam_delayed_init"])
def test_a_result_does_not_depend_on_the_calls_before_it(hostlib, plain):
    H = hostlib
    run = dict(msckf_update=lambda: H.run_msckf_update(HC.scene("mono")),
               slam_delayed_init=lambda: H.run_updater(HC.scene("candidates"), "slam_delayed_init"))[plain]
    before = run()
    _every_option(H)
    _same_bits(before, run())


def _direct_msckf_update(H, sc, ro, N):
    """ovph_run_msckf_update itself on scene sc with options ro, claiming a state of size N"""
    f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)  # noqa: E731
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    ins, outs = np.where(sc.plane_in_state)[0], np.where(~sc.plane_in_state)[0]
    a = [f64(sc.clone_q), f64(sc.clone_p), f64(sc.clone_q_fej), f64(sc.clone_p_fej), f64(sc.calib_q), f64(sc.calib_p), f64(sc.intr),
         f64(sc.cp[ins]), f64(sc.cp_fej[ins]), np.ascontiguousarray(ins + 1, dtype=np.uint64), f64(sc.cp[outs]),
         np.ascontiguousarray(outs + 1, dtype=np.uint64), np.asfortranarray(np.zeros((N, N))), np.ascontiguousarray(sc.uv, dtype=np.float32),
         i32(sc.clone_idx), i32(sc.n_meas), f64(sc.p_FinG), i32(sc.plane_id)]
    o = [np.zeros((sc.C, 4)), np.zeros((sc.C, 3)), np.zeros(4), np.zeros(3), np.zeros(8), np.zeros((max(len(ins), 1), 3)), np.zeros((N, N)),
         np.zeros(sc.F, np.uint8), np.zeros(sc.F, np.uint8), np.zeros(sc.F, np.uint8)]
    return H.lib().ovph_run_msckf_update(
        C.c_int(sc.C), *(p(x) for x in a[:7]), C.c_int(len(ins)), p(a[7]), p(a[8]), p(a[9]), C.c_int(len(outs)), p(a[10]), p(a[11]),
        C.c_int(N), p(a[12]), C.c_int(sc.F), C.c_int(int(sc.uv.shape[1])), *(p(x) for x in a[13:]), C.c_double(1.0), C.c_double(1.0),
        C.c_double(0.01), C.c_int(1), *(p(x) for x in o), C.byref(ro))


@pytest.mark.gpu
def test_an_error_return_arms_nothing(hostlib):
    H = hostlib
    before = H.run_msckf_update(HC.scene("mono"))
    sc = HC.scene("stereo_fit")
    ro = H.RunOpts(sc, HC.FIT, fisheye=1, general_features=1, general_planes=1, general_plane_init=1, fused_plane_fit=1, general_slam=1,
                   dinit_planes=1, slam_rep=2, slam_anchor=1, feat_rep_slam=3)
    ro.borrow("uv_norm", sc.uv_norm, np.float32)
    ro.borrow("p_noplane", sc.p_FinG, np.float64)
    ro.borrow("slam_plane", np.ones(sc.F), np.int32)
    # one more than the state the arrays describe: refused by the harness's own size check, before any updater runs
    assert _direct_msckf_update(H, sc, ro, int(sc.N) + 1) == -11
    _same_bits(before, H.run_msckf_update(HC.scene("mono")))


@pytest.mark.gpu
def test_camera1_comes_back_per_call(hostlib):
    H = hostlib
    sc_a = HC.scene("stereo_fit")
    sc_b = Scene(sc_a)
    sc_b["cam1"] = dict(sc_a.cam1, calib_p=np.asarray(sc_a.cam1["calib_p"]) + np.array([1e-3, -2e-3, 5e-4]))
    a = H.run_msckf_update(sc_a)
    mono = H.run_msckf_update(HC.scene("mono"))
    b = H.run_msckf_update(sc_b)
    assert "cam1" not in mono
    assert not np.array_equal(a["cam1"]["calib_p"], b["cam1"]["calib_p"])
    # each is its own call's: the same calls in the other order, a mono run in between, give the same two results
    b2 = H.run_msckf_update(sc_b)
    assert "cam1" not in H.run_msckf_update(HC.scene("mono"))
    a2 = H.run_msckf_update(sc_a)
    _same_bits(a, a2)
    _same_bits(b, b2)
