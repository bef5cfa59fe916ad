"""CPU checks of ovp_slam_delayed_init_planes (delayed initialisation of candidates that lie on planes of the state, in the device
loop): the library exports the entry and the ctypes struct matches the header; synth.make_dinit_plane_scene is deterministic and
lays its candidates on planes of the state; and the numpy sequential reference (tests/dinit_planes_ref.py) yields, on the scenes
the GPU parity tests use, all three statuses far enough from every threshold that rounding cannot flip a decision."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from ov_plane_amd.synth import make_dinit_plane_scene
from tests.dinit_planes_ref import delayed_init_planes_reference, margins, mono_scene, stereo_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "ovplane_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(ovp_dinit_planes), offsetof(ovp_dinit_planes, n_planes),
         offsetof(ovp_dinit_planes, plane_state_id), offsetof(ovp_dinit_planes, cp), offsetof(ovp_dinit_planes, cp_fej),
         offsetof(ovp_dinit_planes, plane_of_cand), offsetof(ovp_dinit_planes, p_FinG_noplane));
  return 0;
}
"""


def test_library_exports_the_plane_delayed_init_entry(hiplib, tmp_path):
    L = hiplib.lib()
    assert hasattr(L, "ovp_slam_delayed_init_planes")
    assert "ovp_slam_delayed_init_planes" in hiplib.EXPORTS
    for name in ("slam_delayed_init_planes", "plane_table_download"):
        assert callable(getattr(hiplib.Context, name))
    assert L.ovp_slam_delayed_init_planes(None, None, None, None, None, None, None, None, None, 0) == hiplib.OVP_E_ARG
    src = tmp_path / "layout.c"
    src.write_text(_LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    T = hiplib.DinitPlanes
    assert got == [C.sizeof(T)] + [getattr(T, f).offset for f in ("n_planes", "plane_state_id", "cp", "cp_fej", "plane_of_cand",
                                                                 "p_FinG_noplane")]


@pytest.mark.parametrize("stereo", [False, True], ids=["mono", "stereo"])
def test_dinit_plane_scene_is_deterministic_and_on_state_planes(stereo):
    kw = dict(C=11, F=14, n_planes=3, wrong_plane=2, outliers=1, seed=5, stereo=stereo)
    a, b = make_dinit_plane_scene(**kw), make_dinit_plane_scene(**kw)
    for k in ("P", "uv", "clone_idx", "n_meas", "p_FinG", "p_FinG_noplane", "plane_id", "cp", "cp_fej", "plane_state_id", "clone_q"):
        assert np.array_equal(a[k], b[k]), k
    # the candidates are NOT in the state, every plane IS; several candidates per plane
    assert len(a.ids["slam"]) == 0 and len(a.ids["planes"]) == 3
    assert a.plane_in_state.all() and list(a.plane_state_id) == list(a.ids["planes"])
    assert a.N == int(a.ids["planes"][-1]) + 3 and a.P.shape == (a.N, a.N)
    assert (a.plane_id >= 1).all() and (a.plane_id <= 3).all()
    assert min(int((a.plane_id == k).sum()) for k in (1, 2, 3)) >= 3
    assert np.array_equal(a.P, a.P.T) and np.linalg.eigvalsh(a.P).min() > 0.0
    # truth: all but the first wrong_plane candidates lie on their plane, those do not
    n, d = a.truth["cp"] / np.linalg.norm(a.truth["cp"], axis=1, keepdims=True), np.linalg.norm(a.truth["cp"], axis=1)
    dist = np.abs(np.einsum("fk,fk->f", n[a.plane_id - 1], a.truth["p_f"]) - d[a.plane_id - 1])
    assert dist[2:].max() < 1e-9 and dist[:2].min() > 0.05
    if stereo:
        assert a.uv.shape[1] == 22 and (a.cam_idx == 1).any() and a.ids["planes"][0] == 44 + 6 * 11
    else:
        assert "cam_idx" not in a and a.ids["planes"][0] == 30 + 6 * 11


@pytest.mark.parametrize("do_fej", [True, False], ids=["fej", "nofej"])
@pytest.mark.parametrize("make", [mono_scene, stereo_scene], ids=["mono", "stereo"])
def test_reference_decides_all_three_ways_away_from_the_thresholds(make, do_fej):
    """The condition on the INPUTS of the GPU parity tests, checked with the reference alone: at least 4 candidates accepted with
    their plane rows on a plane an earlier accepted candidate already moved, at least 2 accepted by the fallback, at least 1
    rejected, and no deciding chi2 (of either attempt) within 1 % of its threshold."""
    sc = make(do_fej=do_fej)
    assert sc.C == 11 and sc.F >= 12 and len(set(int(k) for k in sc.plane_id)) >= 2
    assert sc.opts["do_calib_pose"] and sc.opts["do_calib_intr"]
    ref = delayed_init_planes_reference(sc)
    st = ref["status"]
    assert int(((st == 1) & ref["moved"]).sum()) >= 4, st
    assert int((st == 2).sum()) >= 2 and int((st == 0).sum()) >= 1, st
    assert margins(ref).min() > 0.01, margins(ref).min()
    # the planes matter: without them the fallback candidates are plain acceptances and the corrections differ
    free = delayed_init_planes_reference(sc, use_planes=False)
    assert (free["status"] <= 1).all() and np.array_equal(free["status"] > 0, st > 0)
    l = int(np.where(st == 1)[0][0])
    assert np.abs(free["dx"][l] - ref["dx"][l]).max() > 1e-4
    if make is stereo_scene:
        cams = [set(int(c) for c in sc.cam_idx[f, : int(sc.n_meas[f])]) for f in range(sc.F)]
        assert {1} in cams and {0, 1} in cams and {0} in cams


def test_host_wrapper_takes_the_plane_delayed_init_option():
    import inspect

    from ov_plane_amd.build import build_host

    build_host()
    from ov_plane_amd import hostlib

    assert hostlib.carries_option("dinit_planes") and hostlib.carries_option("p_noplane")
    assert hostlib.RunOpts().dinit_planes == 0 and not hostlib.RunOpts().p_noplane
    assert hostlib.ROUTE_DEVICE_PLANES == 5
    assert (hostlib.ROUTE_NONE, hostlib.ROUTE_DEVICE_GENERAL, hostlib.ROUTE_DEVICE_MONO, hostlib.ROUTE_DENSE_HOST,
            hostlib.ROUTE_HOST_LOOP) == (0, 1, 2, 3, 4)
    params = inspect.signature(hostlib.run_updater).parameters
    assert params["dinit_planes"].default is False and params["state_planes"].default is False
