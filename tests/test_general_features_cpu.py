"""CPU checks of the general-feature boundary (ovp_cameras_upload / ovp_msckf_general_features / ovp_triangulate_general): the
library exports the entries, the ctypes structs match the header, and the host mirror's C wrapper takes the option."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "ovplane_hip.h"
int main(void) {
  printf("%d %d %d\n", OVP_MAX_CAMERAS, OVP_GEN_MAX_MEAS, OVP_MAX_MEAS);
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(ovp_camera_tables), offsetof(ovp_camera_tables, calib_q),
         offsetof(ovp_camera_tables, calib_p), offsetof(ovp_camera_tables, calib_id), offsetof(ovp_camera_tables, intrinsics),
         offsetof(ovp_camera_tables, intr_id), offsetof(ovp_camera_tables, fisheye));
  printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(ovp_general_batch), offsetof(ovp_general_batch, n_feats),
         offsetof(ovp_general_batch, max_meas), offsetof(ovp_general_batch, uv), offsetof(ovp_general_batch, clone_idx),
         offsetof(ovp_general_batch, cam_idx), offsetof(ovp_general_batch, n_meas), offsetof(ovp_general_batch, p_FinG));
  return 0;
}
"""


def test_library_exports_the_general_feature_entries(hiplib):
    L = hiplib.lib()
    for name in ("ovp_cameras_upload", "ovp_msckf_general_features", "ovp_triangulate_general"):
        assert hasattr(L, name), name
        assert name in hiplib.EXPORTS


def test_general_structs_match_header(hiplib, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(_LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)]).decode().split("\n")
    consts = [int(v) for v in lines[0].split()]
    assert consts == [hiplib.OVP_MAX_CAMERAS, hiplib.OVP_GEN_MAX_MEAS, hiplib.OVP_MAX_MEAS]
    cam = [int(v) for v in lines[1].split()]
    T = hiplib.CameraTables
    assert cam == [C.sizeof(T)] + [getattr(T, f).offset for f in ("calib_q", "calib_p", "calib_id", "intrinsics", "intr_id", "fisheye")]
    gb = [int(v) for v in lines[2].split()]
    G = hiplib.GeneralBatch
    assert gb == [C.sizeof(G)] + [getattr(G, f).offset for f in ("n_feats", "max_meas", "uv", "clone_idx", "cam_idx", "n_meas", "p_FinG")]


def test_host_wrapper_takes_the_general_features_option():
    from ov_plane_amd.build import build_host

    build_host()
    from ov_plane_amd import hostlib

    assert hostlib.carries_option("general_features")
    assert hostlib.RunOpts().general_features == 0 and hostlib.RunOpts(general_features=True).general_features == 1
    import inspect

    assert inspect.signature(hostlib.run_msckf_update).parameters["general_features"].default is False


def test_general_entries_refuse_without_a_context(hiplib):
    L = hiplib.lib()
    assert L.ovp_cameras_upload(None, 1, None) == hiplib.OVP_E_ARG
    assert L.ovp_msckf_general_features(None, None, None, None, None) == hiplib.OVP_E_ARG
    assert L.ovp_triangulate_general(None, None, None, None, None, None) == hiplib.OVP_E_ARG
