"""CPU checks of the host mirror's test harness (csrc/host/host_capi.h / host_capi.cpp, ov_plane_amd/hostlib.py): the ctypes
mirror of ovph_run_opts has the library's layout, the library's defaults are the documented ones, a struct of another size is
refused before anything is built, and the entries that armed process-wide "next call" state are gone."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what used to arm file-scope state for the next ovph_run_*, and what read its results back
REMOVED = ("ovph_set_uv_norm", "ovph_set_fisheye", "ovph_set_slam_rep", "ovph_set_feat_rep_slam", "ovph_set_slam_planes",
           "ovph_set_plane_fit", "ovph_set_second_camera", "ovph_set_general_features", "ovph_set_general_planes",
           "ovph_set_general_plane_init", "ovph_set_fused_plane_fit", "ovph_set_general_slam", "ovph_set_dinit_planes",
           "ovph_set_p_noplane", "ovph_set_shard_comm", "ovph_set_sequence_trace", "ovph_set_sequence_planes",
           "ovph_last_second_camera", "ovph_last_shard")


@pytest.fixture(scope="module")
def hostlib():
    from ov_plane_amd.build import build_host

    build_host()
    from ov_plane_amd import hostlib

    hostlib.lib()
    return hostlib


def test_run_opts_mirror_has_the_library_layout(hostlib):
    size, offsets = hostlib.run_opts_layout()
    assert size == C.sizeof(hostlib.RunOpts)
    assert list(offsets) == [f[0] for f in hostlib.RunOpts._fields_]
    for name, off in offsets.items():
        assert getattr(hostlib.RunOpts, name).offset == off, name
    # the header declares exactly these members, in this order
    hdr = open(os.path.join(ROOT, "ov_plane_amd", "csrc", "host", "host_capi.h")).read()
    body = re.search(r"typedef struct ovph_run_opts \{(.*?)\} ovph_run_opts;", hdr, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    declared = []
    for stmt in body.split(";"):
        declared += [re.sub(r"\[\d+\]", "", d).strip(" *\n") .split()[-1].lstrip("*") for d in stmt.split(",") if d.strip()]
    assert declared == list(offsets)


def test_run_opts_defaults(hostlib):
    o = hostlib.RunOpts.__new__(hostlib.RunOpts)
    C.memset(C.byref(o), 0xFF, C.sizeof(o))
    hostlib.lib().ovph_run_opts_defaults(C.byref(o))
    nonzero = dict(size=C.sizeof(hostlib.RunOpts), fit_min_feat=20, fit_max_cond=100.0, comm_world=1, seq_plane_min_feat=20,
                   seq_sigma_c=0.01)
    for name, _ in hostlib.RunOpts._fields_:
        v = getattr(o, name)
        if name in nonzero:
            assert v == nonzero[name], name
        elif name in ("last_shard", "last_cam1"):
            assert not any(v), name
        else:
            assert not v, name
    # the Python object starts from the same values
    p = hostlib.RunOpts()
    assert bytes(p) == bytes(o)


def test_a_struct_of_another_size_is_refused(hostlib):
    L = hostlib.lib()
    assert hostlib.OVPH_E_OPTS == -40
    for size in (0, C.sizeof(hostlib.RunOpts) - 8, C.sizeof(hostlib.RunOpts) + 8):
        o = hostlib.RunOpts()
        o.size = size
        # C = 0, no arrays: nothing of this may be touched, no State (no device) is made
        rc = L.ovph_run_initialize(0, None, None, 0, None, 0, None, 0, 0, None, 0, None, None, C.c_double(0), C.c_double(0), None,
                                   None, None, None, None, None, None, C.byref(o))
        assert rc == hostlib.OVPH_E_OPTS, size


def test_no_setter_of_next_call_state_is_exported(hostlib):
    L = hostlib.lib()
    for name in REMOVED:
        assert not hasattr(L, name), name
    # these wrap statics of UpdaterSLAM itself and stay
    assert hasattr(L, "ovph_set_slam_force_dense") and hasattr(L, "ovph_last_slam_route")
    src = open(os.path.join(ROOT, "ov_plane_amd", "csrc", "host", "host_capi.cpp")).read()
    assert not re.search(r"^static .*g_", src, re.M)
    assert set(re.findall(r"\bovph_set_\w+", src)) == {"ovph_set_slam_force_dense"}
