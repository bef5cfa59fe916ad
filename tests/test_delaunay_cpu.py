"""CPU tests of the device Delaunay triangulation's surroundings: the new symbols against the header, the binding and the built
library, the options struct that must not grow, the host mirror's option and session switch, and the inputs of the GPU file
(tests/delaunay_cases.py) pinned on the host: on each the library's host triangulation equals the numpy restatement's."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import delaunay_cases as dc
import plane_detect_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_in_header_binding_and_library(hiplib):
    L = hiplib.lib()
    hdr = open(os.path.join(ROOT, "include", "ovplane_hip.h")).read()
    for name in ("ovp_delaunay_device", "ovp_plane_detector_set_device_delaunay"):
        assert hasattr(L, name) and name in hiplib.EXPORTS and re.search(r"\bint %s\s*\(" % name, hdr), name
    assert L.ovp_delaunay_device.argtypes == [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    assert L.ovp_plane_detector_set_device_delaunay.argtypes == [C.c_void_p, C.c_int]
    assert callable(hiplib.delaunay_device) and callable(hiplib.PlaneDetector.set_device_delaunay)
    assert callable(hiplib.PlaneDetector.tris_info) and callable(hiplib.PlaneDetector.delaunay_ms)
    from ov_plane_amd.build import HEADERS, SOURCES

    assert "k_delaunay.hip" in SOURCES and "k_delaunay.h" in HEADERS


def test_options_struct_did_not_grow(hiplib):
    assert C.sizeof(hiplib.TrackPlaneOpts) == 96
    hdr = open(os.path.join(ROOT, "include", "ovplane_hip.h")).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} ovp_trackplane_opts;", hdr).group(1), flags=re.S)
    assert len(re.findall(r"\b(int|double)\s+(\w+)\s*;", body)) == len(hiplib.TrackPlaneOpts._fields_) == 15


def test_entry_checks_that_need_no_device(hiplib):
    """argument and capacity refusals come before anything touches the device: nothing is enqueued, a null context is an error"""
    L = hiplib.lib()
    nt = C.c_int(-1)
    xy = dc.random_pixels(8)
    tris = np.zeros((16, 3), np.int32)
    assert L.ovp_delaunay_device(None, 8, xy.ctypes.data, tris.ctypes.data, 16, C.byref(nt)) == hiplib.OVP_E_ARG
    assert L.ovp_plane_detector_set_device_delaunay(None, 1) == hiplib.OVP_E_ARG


def test_host_mirror_option_and_session_switch():
    from ov_plane_amd import closed_loop, hostlib
    from ov_plane_amd.build import build_host

    lib = C.CDLL(build_host())
    assert hasattr(lib, "ovph_session_set_device_delaunay")
    assert callable(hostlib.Session.set_device_delaunay)
    assert inspect.signature(hostlib.Session.set_device_delaunay).parameters["on"].default is True
    assert inspect.signature(closed_loop.run_session).parameters["device_delaunay"].default is False
    hdr = open(os.path.join(ROOT, "ov_plane_amd", "csrc", "host", "ov_plane_host.h")).read()
    assert "bool gpu_device_delaunay = false;" in hdr
    tp = open(os.path.join(ROOT, "ov_plane_amd", "csrc", "host", "ov_plane_trackplane.h")).read()
    assert "set_device_delaunay(bool on)" in tp and "_device_delaunay = false" in tp


@pytest.mark.parametrize("g", dc.GRID_G)
def test_integer_grid_triangle_count(hiplib, g):
    """exactly cocircular squares: two triangles each, 2 (g - 1)^2"""
    t = hiplib.delaunay(dc.grid(g))
    assert len(t) == 2 * (g - 1) ** 2 == {4: 18, 8: 98, 32: 1922}[g]


CASES = dc.all_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_is_pinned_on_the_host(hiplib, name):
    """the GPU file compares the device against ovp_delaunay; here ovp_delaunay itself is held to the numpy restatement"""
    xy = CASES[name]
    assert xy.dtype == np.float32 and xy.shape == (len(xy), 2)
    got, want = hiplib.delaunay(xy), ref.delaunay(xy)
    assert got.shape == want.shape and np.array_equal(got, want), name
    if len(got):
        assert got.min() >= 0 and got.max() < len(xy) and (got[:, 0] < got[:, 1]).all() and (got[:, 0] < got[:, 2]).all()
        assert (got[1:] != got[:-1]).any(axis=1).all() and (np.lexsort(got.T[::-1]) == np.arange(len(got))).all()  # distinct, sorted


def test_fixture_properties():
    """what each input is there for"""
    assert set(dc.RANDOM_N) == {3, 4, 5, 48, 257, 1024} and dc.GRID_G == (4, 8, 32) and dc.NEAR_G == (16, 32)
    d = dc.every_third_a_duplicate()
    assert len(d) == 1024 and (d[3::3] == d[0]).all()
    c = dc.collinear_but_the_last()
    assert len(c) == 1024 and (c[:-1, 1] == 0).all() and c[-1, 1] != 0
    x = dc.descending_x()
    assert len(x) == 1024 and (np.diff(x[:, 0]) < 0).all() and np.array_equal(x[:, 1], (np.arange(1024) ** 2) % 997)
    e = dc.ellipse().astype(np.float64)
    assert len(e) == 1024 and np.abs(((e[:, 0] - 400) / 300) ** 2 + ((e[:, 1] - 300) / 200) ** 2 - 1).max() < 1e-6
    n = dc.near_grid(32)
    assert n.dtype == np.float32 and n[33, 0] == np.float32(123.456) + np.float32(0.1) * np.float32(1)
