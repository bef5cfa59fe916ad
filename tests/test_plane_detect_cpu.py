"""CPU tests of the plane detector: the numpy restatement (tests/plane_detect_ref.py) on a small two-wall scene, the library's
host Delaunay triangulation, and the new symbols and the options struct against the header."""
import ctypes as C
import os
import re

import numpy as np

import plane_detect_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_finds_the_two_walls_and_no_clutter():
    """Two perpendicular walls (ids 100-119 on x = 3, 120-139 on y = 3) and eight points off them (140-147), eight frames."""
    res, r = ref.run_reference(ref.two_wall_scene(2))
    for k in range(3):  # below feat_init_min_obs nothing has a position, so nothing is triangulated or matched
        assert not res[k]["has"].any() and res[k]["map"] == {}
    expected = {100: 1, 101: 1, 103: 1, 106: 1, 107: 1, 112: 1, 113: 1, 114: 1, 115: 1, 117: 1, 118: 1, 119: 1, 122: 2, 125: 2,
                130: 2, 131: 2, 133: 2, 134: 2, 135: 2, 137: 2, 138: 2, 139: 2}
    assert res[-1]["map"] == expected
    for m in (x["map"] for x in res):
        assert all((f < 120 and p == 1) or (120 <= f < 140 and p == 2) for f, p in m.items())
    # the maps only hold planes of more than three active features
    for x in res:
        cnt = np.unique(list(x["map"].values()), return_counts=True)[1]
        assert (cnt > 3).all()


def _circumcircle_empty(xy, tris):
    xy = xy.astype(np.float64)
    for t in tris:
        a, b, c = xy[t]
        d = 2 * (a[0] * (b[1] - c[1]) + b[0] * (c[1] - a[1]) + c[0] * (a[1] - b[1]))
        ux = ((a @ a) * (b[1] - c[1]) + (b @ b) * (c[1] - a[1]) + (c @ c) * (a[1] - b[1])) / d
        uy = ((a @ a) * (c[0] - b[0]) + (b @ b) * (a[0] - c[0]) + (c @ c) * (b[0] - a[0])) / d
        r = np.hypot(a[0] - ux, a[1] - uy)
        dist = np.hypot(xy[:, 0] - ux, xy[:, 1] - uy)
        dist[t] = np.inf
        if not (dist > r * (1 + 1e-12)).all():
            return False
    return True


def _hull_count(xy):
    xy = xy.astype(np.float64)
    n, h = len(xy), 0
    for i in range(n):  # a hull vertex has a line through it with every other point on one side
        ang = np.sort(np.arctan2(*(np.delete(xy, i, 0) - xy[i]).T[::-1]))
        gaps = np.diff(np.concatenate([ang, [ang[0] + 2 * np.pi]]))
        h += gaps.max() > np.pi
    return h


def test_host_delaunay_on_random_pixels(hiplib):
    rng = np.random.default_rng(48)
    xy = np.stack([rng.uniform(0, 752, 48), rng.uniform(0, 480, 48)], 1).astype(np.float32)
    tris = hiplib.delaunay(xy)
    assert tris.min() >= 0 and tris.max() < 48 and len({tuple(sorted(t)) for t in tris}) == len(tris)
    assert _circumcircle_empty(xy, tris)
    assert len(tris) == 2 * 48 - 2 - _hull_count(xy)
    assert np.array_equal(tris, ref.delaunay(xy))  # the restatement's own triangulation, same canonical order
    try:
        from scipy.spatial import Delaunay
    except ImportError:
        return
    assert np.array_equal(tris, ref.canonical(Delaunay(xy.astype(np.float64)).simplices, xy.astype(np.float64)))


def test_delaunay_degenerate_inputs_stay_in_range(hiplib):
    assert len(hiplib.delaunay(np.zeros((2, 2)))) == 0
    assert len(hiplib.delaunay(np.array([[0, 0], [1, 1], [2, 2], [3, 3]], dtype=np.float32))) == 0
    xy = np.array([[0, 0], [10, 0], [0, 10], [10, 0], [5, 5], [10, 10]], dtype=np.float32)  # a duplicate, a point on an edge
    t = hiplib.delaunay(xy)
    assert t.min() >= 0 and t.max() < 6


def test_plane_detector_symbols_and_options_layout(hiplib):
    L = hiplib.lib()
    hdr = open(os.path.join(ROOT, "include", "ovplane_hip.h")).read()
    for name in ("ovp_trackplane_defaults", "ovp_plane_detector_create", "ovp_plane_detector_destroy", "ovp_plane_detector_reset",
                 "ovp_plane_detect_triangulate", "ovp_plane_detect_planes", "ovp_plane_detector_map", "ovp_delaunay",
                 "ovp_plane_detector_debug", "ovp_plane_spatial_filter", "ovp_plane_detector_merges"):
        assert hasattr(L, name) and name in hiplib.EXPORTS and re.search(r"\b%s\s*\(" % name, hdr), name
    body = re.search(r"typedef struct \{([^}]*)\} ovp_trackplane_opts;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(int|double)\s+(\w+)\s*;", body)
    ctype = {"int": C.c_int, "double": C.c_double}
    assert [(n, ctype[t]) for t, n in fields] == list(hiplib.TrackPlaneOpts._fields_)
    assert C.sizeof(hiplib.TrackPlaneOpts) == 96
    o = hiplib.trackplane_defaults()
    assert {n: getattr(o, n) for n, _ in hiplib.TrackPlaneOpts._fields_} == ref.DEFAULTS  # TrackPlaneOptions.h:44-80
    for macro, val in (("OVP_DET_MAX_POINTS", hiplib.OVP_DET_MAX_POINTS), ("OVP_DET_MAX_NORMS", hiplib.OVP_DET_MAX_NORMS),
                       ("OVP_DET_MAX_FILTER_K", hiplib.OVP_DET_MAX_FILTER_K)):
        assert int(re.search(r"#define %s (\d+)" % macro, hdr).group(1)) == val
