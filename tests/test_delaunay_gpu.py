"""GPU tests of the device Delaunay triangulation (k_delaunay.hip): ovp_delaunay_device against ovp_delaunay, the host function, on
the same f32 input - identical arrays, no tolerance: the contract is the same algorithm, insertion order and predicates - and the
plane detector and the session with the triangulation on the device against the same runs with it on the host."""
import numpy as np
import pytest

import delaunay_cases as dc
import plane_detect_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(hiplib):
    c = hiplib.Context(64, 4, 8)
    yield c
    c.close()


@pytest.fixture(scope="module")
def host_tris(hiplib):
    """the host triangulation of every input, computed once"""
    return {name: (xy, hiplib.delaunay(xy)) for name, xy in dc.all_cases().items()}


def _same(hiplib, ctx, host_tris, name):
    xy, want = host_tris[name]
    got = hiplib.delaunay_device(ctx, xy)
    print(name, "points", len(xy), "triangles", len(want), "device", len(got))
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), name
    return want


@pytest.mark.parametrize("n", dc.RANDOM_N)
def test_random_pixels(hiplib, ctx, host_tris, n):
    """one triangle, a partial wave, several waves, the full table"""
    want = _same(hiplib, ctx, host_tris, "random_%d" % n)
    assert len(want) >= n - 2


@pytest.mark.parametrize("name", ["n0", "n1", "n2", "collinear", "identical"])
def test_inputs_without_a_triangle(hiplib, ctx, host_tris, name):
    assert len(_same(hiplib, ctx, host_tris, name)) == 0


@pytest.mark.parametrize("name", ["every_third_a_duplicate", "six_points", "collinear_but_the_last"])
def test_degenerate_inputs(hiplib, ctx, host_tris, name):
    want = _same(hiplib, ctx, host_tris, name)
    assert len(want) > 0
    if name == "every_third_a_duplicate":
        assert not np.isin(want, np.arange(3, 1024, 3)).any()  # a point at the position of an earlier one is left out


@pytest.mark.parametrize("g", dc.GRID_G)
def test_exactly_cocircular_grid(hiplib, ctx, host_tris, g):
    """exact arithmetic: the result hangs on the insertion order and the strict > 0 alone"""
    assert len(_same(hiplib, ctx, host_tris, "grid_%d" % g)) == 2 * (g - 1) ** 2


@pytest.mark.parametrize("g", dc.NEAR_G)
def test_nearly_cocircular_grid(hiplib, ctx, host_tris, g):
    """the input on which a contracted predicate can take another sign than the host's"""
    _same(hiplib, ctx, host_tris, "near_grid_%d" % g)


@pytest.mark.parametrize("name", ["ellipse", "descending_x"])
def test_hull_insertions(hiplib, ctx, host_tris, name):
    """every point on the hull (large cavities) / every insertion outside the hull (ghost triangles only turn bad first)"""
    _same(hiplib, ctx, host_tris, name)


def test_capacity_refusal_and_the_call_behind_it(hiplib, ctx, host_tris):
    n = hiplib.OVP_DET_MAX_POINTS + 1
    with pytest.raises(hiplib.OvpError) as e:
        hiplib.delaunay_device(ctx, dc.random_pixels(n))
    assert e.value.code == hiplib.OVP_E_CAPACITY
    _same(hiplib, ctx, host_tris, "random_257")


def test_two_runs_give_the_same_bits(hiplib, ctx, host_tris):
    xy, want = host_tris["random_1024"]
    a = hiplib.delaunay_device(ctx, xy)
    b = hiplib.delaunay_device(ctx, xy)
    assert a.tobytes() == b.tobytes() == want.tobytes()


def test_no_detector_is_needed_and_the_switch_needs_one(hiplib):
    c = hiplib.Context(64, 4, 8)
    xy = dc.random_pixels(48)
    assert np.array_equal(hiplib.delaunay_device(c, xy), hiplib.delaunay(xy))
    assert hiplib.lib().ovp_plane_detector_set_device_delaunay(c.handle, 1) == hiplib.OVP_E_STATE
    c.close()


# ---- the detector: triangulation on the device against the host's, two contexts, the same frames --------------------------------
def _frame_record(det, ids):
    feats = []
    for f in ids:
        d = det.feature(int(f))
        feats.append(np.concatenate([[d["count"], d["valid"]], d["p_FinG"], d["avg_norm"], d["normals"].ravel()]).tobytes())
    return det.feature2plane(), det.plane2oldplane(), feats, det.filter_rows().tobytes()


def test_detector_with_device_triangulation_equals_host(hiplib):
    frames = ref.two_wall_scene(2)
    ca, cb = hiplib.Context(64, 4, 8), hiplib.Context(64, 4, 8)
    off, on = hiplib.PlaneDetector(ca), hiplib.PlaneDetector(cb)
    assert not off.tris_info()["device_on"] and not on.tris_info()["device_on"]  # default: off
    on.set_device_delaunay(True)
    n_tris = 0
    for k, (ids, uv, uvn, R, p) in enumerate(frames):
        has_a, pf_a = off.triangulate(ids, uv, uvn, R, p)
        has_b, pf_b = on.triangulate(ids, uv, uvn, R, p)
        assert np.array_equal(has_a, has_b) and pf_a.tobytes() == pf_b.tobytes(), k
        off.planes()
        on.planes()
        ia, ib = off.tris_info(), on.tris_info()
        assert ia["source"] == "host" and ib["source"] == "device" and ib["device_on"] and not ib["overflow"], (k, ia, ib)
        assert ib["vertices"] == int(has_b.sum())
        n_tris += len(hiplib.delaunay(np.asarray(uv, np.float32).reshape(-1, 2)[has_b]))
        assert _frame_record(off, ids) == _frame_record(on, ids), k
    assert n_tris > 100 and len(set(on.feature2plane().values())) == 2  # the frames were triangulated and both walls found
    off.close(), on.close()
    ca.close(), cb.close()


def test_explicit_triangles_with_the_option_on(hiplib):
    """the caller's triangles are used as before: a frame given the host triangulation of its vertices (by the caller) equals the
    frame of a detector with the option off, and one given NO triangle finds no plane"""
    frames = ref.two_wall_scene(2)
    ca, cb, cc = (hiplib.Context(64, 4, 8) for _ in range(3))
    off, on, none = hiplib.PlaneDetector(ca), hiplib.PlaneDetector(cb), hiplib.PlaneDetector(cc)
    on.set_device_delaunay(True)
    none.set_device_delaunay(True)
    for k, (ids, uv, uvn, R, p) in enumerate(frames):
        off.triangulate(ids, uv, uvn, R, p)
        off.planes()
        has, _ = on.triangulate(ids, uv, uvn, R, p)
        on.planes(hiplib.delaunay(np.asarray(uv, np.float32).reshape(-1, 2)[has]))
        assert on.tris_info()["source"] == "caller"
        assert _frame_record(off, ids) == _frame_record(on, ids), k
        none.triangulate(ids, uv, uvn, R, p)
        none.planes(np.zeros((0, 3), np.int32))
        assert none.tris_info()["source"] == "caller" and none.feature2plane() == {}
    assert len(off.feature2plane()) > 0
    for d in (off, on, none):
        d.close()
    for c in (ca, cb, cc):
        c.close()


def test_timed_frame_reports_the_new_kernel_on_its_own(hiplib, ctx):
    frames = ref.two_wall_scene(2)
    det = hiplib.PlaneDetector(ctx)
    det.set_device_delaunay(True)
    det.timer(True)
    for ids, uv, uvn, R, p in frames:
        det.triangulate(ids, uv, uvn, R, p)
        det.planes()
    ms, dl = det.kernel_ms(), det.delaunay_ms()
    print("kernels [triangulate, normals, match, filter] ms", ms, "delaunay [frame, entry] ms", dl)
    assert len(ms) == 4 and ms[0] > 0 and len(dl) == 2 and dl[0] > 0
    xy = dc.random_pixels(257)
    hiplib.delaunay_device(ctx, xy)
    assert det.delaunay_ms()[1] > 0
    det.close()


def test_session_with_device_triangulation_equals_host(hiplib):
    """the closed loop of test_session_takes_its_planes_from_the_detector's scene (0.05 px, 200 planar points), a dozen frames:
    StateOptions::gpu_device_delaunay changes no output"""
    from ov_plane_amd.build import build_host

    build_host()
    from ov_plane_amd import closed_loop
    from ov_plane_amd.sim import Simulator, synthetic_trajectory

    def run(**kw):
        sim = Simulator(synthetic_trajectory(duration=20.0), num_pts=60, num_pts_plane=200, sigma_pix=0.05)
        return closed_loop.run_session(sim, n_frames=12, C=8, planes=2, detect_planes=True, **kw)

    a, b = run(device_delaunay=False), run(device_delaunay=True)
    print("features on detected planes per frame", a["detected_per_frame"][:, 0], "map", a["detected_per_frame"][:, 1])
    assert a["detected_per_frame"][:, 1].max() > 0  # the detector had planes to find within the dozen frames
    assert a["traj"].tobytes() == b["traj"].tobytes() and a["posecov"].tobytes() == b["posecov"].tobytes()
    assert np.array_equal(a["detected_per_frame"], b["detected_per_frame"]) and np.array_equal(a["counts"], b["counts"])
