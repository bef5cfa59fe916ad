"""GPU tests of the plane detector (k_plane_detect.hip) against the numpy restatement of the reference's stage
(tests/plane_detect_ref.py): continuous quantities at 1e-9 relative, decisions identical.  The scenes assert on the restatement
that no thresholded quantity sits within 1e-6 of its threshold, so no feature or edge is left out of a comparison."""
import numpy as np
import pytest

import plane_detect_ref as ref

pytestmark = pytest.mark.gpu
RTOL = 1e-9


def _close(a, b):
    """1e-9 relative, vector by vector (the rows of a 2-D array: a position, a normal) or value by value (1-D)"""
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert a.shape == b.shape
    if a.ndim == 1:
        a, b = a[:, None], b[:, None]
    if a.size == 0:
        return
    scale = np.linalg.norm(b, axis=1)
    err = np.linalg.norm(a - b, axis=1)
    rel = np.where(err == 0.0, 0.0, err / np.where(scale > 0, scale, 1e-300))
    print("max relative difference %.3e" % rel.max())
    assert rel.max() <= RTOL, rel.max()


@pytest.fixture()
def ctx(hiplib):
    c = hiplib.Context(64, 4, 8)
    yield c
    c.close()


def _run(hiplib, ctx, frames, per_frame=None, **opts):
    det = hiplib.PlaneDetector(ctx, hiplib.trackplane_defaults(**opts))
    maps = []
    for k, (ids, uv, uvn, R, p) in enumerate(frames):
        has, pf = det.triangulate(ids, uv, uvn, R, p)
        det.planes()
        maps.append(det.feature2plane())
        if per_frame:
            per_frame(k, det, ids, has, pf)
    det.close()
    return maps


def test_triangulation_positions_and_gates(hiplib, ctx):
    frames = ref.triangulation_scene(3)
    r = ref.TrackPlaneRef()
    det = hiplib.PlaneDetector(ctx)
    for k, (ids, uv, uvn, R, p) in enumerate(frames):
        e_has, e_p, e_acc = r.triangulate(ids, uv, uvn, R, p)
        has, pf = det.triangulate(ids, uv, uvn, R, p)
        assert np.array_equal(has, e_has) and np.array_equal(det.accepted, e_acc), k
        _close(pf, e_p)
        for f in (1, 2, 3, 100, 128):
            if f in ids:
                d = det.feature(f)
                assert d["count"] == r.count[f] and d["valid"] == (f in r.p)
    assert r.min_margin() >= ref.MARGIN
    assert len(frames[-1][0]) == 32 and e_has.sum() == 29 and r.count[1] == 3
    assert not e_has[:3].any()  # the three gates: observations, min_dist, condition number - each feature at its own
    gates = {f: [(k, m) for k, m, g in r.gate_log if g == f] for f in (2, 3)}
    assert all(c <= 8000 and z < 0.1 for c, z in gates[2]) and len(gates[2]) == 3      # only min_dist rejects id 2
    assert all(c > 8000 and 0.1 <= z <= 60 for c, z in gates[3]) and len(gates[3]) == 3  # only the condition number rejects id 3
    det.close()


def test_normal_history_eviction_and_average(hiplib, ctx):
    frames = ref.two_wall_scene(1, n_wall=10, n_off=4, n_frames=7)
    res, r = ref.run_reference(frames, max_norm_count=5)
    assert len(frames[0][0]) == 24 and max(x["max_appended"] for x in res) > 5  # more normals in one frame than the history holds

    def check(k, det, ids, has, pf):
        n = 0
        for f in ids:
            d = det.feature(int(f))
            e = res[k]["norms"].get(int(f), np.zeros((0, 3)))
            assert d["normals"].shape == e.shape, (k, f)
            if len(e):
                _close(d["normals"], e)
                _close(d["avg_norm"], res[k]["avg"][int(f)])
                n += 1
        assert n > 0 or k < 3

    maps = _run(hiplib, ctx, frames, check, max_norm_count=5)
    assert maps == [x["map"] for x in res]


def test_spatial_filter_distances_and_flags(hiplib, ctx):
    """Every plane the filter looks at, over eight frames: one of exactly filter_num_feat + 1 points (each point's neighbours are
    all the others), larger ones with flagged points, and planes at or below filter_num_feat points, which it leaves alone."""
    frames = ref.two_wall_scene(6)
    res, r = ref.run_reference(frames)
    sizes = [c for x in res for c in np.unique([row[1] for row in x["filter"]], return_counts=True)[1]]
    assert 5 in sizes and max(sizes) >= 10 and sum(row[3] for x in res for row in x["filter"]) >= 2
    seen = []

    def check(k, det, ids, has, pf):
        rows, e = det.filter_rows(), np.array(res[k]["filter"], dtype=float).reshape(-1, 4)
        assert np.array_equal(rows[:, [0, 1, 3]], e[:, [0, 1, 3]]), k
        if len(e):
            _close(rows[:, 2], e[:, 2])
        seen.append(len(e))

    maps = _run(hiplib, ctx, frames, check)
    assert maps == [x["map"] for x in res] and sum(seen) == sum(len(x["filter"]) for x in res)


def _plane_patch(rng, n, spread):
    """n points on the plane z = 2 x + 1, scattered over spread x spread"""
    xy = rng.uniform(0, spread, (n, 2))
    return np.column_stack([xy, 2 * xy[:, 0] + 1])


def _filter_truth(P, k, z):
    """TrackPlane.cpp:1010-1057 on one plane, numpy: f32 squared distances as KD_TREE::calc_dist, the rest in f64"""
    P = np.asarray(P).astype(np.float32)
    dv = np.zeros(len(P))
    kth = []
    for i in range(len(P)):
        df = P - P[i]
        d2 = np.sort(np.delete((df[:, 0] * df[:, 0] + df[:, 1] * df[:, 1]) + df[:, 2] * df[:, 2], i))
        dv[i] = d2[:k].astype(np.float64).sum() / float(k)
        kth.append(d2[:k + 1])
    mean = dv.mean()
    zs = np.abs(dv - mean) / np.sqrt(((dv - mean) ** 2).sum() / (len(dv) - 1.0))
    assert (np.abs(zs - z) / z >= ref.MARGIN).all()  # the scene's margin: no z-score at the threshold
    return dv, zs > z


def test_spatial_filter_on_constructed_planes(hiplib, ctx):
    """The filter alone on planes built point by point: exactly filter_num_feat + 1 points (every point's neighbours are all the
    others), 40 points with two planted outliers, 300 points (more than one pass of the workgroup's 256 threads), and a plane of
    filter_num_feat points, which it must leave alone."""
    rng = np.random.default_rng(40)
    k, z = 4, 1.2
    five = _plane_patch(rng, 5, 1.0)
    forty = _plane_patch(rng, 40, 1.0)
    forty[[7, 31]] = [[3.0, 3.0, 7.0], [-2.5, 0.5, -4.0]]  # on the plane, far from the patch
    big = _plane_patch(rng, 300, 4.0)
    four = _plane_patch(rng, 4, 1.0)
    det = hiplib.PlaneDetector(ctx)
    got = det.spatial_filter([five, forty, four, big], k, z)
    for P, (dist, flag) in zip((five, forty, big), (got[0], got[1], got[3])):
        e_d, e_f = _filter_truth(P, k, z)
        _close(dist, e_d)
        assert np.array_equal(flag, e_f)
    # all others are the neighbours of each of the five: the mean over its four distances
    df = five.astype(np.float32)[:, None] - five.astype(np.float32)[None]
    d5 = ((df[..., 0] * df[..., 0] + df[..., 1] * df[..., 1]) + df[..., 2] * df[..., 2]).astype(np.float64)  # f32, as calc_dist
    _close(got[0][0], d5.sum(1) / 4.0)
    # the planted outliers are flagged, and they alone carry the largest neighbour distances
    assert got[1][1][[7, 31]].all() and set(np.argsort(got[1][0])[-2:]) == {7, 31}
    assert not got[2][1].any() and (got[2][0] == 0).all()
    with pytest.raises(hiplib.OvpError) as e:
        det.spatial_filter([_plane_patch(rng, 1025, 4.0)], k, z)
    assert e.value.code == hiplib.OVP_E_CAPACITY
    det.close()


def test_session_takes_its_planes_from_the_detector(hiplib):
    """StateOptions::gpu_plane_detection: no plane label reaches the session (the caller's map is empty), the detector runs on every
    frame's tracked points at the session's own clone pose, and its map is the one the updaters get: features of a step lie on
    detected planes and planes enter the state - which, with no label handed over, they can only do through that map.  The scene
    is the simulator's room with 0.05 px of pixel noise and 200 planar points, on which the stage (restated on the CPU at the
    true poses) keeps 40-70 features on 3-4 planes; at the simulator's default of one pixel it keeps a handful.
    With the option off, handing the tracked points over changes nothing."""
    from ov_plane_amd.build import build_host

    build_host()
    from ov_plane_amd import closed_loop
    from ov_plane_amd.sim import Simulator, synthetic_trajectory

    def sim(**kw):  # (a simulator draws its noise as it goes: every run gets a fresh one)
        return Simulator(synthetic_trajectory(duration=20.0), num_pts=60, **kw)

    r = closed_loop.run_session(sim(num_pts_plane=200, sigma_pix=0.05), n_frames=40, C=8, planes=2, detect_planes=True)
    print("features on detected planes per frame", r["detected_per_frame"][:, 0], "map", r["detected_per_frame"][:, 1],
          "planes in the state", r["counts"][:, 5], "rmse", r["rmse_pos"])
    assert np.isfinite(r["traj"]).all()
    assert r["detected_per_frame"][:, 0].max() >= 6    # plane_min_feat features of one step on detected planes
    assert r["counts"][:, 5].max() >= 1                # at least one plane initialised from them and kept in the state
    with pytest.raises(ValueError):
        closed_loop.run(sim(num_pts_plane=120), planes=0, detect_planes=True)
    off = closed_loop.run_session(sim(num_pts_plane=120), n_frames=12, C=8, planes=2)
    fed = closed_loop.run_session(sim(num_pts_plane=120), n_frames=12, C=8, planes=2, feed_plane_tracks=True)
    assert off["traj"].tobytes() == fed["traj"].tobytes() and off["posecov"].tobytes() == fed["posecov"].tobytes()
    assert np.array_equal(off["counts"], fed["counts"])


def test_two_walls_end_to_end_and_bit_identical_runs(hiplib, ctx):
    frames = ref.two_wall_scene(2)
    res, r = ref.run_reference(frames)
    assert len(frames[0][0]) == 48 and len(set(res[-1]["map"].values())) == 2
    got = []

    def check(k, det, ids, has, pf):
        assert np.array_equal(has, res[k]["has"])
        _close(pf, res[k]["p"])
        merges.append(det.plane2oldplane())
        got.append((has.tobytes(), pf.tobytes(), det.filter_rows().tobytes()))

    merges = []
    maps = _run(hiplib, ctx, frames, check)
    assert maps == [x["map"] for x in res]
    assert merges == [x["merges"] for x in res]  # TrackPlane::get_plane2oldplane after every frame
    first, got[:] = list(got), []
    assert _run(hiplib, ctx, frames, check) == maps and got == first


def test_capacity_refusal_leaves_the_detector_untouched(hiplib, ctx):
    frames = ref.two_wall_scene(2)
    expect = _run(hiplib, ctx, frames)
    det = hiplib.PlaneDetector(ctx)
    n = hiplib.OVP_DET_MAX_POINTS + 1
    for k, (ids, uv, uvn, R, p) in enumerate(frames):
        if k == 4:
            with pytest.raises(hiplib.OvpError) as e:
                det.triangulate(np.arange(n), np.zeros((n, 2)), np.zeros((n, 2)), R, p)
            assert e.value.code == hiplib.OVP_E_CAPACITY
        det.triangulate(ids, uv, uvn, R, p)
        det.planes()
        assert det.feature2plane() == expect[k]
    det.close()


def test_detector_memory_goes_with_the_context(hiplib):
    def live():
        b = np.zeros(2, dtype=np.int64)
        assert hiplib.lib().ovp_debug_read(c.handle, b"live_bytes", b.ctypes.data, 16) == 16
        return b.copy()

    c = hiplib.Context(64, 4, 8)
    before = live()
    hiplib.PlaneDetector(c)
    assert (live() > before).all()
    c2 = hiplib.Context(64, 4, 8)
    c.close()           # the detector was never destroyed by hand
    c = c2
    assert (live() == before).all()
    c.close()
