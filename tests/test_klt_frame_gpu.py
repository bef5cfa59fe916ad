"""GPU tests of the fused hand-over of a frame's tracks (ovp_klt_match_frame through capi.KltTracker.match_frame and
step(.., fused=True)): every comparison is against the unfused sequence of existing entries (track, epipolar, the keep rule on the
host, append) on a second, fresh context, byte for byte - the kernels in front of k_klt_keep_append are the same code and the new
one only decides on integers and copies, so there is no tolerance anywhere in this file."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frame_cases  # noqa: E402
import klt_cases  # noqa: E402

pytestmark = pytest.mark.gpu

W, H, LEVELS = 96, 64, 3


class Rig:
    """a context with a tracker and (S > 0) a feature database"""

    def __init__(self, capi, max_points=64, S=64, M=8, feats=64):
        self.ctx = capi.Context(64, 4, feats)
        self.kt = capi.KltTracker(self.ctx, W, H, LEVELS, 15, max_points)
        self.db = capi.FeatureDatabase(self.ctx, S, M) if S else None

    def close(self):
        if self.db is not None:
            self.db.close()
        self.kt.close()
        self.ctx.close()


def _feature(db, fid):
    f = db.get_feature(int(fid))
    return None if f is None else (f["slot"], f["count"], f["to_delete"], f["ts"].tobytes(), f["uv"].tobytes(), f["uv_norm"].tobytes())


def _database_state(db, ids, stamps):
    """get_feature of every id, the class table and the gathered batch over the time stamps"""
    feats = [_feature(db, i) for i in ids]
    t = db.classify(stamps, stamps[-1], stamps[0], 2, True)
    table = tuple(t[k].tobytes() for k in ("ids", "cls", "count", "cleaned", "flags", "totals"))
    live = [int(i) for i, c in zip(t["ids"], t["cleaned"]) if c > 0]
    db.gather(live, stamps)
    g = db.gathered()
    return feats, table, tuple(g[k].tobytes() for k in ("uv", "uv_norm", "clone_idx", "n_meas"))


def _info_bytes(e):
    return (e["F"].tobytes(), e["count"], e["winner"], e["niters"], e["stop"], e["n_with_model"], e["too_few"], e["no_model"],
            e["mask"].tobytes(), e["uvn1"].tobytes())


def _run_sequence(capi, fused, planted, check, with_mask):
    q, frames, wrong = frame_cases.planted_sequence()
    if not planted:
        frames = q["frames"]
    mask = q["mask"] if with_mask else None
    epi = frame_cases.epipolar_opts(W, H) if check else None
    r = Rig(capi)
    r.kt.camera = frame_cases.camera(W, H)
    trace = []
    try:
        r.kt.step(frames[0], mask, epipolar=epi, database=r.db, timestamp=frame_cases.STAMPS[0], fused=fused)
        r.kt.add_points(q["ids"], q["pts"])
        r.db.update_feature(frame_cases.STAMPS[0], q["ids"], q["pts"], q["pts"])   # the seeds' first observation (:477-491)
        for k in (1, 2):
            n_in = len(r.kt.ids_last)
            ids, pts = r.kt.step(frames[k], mask, epipolar=epi, database=r.db, timestamp=frame_cases.STAMPS[k], fused=fused)
            ran = len(r.kt.last_match[0]) > 0
            trace.append(dict(ids=ids, pts=pts, uvn=r.kt.last_uv_norm.copy(), match=(r.kt.last_match[0].copy(), r.kt.last_match[1].copy()),
                              keep=r.kt.last_keep.copy(), reset=r.kt.last_reset, n_in=n_in,
                              info=_info_bytes(r.kt.last_epipolar) if check and ran else None,
                              epi_mask=r.kt.last_epipolar["mask"].copy() if check and ran else None,
                              db=_database_state(r.db, q["ids"], list(frame_cases.STAMPS[:k + 1]))))
    finally:
        r.close()
    return trace, wrong, q


def _equal_traces(a, b):
    for k, (x, y) in enumerate(zip(a, b)):
        where = "frame %d" % (k + 1)
        assert np.array_equal(x["ids"], y["ids"]) and x["pts"].tobytes() == y["pts"].tobytes(), where
        assert x["uvn"].tobytes() == y["uvn"].tobytes() and x["keep"].tobytes() == y["keep"].tobytes(), where
        assert x["match"][0].tobytes() == y["match"][0].tobytes() and x["match"][1].tobytes() == y["match"][1].tobytes(), where
        assert x["reset"] == y["reset"] and x["info"] == y["info"], where
        assert x["db"][0] == y["db"][0], where + ": get_feature"
        assert x["db"][1] == y["db"][1], where + ": classify"
        assert x["db"][2] == y["db"][2], where + ": gather"


@pytest.fixture(scope="module")
def unfused_traces(hiplib):
    """the unfused sequence of existing entries, computed once per variant"""
    cache = {}

    def get(planted, check, with_mask):
        key = (planted, check, with_mask)
        if key not in cache:
            cache[key] = _run_sequence(hiplib, False, *key)
        return cache[key]
    return get


@pytest.mark.parametrize("with_mask", [True, False], ids=["mask", "no_mask"])
@pytest.mark.parametrize("check", [True, False], ids=["check", "no_check"])
@pytest.mark.parametrize("planted", [False, True], ids=["plain", "planted"])
def test_sequence_equals_the_unfused_entries(hiplib, unfused_traces, planted, check, with_mask):
    want, wrong, q = unfused_traces(planted, check, with_mask)
    got, _, _ = _run_sequence(hiplib, True, planted, check, with_mask)
    _equal_traces(got, want)
    f1, f2 = want
    # the sequence does what it was built for
    assert f1["n_in"] == 14 and len(f1["uvn"]) == len(f1["ids"]) > 0
    if with_mask and not check:
        assert 112 not in f1["ids"] and f1["match"][1][12] == 1, "the point that tracks into the mask goes in the second frame"
    if not check:
        assert 113 in f1["ids"] and 113 not in f2["ids"], "the point that leaves the image goes in the third frame"
    if check and planted:
        gone = f1["epi_mask"][np.isin(q["ids"], wrong)] == 0
        assert gone.any() and not np.isin(wrong[gone], f1["ids"]).any(), "the check removes a planted wrong track"
    assert any(s is not None and s[1] == 2 for s in f1["db"][0]), "survivors hold two observations after the second frame"


def test_two_runs_give_the_same_bytes(hiplib):
    a, _, _ = _run_sequence(hiplib, True, True, True, True)
    b, _, _ = _run_sequence(hiplib, True, True, True, True)
    _equal_traces(a, b)


# ---- compaction edges -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_rigs(hiplib):
    img = klt_cases.sequence()["frames"][0]
    rigs = [Rig(hiplib, 4096, 4096, 2, 4096) for _ in range(2)]
    for r in rigs:
        r.kt.camera = frame_cases.camera(W, H)
        r.kt.step(img)          # the same image twice: zero motion
    yield rigs, img
    for r in rigs:
        r.close()


def _edge_step(r, img, ids, pts, mask, fused, epi=None):
    r.db.reset()
    r.kt.ids_last, r.kt.pts_last = ids.copy(), pts.copy()
    out = r.kt.step(img, mask, epipolar=epi, database=r.db, timestamp=3.5, fused=fused)
    return out, r.kt.last_keep.copy(), r.kt.last_uv_norm.copy()


def _edge_database(r, ids, n):
    """the read-back: every feature below 66 points, the first, the last and a stride above; the gathered batch of all"""
    some = ids if n <= 65 else np.concatenate([ids[:2], ids[-2:], ids[::97]])
    feats = [_feature(r.db, i) for i in some]
    dims = r.db.dims()
    g = None
    if len(ids):
        r.db.gather(ids, [3.5])
        g = tuple(r.db.gathered()[k].tobytes() for k in ("uv", "uv_norm", "clone_idx", "n_meas"))
    return feats, dims[2], g


@pytest.mark.parametrize("name", frame_cases.PATTERNS)
@pytest.mark.parametrize("n", frame_cases.EDGE_SIZES)
def test_compaction_edges(edge_rigs, n, name):
    (fu, un), img = edge_rigs
    ids, pts = frame_cases.edge_points(n)
    mask = frame_cases.mask_of(name, n, pts, W, H)
    (ids_u, pts_u), keep_u, uvn_u = _edge_step(un, img, ids, pts, mask, False)
    assert np.array_equal(keep_u, frame_cases.pattern(name, n)), "the unfused path keeps exactly the intended pattern"
    (ids_f, pts_f), keep_f, uvn_f = _edge_step(fu, img, ids, pts, mask, True)
    raw = fu.kt.last_frame_raw
    assert keep_f.tobytes() == keep_u.tobytes() and raw[0].n_kept == keep_u.sum()
    assert np.array_equal(raw[6][:raw[0].n_kept], np.flatnonzero(keep_u)), "kept_index"
    assert np.array_equal(ids_f, ids_u) and pts_f.tobytes() == pts_u.tobytes() and uvn_f.tobytes() == uvn_u.tobytes()
    # the survivors as the device compacted them
    r = fu.kt.match_frame(pts, ids + 1, 3.5, mask, dict(camera=fu.kt.camera, max_iters=1), compacted=True)
    assert r["kept_uv"].tobytes() == pts_u.tobytes() and r["kept_uvn"].tobytes() == uvn_u.tobytes()
    assert _edge_database(fu, ids_f, n) == _edge_database(un, ids_u, n)


def test_compaction_with_the_check_at_65(edge_rigs):
    """65 points spread over the image, the sequence's motion between the two frames (the check needs one) and its mask"""
    (fu, un), _ = edge_rigs
    q = klt_cases.sequence()
    ids, pts = (v[::64] for v in frame_cases.edge_points(4160))
    assert len(ids) == 65
    epi = frame_cases.epipolar_opts(W, H)
    for r in (fu, un):
        r.kt.step(q["frames"][0])
    (ids_u, pts_u), keep_u, uvn_u = _edge_step(un, q["frames"][1], ids, pts, q["mask"], False, epi)
    (ids_f, pts_f), keep_f, uvn_f = _edge_step(fu, q["frames"][1], ids, pts, q["mask"], True, epi)
    for r in (fu, un):          # the module's rigs hold the same image twice again
        r.kt.step(q["frames"][0]), r.kt.step(q["frames"][0])
    print("n = 65 with the check: %d kept" % keep_u.sum())
    assert keep_u.any() and not keep_u.all()
    assert keep_f.tobytes() == keep_u.tobytes() and np.array_equal(ids_f, ids_u) and pts_f.tobytes() == pts_u.tobytes()
    assert uvn_f.tobytes() == uvn_u.tobytes() and _info_bytes(fu.kt.last_epipolar) == _info_bytes(un.kt.last_epipolar)
    assert _edge_database(fu, ids_f, 65) == _edge_database(un, ids_u, 65)


# ---- slot order -----------------------------------------------------------------------------------------------------------------
def _slot_order_run(capi, fused):
    c = frame_cases.slot_order_case()
    img = klt_cases.sequence()["frames"][0]
    r = Rig(capi, 64, c["S"], c["M"])
    r.kt.camera = frame_cases.camera(W, H)
    try:
        r.kt.step(img)
        _, p6 = frame_cases.edge_points(6)
        r.db.update_feature(1.0, c["first_ids"], p6, p6)
        r.db.mark_deleted(c["marked"])
        r.db.cleanup()
        ids, pts = c["frame_ids"], frame_cases.edge_points(len(c["frame_ids"]))[1]
        mask = np.zeros((H, W), dtype=np.uint8)
        gone = ~c["frame_keep"]
        mask[pts[gone, 1].astype(int), pts[gone, 0].astype(int)] = 255
        r.kt.ids_last, r.kt.pts_last = ids.copy(), pts.copy()
        kept, _ = r.kt.step(img, mask, database=r.db, timestamp=2.0, fused=fused)
        every = np.concatenate([c["first_ids"], np.arange(11, 16)])
        after_frame = [_feature(r.db, i) for i in every]
        # a following update_feature and cleanup
        r.db.update_feature(3.0, np.array([21, 11, 22], dtype=np.int64), p6[:3], p6[:3])
        r.db.mark_deleted(np.array([1, 13], dtype=np.int64))
        cl = r.db.cleanup().tobytes()
        r.db.update_feature(4.0, np.array([31, 32], dtype=np.int64), p6[:2], p6[:2])
        later = [_feature(r.db, i) for i in list(every) + [21, 22, 31, 32]]
        return kept, r.kt.last_keep.copy(), after_frame, cl, later
    finally:
        r.close()


def test_slot_order_equals_the_unfused_sequence(hiplib):
    c = frame_cases.slot_order_case()
    ku, keep_u, frame_u, cl_u, later_u = _slot_order_run(hiplib, False)
    kf, keep_f, frame_f, cl_f, later_f = _slot_order_run(hiplib, True)
    assert np.array_equal(keep_u, c["frame_keep"]), "the unfused path keeps what the case intends"
    assert np.array_equal(kf, ku) and keep_f.tobytes() == keep_u.tobytes()
    assert frame_f == frame_u, "every survivor's slot and observations"
    slots = [f[0] for f in frame_u if f is not None]
    assert len(set(slots)) == len(slots) and sorted(slots) != slots, "the free list was out of order"
    assert frame_u[6 + 1] is None and frame_u[6 + 0] is not None, "a masked fresh id takes no slot"
    assert cl_f == cl_u and later_f == later_u


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def _refused(capi, kt, code, pts, ids, **kw):
    with pytest.raises(capi.OvpError) as e:
        kt.match_frame(pts, ids, **kw)
    assert e.value.code == code, (e.value.code, code)
    r, keep, out, st, me, uvn, idx = kt.last_frame_raw
    assert r.n_kept == -7 and r.info.winner_h == -7 and (keep == 255).all() and (st == 255).all() and (me == 255).all()
    assert (out == -1.0).all() and (uvn == -1.0).all() and (idx == -1).all()


def test_refusals_touch_nothing(hiplib):
    capi = hiplib
    E_ARG, E_CAP, E_STATE = -1, capi.OVP_E_CAPACITY, capi.OVP_E_STATE
    q = klt_cases.sequence()
    img = q["frames"][0]
    ids, pts = frame_cases.edge_points(12)
    cam = dict(camera=frame_cases.camera(W, H), max_iters=64, seed=3)
    r = Rig(capi, 16, 4, 2)
    fresh = Rig(capi, 16, 4, 2)
    try:
        kt, db = r.kt, r.db
        kt.feed_image(img)
        _refused(capi, kt, E_STATE, pts, ids, epipolar=cam)                      # fewer than two images
        kt.feed_image(img)
        db.update_feature(1.0, ids[:2], pts[:2], pts[:2])
        db.update_feature(2.0, ids[:1], pts[:1], pts[:1])                        # id 0 holds max_meas = 2 observations
        before = [_feature(db, i) for i in ids]
        big_ids, big = frame_cases.edge_points(17)
        _refused(capi, kt, E_CAP, big, big_ids, epipolar=cam)                    # n > max_points
        _refused(capi, kt, E_CAP, pts[:1], ids[:1], epipolar=cam, database=db, timestamp=3.0)   # the slot is full
        _refused(capi, kt, E_CAP, pts[2:5], ids[2:5], epipolar=cam, database=db, timestamp=3.0)  # 2 live + 3 fresh > 4 slots
        bad = pts.copy()
        bad[5, 1] = np.nan
        _refused(capi, kt, E_ARG, bad, ids, epipolar=cam)
        bad[5, 1] = np.inf
        _refused(capi, kt, E_ARG, bad, ids, epipolar=cam)
        dup = ids.copy()
        dup[7] = dup[3]
        _refused(capi, kt, E_ARG, pts, dup, epipolar=cam)
        _refused(capi, kt, E_ARG, pts, ids, check=True)                          # the check without a camera
        _refused(capi, kt, E_ARG, pts[2:4], ids[2:4], database=db, timestamp=3.0)   # the database without a camera
        for kw in (dict(threshold=0.0), dict(confidence=1.0), dict(max_iters=0), dict(max_iters=1025)):
            _refused(capi, kt, E_ARG, pts, ids, epipolar=dict(cam, **kw), check=True)
        _refused(capi, kt, E_ARG, pts, ids, epipolar=dict(camera=(3, [1.0] * 8)))
        # through the structures: a null input, n < 0, a short mask stride, no tracker, no database
        a, o = capi.KltFrameIn(), capi.KltFrameOut()
        L = capi.lib()
        a.n, a.pts_prev, a.ids = 12, None, ids.ctypes.data
        o.n_kept = -7
        assert L.ovp_klt_match_frame(r.ctx.handle, C.byref(a), C.byref(o)) == E_ARG
        a.pts_prev, a.ids = pts.ctypes.data, None
        assert L.ovp_klt_match_frame(r.ctx.handle, C.byref(a), C.byref(o)) == E_ARG
        a.ids, a.n = ids.ctypes.data, -1
        assert L.ovp_klt_match_frame(r.ctx.handle, C.byref(a), C.byref(o)) == E_ARG
        assert L.ovp_klt_match_frame(r.ctx.handle, None, C.byref(o)) == E_ARG and L.ovp_klt_match_frame(r.ctx.handle, C.byref(a), None) == E_ARG
        m = np.zeros((H, W), dtype=np.uint8)
        a.n, a.mask, a.mask_stride = 12, m.ctypes.data, W - 1
        assert L.ovp_klt_match_frame(r.ctx.handle, C.byref(a), C.byref(o)) == E_ARG
        a.mask, a.mask_stride = None, 0
        bare = capi.Context(64, 4, 8)
        assert L.ovp_klt_match_frame(bare.handle, C.byref(a), C.byref(o)) == E_STATE
        bare.close()
        assert o.n_kept == -7
        nodb = Rig(capi, 16, 0)
        nodb.kt.feed_image(img), nodb.kt.feed_image(img)
        _refused(capi, nodb.kt, E_STATE, pts, ids, epipolar=cam, database=db, timestamp=3.0)   # (to_database, and this context has none)
        nodb.close()
        assert [_feature(db, i) for i in ids] == before, "the database is untouched"
        # a following valid call gives the bytes of a fresh context
        fresh.kt.feed_image(img), fresh.kt.feed_image(img)
        fresh.db.update_feature(1.0, ids[:2], pts[:2], pts[:2])
        fresh.db.update_feature(2.0, ids[:1], pts[:1], pts[:1])
        got = kt.match_frame(pts[1:3], ids[1:3], 3.0, None, cam, database=db, compacted=True)
        want = fresh.kt.match_frame(pts[1:3], ids[1:3], 3.0, None, cam, database=fresh.db, compacted=True)
        for k in ("keep", "pts", "status", "mask", "uvn", "kept_index", "kept_uv", "kept_uvn"):
            assert got[k].tobytes() == want[k].tobytes(), k
        assert got["n_kept"] == want["n_kept"] == 2
        assert [_feature(db, i) for i in ids] == [_feature(fresh.db, i) for i in ids]
    finally:
        r.close()
        fresh.close()


def test_option_refusals_equal_the_epipolar_entrys(hiplib):
    """ovp_klt_match_frame states ovp_klt_epipolar's option checks a second time (that entry stays as it is): option by option -
    every field, at its bounds, in every camera mode - both entries give the same verdict, and the verdict is the one listed."""
    capi = hiplib
    ids, pts = frame_cases.edge_points(12)
    img = klt_cases.sequence()["frames"][0]
    intr = [70.0, 71.0, 47.5, 31.5, 0.01, -0.02, 0.001, 0.002]
    nan, inf = float("nan"), float("inf")

    def with_intr(k, v):
        return [v if j == k else x for j, x in enumerate(intr)]

    cases = [((m, intr), {}, True) for m in (0, 1, 2)] + [((m, intr), {}, False) for m in (3, -1)]
    cases += [((1, intr), dict(threshold=v), ok) for v, ok in ((0.0, False), (-1.0, False), (nan, False), (inf, False), (1e-300, True))]
    cases += [((2, intr), dict(confidence=v), ok) for v, ok in ((0.0, False), (1.0, False), (-0.1, False), (nan, False), (1e-9, True),
                                                                (0.999999, True))]
    cases += [((0, intr), dict(max_iters=v), ok) for v, ok in ((0, False), (-1, False), (1, True), (1024, True), (1025, False))]
    cases += [((m, with_intr(k, nan)), {}, False) for m in (0, 1) for k in range(8)] + [((2, with_intr(4, inf)), {}, False)]
    cases += [((1, with_intr(0, 0.0)), {}, False), ((2, with_intr(1, 0.0)), {}, False), ((0, with_intr(0, 0.0)), {}, True),
              ((0, with_intr(1, 0.0)), {}, True), ((1, with_intr(2, 0.0)), {}, True)]
    r = Rig(capi, 16, 0)
    try:
        kt = r.kt
        kt.feed_image(img), kt.feed_image(img)

        def code(call):
            try:
                call()
            except capi.OvpError as e:
                return e.code
            return 0

        for cam, kw, ok in cases:
            o = dict(dict(max_iters=4, seed=1), camera=cam, **kw)
            unfused = code(lambda: kt.epipolar(pts, pts, None, **o))
            fused = code(lambda: kt.match_frame(pts, ids, 0.0, None, o, check=True))
            undistort_only = code(lambda: kt.match_frame(pts, ids, 0.0, None, o))
            assert unfused == fused == undistort_only == (0 if ok else capi.OVP_E_ARG), (cam, kw, unfused, fused, undistort_only)
    finally:
        r.close()


# ---- few and no points ----------------------------------------------------------------------------------------------------------
def test_few_and_no_points(hiplib):
    q = klt_cases.sequence()
    epi = frame_cases.epipolar_opts(W, H)
    r = Rig(hiplib)
    try:
        kt, db = r.kt, r.db
        kt.step(q["frames"][0], q["mask"], epipolar=epi, database=db, timestamp=1.0, fused=True)
        assert not kt.last_reset, "the first image only seeds"
        kt.step(q["frames"][1], q["mask"], epipolar=epi, database=db, timestamp=2.0, fused=True)
        assert kt.last_reset, "no points: the reset of :520-530"
        few = kt.match_frame(q["pts"][:9], q["ids"][:9], 2.0, q["mask"], epi, check=True, database=db)
        assert few["too_few"] and few["n_kept"] == 0 and not few["keep"].any() and not few["mask"].any() and few["winner"] == (-1, -1)
        assert (kt.last_frame_raw[2] == -1.0).all(), "no KLT ran"
        assert db.dims()[2] == 0, "nothing appended"
        none = kt.match_frame(q["pts"][:0], q["ids"][:0], 2.0, q["mask"], epi, check=True, database=db)
        assert none["n_kept"] == 0 and kt.last_frame_raw[0].info.winner_h == -7, "n = 0 returns at once"
        kt.add_points(q["ids"][:9], q["pts"][:9])
        ids, pts = kt.step(q["frames"][2], q["mask"], epipolar=epi, database=db, timestamp=3.0, fused=True)
        assert len(ids) == 0 and len(kt.last_match[0]) == 0 and not kt.last_reset, "fewer than ten points: no KLT, nothing kept"
        assert db.dims()[2] == 0
        kt.add_points(q["ids"][:9], q["pts"][:9])
        ids, pts = kt.step(q["frames"][2], q["mask"], fused=True)      # without the check nine points are tracked
        assert len(ids) > 0 and len(kt.last_match[0]) == 9 and len(kt.last_uv_norm) == 0
    finally:
        r.close()


# ---- the C++ mirror --------------------------------------------------------------------------------------------------------------
def test_mirror_equals_the_python_fused_path(hiplib):
    """ov_plane::TrackPlane::feed_monocular with a FeatureDatabase attached (hostlib.run_klt_frame_sequence) on the planted sequence"""
    from ov_plane_amd import hostlib

    q, frames, _ = frame_cases.planted_sequence()
    mode, intr = frame_cases.camera(W, H)
    cpp, cdb = hostlib.run_klt_frame_sequence(np.stack(frames), q["mask"], q["ids"], q["pts"], (1, intr), frame_cases.STAMPS, check=True,
                                              max_iters=64, seed=3, max_slots=64, max_meas=8, pyr_levels=LEVELS - 1)
    epi = frame_cases.epipolar_opts(W, H)
    r = Rig(hiplib)
    try:
        r.kt.step(frames[0], q["mask"], epipolar=epi, database=r.db, timestamp=frame_cases.STAMPS[0], fused=True)
        r.kt.add_points(q["ids"], q["pts"])
        r.db.update_feature(frame_cases.STAMPS[0], q["ids"], q["pts"], q["pts"])
        assert len(cpp[0]["ids"]) == 14
        for k in (1, 2):
            ids, pts = r.kt.step(frames[k], q["mask"], epipolar=epi, database=r.db, timestamp=frame_cases.STAMPS[k], fused=True)
            assert np.array_equal(cpp[k]["ids"], ids) and cpp[k]["pts"].tobytes() == pts.tobytes(), "frame %d" % k
            assert cpp[k]["uv_norm"].tobytes() == r.kt.last_uv_norm.tobytes() and cpp[k]["reset"] == r.kt.last_reset, "frame %d" % k
        assert len(cpp[1]["ids"]) > 0
        for i in q["ids"]:
            f, g = r.db.get_feature(int(i)), cdb[int(i)]
            assert (f is None) == (g is None), i
            if f is not None:
                assert (f["slot"], f["count"]) == (g["slot"], g["count"]), i
                assert f["ts"].tobytes() == g["ts"].tobytes() and f["uv"].tobytes() == g["uv"].tobytes() and f["uv_norm"].tobytes() == g["uv_norm"].tobytes(), i
    finally:
        r.close()


# ---- timer slot -----------------------------------------------------------------------------------------------------------------
def test_timer_slot_behind_the_existing_ones(hiplib):
    q, frames, _ = frame_cases.planted_sequence()
    epi = frame_cases.epipolar_opts(W, H)
    r = Rig(hiplib)
    try:
        kt = r.kt
        kt.feed_image(frames[0]), kt.feed_image(frames[1])
        kt.timer(True)
        got = kt.match_frame(q["pts"], q["ids"], 1.0, q["mask"], epi, check=True, database=r.db)
        t = kt._debug(b"time", 0, 56, np.float32)
        old = kt._debug(b"time", 0, 52, np.float32)
        kt.timer(False)
        assert len(t) == 14 and len(old) == 13 and t[:13].tobytes() == old.tobytes(), "existing readers see what they saw"
        assert t[13] > 0 and t[13] < 50.0, t
        assert t[2] > 0 and (t[6:10] > 0).all(), "k_klt_track and the four epipolar kernels, in their own slots"
        assert kt.kernel_ms()["keep_append"] == float(t[13])
        print("k_klt_keep_append %.4f ms at n = 14 (k_klt_track %.4f)" % (t[13], t[2]))
        # the epipolar slots are the last call's own: the undistortion alone without the check, zeros without a camera
        kt.timer(True)
        kt.match_frame(q["pts"], q["ids"], 1.0, q["mask"], dict(epi, max_iters=1))
        t = kt._debug(b"time", 0, 56, np.float32)
        assert t[6] > 0 and (t[7:10] == 0).all() and t[13] > 0, t
        kt.match_frame(q["pts"], q["ids"], 1.0, q["mask"], None)
        t = kt._debug(b"time", 0, 56, np.float32)
        kt.timer(False)
        assert (t[6:10] == 0).all() and t[2] > 0 and t[13] > 0, t
        again = Rig(hiplib)
        again.kt.feed_image(frames[0]), again.kt.feed_image(frames[1])
        want = again.kt.match_frame(q["pts"], q["ids"], 1.0, q["mask"], epi, check=True, database=again.db)
        again.close()
        assert got["keep"].tobytes() == want["keep"].tobytes() and got["pts"].tobytes() == want["pts"].tobytes(), "the timed path computes the same"
    finally:
        r.close()
