"""GPU tests of the epipolar check (ovp_klt_epipolar through capi.KltTracker.epipolar and the debug reads) against tests/epi_ref.py:
samples and table bit-equal, n_models equal on every settled hypothesis, counts inside the near allowances, the winner, the stop
index and niters equal, the mask equal outside the winner's near points, F and the undistorted coordinates within four times the
spread of the restatement's variants (epi_cases.compare, epi_cases.undistort_reference); two runs give equal bytes; the refusals
leave the outputs untouched; step(epipolar=...) on a sequence with planted wrong tracks equals the restatement on the device's own
tracks and the C++ mirror's feed_new_camera(.., epipolar = true) byte for byte; the timed path and the debug reads."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epi_cases  # noqa: E402
import epi_ref  # noqa: E402
import klt_cases  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kt(hiplib):
    c = hiplib.Context(64, 4, 8)
    t = hiplib.KltTracker(c, 64, 48, 1, 15, 512)
    yield t
    t.close()
    c.close()


def _run(kt, cid):
    c = epi_cases.case(cid)
    o = c["opts"]
    return kt.epipolar(c["pts0"], c["pts1"], c["status"], threshold=o["threshold"], confidence=o["confidence"], max_iters=o["max_iters"],
                       seed=o["seed"])


@pytest.mark.parametrize("cid", epi_cases.IDS)
def test_case_against_the_restatement(kt, cid):
    ref = epi_cases.reference(cid)
    r = _run(kt, cid)
    again = _run(kt, cid)
    for k in ("mask", "uvn0", "uvn1", "F"):
        assert r[k].tobytes() == again[k].tobytes(), "two runs differ in %s" % k
    assert all(r[k] == again[k] for k in ("count", "winner", "niters", "stop", "n_with_model", "too_few", "no_model"))
    c = epi_cases.case(cid)
    assert r["uvn0"].tobytes() == c["pts0"].tobytes() and r["uvn1"].tobytes() == c["pts1"].tobytes(), "mode 0 passes the points through"
    assert np.isfinite(r["F"]).all() and set(np.unique(r["mask"])) <= {0, 1}
    if ref["too_few"]:
        assert r["too_few"] and not r["no_model"] and not r["mask"].any() and r["winner"] == (-1, -1)
        return
    if cid in epi_cases.UNCOMPARED:
        return
    dev = dict(kt.epipolar_stages(), mask=r["mask"], F=r["F"].ravel(), count=r["count"], winner=r["winner"], niters=r["niters"],
               n_with_model=r["n_with_model"], too_few=r["too_few"], no_model=r["no_model"])
    fail, fig = epi_cases.compare(cid, dev)
    print("%s: stop %d (reference %d), %s" % (cid, r["stop"], ref["stop"], fig))
    assert r["stop"] == ref["stop"]
    assert not fail, fail


@pytest.mark.parametrize("cam", ["radtan", "equidistant"])
def test_undistortion(kt, cam):
    mode, intr = epi_cases.undistort_cameras()[cam]
    px = epi_cases.undistort_pixels()
    want, bound, spread = epi_cases.undistort_reference(cam)
    r = kt.epipolar(px, px[::-1].copy(), camera=(cam, intr), max_iters=8)
    e0 = np.abs(r["uvn0"].astype(np.float64) - want)
    e1 = np.abs(r["uvn1"].astype(np.float64) - want[::-1])
    print("%s: worst |device - restatement| over bound %.3f, unequal floats %d of %d" % (
        cam, max((e0 / bound).max(), (e1 / bound[::-1]).max()), (e0 > 0).sum() + (e1 > 0).sum(), 2 * e0.size))
    assert (e0 <= bound).all() and (e1 <= bound[::-1]).all()
    few = kt.epipolar(px[:4], px[:4], camera=(cam, intr))
    assert few["too_few"] and few["uvn0"].tobytes() == r["uvn0"][:4].tobytes(), "a short set is still undistorted"


def test_refusals_leave_the_outputs_untouched(hiplib, kt):
    c = epi_cases.case("n64")

    def refused(code, p0, p1, status=None, camera=None, **kw):
        with pytest.raises(hiplib.OvpError) as e:
            kt.epipolar(p0, p1, status, camera, **kw)
        assert e.value.code == code, (e.value.code, code, kw)
        mask, u0, u1, info = kt.last_epipolar_raw
        assert (mask == 255).all() and (u0 == -1.0).all() and (u1 == -1.0).all() and info.winner_h == -7
    E_ARG, E_CAP, E_STATE = -1, hiplib.OVP_E_CAPACITY, hiplib.OVP_E_STATE
    p0, p1 = c["pts0"], c["pts1"]
    bad = p0.copy()
    bad[5, 1] = np.nan
    refused(E_ARG, bad, p1)
    bad[5, 1] = np.inf
    refused(E_ARG, p0, bad)
    for kw in (dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=float("nan")), dict(confidence=0.0), dict(confidence=1.0),
               dict(max_iters=0), dict(max_iters=1025)):
        refused(E_ARG, p0, p1, **kw)
    refused(E_ARG, p0, p1, camera=(3, [1.0] * 8))
    refused(E_ARG, p0, p1, camera=(1, [float("nan")] + [1.0] * 7))
    big = np.zeros((513, 2), dtype=np.float32)
    refused(E_CAP, big, big)
    r = kt.epipolar(p0[:0], p1[:0])            # n = 0 returns at once
    assert len(r["mask"]) == 0 and kt.last_epipolar_raw[3].winner_h == -7
    other = hiplib.Context(64, 4, 8)           # a context without a tracker
    o = hiplib.EpipolarOpts()
    hiplib.lib().ovp_epipolar_defaults(__import__("ctypes").byref(o))
    m = np.full(64, 255, dtype=np.uint8)
    rc = hiplib.lib().ovp_klt_epipolar(other.handle, __import__("ctypes").byref(o), 64, p0.ctypes.data, p1.ctypes.data, None, m.ctypes.data,
                                       None, None, None)
    other.close()
    assert rc == E_STATE and (m == 255).all()
    good = _run(kt, "n64")
    assert good["winner"] == tuple(epi_cases.reference("n64")["winner"])


def test_null_outputs_and_status(kt):
    """any output may be NULL; the RANSAC uses the status-0 points and the mask drops them"""
    import ctypes

    from ov_plane_amd import capi

    c = epi_cases.case("n80_status")
    o = capi.EpipolarOpts()
    capi.lib().ovp_epipolar_defaults(ctypes.byref(o))
    o.threshold, o.max_iters, o.seed = c["opts"]["threshold"], c["opts"]["max_iters"], c["opts"]["seed"]
    p0, p1 = c["pts0"], c["pts1"]
    assert capi.lib().ovp_klt_epipolar(kt.ctx.handle, ctypes.byref(o), len(p0), p0.ctypes.data, p1.ctypes.data, None, None, None, None, None) == 0
    r = _run(kt, "n80_status")
    ref = epi_cases.reference("n80_status")
    gone = c["status"] == 0
    assert not r["mask"][gone].any() and r["count"] == ref["count"] and r["count"] > r["mask"].sum()
    assert np.isin(np.where(gone)[0], kt.epipolar_stages()["samples"]).any()


def _planted_sequence():
    """the three-frame sequence of klt_cases with three wrong tracks planted: around three of its points the patch of frame 0 is
    pasted into frame 1 away from where the scene's motion (4 px to the right) takes it - by (0, 5), (6, 0) and (-5, -5) px, the
    threshold being 2 px - so the KLT follows it there.  The scene is one plane: its true tracks leave the epipole free (F = [e]x H
    for any e), and each wrong track asks only that e lie on one line, so a model may absorb two of the three - three lines in
    general position have no common point - and at least one must go."""
    q = klt_cases.sequence()
    frames = [f.copy() for f in q["frames"]]
    h, w = frames[0].shape
    pick = [i for i, (x, y) in enumerate(q["pts"][:12]) if 16 <= y <= 45 and 12 <= x <= 44][:3]
    assert len(pick) == 3
    for i, (dx, dy) in zip(pick, PLANTED_SHIFTS):
        x, y = int(round(q["pts"][i][0])), int(round(q["pts"][i][1]))
        frames[1][y - 10 + dy:y + 11 + dy, x - 10 + 4 + dx:x + 11 + 4 + dx] = q["frames"][0][y - 10:y + 11, x - 10:x + 11]
    return q, frames, q["ids"][pick]


PLANTED_SHIFTS = [(0, 5), (6, 0), (-5, -5)]


def test_step_with_the_check_equals_the_restatement_and_the_mirror(hiplib):
    """step(epipolar=...) on the planted sequence: the mask, the winner and the undistorted coordinates equal epi_ref.epipolar on
    the device's own tracks (the mask outside the winner's near points, as epi_cases.compare has it), the kept set equals the
    restatement's frame logic on the restatement's mask, the planted tracks go, and the C++ mirror's
    feed_new_camera(.., epipolar = true) returns the same bytes"""
    from ov_plane_amd import hostlib

    q, frames, wrong = _planted_sequence()
    w, h = q["width"], q["height"]
    intr = [0.9 * w, 0.9 * w, 0.5 * (w - 1), 0.5 * (h - 1), 0.0, 0.0, 0.0, 0.0]
    epi = dict(camera=("radtan", intr), max_iters=64, seed=3)
    opts = dict(mode=1, intrinsics=intr, threshold=2.0 / (0.9 * w), confidence=0.999, max_iters=64, seed=3)
    ctx = hiplib.Context(64, 4, 8)
    kt = hiplib.KltTracker(ctx, w, h, q["levels"], 15, 64)
    kt.step(frames[0], q["mask"], epipolar=epi)
    kt.add_points(q["ids"], q["pts"])
    per_frame = [(kt.ids_last.copy(), kt.pts_last.copy(), np.zeros((0, 2), np.float32))]
    # frame 1: all 14 points go in (at least ten: the check runs)
    ids0, pts0 = kt.ids_last.copy(), kt.pts_last.copy()
    assert len(ids0) == 14
    ids, pts = kt.step(frames[1], q["mask"], epipolar=epi)
    per_frame.append((ids, pts, kt.last_uv_norm.copy()))
    p, st = kt.last_match
    e = kt.last_epipolar
    moved = p[np.isin(ids0, wrong)] - pts0[np.isin(ids0, wrong)]
    # (the patches overlap where two of the points are close: a track follows whichever patch covers it - off the motion either way)
    assert st[np.isin(ids0, wrong)].all() and (np.hypot(*(moved - [4.0, 0.0]).T) > 2.5).all(), "the planted tracks leave the scene's motion"
    c = dict(pts0=pts0, pts1=p, status=st, opts=opts)
    ref = epi_ref.epipolar(pts0, p, st, opts)
    al = epi_cases.allowances_of(c, ref)
    assert e["winner"] == tuple(ref["winner"]) and e["winner"][0] >= 0 and e["niters"] == ref["niters"] and e["stop"] == ref["stop"]
    hh, mm = ref["winner"]
    near = al["near"][hh, mm]
    print("frame 1: winner %s, %d inliers of 14, %d near, mask %s" % (e["winner"], e["count"], near.sum(), e["mask"].tolist()))
    assert near.sum() <= 1, "klt_cases.near_cap: one point below 50"
    assert np.array_equal(e["mask"][~near], ref["mask"][~near])
    step32 = epi_cases.f32_step(ref["uvn1"])
    assert (np.abs(e["uvn1"].astype(np.float64) - ref["uvn1"]) <= step32).all() and (np.abs(e["uvn0"].astype(np.float64) - ref["uvn0"]) <= epi_cases.f32_step(ref["uvn0"])).all()
    gone = e["mask"][np.isin(ids0, wrong)] == 0
    assert gone.any() and not np.isin(wrong[gone], ids).any(), "the check removes a planted wrong track"
    assert e["mask"][~np.isin(ids0, wrong) & (st != 0)].sum() >= 9, "and keeps the true ones"
    want = epi_ref.feed_monocular(ids0, pts0, lambda _: (p, st), w, h, q["mask"], lambda a, b, s: dict(mask=np.where(near, e["mask"], ref["mask"]), uvn1=e["uvn1"]))
    assert np.array_equal(ids, want[0]) and pts.tobytes() == want[1].tobytes() and kt.last_uv_norm.tobytes() == want[2].tobytes()
    assert len(ids) >= 8
    # frame 2: what is left goes in; fewer than ten keep nothing and run no KLT, ten or more run the check again
    n1 = len(ids)
    ids2, pts2 = kt.step(frames[2], q["mask"], epipolar=epi)
    per_frame.append((ids2, pts2, kt.last_uv_norm.copy()))
    if n1 < 10:
        assert len(ids2) == 0 and len(kt.last_match[0]) == 0 and not kt.last_reset
    else:
        assert kt.last_epipolar["winner"][0] >= 0 and len(ids2) <= n1
    kt.close()
    ctx.close()
    cpp = hostlib.run_klt_epipolar_sequence(np.stack(frames), q["mask"], q["ids"], q["pts"], (1, intr), max_iters=64, seed=3,
                                            pyr_levels=q["levels"] - 1)
    for f in (1, 2):
        assert np.array_equal(cpp[f]["ids"], per_frame[f][0]) and cpp[f]["pts"].tobytes() == per_frame[f][1].tobytes(), "frame %d" % f
        assert cpp[f]["uv_norm"].tobytes() == per_frame[f][2].tobytes() and not cpp[f]["reset"]
    assert len(cpp[0]["ids"]) == 14


def test_step_rules_for_few_and_no_points(hiplib):
    q = klt_cases.sequence()
    w, h = q["width"], q["height"]
    epi = dict(camera=("radtan", [0.9 * w, 0.9 * w, 0.5 * (w - 1), 0.5 * (h - 1), 0.0, 0.0, 0.0, 0.0]), max_iters=64, seed=3)
    ctx = hiplib.Context(64, 4, 8)
    kt = hiplib.KltTracker(ctx, w, h, q["levels"], 15, 64)
    kt.step(q["frames"][0], q["mask"], epipolar=epi)
    assert not kt.last_reset, "the first image only seeds"
    kt.step(q["frames"][1], q["mask"], epipolar=epi)
    assert kt.last_reset, "no points: the reset of :520-530"
    kt.add_points(q["ids"][:9], q["pts"][:9])
    ids, pts = kt.step(q["frames"][2], q["mask"], epipolar=epi)
    assert len(ids) == 0 and len(kt.last_match[0]) == 0 and not kt.last_reset, "fewer than ten points: no KLT, nothing kept"
    kt.add_points(q["ids"][:9], q["pts"][:9])
    ids, pts = kt.step(q["frames"][2], q["mask"])     # the default leaves step as it was: nine points are tracked
    assert len(ids) > 0 and len(kt.last_match[0]) == 9
    kt.close()
    ctx.close()


def test_timed_path_fills_the_four_new_slots(kt):
    kt.timer(True)
    r = _run(kt, "n300_out30")
    t = kt._debug(b"time", 0, 40, np.float32)
    kt.timer(False)
    assert len(t) == 10 and (t[6:] > 0).all() and (t[6:] < 50.0).all(), t
    assert r["winner"] == tuple(epi_cases.reference("n300_out30")["winner"]), "the timed path computes the same"
    print("k_epi_undistort %.4f, k_epi_models %.4f, k_epi_count %.4f, k_epi_select %.4f ms" % tuple(t[6:]))


def test_debug_reads_stay_with_their_run(kt):
    """a too-few call behind a full one leaves every epi_* read of the full run in place, the table included"""
    _run(kt, "n64")
    a = kt.epipolar_stages()
    shape = kt._epi_shape
    few = _run(kt, "n9_too_few")
    assert few["too_few"]
    kt._epi_shape = shape
    b = kt.epipolar_stages()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
