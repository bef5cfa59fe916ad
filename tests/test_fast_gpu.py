"""GPU tests of the detector (ovp_klt_detect, capi.KltTracker.detect / step(detect=True), the C++ mirror) against tests/fast_ref.py:
the score map, the suppressed map and the candidate list bit-equal on every case, no point excluded; the refined positions within
four times the case's own spread among the restatement's variants (fast_cases.compare_refined); the host logic's ids and positions
equal to the restatement run on the device's candidates; the loop; the refusals."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fast_cases  # noqa: E402
import fast_ref  # noqa: E402
import klt_cases  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(hiplib):
    c = hiplib.Context(64, 4, 8)
    yield c
    c.close()


def _tracker(hiplib, ctx, img, half=0, max_points=1024, detector=None):
    h, w = img.shape
    kt = hiplib.KltTracker(ctx, w, h, 1, 15, max_points, detector=detector)
    kt.feed_image(img, "NONE")
    if half:
        kt.feed_image(255 - img, "NONE")  # the image is the previous half's now
    return kt


# every case on the current half, the small ones and one 752 x 480 configuration on the previous half as well
RUNS = [(cid, 0) for cid in fast_cases.IDS] + [(cid, 1) for cid in fast_cases.SMALL + ["sim_752x480"]]


@pytest.mark.parametrize("cid,half", RUNS, ids=["%s-half%d" % r for r in RUNS])
def test_integer_stages_are_bit_equal(hiplib, ctx, cid, half):
    img, nf, gx, gy, th = fast_cases.CASES[cid]
    ref = fast_cases.reference(cid)
    kt = _tracker(hiplib, ctx, img, half)
    c = kt.detect_candidates(half, nf, gx, gy, th)
    assert np.array_equal(kt.score_map("score"), ref["score"]), "score map"
    assert np.array_equal(kt.score_map("nms"), ref["nms"]), "suppressed map"
    assert np.array_equal(c["xy"], ref["xy"]) and np.array_equal(c["response"], ref["response"]) and np.array_equal(c["cell"], ref["cell"])
    c2 = kt.detect_candidates(half, nf, gx, gy, th)
    for k in c:
        assert c[k].tobytes() == c2[k].tobytes(), "two runs differ in %s" % k
    if not half and cid in fast_cases.REFINED:
        r = fast_cases.compare_refined(cid, c["refined"])
        print("%s: worst |device - restatement| %.3e px (bound %.3e), near the stop threshold %s (worst %.3e), left out %s" % (
            cid, r["worst"], r["bound"], r["near_stop"], r["worst_near_stop"], r["left_out"]))
        assert not r["failures"], r["failures"]
    if not half and cid in fast_cases.COARSE:
        r = fast_cases.compare_coarse(cid, c["refined"])
        print("%s: %d points, worst |device - restatement| %.3e px (bound %.0e), left out %s" % (cid, len(c["refined"]), r["worst"],
                                                                                                 fast_cases.COARSE_PX, r["left_out"]))
        assert not r["failures"], r["failures"]
    kt.close()


@pytest.mark.parametrize("name", list(fast_cases.probes()))
def test_refinement_probes(hiplib, ctx, name):
    """the branches no detected candidate meets (singular, left the image), through the debug entry "refine": held to the float64
    restatement within four float ulps of the image's largest coordinate; a singular or reverted point returns its start exactly"""
    img, pts = fast_cases.probes()[name]
    xy = np.array(pts, dtype=np.float32)
    kt = _tracker(hiplib, ctx, img)
    got = kt.refine(xy)
    want, rep = fast_ref.corner_subpix(img, xy, patch_dtype=np.float64)
    back = rep["singular"] & (rep["iters"] == 0) | rep["reverted"]
    assert got[back].tobytes() == xy[back].tobytes()
    bound = 4 * float(np.spacing(np.float32(max(img.shape) - 1)))
    err = float(np.abs(got.astype(np.float64) - want).max())
    print("%s: worst |device - restatement| %.3e px (bound %.3e); singular %s, left %s, reverted %s" % (
        name, err, bound, rep["singular"].tolist(), rep["left_image"].tolist(), rep["reverted"].tolist()))
    assert err <= bound
    assert got.tobytes() == kt.refine(xy).tobytes()
    kt.close()


def test_host_logic_through_the_binding(hiplib, ctx):
    hc = fast_cases.host_case()
    img, mask, opts = hc["img"], hc["mask"], hc["opts"]
    rows, cols = img.shape
    kt = _tracker(hiplib, ctx, img, detector=opts)
    for m, pts, ids in ((mask, hc["pts"], hc["ids"]), (None, None, None)):
        kt.currid = 40
        p, i = kt.detect(0, m, pts, ids)
        c = kt.detect_candidates(0)
        z = (np.zeros((0, 2), np.float32), np.zeros(0, np.int64))
        wp, wi, cur, det = fast_ref.perform_detection(cols, rows, lambda: (c["xy"], c["refined"]), m, z[0] if pts is None else pts,
                                                      z[1] if ids is None else ids, opts, 40)
        assert det and kt.currid == cur and np.array_equal(i, wi) and p.tobytes() == wp.tobytes()
    # the 5 % boundary: 19 of 20 kept returns without a detection, 18 detects
    xs, ys = np.meshgrid(np.arange(12, 54, 6), np.arange(12, 38, 6))
    grid = np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.float32) + np.float32(0.25)
    for kept, want in ((19, False), (18, True)):
        p, i = kt.detect(0, None, grid[:kept], np.arange(1, kept + 1))
        assert kt.last_detected == want and np.array_equal(i[:kept], np.arange(1, kept + 1))
    kt.close()


def test_masked_point_uses_up_a_slot_on_the_device_path(hiplib, ctx):
    """the drawn image with the strongest of three equal corners of a K = 2 cell masked: the device returns it (mask-independent),
    KltTracker.detect drops it behind the selection, and the third corner does not move up"""
    img, mask, nf, gx, gy, th = fast_cases.masked_case()
    rows, cols = img.shape
    opts = dict(num_features=nf, grid_x=gx, grid_y=gy, threshold=th, min_px_dist=5)
    kt = _tracker(hiplib, ctx, img, detector=opts)
    c = kt.detect_candidates(0)
    on_mask = mask[c["xy"][:, 1], c["xy"][:, 0]] > 127
    assert on_mask.sum() == 1, "the device's candidates hold the masked corner"
    p, i = kt.detect(0, mask)
    none = (np.zeros((0, 2), np.float32), np.zeros(0, np.int64))
    wp, wi, cur, det = fast_ref.perform_detection(cols, rows, lambda: (c["xy"], c["refined"]), mask, none[0], none[1], opts, 0)
    assert det and np.array_equal(i, wi) and p.tobytes() == wp.tobytes()
    # the restatement on its own candidates: the same ids, and what the mask-before-selection mutant would add is not there
    rp, ri, _ = fast_ref.detect_on_image(img, mask, none[0], none[1], opts)
    mp, mi, _ = fast_ref.detect_on_image(img, mask, none[0], none[1], opts, conv=fast_ref.mutant("mask_before_selection"))
    assert np.array_equal(i, ri) and np.abs(p.astype(np.float64) - rp).max() <= 4 * fast_cases.spread_px("drawn64x48_g2x2_t15")
    assert len(mi) == len(ri) + 1
    kt.close()


def test_loop_seeds_tops_up_and_equals_the_mirror(hiplib, ctx):
    from ov_plane_amd import hostlib

    q = fast_cases.loop_sequence()
    det = q["detector"]
    g = fast_ref.grid(q["width"], q["height"], det["num_features"], det["grid_x"], det["grid_y"])
    most = g["K"] * g["ct_cols"] * g["ct_rows"] + det["num_features"]
    kt = hiplib.KltTracker(ctx, q["width"], q["height"], q["levels"], 15, 256, detector=det)
    seen, per_frame = set(), []
    for f, img in enumerate(q["frames"]):
        before, before_pts, currid = kt.ids_last.copy(), kt.pts_last.copy(), kt.currid
        ids, pts = kt.step(img, q["mask"], detect=True)
        per_frame.append((ids, pts))
        # the restatement's host logic on the device's own candidates of the half the step detected on, from the step's own tracks
        c = kt.detect_candidates(1 if f else 0)
        wp, wi, wcur, wdet = fast_ref.perform_detection(q["width"], q["height"], lambda: (c["xy"], c["refined"]), q["mask"], before_pts, before,
                                                        det, currid)
        assert kt.currid == wcur and kt.last_detected == wdet
        if f == 0:
            assert len(ids) and kt.last_detected and ids[0] == 1, "the first frame seeds"
            assert np.array_equal(ids, wi) and pts.tobytes() == wp.tobytes()
        else:
            top_ids, top_pts = kt.last_topped
            assert np.array_equal(top_ids, wi) and top_pts.tobytes() == wp.tobytes(), "the top-up on the previous half"
            assert np.array_equal(top_ids[:len(np.intersect1d(top_ids, before))], np.intersect1d(top_ids, before)), "the old points keep their order"
            fresh = [i for i in top_ids if i not in seen]
            assert fresh == sorted(fresh) and (not fresh or min(fresh) > max(seen)), "new ids increase and never repeat"
            seen.update(int(i) for i in top_ids)
        seen.update(int(i) for i in ids)
        assert len(ids) <= most
    assert any(len(set(per_frame[f][0]) - set(per_frame[f - 1][0])) for f in range(1, len(per_frame))), "no frame was topped up"
    kt.close()
    cpp = hostlib.run_klt_detect_sequence(q["frames"], q["mask"], det, pyr_levels=q["levels"] - 1, max_points=256)
    for f, (ids, pts) in enumerate(per_frame):
        assert np.array_equal(cpp[f]["ids"], ids) and cpp[f]["pts"].tobytes() == pts.tobytes(), "frame %d" % f


def test_refusals_leave_the_outputs_untouched(hiplib, ctx):
    img, nf, gx, gy, th = fast_cases.CASES["tex64x48_g2x2_t15"]
    h, w = img.shape
    kt = hiplib.KltTracker(ctx, w, h, 1, 15, 64)

    def refused(code, *a, **kw):
        with pytest.raises(hiplib.OvpError) as e:
            kt.detect_candidates(*a, **kw)
        assert e.value.code == code, (e.value.code, code, a, kw)
        n, xy, resp, ref, cell = kt.last_detect_raw
        assert n == -1 and (xy == -1).all() and (resp == -1).all() and (ref == -1.0).all() and (cell == -1).all()
    E_ARG, E_CAP, E_STATE = -1, hiplib.OVP_E_CAPACITY, hiplib.OVP_E_STATE
    refused(E_STATE, 0, nf, gx, gy, th)                  # no image yet
    kt.feed_image(img, "NONE")
    refused(E_STATE, 1, nf, gx, gy, th)                  # no previous half yet
    for bad in ((nf, gx, gy, -1), (nf, gx, gy, 256), (0, gx, gy, th), (nf, 0, gy, th), (nf, gx, 0, th), (4000, w + 1, 2, th), (4000, 2, h + 1, th)):
        refused(E_ARG, 0, *bad)
    refused(E_CAP, 0, 64 * 48, 64, 48, th)               # 3072 cells of one pixel: K cells above max_points
    refused(E_CAP, 0, nf, gx, gy, th, cap=3)             # K cells = 12 above cap
    refused(E_CAP, 0, 300, 1, 1, th)                     # K = 301 above OVP_FAST_MAX_K
    good = kt.detect_candidates(0, nf, gx, gy, th)
    kt.close()
    fresh = _tracker(hiplib, ctx, img)
    want = fresh.detect_candidates(0, nf, gx, gy, th)
    fresh.close()
    for k in good:
        assert good[k].tobytes() == want[k].tobytes(), k
    assert np.array_equal(good["xy"], fast_cases.reference("tex64x48_g2x2_t15")["xy"])
