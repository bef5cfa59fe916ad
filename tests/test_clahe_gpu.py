"""GPU tests of the intake options (ovp_klt_feed_image_opts, ovp_klt_halve, capi.KltTracker.feed_image_opts / halve /
step(intake=), the C++ mirror) against tests/clahe_ref.py: the LUT table, the equalised level 0 and every pyramid level bit-equal
on every case of tests/clahe_cases.py, no pixel excluded; two runs give the same bytes; every mutant of the restatement fails that
comparison on some case; the plain methods through the new entry equal the old one; the halving; the refusals; the loop."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clahe_cases  # noqa: E402
import clahe_ref  # noqa: E402
import klt_cases  # noqa: E402
import klt_ref  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(hiplib):
    c = hiplib.Context(64, 4, 8)
    yield c
    c.close()


def _run(hiplib, ctx, cid):
    """the device's (pyramid, LUT table) of a case, twice; asserts that the two runs give the same bytes"""
    c = clahe_cases.cases()[cid]
    h, w = c["img"].shape
    tx, ty = c["tiles"]
    kt = hiplib.KltTracker(ctx, w, h, c["levels"], 3, 1)
    o = hiplib.intake_defaults(hist_method="CLAHE", clahe_clip=c["clip"], clahe_tiles_x=tx, clahe_tiles_y=ty)
    runs = []
    for _ in range(2):
        kt.feed_image_opts(c["img"], o)
        runs.append(([kt.level(lvl) for lvl in range(c["levels"])], kt.clahe_lut(tx, ty), kt.equalized()))
    kt.close()
    (pyr, lut, eq), (pyr2, lut2, eq2) = runs
    assert clahe_cases.same(lut, lut2) and clahe_cases.same(eq, eq2) and all(clahe_cases.same(a, b) for a, b in zip(pyr, pyr2)), "two runs differ"
    assert clahe_cases.same(eq, pyr[0])
    return pyr, lut


_DEVICE = {}


def _device(hiplib, ctx, cid):
    if cid not in _DEVICE:
        _DEVICE[cid] = _run(hiplib, ctx, cid)
    return _DEVICE[cid]


def _equal(dev, ref):
    (pyr, lut), (rpyr, rlut) = dev, ref
    return clahe_cases.same(lut, rlut) and len(pyr) == len(rpyr) and all(clahe_cases.same(a, b) for a, b in zip(pyr, rpyr))


@pytest.mark.parametrize("cid", clahe_cases.IDS)
def test_lut_table_and_every_level_are_bit_equal(hiplib, ctx, cid):
    pyr, lut = _device(hiplib, ctx, cid)
    rpyr, rlut = clahe_cases.reference(cid)
    assert lut.shape == rlut.shape
    assert np.array_equal(lut, rlut), "LUT table: tiles %s differ" % np.argwhere((lut != rlut).any(axis=2)).tolist()[:8]
    for lvl, (a, b) in enumerate(zip(pyr, rpyr)):
        assert a.shape == b.shape and np.array_equal(a, b), "level %d: %d pixels differ" % (lvl, int((a != b).sum()))


@pytest.mark.parametrize("name", [m for m in clahe_ref.MUTANTS if m != "halve_to_ceil"])
def test_mutant_fails_the_device_comparison(hiplib, ctx, name):
    caught = [cid for cid in clahe_cases.SMALL if not _equal(_device(hiplib, ctx, cid), clahe_cases.reference(cid, name))]
    print("%s: the device differs from the mutant on %d cases: %s" % (name, len(caught), caught[:5]))
    assert caught, "the device equals the mutant %s on every case" % name


def test_plain_methods_through_the_new_entry_equal_the_old_one(hiplib, ctx):
    wide = np.random.default_rng(3).integers(0, 256, size=(31, 64)).astype(np.uint8)
    for img, levels in ((klt_cases.scene("rot2_47x31").img0, 3), (wide[:, 3:50], 3), (klt_cases.scene("subpixel_64x48").img0, 6)):
        h, w = img.shape
        kt = hiplib.KltTracker(ctx, w, h, levels, 3, 1)
        for hist in ("NONE", "HISTOGRAM"):
            kt.feed_image(img, hist)
            old = [kt.level(lvl) for lvl in range(levels)]
            kt.feed_image(255 - np.ascontiguousarray(img), hist)   # (something else into the other half and back: nothing is left over)
            kt.feed_image_opts(img, hiplib.intake_defaults(hist_method=hist))
            new = [kt.level(lvl) for lvl in range(levels)]
            assert all(clahe_cases.same(a, b) for a, b in zip(old, new)), hist
            ref = klt_ref.build_pyramid(np.ascontiguousarray(img), levels, hist)
            assert all(clahe_cases.same(a, b) for a, b in zip(new, ref)), hist
        kt.close()


@pytest.mark.parametrize("key", list(clahe_cases.halving_cases()))
def test_halve_is_bit_equal(hiplib, ctx, key):
    img = clahe_cases.halving_cases()[key]
    kt = hiplib.KltTracker(ctx, 47, 31, 3, 3, 1)   # (the entry takes any size, whatever the tracker's)
    got = kt.halve(img)
    assert clahe_cases.same(got, clahe_ref.halve(img)) and clahe_cases.same(got, kt.halve(img))
    if img.shape[0] % 2 or img.shape[1] % 2:
        assert not clahe_cases.same(got, clahe_ref.halve(img, clahe_ref.mutant("halve_to_ceil")))
    wide = np.zeros((img.shape[0], img.shape[1] + 17), dtype=np.uint8)
    wide[:, 5:5 + img.shape[1]] = img
    assert clahe_cases.same(kt.halve(wide[:, 5:5 + img.shape[1]]), got), "rows further apart than the width"
    kt.close()


@pytest.mark.parametrize("size", [(94, 62), (95, 63)])
@pytest.mark.parametrize("hist", ["CLAHE", "HISTOGRAM", "NONE"])
def test_feed_with_downsample_is_bit_equal(hiplib, ctx, size, hist):
    img = clahe_cases.halving_cases()["%dx%d_texture" % size]
    kt = hiplib.KltTracker(ctx, size[0] // 2, size[1] // 2, 3, 3, 1)
    o = hiplib.intake_defaults(hist_method=hist, downsample=1)
    rpyr, rlut = clahe_ref.intake(img, 3, hist, True)
    for _ in range(2):
        kt.feed_image_opts(img, o)
        for lvl in range(3):
            assert clahe_cases.same(kt.level(lvl), rpyr[lvl]), "level %d" % lvl
        if hist == "CLAHE":
            assert clahe_cases.same(kt.clahe_lut(8, 8), rlut)
    # the same bytes as a feed of the image halved beforehand
    kt.feed_image_opts(kt.halve(img), hiplib.intake_defaults(hist_method=hist))
    assert all(clahe_cases.same(kt.level(lvl), rpyr[lvl]) for lvl in range(3))
    kt.close()


def test_refusals_leave_the_current_half_untouched(hiplib, ctx):
    img = clahe_cases.cases()["47x31_texture_clip10"]["img"]
    big = clahe_cases.halving_cases()["95x63_texture"]
    L = hiplib.lib()
    kt = hiplib.KltTracker(ctx, 47, 31, 3, 3, 1)
    with pytest.raises(hiplib.OvpError) as e:
        kt.clahe_lut(8, 8)
    assert e.value.code == -6   # OVP_E_STATE before a CLAHE feed
    good = hiplib.intake_defaults(hist_method="CLAHE")
    kt.feed_image_opts(img, good)
    before = [kt.level(lvl) for lvl in range(3)], kt.clahe_lut(8, 8)
    other = np.ascontiguousarray(255 - img)

    def refused(src, stride, **over):
        o = hiplib.intake_defaults(**dict(dict(hist_method="CLAHE", src_width=src.shape[1], src_height=src.shape[0]), **over))
        assert L.ovp_klt_feed_image_opts(ctx.handle, src.ctypes.data, stride, ctypes.byref(o)) == -1, over
        now = [kt.level(lvl) for lvl in range(3)], kt.clahe_lut(8, 8)
        assert all(clahe_cases.same(a, b) for a, b in zip(before[0], now[0])) and clahe_cases.same(before[1], now[1]), over

    for over in (dict(clahe_tiles_x=0), dict(clahe_tiles_x=17), dict(clahe_tiles_y=0), dict(clahe_tiles_y=17), dict(clahe_clip=-1.0),
                 dict(clahe_clip=float("nan")), dict(clahe_clip=float("inf")), dict(hist_method=3), dict(hist_method=-1), dict(downsample=2),
                 dict(src_width=46), dict(src_height=32), dict(src_width=0, src_height=0), dict(downsample=1),
                 dict(hist_method="NONE", clahe_tiles_x=0), dict(hist_method="HISTOGRAM", clahe_clip=-1.0)):
        refused(other, 47, **over)
    refused(other, 46)                                             # stride < src_width
    refused(big, 94, downsample=1)                                 # the same with a source that halves to the tracker's size
    refused(big, 95, downsample=1, src_width=96)                   # 96 / 2 is not 47
    refused(np.zeros((63, 1), dtype=np.uint8), 1, downsample=1)    # src_width / 2 < 1
    refused(np.zeros((1, 95), dtype=np.uint8), 95, downsample=1)   # src_height / 2 < 1
    o = hiplib.intake_defaults(hist_method="CLAHE", src_width=47, src_height=31)
    assert L.ovp_klt_feed_image_opts(ctx.handle, None, 47, ctypes.byref(o)) == -1
    assert L.ovp_klt_feed_image_opts(ctx.handle, other.ctypes.data, 47, None) == -1
    now = [kt.level(lvl) for lvl in range(3)], kt.clahe_lut(8, 8)
    assert all(clahe_cases.same(a, b) for a, b in zip(before[0], now[0])) and clahe_cases.same(before[1], now[1])
    # the halving's own refusals leave dst alone
    dst = np.full((31, 47), 7, dtype=np.uint8)
    for args in ((None, 95, 95, 63, dst.ctypes.data), (big.ctypes.data, 95, 95, 63, None), (big.ctypes.data, 94, 95, 63, dst.ctypes.data),
                 (big.ctypes.data, 95, 1, 63, dst.ctypes.data), (big.ctypes.data, 95, 95, 1, dst.ctypes.data)):
        assert L.ovp_klt_halve(ctx.handle, *args) == -1, args
    assert (dst == 7).all()
    # a refused call is not a fed image: the next good one goes where the refused ones would have gone
    kt.feed_image_opts(other, good)
    assert clahe_cases.same(kt.level(0, "prev"), before[0][0])
    kt.close()
    assert L.ovp_klt_feed_image_opts(ctx.handle, other.ctypes.data, 47, ctypes.byref(o)) == -6   # OVP_E_STATE without ovp_klt_create
    assert L.ovp_klt_halve(ctx.handle, big.ctypes.data, 95, 95, 63, dst.ctypes.data) == -6


def test_the_old_door_still_refuses_clahe(hiplib, ctx):
    img = clahe_cases.cases()["47x31_texture_clip10"]["img"]
    kt = hiplib.KltTracker(ctx, 47, 31, 3, 3, 1)
    kt.feed_image_opts(img, hiplib.intake_defaults(hist_method="CLAHE"))
    before = kt.level(0)
    with pytest.raises(hiplib.OvpError) as e:
        kt.feed_image(np.ascontiguousarray(255 - img), "CLAHE")
    assert e.value.code == -1 and clahe_cases.same(kt.level(0), before)
    kt.close()


@pytest.mark.parametrize("downsample", [False, True])
def test_step_with_an_intake_equals_the_mirror_and_the_restatement(hiplib, ctx, downsample):
    """three frames of klt_cases' sequence through step(intake=CLAHE, detect=True) and through ov_plane::TrackPlane under
    set_intake (ovph_run_klt_intake_sequence): ids and positions bit-equal; level 0 of every frame is the restatement's"""
    from ov_plane_amd import hostlib
    from ov_plane_amd.build import build_host

    build_host()
    q = clahe_cases.sequence()
    frames, mask = (q["big_frames"], q["big_mask"]) if downsample else (q["frames"], q["mask"])
    o = hiplib.intake_defaults(hist_method="CLAHE", downsample=1 if downsample else 0)
    kt = hiplib.KltTracker(ctx, q["width"], q["height"], q["levels"], klt_cases.WIN, 256, detector=q["detector"])
    per_frame = []
    for f in range(3):
        ids, pts = kt.step(frames[f], mask, detect=True, intake=o)
        per_frame.append((ids, pts))
        rpyr, _ = clahe_ref.intake(frames[f], q["levels"], "CLAHE", downsample)
        assert all(clahe_cases.same(kt.level(lvl), rpyr[lvl]) for lvl in range(q["levels"])), "frame %d" % f
        if downsample:
            assert clahe_cases.same(kt._mask_last, clahe_ref.halve(mask)), "the detector's mask is the halved one"
    kt.close()
    assert len(per_frame[0][0]) >= 10 and len(np.intersect1d(per_frame[0][0], per_frame[2][0])) >= 5, "points are detected and tracked"
    m = q["mask"] if not downsample else clahe_ref.halve(mask)
    for ids, pts in per_frame[1:]:
        xi, yi = pts[:, 0].astype(int), pts[:, 1].astype(int)
        assert not (m[yi, xi] > 127).any()
    cpp = hostlib.run_klt_intake_sequence(frames, mask, q["detector"], hist="CLAHE", downsample=downsample, pyr_levels=q["levels"] - 1,
                                          win=klt_cases.WIN, max_points=256)
    for f, (ids, pts) in enumerate(per_frame):
        assert np.array_equal(cpp[f]["ids"], ids) and cpp[f]["pts"].tobytes() == pts.tobytes(), "frame %d" % f
