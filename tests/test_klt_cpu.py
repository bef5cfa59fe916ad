"""CPU tests of the KLT stage's yardstick (tests/klt_ref.py, tests/klt_cases.py) and of the library's boundary: the restatement
against independent statements of pyrDown and equalizeHist, the float64 Lucas-Kanade against the scenes' closed form, the figures
klt_cases.py records for the GPU test, and the new symbols."""
import os
import sys

import numpy as np
import pytest
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import klt_cases  # noqa: E402
import klt_ref  # noqa: E402


def _pyr_down_independent(img):
    k = np.array(klt_ref.PYR_TAPS, dtype=np.int64)
    s = ndimage.correlate1d(img.astype(np.int64), k, axis=1, mode="mirror")
    s = ndimage.correlate1d(s, k, axis=0, mode="mirror")
    return ((s + 128) >> 8)[::2, ::2].astype(np.uint8)


@pytest.mark.parametrize("name", klt_cases.NAMES + ["1x5", "5x1"])
def test_pyr_down_equals_an_independent_statement(name):
    if name in klt_cases.NAMES:
        sc = klt_cases.scene(name)
        imgs = klt_ref.build_pyramid(sc.img0, max(sc.levels, 2), "NONE")[:-1]
    else:
        w, h = (int(v) for v in name.split("x"))
        imgs = [np.random.default_rng(4).integers(0, 256, size=(h, w)).astype(np.uint8)]
    for img in imgs:
        got = klt_ref.pyr_down(img)
        assert got.shape == ((img.shape[0] + 1) // 2, (img.shape[1] + 1) // 2)
        assert np.array_equal(got, _pyr_down_independent(img))


def _equalize_independent(img):
    hist = np.bincount(img.ravel(), minlength=256)
    cdf = np.cumsum(hist)
    first = int(np.argmax(hist > 0))
    if cdf[first] == img.size:
        return img.copy()
    scale = np.float32(255.0) / np.float32(img.size - cdf[first])
    lut = np.clip(np.rint((cdf - cdf[first]).astype(np.float32) * scale), 0, 255).astype(np.uint8)
    return lut[img]


def test_equalize_hist_equals_an_independent_statement():
    rng = np.random.default_rng(8)
    cases = [klt_cases.scene(n).img1 for n in klt_cases.SMALL]
    cases.append(np.full((9, 13), 77, dtype=np.uint8))                              # constant: maps to itself
    cases.append(np.where(rng.random((11, 7)) < 0.3, 40, 200).astype(np.uint8))     # two-valued: -> 0 and 255
    cases.append(rng.integers(100, 140, size=(31, 47)).astype(np.uint8))
    for img in cases:
        assert np.array_equal(klt_ref.equalize_hist(img), _equalize_independent(img))
    assert np.array_equal(klt_ref.equalize_hist(cases[-3]), cases[-3])
    assert sorted(np.unique(klt_ref.equalize_hist(cases[-2])).tolist()) == [0, 255]


@pytest.mark.parametrize("name", klt_cases.NAMES)
def test_lk_float64_recovers_the_closed_form_and_the_recorded_figure_holds(name):
    sc = klt_cases.scene(name)
    p, st, rep = sc.reference(np.float64)
    ok = (st == 1) & sc.regular
    assert ok.sum() == sc.regular.sum(), "a regular point lost its track"
    err = float(np.abs(p[ok] - sc.truth[ok]).max())
    rec = klt_cases.CLOSED_FORM_PX[name]
    print("%s: worst |restatement - closed form| %.5f px over %d points, recorded %.5f" % (name, err, ok.sum(), rec))
    assert err <= rec <= 1.26 * err + 1e-5, "klt_cases.CLOSED_FORM_PX is not this scene's error with 25 %% headroom"
    assert err < 0.6  # LK has found the motion, not a neighbouring minimum
    if name == "mixed3px_96x64":
        n_reg = int(sc.regular.sum())
        assert not st[n_reg:n_reg + 8].any(), "a point on the textureless patch passed the texture gate"
        assert not st[n_reg + 16:].any(), "a point outside the image or with a guess 500 px off kept status 1"


@pytest.mark.parametrize("name", klt_cases.NAMES)
def test_near_decision_exclusion_cap(name):
    sc = klt_cases.scene(name)
    near = sc.reference(np.float64)[2]["near"]
    n = len(near)
    cap = int(0.02 * n) if n >= 50 else 1
    print("%s: %d of %d points near a decision (cap %d)" % (name, near.sum(), n, cap))
    assert near.sum() <= cap


def test_float32_spread_is_the_recorded_one():
    worst = 0.0
    for name in klt_cases.NAMES:
        sc = klt_cases.scene(name)
        p64, s64, _ = sc.reference(np.float64)
        p32, s32, _ = sc.reference(np.float32)
        both = (s64 == 1) & (s32 == 1)
        worst = max(worst, float(np.abs(p64[both] - p32[both].astype(np.float64)).max()))
    print("largest |float32 - float64| of the restatement: %.3e px, recorded %.3e" % (worst, klt_cases.F32_SPREAD_PX))
    assert worst <= klt_cases.F32_SPREAD_PX * (1 + 1e-3) and klt_cases.F32_SPREAD_PX <= 1.05 * worst
    if 4 * klt_cases.F32_SPREAD_PX > 0.02:
        print("FINDING: 4 x F32_SPREAD_PX exceeds 0.02 px - the restatement is ill-conditioned somewhere")


def test_sequence_bookkeeping_drops_the_masked_and_the_leaving_point():
    q = klt_cases.sequence()
    rt = klt_ref.RefTracker(q["width"], q["height"], q["levels"], klt_cases.WIN)
    rt.step(q["frames"][0], q["mask"])
    rt.add_points(q["ids"], q["pts"])
    ids1, _ = rt.step(q["frames"][1], q["mask"])
    assert not rt.near.any()
    ids2, _ = rt.step(q["frames"][2], q["mask"])
    assert not rt.near.any()
    assert 112 not in ids1 and 113 in ids1, "the point that tracks into the mask goes in the second frame"
    assert 113 not in ids2, "the point that leaves the image goes in the third frame"
    assert len(ids2) == 12


def test_library_exports_the_klt_symbols(hiplib):
    L = hiplib.lib()
    for s in ("ovp_klt_create", "ovp_klt_destroy", "ovp_klt_reset", "ovp_klt_feed_image", "ovp_klt_track", "ovp_klt_debug"):
        assert s in hiplib.EXPORTS and hasattr(L, s), s
    assert L.ovp_klt_create(None, 64, 48, 3, 15, 16) == -1  # OVP_E_ARG on a null context
