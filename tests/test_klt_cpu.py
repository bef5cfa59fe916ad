"""CPU tests of the KLT stage's yardstick (tests/klt_ref.py, tests/klt_cases.py) and of the library's boundary: the restatement
against independent statements of pyrDown and equalizeHist, the float64 Lucas-Kanade against the scenes' closed form, the figures
klt_cases.py records for the GPU test, and the new symbols; the window cases (every window width, all four k_klt_track
instantiations): their caps and recorded figures, the branches they take, and the mutants of the restatement - one convention
changed at a time - that the GPU test's comparison must catch in every instantiation."""
import contextlib
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


# ---- the restatement reports what it did: not one bit of (pts, status, near, iters) has moved ------------------------------------
def _parent_bilinear(read, ix, iy, a, b, win, T):
    r = np.arange(win)
    X = ix[:, None, None] + r[None, None, :] + np.zeros((1, win, 1), dtype=np.int64)
    Y = iy[:, None, None] + r[None, :, None] + np.zeros((1, 1, win), dtype=np.int64)
    a, b = a[:, None, None], b[:, None, None]
    one = T(1)
    w00, w01, w10, w11 = (one - a) * (one - b), a * (one - b), (one - a) * b, a * b
    return w00 * read(X, Y) + w01 * read(X + 1, Y) + w10 * read(X, Y + 1) + w11 * read(X + 1, Y + 1)


def _parent_lk_track(pyr_prev, pyr_cur, pts_prev, guess=None, win=15, dtype=np.float64):
    """klt_ref.lk_track as it stood before it reported its branches, statement for statement (kept here for the comparison below)"""
    R = klt_ref
    T = dtype
    pts_prev = np.asarray(pts_prev, dtype=np.float32).reshape(-1, 2)
    guess = pts_prev if guess is None else np.asarray(guess, dtype=np.float32).reshape(-1, 2)
    n, nl = len(pts_prev), len(pyr_prev)
    top = nl - 1
    alive = np.isfinite(pts_prev).all(axis=1) & np.isfinite(guess).all(axis=1)
    status = alive.astype(np.uint8)
    near = np.zeros(n, dtype=bool)
    iters = np.zeros((n, nl), dtype=np.int32)
    P = np.where(alive[:, None], pts_prev, 0).astype(T)
    with np.errstate(over="ignore", invalid="ignore"):
        g = np.where(alive[:, None], guess, 0).astype(T) * T(1.0 / (1 << top))
    half = T((win - 1) * 0.5)
    for lvl in range(top, -1, -1):
        with np.errstate(over="ignore", invalid="ignore"):
            if lvl != top:
                g = g * T(2)
        I8, J8 = pyr_prev[lvl], pyr_cur[lvl]
        rows, cols = I8.shape
        pw = P * T(1.0 / (1 << lvl)) - half
        ins = R._inside(pw, win, cols, rows)
        near |= alive & R._near_corner(pw, win, cols, rows)
        if lvl == 0:
            status[alive & ~ins] = 0
        act = np.nonzero(alive & ins)[0]
        if len(act) == 0:
            continue
        gx, gy = R.scharr(I8, T)
        fl = np.floor(pw[act])
        ip = fl.astype(np.int64)
        a, b = (pw[act] - fl)[:, 0], (pw[act] - fl)[:, 1]
        Iw = _parent_bilinear(R._img_reader(I8, T), ip[:, 0], ip[:, 1], a, b, win, T)
        Ix = _parent_bilinear(R._grad_reader(gx), ip[:, 0], ip[:, 1], a, b, win, T)
        Iy = _parent_bilinear(R._grad_reader(gy), ip[:, 0], ip[:, 1], a, b, win, T)
        sc = T(1.0 / R.GATE_SCALE)
        A11, A12, A22 = (Ix * Ix).sum(axis=(1, 2)) * sc, (Ix * Iy).sum(axis=(1, 2)) * sc, (Iy * Iy).sum(axis=(1, 2)) * sc
        D = A11 * A22 - A12 * A12
        min_eig = (A22 + A11 - np.sqrt((A11 - A22) * (A11 - A22) + T(4) * A12 * A12)) / T(2 * win * win)
        bad = (min_eig < T(R.MIN_EIG_THRESHOLD)) | (D < T(R.FLT_EPSILON))
        near[act] |= (np.abs(min_eig.astype(np.float64) / R.MIN_EIG_THRESHOLD - 1) < R.NEAR_GATE_REL) | \
                     (np.abs(D.astype(np.float64) / R.FLT_EPSILON - 1) < R.NEAR_GATE_REL)
        if lvl == 0:
            status[act[bad]] = 0
        keep = ~bad
        act, Iw, Ix, Iy, A11, A12, A22, D = act[keep], Iw[keep], Ix[keep], Iy[keep], A11[keep], A12[keep], A22[keep], D[keep]
        v = g[act] - half
        run = np.ones(len(act), dtype=bool)
        pd = np.zeros((len(act), 2), dtype=T)
        Jr = R._img_reader(J8, T)
        for j in range(R.MAX_ITERS):
            if not run.any():
                break
            ins = R._inside(v, win, cols, rows)
            near[act[run]] |= R._near_corner(v[run], win, cols, rows)
            out = run & ~ins
            if lvl == 0:
                status[act[out]] = 0
            run = run & ins
            k = np.nonzero(run)[0]
            if len(k) == 0:
                break
            iters[act[k], lvl] += 1
            fl = np.floor(v[k])
            iq = fl.astype(np.int64)
            Jw = _parent_bilinear(Jr, iq[:, 0], iq[:, 1], (v[k] - fl)[:, 0], (v[k] - fl)[:, 1], win, T)
            diff = Jw - Iw[k]
            b1, b2 = (diff * Ix[k]).sum(axis=(1, 2)) * sc, (diff * Iy[k]).sum(axis=(1, 2)) * sc
            d = np.stack([(A12[k] * b2 - A22[k] * b1) / D[k], (A12[k] * b1 - A11[k] * b2) / D[k]], axis=1)
            v[k] = v[k] + d
            stop = (d * d).sum(axis=1) <= T(R.STOP_EPS * R.STOP_EPS)
            s = np.abs(d + pd[k])
            osc = (j > 0) & ~stop & (s[:, 0] < T(R.OSC_EPS)) & (s[:, 1] < T(R.OSC_EPS))
            if j > 0:
                near[act[k]] |= ~stop & (np.abs(s.astype(np.float64).max(axis=1) - R.OSC_EPS) < R.NEAR_OSC)
            v[k[osc]] = v[k[osc]] - d[osc] * T(0.5)
            pd[k] = d
            run[k[stop | osc]] = False
        g[act] = v + half
    return g, status, dict(near=near, iters=iters)


@pytest.mark.parametrize("name", klt_cases.NAMES)
def test_lk_track_with_its_report_is_the_parents_bit_for_bit(name):
    sc = klt_cases.scene(name)
    for T in (np.float64, np.float32):
        p, st, rep = sc.reference(T)
        q, sq, rq = _parent_lk_track(*sc.pyramids, sc.pts, sc.guess, klt_cases.WIN, T)
        assert p.dtype == q.dtype and p.tobytes() == q.tobytes() and st.tobytes() == sq.tobytes()
        assert rep["near"].tobytes() == rq["near"].tobytes() and rep["iters"].tobytes() == rq["iters"].tobytes()


# ---- window cases ----------------------------------------------------------------------------------------------------------------
FLAGS = ("osc", "exhausted", "gate_upper", "gate_l0", "left_upper", "left_l0", "left_in_loop", "neg_corner", "border_grad")


def test_window_table_covers_every_width_and_instantiation():
    by_win, by_inst = {}, {}
    for name, levels, win, *_ in klt_cases.WINDOW_CASES:
        by_win.setdefault(win, set()).add(name)
        by_inst.setdefault(klt_cases.instantiation(win), []).append((name, levels, win))
    assert sorted(by_win) == list(range(3, 22, 2))
    assert all(len(v) >= 2 for v in by_win.values()), "a width on one scene only"
    assert sorted(by_inst) == [1, 2, 4, 7] and all(len(v) >= 3 for v in by_inst.values())
    assert {klt_cases.instantiation(w) for w in (3, 5, 7)} == {1} and {klt_cases.instantiation(w) for w in (9, 11)} == {2}
    assert {klt_cases.instantiation(w) for w in (13, 15)} == {4} and {klt_cases.instantiation(w) for w in (17, 19, 21)} == {7}
    deep = {(n, l, w) for n, l, w, *_ in klt_cases.WINDOW_CASES}
    assert ("subpixel_64x48", 6, 3) in deep and ("subpixel_64x48", 6, 21) in deep and any(n == "rot2_47x31" and l == 5 for n, l, _ in deep)
    assert klt_cases.case("subpixel_64x48-L6-w21").pyramids[0][-1].shape == (2, 2)
    assert klt_cases.case("rot2_47x31-L5-w21").pyramids[0][-1].shape == (2, 3)
    assert set(klt_cases.SPREAD_PX) == set(klt_cases.CASE_IDS)


@pytest.mark.parametrize("cid", klt_cases.CASE_IDS)
def test_window_case_caps_and_recorded_spread(cid):
    c = klt_cases.case(cid)
    p64, s64, r64 = c.reference(np.float64)
    p32, s32, r32 = c.reference(np.float32)
    n, near, ns = len(s64), r64["near"], r64["near_stop"]
    cap = klt_cases.near_cap(n)
    print("%s: %d points, near %d, near_stop %d (cap %d each)" % (cid, n, near.sum(), ns.sum(), cap))
    assert near.sum() <= cap and ns.sum() <= cap
    assert np.array_equal(s32[~near], s64[~near]), "float32 and float64 differ in status outside near"
    sure = ~(near | ns)
    assert np.array_equal(r32["iters"][sure], r64["iters"][sure]), "float32 and float64 differ in iterations outside near | near_stop"
    ok = (s64 == 1) & sure
    worst = float(np.abs(p64[ok] - p32[ok].astype(np.float64)).max())
    rec = klt_cases.SPREAD_PX[cid]
    print("%s: float32 - float64 spread %.3e px over %d points, recorded %.3e" % (cid, worst, ok.sum(), rec))
    assert worst <= rec * (1 + 1e-3) and rec <= 1.05 * worst
    assert 4 * rec < klt_ref.STOP_EPS / 10, "the bound is no longer far below a stopping step"
    # the unmutated float32 run passes what the GPU test asks of the device
    res = klt_cases.compare(c, p32, s32, r32["iters"])
    assert not res["failures"], res["failures"]


def _reversed_window(win):
    k = np.arange(win * win)[::-1]
    return k // win, k % win


@pytest.mark.parametrize("inst", (1, 2, 4, 7))
def test_float32_in_another_summation_order_passes_every_window_case(inst, monkeypatch):
    """the device sums a window lane by lane and through a butterfly: a float32 run that sums it backwards stands in for that"""
    monkeypatch.setattr(klt_ref, "_window", _reversed_window)
    for cid in klt_cases.CASE_IDS:
        c = klt_cases.case(cid)
        if klt_cases.instantiation(c.win) != inst:
            continue
        c.reference(np.float64)
        p, st, rep = klt_ref.lk_track(*c.pyramids, c.pts, c.guess, c.win, np.float32)
        res = klt_cases.compare(c, p, st, rep["iters"])
        print("%s: worst %.3e px of %.3e" % (cid, res["worst"], res["bound"]))
        assert not res["failures"], (cid, res["failures"])


def test_near_stop_margin_is_the_measured_one():
    worst, E = 0.0, klt_ref.STOP_EPS
    for cid in klt_cases.CASE_IDS:
        c = klt_cases.case(cid)
        _, s64, r64 = c.reference(np.float64)
        _, _, r32 = c.reference(np.float32)
        d64, d32 = r64["dnorm"][:, 0], r32["dnorm"][:, 0]
        with np.errstate(invalid="ignore"):
            m = (s64 == 1) & ~r64["near"] & (r64["iters"] == r32["iters"]).all(axis=1) & (r64["iters"][:, 0] > 0) & (d64 <= E) & (d32 <= E)
        if m.any():
            worst = max(worst, float(np.abs(d64[m] - d32[m]).max() / E))
    rec = klt_ref.NEAR_STOP_MEASURED
    print("largest float32 - float64 difference of |delta| / STOP_EPS where level 0 stopped: %.4e, recorded %.4e" % (worst, rec))
    assert worst <= rec * (1 + 1e-3) and rec <= 1.05 * worst
    assert klt_ref.NEAR_STOP_REL == 4 * rec


def test_branch_table():
    """every branch of k_klt_track's loop is taken by at least two points outside `near` in at least one case of each instantiation"""
    table = {}
    print("%-28s %s" % ("case (points outside near)", " ".join("%12s" % f for f in FLAGS)))
    for cid in klt_cases.CASE_IDS:
        c = klt_cases.case(cid)
        rep = c.reference(np.float64)[2]
        counts = [int(((rep[f] > 0) & ~rep["near"]).sum()) for f in FLAGS]
        print("%-28s %s" % ("<%d> %s" % (klt_cases.instantiation(c.win), cid), " ".join("%12d" % k for k in counts)))
        row = table.setdefault(klt_cases.instantiation(c.win), dict.fromkeys(FLAGS, 0))
        for f, k in zip(FLAGS, counts):
            if f in ("gate_l0", "left_l0") and not cid.startswith("mixed3px"):
                continue  # (these two are asked of the mixed scene's flat patch, border, outside and far-guess points)
            row[f] = max(row[f], k)
    for inst in (1, 2, 4, 7):
        missing = [f for f in FLAGS if table[inst][f] < 2]
        assert not missing, "instantiation <%d>: no case takes %s on two points" % (inst, missing)
    # the floats OpenCV would truncate: a negative corner is floored (the restatement's own arithmetic on such a corner)
    assert klt_ref._corner_floor(np.array([-0.25]))[0] == -1.0


# ---- mutants: one convention of the restatement changed; the GPU test's comparison must notice in every instantiation -------------
_REFLECT = klt_ref.reflect101


def _grad_reader_reflecting(g):
    h, w = g.shape
    return lambda X, Y: g[_REFLECT(Y, h), _REFLECT(X, w)]


def _window_less_last_slot(win):
    k = np.arange(64 * (win * win // 64))
    return k // win, k % win


def _window_one_more(win):
    k = np.arange(win * win + 1)
    return k // win, k % win


def _window_cur_swapped(win):
    r, c = klt_ref._window(win)
    return c, r


MUTANTS = {
    "a_sobel_for_scharr": dict(SCHARR_SMOOTH=(1, 2, 1), SCHARR_NORM=8.0),
    "b_gradient_reads_reflect": dict(_grad_reader=_grad_reader_reflecting),
    "c_image_reads_clamp": dict(reflect101=lambda i, n: np.clip(np.asarray(i, dtype=np.int64), 0, n - 1)),
    "d_no_back_step": dict(OSC_BACK=0.0),
    "e_oscillation_from_third_iteration": dict(OSC_FROM=2),
    "f_29_iterations": dict(MAX_ITERS=29),
    "g_stop_eps_0.03": dict(STOP_EPS=0.03),
    "h_corner_truncated": dict(_corner_floor=np.trunc),
    "i_top_guess_unscaled": dict(_top_scale=lambda top, T: T(1.0)),
    "j_last_partial_slot_dropped": dict(_window=_window_less_last_slot),
    "k_one_pixel_too_many": dict(_window=_window_one_more),
    # (rows and columns swapped at both sites is the same window: the mutant swaps them where the current image is read)
    "l_row_and_column_swapped": dict(_window_cur=_window_cur_swapped),
}


@contextlib.contextmanager
def _mutated(changes):
    saved = {k: getattr(klt_ref, k) for k in changes}
    try:
        for k, v in changes.items():
            setattr(klt_ref, k, v)
        yield
    finally:
        for k, v in saved.items():
            setattr(klt_ref, k, v)


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_tracking_mutant_is_caught_in_every_instantiation(mutant):
    caught = {}
    for cid in klt_cases.CASE_IDS:
        c = klt_cases.case(cid)
        inst = klt_cases.instantiation(c.win)
        if inst in caught:
            continue
        pyr0, pyr1 = c.pyramids            # (built and the reference run before the convention changes)
        c.reference(np.float64)
        with _mutated(MUTANTS[mutant]):
            p, st, rep = klt_ref.lk_track(pyr0, pyr1, c.pts, c.guess, c.win, np.float64)
        res = klt_cases.compare(c, p, st, rep["iters"])
        if res["failures"]:
            caught[inst] = (cid, res["failures"][0])
    for inst in sorted(caught):
        print("%s: <%d> caught by %s: %s" % (mutant, inst, *caught[inst]))
    assert sorted(caught) == [1, 2, 4, 7], "%s slips through instantiation(s) %s" % (mutant, sorted({1, 2, 4, 7} - set(caught)))


@pytest.mark.parametrize("mutant,changes", [("pyr_round_127", dict(PYR_ROUND=127)), ("lut_truncated", dict(_lut_round=np.floor))])
def test_image_mutant_breaks_bit_equality_on_an_uploaded_image(mutant, changes):
    broken = []
    for key, (img, levels) in klt_cases.image_cases().items():
        if img.size > 1 << 16:
            continue  # (the small images are enough)
        for hist in ("HISTOGRAM", "NONE"):
            ref = klt_ref.build_pyramid(img, levels, hist)
            with _mutated(changes):
                got = klt_ref.build_pyramid(img, levels, hist)
            if any(not np.array_equal(a, b) for a, b in zip(ref, got)):
                broken.append("%s/%s" % (key, hist))
    print("%s breaks %s" % (mutant, broken))
    assert broken


@pytest.mark.parametrize("name", sorted(klt_cases.SCENE_SPREAD_PX))
def test_scene_spread_is_the_recorded_one(name):
    sc = klt_cases.scene(name)
    p64, s64, r64 = sc.reference(np.float64)
    p32, s32, r32 = sc.reference(np.float32)
    sure = ~(r64["near"] | r64["near_stop"])
    assert np.array_equal(r32["iters"][sure], r64["iters"][sure])
    ok = (s64 == 1) & (s32 == 1) & sure
    worst = float(np.abs(p64[ok] - p32[ok].astype(np.float64)).max())
    rec = klt_cases.SCENE_SPREAD_PX[name]
    print("%s: float32 - float64 spread %.3e px outside near | near_stop, recorded %.3e" % (name, worst, rec))
    assert worst <= rec * (1 + 1e-3) and rec <= 1.05 * worst


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
