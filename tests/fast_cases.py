"""Cases of the detection tests (tests/test_fast_cpu.py, tests/test_fast_gpu.py): images, grids and thresholds at the smallest
sizes each rule of tests/fast_ref.py can go wrong at, drawn patterns that force the branches the textures do not meet, and the
figures the CPU test records for the GPU test."""
import functools

import numpy as np

import fast_ref
import klt_cases

BG = 100


def _stamp(img, x, y, ks, value, centre=None):
    """sets the circle pixels ks of the pixel (x, y) to value (and the pixel itself to centre)"""
    for k in ks:
        dx, dy = fast_ref.CIRCLE[k % 16]
        img[y + dy, x + dx] = value
    if centre is not None:
        img[y, x] = centre


def _line_tip(img, x, y, top, width=2, brighter_right=0):
    """a vertical line of `width` columns from row `top` down to its tip at row y, 200 at the tip and 10 less per row above it, on a
    background of 50; brighter_right: added to the tip's right pixel"""
    for r in range(top, y + 1):
        img[r, x:x + width] = max(200 - 10 * (y - r), 60)
    img[y, x + width - 1] += brighter_right


@functools.lru_cache(maxsize=None)
def drawn_64x48():
    """64 x 48 under a 2 x 2 grid (cells 32 x 24) and threshold 15: one pattern per forced branch of the segment test and of the
    suppression.  Background 100; the line tips stand on a background of 50 inside a box of their own."""
    img = np.full((48, 64), BG, dtype=np.uint8)
    _stamp(img, 8, 8, range(2, 11), 160)           # bright arc of 9, not wrapping
    _stamp(img, 18, 8, range(3, 12), 40)           # dark arc of 9
    _stamp(img, 8, 17, range(12, 21), 170)         # arc 12..15, 0..4: wraps index 15 -> 0
    _stamp(img, 18, 17, range(0, 8), 160)          # exactly 8 contiguous: no corner
    _stamp(img, 26, 8, range(2, 11), BG + 15)      # |diff| == t: no corner
    _stamp(img, 3, 12, range(2, 11), 180)          # a corner on the first tested column (x = 3 of its cell)
    # second cell (x 32..63, y 0..23): three corners of one score: a tie at the K-th place for K = 2
    for cx in (38, 47, 56):
        _stamp(img, cx, 6, range(2, 11), 150)
    # third cell (x 0..31, y 24..47): a line tip of two equal pixels - neighbours of one score, both suppressed
    img[26:46, 4:30] = 50
    _line_tip(img, 10, 40, 30)
    # fourth cell (x 32..63, y 24..47): a line tip whose left pixel is on the last tested column of the third cell (x = 28) and whose
    # right, brighter one on the untested x = 29: the stronger neighbour is never scored, the corner is kept
    img[26:46, 30] = 50
    _line_tip(img, 28, 36, 29, brighter_right=10)
    return img


@functools.lru_cache(maxsize=None)
def drawn_strip_64x48():
    """under the 5 x 3 grid (cells 12 x 16, the columns 60..63 in no cell): a corner in the strip, one in a cell, and a 0 / 255 one
    that survives threshold 254"""
    img = np.full((48, 64), BG, dtype=np.uint8)
    _stamp(img, 60, 20, range(2, 11), 170)
    _stamp(img, 30, 8, range(2, 11), 170)
    _stamp(img, 18, 24, range(0, 12), 255, centre=0)
    return img


@functools.lru_cache(maxsize=None)
def drawn_21x14():
    """3 x 2 cells of exactly 7 x 7: one testable pixel each; corners at two of them"""
    img = np.full((14, 21), BG, dtype=np.uint8)
    _stamp(img, 3, 3, range(2, 11), 160)
    _stamp(img, 17, 10, range(5, 15), 30)
    return img


@functools.lru_cache(maxsize=None)
def drawn_50x40():
    rng = np.random.default_rng(5)
    return rng.integers(0, 256, size=(40, 50)).astype(np.uint8)


def _tex(name):
    return klt_cases.scene(name).img0


@functools.lru_cache(maxsize=None)
def big():
    return klt_cases.scene("trans12_752x480").img0


# id -> (image, num_features, grid_x, grid_y, threshold)
def _table():
    t = {
        "tex47x31_g2x2_t15": (_tex("rot2_47x31"), 8, 2, 2, 15),
        "tex64x48_g1x1_t15": (_tex("subpixel_64x48"), 6, 1, 1, 15),
        "tex64x48_g2x2_t15": (_tex("subpixel_64x48"), 8, 2, 2, 15),
        "tex64x48_g5x3_t0": (_tex("subpixel_64x48"), 30, 5, 3, 0),
        "tex64x48_g9x7_t15": (_tex("subpixel_64x48"), 63, 9, 7, 15),       # cells 7 x 6: nothing
        "tex64x48_regrid_t15": (_tex("subpixel_64x48"), 6, 5, 3, 15),      # 6 < 15: regridded to 4 x 2
        "drawn64x48_g2x2_t15": (drawn_64x48(), 4, 2, 2, 15),
        "strip64x48_g5x3_t15": (drawn_strip_64x48(), 15, 5, 3, 15),
        "strip64x48_g5x3_t254": (drawn_strip_64x48(), 15, 5, 3, 254),
        "strip64x48_g5x3_t255": (drawn_strip_64x48(), 15, 5, 3, 255),
        "drawn21x14_g3x2_t15": (drawn_21x14(), 6, 3, 2, 15),
        "noise50x40_g20x20_t15": (drawn_50x40(), 400, 20, 20, 15),        # cells 2 x 2, ct_cols = 25 > 20
        "noise50x40_g2x2_t15": (drawn_50x40(), 8, 2, 2, 15),
        "constant64x48": (np.full((48, 64), 77, dtype=np.uint8), 8, 2, 2, 15),
        "sim_752x480": (big(), 250, 20, 20, 15),
        "euroc_752x480": (big(), 200, 12, 12, 15),
        "rpng_752x480": (big(), 200, 12, 12, 30),
    }
    return t


CASES = _table()
IDS = list(CASES)
SMALL = [k for k in IDS if not k.endswith("752x480")]
# the cases whose refined positions are compared (those with candidates)
# the cases whose refined positions are compared: those with candidates that hold the cap on points near a decision (2 %, 1 point
# below 50 points: klt_cases.near_cap) under the restatement's own variants.  Not among them for that reason: tex64x48_g5x3_t0
# (5 of 41 near the stop threshold), sim_752x480 and euroc_752x480 (half of their points wander for 20 iterations on the smooth
# texture; the variants then differ by up to 3e-4 px and a third of the points sit within that of the stop threshold).
REFINED = ["tex47x31_g2x2_t15", "tex64x48_g1x1_t15", "tex64x48_g2x2_t15", "drawn64x48_g2x2_t15", "noise50x40_g2x2_t15", "rpng_752x480"]

# ---- figures recorded by tests/test_fast_cpu.py (measured on the CPU): per case the largest difference of a refined position
# among the restatement's variants - float64 patch arithmetic, float32 patch with numpy's summation order, forward and reverse
# order - over the points away from a decision, in px.  The GPU test allows four times it.  test_fast_cpu.py re-measures each to
# within +0.1 % / -5 %.
SPREAD_PX = {
    "tex47x31_g2x2_t15": 3.815e-06,    # 5 points, 0 near the stop threshold, 0 left out
    "tex64x48_g1x1_t15": 7.630e-06,    # 7 points, 1 near the stop threshold, 0 left out
    "tex64x48_g2x2_t15": 7.630e-06,    # 9 points, 0, 0
    "drawn64x48_g2x2_t15": 9.537e-07,  # 6 points, 0, 0
    "noise50x40_g2x2_t15": 3.815e-06,  # 12 points, 0, 0
    "rpng_752x480": 0.0,               # 2 points, 0, 0
}


def spread_floor_px(cid):
    """one float ulp of the image's largest coordinate: positions are floats, a spread below their spacing is taken as it"""
    return float(np.spacing(np.float32(max(CASES[cid][0].shape) - 1)))


@functools.lru_cache(maxsize=None)
def reference(cid):
    """the restatement's run of a case (mask-independent, as the device's entry), computed once and shared"""
    img, nf, gx, gy, th = CASES[cid]
    return fast_ref.detect_candidates(img, nf, gx, gy, th)


@functools.lru_cache(maxsize=None)
def variants(cid):
    """the refined positions of a case's candidates under the four variants -> dict(name: (pts, report))"""
    img = CASES[cid][0]
    xy = reference(cid)["xy"].astype(np.float32)
    return {
        "f64": fast_ref.corner_subpix(img, xy, patch_dtype=np.float64),
        "f32_numpy": fast_ref.corner_subpix(img, xy, patch_dtype=np.float32, order="numpy"),
        "f32_forward": fast_ref.corner_subpix(img, xy, patch_dtype=np.float32, order="forward"),
        "f32_reverse": fast_ref.corner_subpix(img, xy, patch_dtype=np.float32, order="reverse"),
    }


def measure_spread(cid):
    """(spread px over the points away from a decision, relative spread) among the variants, against the float64 one"""
    v = variants(cid)
    base = v["f64"][1]["unreverted"].astype(np.float64)
    d = np.zeros(len(base))
    for k in ("f32_numpy", "f32_forward", "f32_reverse"):
        with np.errstate(all="ignore"):
            d = np.maximum(d, np.nan_to_num(np.abs(v[k][1]["unreverted"].astype(np.float64) - base).max(axis=1), nan=np.inf, posinf=np.inf))
    return d


def near_decision(cid, spread_px):
    """(near_stop [n], near_other [n]) of the float64 restatement's run: a point whose last squared step lies within the relative
    spread of the stop threshold (the step is about 1e-3 px there: a spread of s px moves its square by 2e-3 s), and a point
    whose unreverted result lies within the spread of the 5 px rule or of the image's edge"""
    img = CASES[cid][0]
    rows, cols = img.shape
    rep = variants(cid)["f64"][1]
    s2 = rep["last_step2"]
    margin = 4 * spread_px
    with np.errstate(all="ignore"):
        step = np.sqrt(s2)
        near_stop = np.abs(step - 1e-3) <= margin
        u = rep["unreverted"].astype(np.float64)
        start = reference(cid)["xy"].astype(np.float64)
        off = np.abs(u - start)
        near_rev = (np.abs(off - 5.0) <= margin).any(axis=1)
        near_edge = (np.abs(u[:, 0]) <= margin) | (np.abs(u[:, 0] - cols) <= margin) | (np.abs(u[:, 1]) <= margin) | (np.abs(u[:, 1] - rows) <= margin)
    return near_stop, (near_rev | near_edge | ~np.isfinite(u).all(axis=1)) & ~near_stop


def spread_px(cid):
    return max(SPREAD_PX[cid], spread_floor_px(cid))


def compare_refined(cid, refined):
    """what the GPU test asserts of the refined positions of a case -> dict(failures, worst, bound, near_stop, left_out)"""
    ref = variants(cid)["f64"][0].astype(np.float64)
    spread = spread_px(cid)
    ns, other = near_decision(cid, spread)
    sure = ~ns & ~other
    err = np.abs(np.asarray(refined, dtype=np.float64) - ref).max(axis=1) if len(ref) else np.zeros(0)
    worst = float(err[sure].max()) if sure.any() else 0.0
    worst_ns = float(err[ns].max()) if ns.any() else 0.0
    fails = []
    if not worst <= 4 * spread:
        fails.append("refined position %.3e px off, bound %.3e (point %d)" % (worst, 4 * spread, int(np.argmax(np.where(sure, err, -1)))))
    if not worst_ns <= 1e-3:
        fails.append("refined position of a point near the stop threshold %.3e px off, bound 1e-3" % worst_ns)
    if ns.sum() + other.sum() > klt_cases.near_cap(len(ref)):
        fails.append("%d points near a decision, cap %d" % (ns.sum() + other.sum(), klt_cases.near_cap(len(ref))))
    return dict(failures=fails, worst=worst, bound=4 * spread, worst_near_stop=worst_ns, near_stop=np.nonzero(ns)[0].tolist(),
                left_out=np.nonzero(other)[0].tolist())


# ---- probes of the refinement ----
@functools.lru_cache(maxsize=None)
def probes():
    """starting positions for the refinement branches no candidate meets -> {name: (image, points)}: singular (a flat patch, a
    pure edge), left the image and reverted (a nearly singular edge near the border: one step of 9 px), and a determinant between
    DBL_EPSILON^2 and DBL_EPSILON: a black image with one grey level at (23, 16) and at (16, 23), one pixel beyond the 13 x 13
    patch of the pixel (16, 16); from 2^-14 px beside that pixel the bilinear weights let 6e-5 of each into the patch's last
    column and row, the only two gradients of the window are (6e-5, 0) and (0, 6e-5), and det = w^2 g^4 is about 1e-19"""
    tiny = np.zeros((40, 40), dtype=np.uint8)
    tiny[16, 23] = tiny[23, 16] = 1
    flat = np.full((32, 32), 90, dtype=np.uint8)
    edge = np.full((32, 32), 50, dtype=np.uint8)
    edge[:, 16:] = 200                       # a vertical edge: every gradient along x, det = 0
    noisy_edge = np.full((16, 16), 50, dtype=np.int64)   # an edge with one grey level of noise: nearly singular, a step of 9 px
    noisy_edge[:, 3:] = 200
    noisy_edge = (noisy_edge + np.random.default_rng(1).integers(0, 2, size=(16, 16))).astype(np.uint8)
    return {"noisy_edge": (noisy_edge, [[1.0, 13.0]]), "flat": (flat, [[10.0, 10.0]]), "edge": (edge, [[15.0, 12.0]]),
            "tiny_det": (tiny, [[16.0 + 2.0 ** -14, 16.0 + 2.0 ** -14]])}


def masked_case():
    """the drawn image with the strongest corner of the tie cell masked: the masked point uses up one of the K = 2 slots
    -> (image, mask, num_features, grid_x, grid_y, threshold)"""
    img, nf, gx, gy, th = CASES["drawn64x48_g2x2_t15"]
    mask = np.zeros(img.shape, dtype=np.uint8)
    mask[4:9, 36:41] = 255
    return img, mask, nf, gx, gy, th


# the 752 x 480 cases whose refined positions are held to the coarse bound below instead of compare_refined
COARSE = ["sim_752x480", "euroc_752x480"]
COARSE_PX = 1e-3


def compare_coarse(cid, refined):
    """the 752 x 480 cases that miss the near-decision cap (REFINED above says why) are still refined on the device, some 250
    points over 64 and more workgroups of k_fast_subpix: every point is held to the float64 restatement within 1e-3 px, the
    stage's own stopping step - the tolerance the issue gives a point near the stop threshold, which is what keeps these cases
    out of REFINED; the restatement's own variants differ by at most 3e-4 px there.  Left out: points whose unreverted result lies
    within that bound of the 5 px revert rule or of the image's edge, where 1e-3 px decides between the start and the result.
    -> dict(failures, worst, left_out)"""
    img = CASES[cid][0]
    rows, cols = img.shape
    want, rep = variants(cid)["f64"]
    u = rep["unreverted"].astype(np.float64)
    start = reference(cid)["xy"].astype(np.float64)
    with np.errstate(all="ignore"):
        off = np.abs(u - start)
        out = (np.abs(off - 5.0) <= COARSE_PX).any(axis=1) | ~np.isfinite(u).all(axis=1)
        out |= (np.abs(u[:, 0]) <= COARSE_PX) | (np.abs(u[:, 0] - cols) <= COARSE_PX) | (np.abs(u[:, 1]) <= COARSE_PX) | (np.abs(u[:, 1] - rows) <= COARSE_PX)
    err = np.abs(np.asarray(refined, dtype=np.float64) - want.astype(np.float64)).max(axis=1)
    worst = float(err[~out].max())
    fails = [] if worst <= COARSE_PX else ["refined position %.3e px off, bound %.0e (point %d)" % (worst, COARSE_PX, int(np.argmax(np.where(out, -1, err))))]
    if out.sum() > klt_cases.near_cap(len(err)):
        fails.append("%d points left out, cap %d" % (out.sum(), klt_cases.near_cap(len(err))))
    return dict(failures=fails, worst=worst, left_out=np.nonzero(out)[0].tolist())


# ---- host logic ------------------------------------------------------------------------------------------------------------------
HOST_OPTS = dict(num_features=20, grid_x=2, grid_y=2, threshold=15, min_px_dist=5)


@functools.lru_cache(maxsize=None)
def host_case():
    """64 x 48 texture; existing points: one within 10 px of the border, two in one occupancy cell, one on the mask, one whose
    rectangle does not fit, regular ones; a mask rectangle"""
    img = _tex("subpixel_64x48")
    mask = np.zeros((48, 64), dtype=np.uint8)
    mask[10:20, 40:50] = 255
    pts = np.array([[5.2, 20.1], [21.3, 22.4], [22.6, 23.9], [44.0, 15.0], [12.5, 30.5], [30.7, 30.2], [50.1, 36.8], [63.0, 47.0]], dtype=np.float32)
    ids = np.array([3, 5, 6, 9, 11, 12, 14, 17], dtype=np.int64)
    return dict(img=img, mask=mask, pts=pts, ids=ids, opts=dict(HOST_OPTS))


@functools.lru_cache(maxsize=None)
def loop_sequence():
    """four 64 x 48 frames of one texture, 2 px to the right per frame"""
    width, height = 64, 48
    sample = klt_cases.texture(width, height, 33)
    frames = [klt_cases.render(sample, width, height, klt_cases.homography(width, height, t=(k * 0.139, 0.0, 0.0)) if k else None) for k in range(4)]
    mask = np.zeros((height, width), dtype=np.uint8)
    mask[0:12, 0:20] = 255
    return dict(frames=np.stack(frames), mask=mask, levels=3, width=width, height=height,
                detector=dict(num_features=12, grid_x=3, grid_y=2, threshold=10, min_px_dist=6))
