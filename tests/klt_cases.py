"""Deterministic scenes for the KLT tests: a band-limited random texture of 8-bit range on a plane, seen by two camera poses.  The
second image is the first one's texture resampled through the homography the plane and the two poses induce
(scipy.ndimage.map_coordinates), so every point's true position in the second image is known in closed form.  No BLAS products:
the 3 x 3 algebra is written out."""
import functools

import numpy as np
from scipy import ndimage

import klt_ref

WIN = 15

# ---- figures recorded by tests/test_klt_cpu.py (measured on the CPU, float64 restatement against the closed form, status-1 points
# of a scene's `regular` set; worst per scene with 25 % headroom) - the GPU test uses these, test_klt_cpu.py re-measures them --------
CLOSED_FORM_PX = {
    "subpixel_64x48": 0.03140,
    "rot2_47x31": 0.17717,
    "scale5_96x64_l1": 0.33034,
    "mixed3px_96x64": 0.00106,
    "ramp3px_96x64": 0.59884,
    "trans12_752x480": 0.01011,
}
# largest position difference between the restatement in float32 and in float64 over all scenes (status-1 points of both)
F32_SPREAD_PX = 3.026e-05
# the same per scene over the status-1 points outside near | near_stop, where that sets a sharper bound than F32_SPREAD_PX (not
# trans12_752x480: its worst point is the one F32_SPREAD_PX records)
SCENE_SPREAD_PX = {
    "subpixel_64x48": 3.215e-06,
    "rot2_47x31": 2.724e-06,
    "scale5_96x64_l1": 3.533e-06,
    "mixed3px_96x64": 2.327e-06,
    "ramp3px_96x64": 4.404e-06,
}


def _mat3(a, b):
    return [[sum(a[i][k] * b[k][j] for k in range(3)) for j in range(3)] for i in range(3)]


def _inv3(m):
    (a, b, c), (d, e, f), (g, h, i) = m
    det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)
    return [[(e * i - f * h) / det, (c * h - b * i) / det, (b * f - c * e) / det],
            [(f * g - d * i) / det, (a * i - c * g) / det, (c * d - a * f) / det],
            [(d * h - e * g) / det, (b * g - a * h) / det, (a * e - b * d) / det]]


def homography(width, height, rot_deg=0.0, t=(0.0, 0.0, 0.0), depth=4.0):
    """H = K (R + t n^T / d) K^-1 of the plane z = depth (n = e_z) in front of camera 1, camera 2 = (R about the optical axis, t)"""
    f = 0.9 * width
    K = [[f, 0.0, 0.5 * (width - 1)], [0.0, f, 0.5 * (height - 1)], [0.0, 0.0, 1.0]]
    c, s = np.cos(np.deg2rad(rot_deg)), np.sin(np.deg2rad(rot_deg))
    M = [[c, -s, t[0] / depth], [s, c, t[1] / depth], [0.0, 0.0, 1.0 + t[2] / depth]]
    return _mat3(_mat3(K, M), _inv3(K))


def apply_h(H, xy):
    xy = np.asarray(xy, dtype=np.float64)
    x, y = xy[..., 0], xy[..., 1]
    w = H[2][0] * x + H[2][1] * y + H[2][2]
    return np.stack([(H[0][0] * x + H[0][1] * y + H[0][2]) / w, (H[1][0] * x + H[1][1] * y + H[1][2]) / w], axis=-1)


def texture(width, height, seed, cell=5.0, flat=None):
    """the plane's texture on a canvas with a margin: random values on a coarse grid, cubic-spline interpolated (band-limited at
    `cell` pixels); flat = (x0, y0, x1, y1): a constant patch in image-1 pixels.  Returns sample(xy [.., 2]) -> grey values."""
    rng = np.random.default_rng(seed)
    margin = 40
    octaves = []  # three octaves (cell, 4 cell, 16 cell), equal weights: every pyramid level sees structure at its own scale
    for k in range(3):
        c = cell * 4 ** k
        gw, gh = int((width + 2 * margin) / c) + 4, int((height + 2 * margin) / c) + 4
        octaves.append((c, ndimage.spline_filter(rng.uniform(0.0, 255.0, size=(gh, gw)), order=3, mode="mirror")))

    def sample(xy):
        xy = np.asarray(xy, dtype=np.float64)
        v = 0.0
        for c, coef in octaves:
            gx, gy = (xy[..., 0] + margin) / c + 1.0, (xy[..., 1] + margin) / c + 1.0
            v = v + ndimage.map_coordinates(coef, [gy, gx], order=3, mode="mirror", prefilter=False) / len(octaves)
        if flat is not None:
            x0, y0, x1, y1 = flat
            v = np.where((xy[..., 0] >= x0) & (xy[..., 0] <= x1) & (xy[..., 1] >= y0) & (xy[..., 1] <= y1), 128.0, v)
        return v
    return sample


def render(sample, width, height, H=None, ramp=0.0):
    """the 8-bit image a camera sees: pixel p of the second image shows the texture at H^-1 p"""
    yy, xx = np.mgrid[0:height, 0:width]
    xy = np.stack([xx, yy], axis=-1).astype(np.float64)
    if H is not None:
        xy = apply_h(_inv3(H), xy)
    v = sample(xy)
    if ramp:
        v = v * (1.0 + ramp * (xx / (width - 1.0) - 0.5)) + 20.0 * ramp
    return np.clip(np.rint(0.15 * 255 + 0.7 * v), 0, 255).astype(np.uint8)


def _grid_points(rng, width, height, n, margin):
    """n points on a jittered grid inside the margin (so that no two share a window exactly and none sits on an integer)"""
    cols = int(np.ceil(np.sqrt(n * (width - 2 * margin) / max(height - 2 * margin, 1))))
    rows = int(np.ceil(n / cols))
    xs = margin + (np.arange(cols) + 0.5) * (width - 2 * margin) / cols
    ys = margin + (np.arange(rows) + 0.5) * (height - 2 * margin) / rows
    p = np.stack(np.meshgrid(xs, ys), axis=-1).reshape(-1, 2)[:n]
    return (p + rng.uniform(-0.4, 0.4, size=p.shape)).astype(np.float32)


class Scene:
    def __init__(self, name, width, height, levels, n, seed, rot=0.0, t=(0, 0, 0), ramp=0.0, hist="NONE", mixed=False, cell=5.0):
        self.name, self.width, self.height, self.levels, self.hist = name, width, height, levels, hist
        rng = np.random.default_rng(seed + 1000)
        flat = (60.0, 20.0, 90.0, 50.0) if mixed else None
        sample = texture(width, height, seed, cell=cell, flat=flat)
        self.H = homography(width, height, rot, t)
        self.img0 = render(sample, width, height)
        self.img1 = render(sample, width, height, self.H, ramp)
        n_reg = n - 24 if mixed else n
        pts = _grid_points(rng, 58 if mixed else width, height, n_reg, 11)
        guess = None
        if mixed:
            flat_pts = np.array([[75.0, 35.0]]) + rng.uniform(-3.0, 3.0, size=(8, 2))        # 8 on the textureless patch
            s = rng.uniform(0.2, 2.8, size=8)
            border = np.array([[s[0], 20.3], [95.0 - s[1], 40.6], [30.4, s[2]], [50.7, 63.0 - s[3]],
                               [s[4], s[5]], [95.0 - s[6], 63.0 - s[7]], [44.2, 63.0 - s[0]], [95.0 - s[3], 12.9]])  # 8 within 3 px of a border
            outside = np.array([[-30.5, 20.0], [140.2, 30.0], [40.0, -25.7], [300.0, 500.0]])  # 4 outside the image
            far = _grid_points(rng, 58, height, 4, 14)                                        # 4 with a guess 500 px off the image
            pts = np.concatenate([pts, flat_pts, border, outside, far]).astype(np.float32)
            guess = pts.copy()
            guess[-4:] += np.array([[600.0, 0.0], [-500.0, 0.0], [0.0, 570.0], [-500.0, -500.0]], dtype=np.float32)
        self.pts, self.guess = pts, guess
        self.regular = np.arange(len(pts)) < n_reg    # the points the closed form is asked of
        self.truth = apply_h(self.H, pts.astype(np.float64))

    @functools.cached_property
    def pyramids(self):
        return klt_ref.build_pyramid(self.img0, self.levels, self.hist), klt_ref.build_pyramid(self.img1, self.levels, self.hist)

    @functools.lru_cache(maxsize=None)
    def reference(self, dtype=np.float64, win=WIN):
        """(pts, status, report) of the restatement, computed once and shared (do not write into it)"""
        p, s, r = klt_ref.lk_track(*self.pyramids, self.pts, self.guess, win, dtype)
        for a in (p, s, *r.values()):
            a.setflags(write=False)
        return p, s, r


SPECS = [
    dict(name="subpixel_64x48", width=64, height=48, levels=3, n=65, seed=3, t=(0.0247, -0.0163, 0.0)),
    dict(name="rot2_47x31", width=47, height=31, levels=3, n=20, seed=5, rot=2.0),
    dict(name="scale5_96x64_l1", width=96, height=64, levels=1, n=30, seed=7, t=(0.0, 0.0, -0.19)),
    dict(name="mixed3px_96x64", width=96, height=64, levels=4, n=40, seed=9, t=(0.1389, 0.0, 0.0), mixed=True),
    dict(name="ramp3px_96x64", width=96, height=64, levels=3, n=30, seed=11, t=(0.1389, 0.02, 0.0), ramp=0.1, hist="HISTOGRAM"),
    dict(name="trans12_752x480", width=752, height=480, levels=6, n=150, seed=13, t=(0.0709, 0.0, 0.0)),
]
NAMES = [s["name"] for s in SPECS]
SMALL = NAMES[:-1]


@functools.lru_cache(maxsize=None)
def scene(name, levels=None):
    """the scene of that name; levels: the same images and points under a pyramid of another depth"""
    spec = next(s for s in SPECS if s["name"] == name)
    return Scene(**(spec if levels is None else dict(spec, levels=levels)))


# ---- window cases: (scene, levels, win[, points]) - every odd width 3..21, at least three cases per k_klt_track instantiation
# (<1>: 3 5 7, <2>: 9 11, <4>: 13 15, <7>: 17 19 21), every width on two scenes.  A case is in the table only if it holds the caps
# test_klt_cpu.py checks on the float64 restatement (near and near_stop at most 2 % of its points, 1 below 50; float32 equal to
# float64 in status outside near and in iterations outside near | near_stop).  Not in it for that reason: subpixel_64x48 at
# three levels with win 3, 5, 9, 13, 17, 19, rot2_47x31 at five levels with win 3, 5, mixed3px_96x64 at four levels with win 7, 9, 19 and at three with win 7,
# ramp3px_96x64 with win 3.  rot2_47x31 at five levels has a 3 x 2 top level, subpixel_64x48 at six levels a 2 x 2 one: levels smaller
# than any window, where every read wraps several times.  Under six levels most points of subpixel_64x48 wander for 30 iterations
# over the 2 x 2 and 4 x 3 levels and a quarter of them end where the number format decides; those cases take the listed points,
# on which the float64 run, the float32 run and a float32 run that sums the window in reverse order agree in status and iterations
# (win 3: less point 64, whose float32 and float64 flows enter level 0 3e-5 px apart), and of those the ones no level of which runs
# out its 30 iterations: every such level there still moves 0.2 to 2.3 px per step on a 4 x 3 or 2 x 2 image, and the flow it hands
# down is rounding's (on the device three such points ran one iteration more or less at the level below, positions equal).
# Exhausted levels are covered by the whole-scene cases: mixed3px_96x64, rot2_47x31 and ramp3px_96x64 at five levels (6 x 4 top).
_DEEP_W3 = [0, 1, 5, 8, 9, 11, 12, 15, 16, 19, 20, 21, 23, 26, 27, 29, 30, 31, 32, 33, 36, 37, 38, 39, 40, 41, 42, 43, 47, 48, 49, 50, 52,
            53, 54, 62, 63]
_DEEP_W9 = [0, 1, 2, 4, 5, 8, 9, 10, 11, 12, 15, 16, 19, 20, 21, 30, 31, 33, 34, 35, 36, 37, 38, 39, 40, 42, 45, 48, 49, 52, 53, 54, 55,
            57, 59, 60, 61, 63, 64]
_DEEP_W13 = [0, 1, 2, 4, 5, 8, 9, 10, 11, 12, 16, 19, 20, 21, 31, 33, 34, 37, 38, 42, 44, 45, 48, 49, 52, 53, 54, 55, 57, 59, 60, 61, 63,
             64]  # (and less the four points that leave the 4 x 3 level: one of them does so after 17 steps of over 2 px)
_DEEP_W21 = [0, 1, 2, 4, 5, 8, 9, 11, 12, 15, 16, 19, 20, 21, 24, 30, 31, 33, 36, 37, 38, 40, 41, 42, 44, 45, 48, 49, 52, 53, 54, 55, 57,
             59, 63, 64]
WINDOW_CASES = [
    # <1>
    ("mixed3px_96x64", 4, 3), ("scale5_96x64_l1", 1, 3), ("subpixel_64x48", 6, 3, _DEEP_W3),
    ("mixed3px_96x64", 4, 5), ("rot2_47x31", 3, 5), ("ramp3px_96x64", 3, 5),
    ("subpixel_64x48", 3, 7), ("rot2_47x31", 5, 7), ("ramp3px_96x64", 3, 7),
    # <2>
    ("rot2_47x31", 5, 9), ("mixed3px_96x64", 3, 9), ("ramp3px_96x64", 5, 9), ("subpixel_64x48", 6, 9, _DEEP_W9),
    ("mixed3px_96x64", 4, 11), ("rot2_47x31", 5, 11), ("subpixel_64x48", 3, 11),
    # <4> (win 13: three live slots of four)
    ("mixed3px_96x64", 4, 13), ("rot2_47x31", 5, 13), ("ramp3px_96x64", 3, 13), ("ramp3px_96x64", 5, 13), ("subpixel_64x48", 6, 13, _DEEP_W13),
    ("mixed3px_96x64", 4, 15), ("subpixel_64x48", 3, 15), ("rot2_47x31", 5, 15),
    # <7> (win 17, 19: five and six live slots of seven)
    ("mixed3px_96x64", 4, 17), ("rot2_47x31", 5, 17), ("ramp3px_96x64", 5, 17),
    ("mixed3px_96x64", 3, 19), ("rot2_47x31", 5, 19), ("ramp3px_96x64", 3, 19),
    ("mixed3px_96x64", 4, 21), ("rot2_47x31", 5, 21), ("subpixel_64x48", 6, 21, _DEEP_W21),
]
CASE_IDS = ["%s-L%d-w%d" % c[:3] for c in WINDOW_CASES]
# worst float32 - float64 position difference of the restatement over a case's status-1 points outside near | near_stop (measured on
# the CPU; test_klt_cpu.py re-measures each to within +0.1 % / -5 %).  The GPU test allows four times it.
SPREAD_PX = {
    "mixed3px_96x64-L4-w3": 5.887e-06,  # 40 points, 0 near, 0 near_stop
    "scale5_96x64_l1-L1-w3": 4.054e-06,  # 30 points, 0 near, 0 near_stop
    "subpixel_64x48-L6-w3": 5.688e-06,  # 37 points, 0 near, 1 near_stop
    "mixed3px_96x64-L4-w5": 8.008e-06,  # 40 points, 0 near, 1 near_stop
    "rot2_47x31-L3-w5": 4.283e-06,  # 20 points, 1 near, 0 near_stop
    "ramp3px_96x64-L3-w5": 4.532e-06,  # 30 points, 1 near, 1 near_stop
    "subpixel_64x48-L3-w7": 2.873e-06,  # 65 points, 0 near, 0 near_stop
    "rot2_47x31-L5-w7": 2.426e-06,  # 20 points, 0 near, 1 near_stop
    "ramp3px_96x64-L3-w7": 4.687e-06,  # 30 points, 1 near, 0 near_stop
    "rot2_47x31-L5-w9": 2.086e-06,  # 20 points, 0 near, 0 near_stop
    "mixed3px_96x64-L3-w9": 3.775e-06,  # 40 points, 1 near, 0 near_stop
    "ramp3px_96x64-L5-w9": 4.026e-06,  # 30 points, 1 near, 0 near_stop
    "subpixel_64x48-L6-w9": 2.222e-06,  # 39 points, 0 near, 0 near_stop
    "mixed3px_96x64-L4-w11": 3.555e-06,  # 40 points, 0 near, 0 near_stop
    "rot2_47x31-L5-w11": 1.752e-06,  # 20 points, 0 near, 1 near_stop
    "subpixel_64x48-L3-w11": 2.805e-06,  # 65 points, 1 near, 1 near_stop
    "mixed3px_96x64-L4-w13": 3.173e-06,  # 40 points, 0 near, 0 near_stop
    "rot2_47x31-L5-w13": 2.289e-06,  # 20 points, 0 near, 0 near_stop
    "ramp3px_96x64-L3-w13": 3.903e-06,  # 30 points, 0 near, 0 near_stop
    "ramp3px_96x64-L5-w13": 4.083e-06,  # 30 points, 1 near, 0 near_stop
    "subpixel_64x48-L6-w13": 2.927e-06,  # 34 points, 0 near, 0 near_stop
    "mixed3px_96x64-L4-w15": 2.327e-06,  # 40 points, 0 near, 0 near_stop
    "subpixel_64x48-L3-w15": 3.215e-06,  # 65 points, 0 near, 1 near_stop
    "rot2_47x31-L5-w15": 1.347e-06,  # 20 points, 0 near, 1 near_stop
    "mixed3px_96x64-L4-w17": 3.093e-06,  # 40 points, 0 near, 0 near_stop
    "rot2_47x31-L5-w17": 2.063e-06,  # 20 points, 0 near, 0 near_stop
    "ramp3px_96x64-L5-w17": 5.695e-06,  # 30 points, 0 near, 1 near_stop
    "mixed3px_96x64-L3-w19": 4.295e-06,  # 40 points, 0 near, 0 near_stop
    "rot2_47x31-L5-w19": 1.267e-06,  # 20 points, 0 near, 0 near_stop
    "ramp3px_96x64-L3-w19": 5.488e-06,  # 30 points, 0 near, 1 near_stop
    "mixed3px_96x64-L4-w21": 3.362e-06,  # 40 points, 0 near, 0 near_stop
    "rot2_47x31-L5-w21": 1.138e-06,  # 20 points, 0 near, 0 near_stop
    "subpixel_64x48-L6-w21": 2.723e-06,  # 36 points, 0 near, 0 near_stop
}


@functools.lru_cache(maxsize=None)
def case(case_id):
    return Case(*WINDOW_CASES[CASE_IDS.index(case_id)])


def instantiation(win):
    """window pixels per lane of the k_klt_track instantiation ovp_klt_track dispatches a window width to"""
    npl = (win * win + 63) // 64
    return 1 if npl <= 1 else 2 if npl <= 2 else 4 if npl <= 4 else 7


def near_cap(n):
    """the points of a case that may sit near a decision: 2 %, 1 point below 50 points"""
    return int(0.02 * n) if n >= 50 else 1


class Case:
    """a window case: a small scene under a pyramid depth and a window width of its own, all of its points or a subset"""

    def __init__(self, name, levels, win, points=None):
        self.scene, self.levels, self.win = scene(name, levels), levels, win
        self.id = "%s-L%d-w%d" % (name, levels, win)
        sc = self.scene
        self.idx = np.arange(len(sc.pts)) if points is None else np.asarray(points)
        self.pts = sc.pts[self.idx]
        self.guess = None if sc.guess is None else sc.guess[self.idx]
        self.width, self.height, self.hist, self.img0, self.img1 = sc.width, sc.height, sc.hist, sc.img0, sc.img1

    @property
    def pyramids(self):
        return self.scene.pyramids

    @functools.lru_cache(maxsize=None)
    def reference(self, dtype=np.float64):
        """(pts, status, report) of the restatement, computed once and shared (do not write into it)"""
        p, s, r = klt_ref.lk_track(*self.pyramids, self.pts, self.guess, self.win, dtype)
        for a in (p, s, *r.values()):
            a.setflags(write=False)
        return p, s, r


def compare(case, p, st, iters):
    """what the GPU test asserts of a run (p [n, 2], st [n], iters [n, levels]) of a window case against the float64 restatement:
    status outside `near`, iterations outside `near | near_stop`, positions of status-1 points within 4 x SPREAD_PX[case] outside
    `near | near_stop` and within 2 x STOP_EPS on `near_stop` points.  Returns dict(failures [str], worst, bound, excluded)."""
    ref_p, ref_s, rep = case.reference(np.float64)
    near, ns = rep["near"], rep["near_stop"] & ~rep["near"]
    sure = ~near & ~ns
    fails = []
    if not np.array_equal(np.asarray(st)[~near], ref_s[~near]):
        fails.append("status differs on points %s" % np.nonzero((np.asarray(st) != ref_s) & ~near)[0].tolist())
    bad_it = (np.asarray(iters) != rep["iters"]).any(axis=1) & sure
    if bad_it.any():
        fails.append("iterations differ on points %s" % "; ".join("%d: %s for %s (|delta| ended %s)" % (
            i, np.asarray(iters)[i].tolist(), rep["iters"][i].tolist(), np.round(rep["dnorm"][i], 5).tolist()) for i in np.nonzero(bad_it)[0]))
    err = np.abs(np.asarray(p, dtype=np.float64) - ref_p).max(axis=1)
    ok = (np.asarray(st) == 1) & (ref_s == 1)
    bound = 4 * SPREAD_PX[case.id]
    worst = float(err[ok & sure].max()) if (ok & sure).any() else 0.0
    worst_ns = float(err[ok & ns].max()) if (ok & ns).any() else 0.0
    if not worst <= bound:
        fails.append("position %.3e px off, bound %.3e" % (worst, bound))
    if not worst_ns <= 2 * klt_ref.STOP_EPS:
        fails.append("position of a point near the stop threshold %.3e px off, bound %.3e" % (worst_ns, 2 * klt_ref.STOP_EPS))
    return dict(failures=fails, worst=worst, bound=bound, worst_near_stop=worst_ns, near=np.nonzero(near)[0].tolist(),
                near_stop=np.nonzero(ns)[0].tolist())


@functools.lru_cache(maxsize=None)
def image_cases():
    """the images the GPU test of the image kernels uploads: {id: (image, levels)} - the regimes of k_klt_hist / k_klt_equalize
    (16-byte body, tail of block 0, grid cap of 256 blocks of 256 lanes of 16 pixels) and the histogram's edges"""
    rng = np.random.default_rng(17)
    rnd = lambda w, h: rng.integers(0, 256, size=(h, w)).astype(np.uint8)  # noqa: E731
    one = np.full((7, 9), 100, dtype=np.uint8)
    one[3, 4] = 200
    return {
        "4x3_tail_only": (rnd(4, 3), 1),
        "4x4_no_tail": (rnd(4, 4), 1),
        "15x17": (rnd(15, 17), 1),
        "1039x1011_grid_cap": (rnd(1039, 1011), 1),           # 1 050 429 pixels: more than 256 x 256 x 16, 13 in the tail
        "all_equal_but_one": (one, 1),                        # total - hist[first] == 1
        "constant_255": (np.full((5, 8), 255, dtype=np.uint8), 1),
        "constant_0": (np.zeros((5, 8), dtype=np.uint8), 1),
        "only_0_and_255": (np.where(rng.random((11, 13)) < 0.3, 0, 255).astype(np.uint8), 1),
        "first_bin_254": (np.where(rng.random((11, 13)) < 0.6, 254, 255).astype(np.uint8), 1),
        "47x31_to_3x2": (scene("rot2_47x31").img0, 5),
        "64x48_to_2x2": (scene("subpixel_64x48").img0, 6),
    }


@functools.lru_cache(maxsize=None)
def sequence():
    """three frames of one texture, 4 px to the right per frame, 96 x 64, three levels; a mask rectangle; seeded points of which one
    tracks into the mask in the second frame and one leaves the image in the third -> dict(frames, mask, ids, pts, levels)"""
    width, height = 96, 64
    sample = texture(width, height, 21)
    frames = [render(sample, width, height, homography(width, height, t=(k * 0.1852, 0.0, 0.0)) if k else None) for k in range(3)]
    mask = np.zeros((height, width), dtype=np.uint8)
    mask[20:41, 60:71] = 255
    rng = np.random.default_rng(1021)
    pts = np.concatenate([_grid_points(rng, 56, height, 12, 12), np.array([[57.3, 30.2], [89.6, 33.4]], dtype=np.float32)])
    return dict(frames=frames, mask=mask, ids=np.arange(100, 100 + len(pts)), pts=pts.astype(np.float32), levels=3, width=width, height=height)
