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
    def reference(self, dtype=np.float64):
        """(pts, status, report) of the restatement, computed once and shared (do not write into it)"""
        p, s, r = klt_ref.lk_track(*self.pyramids, self.pts, self.guess, WIN, dtype)
        for a in (p, s, r["near"], r["iters"]):
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
def scene(name):
    return Scene(**next(s for s in SPECS if s["name"] == name))


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
