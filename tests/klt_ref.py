"""numpy restatement of the image front end the device runs (k_klt.hip): cv::equalizeHist, cv::pyrDown on 8-bit data and Bouguet's
pyramidal Lucas-Kanade with OpenCV's externally visible conventions (track_plane/TrackPlane.cpp:65, :40-92, :1299-1357).

UNPINNED: OpenCV is neither on the build machine nor in the reference tree.  Every convention below is recalled from OpenCV's
published behaviour, not verified against a file; each is one named constant (or one short function) here so that someone with
OpenCV at hand can correct one line.  The LK arithmetic runs in `dtype`: float64 is the truth the tests hold the device to,
float32 measures what the number format alone moves."""
import numpy as np

# ---- conventions (recalled, not verified against OpenCV's source) -------------------------------------------------------------
PYR_TAPS = (1, 4, 6, 4, 1)      # cv::pyrDown's separable kernel on 8-bit data; result (sum + PYR_ROUND) >> PYR_SHIFT
PYR_ROUND, PYR_SHIFT = 128, 8
SCHARR_SMOOTH = (3, 10, 3)      # Scharr: (3, 10, 3) across, (-1, 0, 1) along; SCHARR_NORM turns it into grey levels per pixel
SCHARR_NORM = 32.0
MAX_ITERS = 30                  # term_crit (TrackPlane.cpp:1328): COUNT 30 ...
STOP_EPS = 0.01                 # ... + EPS 0.01, compared as |delta|^2 <= STOP_EPS^2
OSC_EPS = 0.01                  # from the second iteration on: |delta + delta_prev| < OSC_EPS in both axes -> back by delta / 2
OSC_FROM, OSC_BACK = 1, 0.5     # (the second iteration is index 1; the back-step is OSC_BACK x delta)
MIN_EIG_THRESHOLD = 1e-4        # calcOpticalFlowPyrLK's default minEigThreshold
GATE_SCALE = 1024.0             # OpenCV's fixed-point scale: A = G / GATE_SCALE, minEig = lambda_min(A) / w^2, det(A) < FLT_EPSILON
FLT_EPSILON = float(np.finfo(np.float32).eps)
# initial flow: guess / 2^L at the top level (OPTFLOW_USE_INITIAL_FLOW, :1329), doubled from level to level
# window: top-left corner = p - (w - 1) / 2; a corner whose floor is < -w or >= the level's size leaves the level (status 0 at level 0)
# borders: image reads outside a level reflect-101, gradient reads outside a level are zero

# "near a decision" margins of the report
NEAR_GATE_REL = 0.01
NEAR_CORNER_PX = 1e-3
NEAR_OSC = 1e-4
NEAR_KEEP_PX = 1e-3
# |delta| / STOP_EPS within NEAR_STOP_REL of 1 at some iteration: the stop decision may fall either way in another arithmetic.
# NEAR_STOP_MEASURED is the largest float32 - float64 difference of |delta| / STOP_EPS at the iteration that stopped level 0, over
# the status-1 points outside `near` of the window cases of tests/klt_cases.py whose iteration counts agree (level 0: both runs
# enter it with the same flow to within the position spread; above it a wandering point's differing entry flow, not the
# arithmetic, sets the difference - up to 0.38 there).  Times 4 for a summation order other than numpy's, as the position bound has
# it.  tests/test_klt_cpu.py re-measures it.
NEAR_STOP_MEASURED = 1.145e-3
NEAR_STOP_REL = 4 * NEAR_STOP_MEASURED


def _corner_floor(x):
    """a window corner's integer part: floor, not truncation (a negative corner rounds down)"""
    return np.floor(x)


def _top_scale(top, T):
    """the initial flow is guess / 2^top at the top level"""
    return T(1.0 / (1 << top))


def _window(win):
    """(rows, cols) of the window's pixels, row-major: pixel k is row k / win, column k % win, k < win^2 (on the device lane + 64 j)"""
    k = np.arange(win * win)
    return k // win, k % win


def _window_cur(win):
    """the same pixels where the current image is read in the iterations (one layout, two sites on the device)"""
    return _window(win)


def _lut_round(x):
    """cv::saturate_cast<uchar>(float): to nearest, ties to even"""
    return np.rint(x)


def reflect101(i, n):
    """BORDER_REFLECT_101 index of any integer i into [0, n)"""
    i = np.asarray(i, dtype=np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i >= n, p - i, i)


def equalize_hist(img):
    """cv::equalizeHist: LUT from the cumulative sum behind the first non-empty bin, scaled by 255 / (total - hist[first]) in f32,
    rounded to nearest (ties to even) with saturation; a constant image maps to itself."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    hist = np.bincount(img.reshape(-1), minlength=256).astype(np.int64)
    total = int(img.size)
    first = int(np.nonzero(hist)[0][0])
    if hist[first] == total:
        return img.copy()
    scale = np.float32(255.0) / np.float32(total - hist[first])
    lut = np.zeros(256, dtype=np.uint8)
    s = 0
    for i in range(first + 1, 256):
        s += int(hist[i])
        lut[i] = np.uint8(min(255.0, float(_lut_round(np.float32(s) * scale))))
    return lut[img]


def pyr_down(img):
    """one level of cv::pyrDown on 8-bit data: [1 4 6 4 1] in both axes, reflect-101, (sum + 128) >> 8, size ((w+1)/2, (h+1)/2)"""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w = img.shape
    ho, wo = (h + 1) // 2, (w + 1) // 2
    src = img.astype(np.int64)
    rows = np.zeros((h, wo), dtype=np.int64)
    xs = 2 * np.arange(wo)
    for k, t in enumerate(PYR_TAPS):
        rows += t * src[:, reflect101(xs + k - 2, w)]
    out = np.zeros((ho, wo), dtype=np.int64)
    ys = 2 * np.arange(ho)
    for k, t in enumerate(PYR_TAPS):
        out += t * rows[reflect101(ys + k - 2, h), :]
    return ((out + PYR_ROUND) >> PYR_SHIFT).astype(np.uint8)


def build_pyramid(img, n_levels, hist="HISTOGRAM"):
    """feed_new_camera (:40-92): equalise (HISTOGRAM) or not (NONE), then n_levels images (maxLevel = n_levels - 1)"""
    if hist == "HISTOGRAM":
        img = equalize_hist(img)
    elif hist != "NONE":
        raise ValueError("CLAHE is not built")
    pyr = [np.ascontiguousarray(img, dtype=np.uint8)]
    for _ in range(n_levels - 1):
        pyr.append(pyr_down(pyr[-1]))
    return pyr


def scharr(img, T):
    """(gx, gy) of a level, normalised to grey levels per pixel; image reads reflect-101 (exact in f32: integers below 2^13 / 32)"""
    h, w = img.shape
    I = img.astype(T)
    ym, y0, yp = reflect101(np.arange(h) - 1, h), np.arange(h), reflect101(np.arange(h) + 1, h)
    xm, x0, xp = reflect101(np.arange(w) - 1, w), np.arange(w), reflect101(np.arange(w) + 1, w)
    a, b, c = (T(v) for v in SCHARR_SMOOTH)
    sx = lambda X: a * I[np.ix_(ym, X)] + b * I[np.ix_(y0, X)] + c * I[np.ix_(yp, X)]  # noqa: E731
    sy = lambda Y: a * I[np.ix_(Y, xm)] + b * I[np.ix_(Y, x0)] + c * I[np.ix_(Y, xp)]  # noqa: E731
    return (sx(xp) - sx(xm)) / T(SCHARR_NORM), (sy(yp) - sy(ym)) / T(SCHARR_NORM)


def _bilinear(read, ix, iy, a, b, pix, T):
    """[m, len(pix)] samples of `read(xi, yi)` at (ix + c + a, iy + r + b) for the window pixels pix = (r, c)"""
    X = ix[:, None] + pix[1][None, :]
    Y = iy[:, None] + pix[0][None, :]
    a, b = a[:, None], b[:, None]
    one = T(1)
    w00, w01, w10, w11 = (one - a) * (one - b), a * (one - b), (one - a) * b, a * b
    return w00 * read(X, Y) + w01 * read(X + 1, Y) + w10 * read(X, Y + 1) + w11 * read(X + 1, Y + 1)


def _img_reader(img, T):
    h, w = img.shape
    I = img.astype(T)
    return lambda X, Y: I[reflect101(Y, h), reflect101(X, w)]


def _grad_reader(g):
    h, w = g.shape
    def read(X, Y):
        ok = (X >= 0) & (X < w) & (Y >= 0) & (Y < h)
        return np.where(ok, g[np.clip(Y, 0, h - 1), np.clip(X, 0, w - 1)], g.dtype.type(0))
    return read


def _inside(c, win, cols, rows):
    """the window rule on a corner [m, 2] (floats compared, which is floor(c) compared; false for a non-finite corner)"""
    with np.errstate(invalid="ignore"):
        return (c[:, 0] >= -win) & (c[:, 0] < cols) & (c[:, 1] >= -win) & (c[:, 1] < rows)


def _near_corner(c, win, cols, rows):
    lim = np.array([[-win, -win], [cols, rows]], dtype=np.float64)
    c = c.astype(np.float64)
    return (np.abs(c[:, None, :] - lim[None, :, :]) < NEAR_CORNER_PX).any(axis=(1, 2))


def _border_grad(ip, a, b, pix, cols, rows):
    """[m] bool: a gradient read of the window at corner ip + (a, b) falls outside the level with a non-zero bilinear weight"""
    X, Y = ip[:, 0, None] + pix[1][None, :], ip[:, 1, None] + pix[0][None, :]
    ox0, ox1, oy0, oy1 = (X < 0) | (X >= cols), (X + 1 < 0) | (X + 1 >= cols), (Y < 0) | (Y >= rows), (Y + 1 < 0) | (Y + 1 >= rows)
    pa, pb = (a > 0)[:, None], (b > 0)[:, None]
    return ((ox0 | oy0) | (pa & (ox1 | oy0)) | (pb & (ox0 | oy1)) | (pa & pb & (ox1 | oy1))).any(axis=1)


def _neg_corner(c, fl):
    """[m] bool: a coordinate of the corner c is negative and no integer - floor and truncation differ"""
    return ((c < 0) & (c != fl)).any(axis=1)


def lk_track(pyr_prev, pyr_cur, pts_prev, guess=None, win=15, dtype=np.float64):
    """cv::calcOpticalFlowPyrLK(pyr_prev, pyr_cur, pts_prev, guess, OPTFLOW_USE_INITIAL_FLOW) for every point at once.
    Returns (pts [n, 2] dtype, status [n] uint8, report) with report = dict(near [n] bool: a gated quantity of the point sat near its
    threshold at some level, iters [n, levels] iterations run per level, level 0 first) and what the run did, per point:
      near_stop [n] bool        |delta| / STOP_EPS within NEAR_STOP_REL of 1 at some iteration
      osc [n] int               back-steps taken
      exhausted [n] bool        a level ran MAX_ITERS iterations and neither the stop nor the back-step ended it
      gate_upper, gate_l0       the texture gate failed above / at level 0
      left_upper, left_l0       the window rule failed above / at level 0 (at the point's own window or in the iterations)
      left_in_loop              the window rule failed inside the iteration loop
      neg_corner                a window corner with a negative non-integer coordinate was floored
      border_grad               a gradient read outside a level returned zero with a non-zero bilinear weight
      dnorm [n, levels] f64     |delta| of the last iteration a level ran (nan where it ran none)"""
    T = dtype
    pts_prev = np.asarray(pts_prev, dtype=np.float32).reshape(-1, 2)
    guess = pts_prev if guess is None else np.asarray(guess, dtype=np.float32).reshape(-1, 2)
    n, nl = len(pts_prev), len(pyr_prev)
    top = nl - 1
    alive = np.isfinite(pts_prev).all(axis=1) & np.isfinite(guess).all(axis=1)
    status = alive.astype(np.uint8)
    near = np.zeros(n, dtype=bool)
    iters = np.zeros((n, nl), dtype=np.int32)
    flags = {k: np.zeros(n, dtype=bool) for k in ("near_stop", "exhausted", "gate_upper", "gate_l0", "left_upper", "left_l0",
                                                   "left_in_loop", "neg_corner", "border_grad")}
    n_osc = np.zeros(n, dtype=np.int32)
    dnorm = np.full((n, nl), np.nan)
    pix, pix_cur = _window(win), _window_cur(win)
    P = np.where(alive[:, None], pts_prev, 0).astype(T)
    with np.errstate(over="ignore", invalid="ignore"):
        g = np.where(alive[:, None], guess, 0).astype(T) * _top_scale(top, T)
    half = T((win - 1) * 0.5)
    for lvl in range(top, -1, -1):
        gate_f, left_f = (flags["gate_l0"], flags["left_l0"]) if lvl == 0 else (flags["gate_upper"], flags["left_upper"])
        with np.errstate(over="ignore", invalid="ignore"):
            if lvl != top:
                g = g * T(2)
        I8, J8 = pyr_prev[lvl], pyr_cur[lvl]
        rows, cols = I8.shape
        pw = P * T(1.0 / (1 << lvl)) - half
        ins = _inside(pw, win, cols, rows)
        near |= alive & _near_corner(pw, win, cols, rows)
        left_f |= alive & ~ins
        if lvl == 0:
            status[alive & ~ins] = 0
        act = np.nonzero(alive & ins)[0]
        if len(act) == 0:
            continue
        gx, gy = scharr(I8, T)
        fl = _corner_floor(pw[act])
        ip = fl.astype(np.int64)
        a, b = (pw[act] - fl)[:, 0], (pw[act] - fl)[:, 1]
        flags["neg_corner"][act] |= _neg_corner(pw[act], np.floor(pw[act]))
        flags["border_grad"][act] |= _border_grad(ip, a, b, pix, cols, rows)
        Iw = _bilinear(_img_reader(I8, T), ip[:, 0], ip[:, 1], a, b, pix, T)
        Ix = _bilinear(_grad_reader(gx), ip[:, 0], ip[:, 1], a, b, pix, T)
        Iy = _bilinear(_grad_reader(gy), ip[:, 0], ip[:, 1], a, b, pix, T)
        sc = T(1.0 / GATE_SCALE)
        A11, A12, A22 = (Ix * Ix).sum(axis=1) * sc, (Ix * Iy).sum(axis=1) * sc, (Iy * Iy).sum(axis=1) * sc
        D = A11 * A22 - A12 * A12
        min_eig = (A22 + A11 - np.sqrt((A11 - A22) * (A11 - A22) + T(4) * A12 * A12)) / T(2 * win * win)
        bad = (min_eig < T(MIN_EIG_THRESHOLD)) | (D < T(FLT_EPSILON))
        near[act] |= (np.abs(min_eig.astype(np.float64) / MIN_EIG_THRESHOLD - 1) < NEAR_GATE_REL) | \
                     (np.abs(D.astype(np.float64) / FLT_EPSILON - 1) < NEAR_GATE_REL)
        gate_f[act[bad]] = True
        if lvl == 0:
            status[act[bad]] = 0
        keep = ~bad
        act, Iw, Ix, Iy, A11, A12, A22, D = act[keep], Iw[keep], Ix[keep], Iy[keep], A11[keep], A12[keep], A22[keep], D[keep]
        v = g[act] - half  # the window's corner in the current image
        run = np.ones(len(act), dtype=bool)
        pd = np.zeros((len(act), 2), dtype=T)
        Jr = _img_reader(J8, T)
        for j in range(MAX_ITERS):
            if not run.any():
                break
            ins = _inside(v, win, cols, rows)
            near[act[run]] |= _near_corner(v[run], win, cols, rows)
            out = run & ~ins
            left_f[act[out]] = True
            flags["left_in_loop"][act[out]] = True
            if lvl == 0:
                status[act[out]] = 0
            run = run & ins
            k = np.nonzero(run)[0]
            if len(k) == 0:
                break
            iters[act[k], lvl] += 1
            fl = _corner_floor(v[k])
            iq = fl.astype(np.int64)
            flags["neg_corner"][act[k]] |= _neg_corner(v[k], np.floor(v[k]))
            Jw = _bilinear(Jr, iq[:, 0], iq[:, 1], (v[k] - fl)[:, 0], (v[k] - fl)[:, 1], pix_cur, T)
            diff = Jw - Iw[k]
            b1, b2 = (diff * Ix[k]).sum(axis=1) * sc, (diff * Iy[k]).sum(axis=1) * sc
            d = np.stack([(A12[k] * b2 - A22[k] * b1) / D[k], (A12[k] * b1 - A11[k] * b2) / D[k]], axis=1)
            v[k] = v[k] + d
            stop = (d * d).sum(axis=1) <= T(STOP_EPS * STOP_EPS)
            dn = np.sqrt((d.astype(np.float64) ** 2).sum(axis=1))
            dnorm[act[k], lvl] = dn
            with np.errstate(invalid="ignore"):
                flags["near_stop"][act[k]] |= np.abs(dn / STOP_EPS - 1) < NEAR_STOP_REL
            s = np.abs(d + pd[k])
            osc = (j >= OSC_FROM) & ~stop & (s[:, 0] < T(OSC_EPS)) & (s[:, 1] < T(OSC_EPS))
            if j >= OSC_FROM:
                # (the test is max(|sx|, |sy|) < OSC_EPS: that maximum is what sits near the threshold or does not)
                near[act[k]] |= ~stop & (np.abs(s.astype(np.float64).max(axis=1) - OSC_EPS) < NEAR_OSC)
            v[k[osc]] = v[k[osc]] - d[osc] * T(OSC_BACK)
            n_osc[act[k[osc]]] += 1
            pd[k] = d
            run[k[stop | osc]] = False
        else:
            flags["exhausted"][act[run]] = True
        g[act] = v + half
    return g, status, dict(near=near, iters=iters, osc=n_osc, dnorm=dnorm, **flags)


def keep_rule(pts, status, cols, rows, mask=None):
    """feed_monocular :536-551: a point is dropped for x < 0, y < 0, (int) x >= cols, (int) y >= rows, a mask value above 127 at the
    truncated pixel, or status 0.  Returns (keep [n] bool, near [n] bool: x or y within NEAR_KEEP_PX of an integer the rule truncates
    at a border or a mask edge)."""
    pts = np.asarray(pts)
    n = len(pts)
    keep = np.zeros(n, dtype=bool)
    near = np.zeros(n, dtype=bool)
    for i in range(n):
        x, y = float(pts[i, 0]), float(pts[i, 1])
        if not status[i] or not (np.isfinite(x) and np.isfinite(y)):
            continue
        def decide(x, y):
            if x < 0 or y < 0 or int(x) >= cols or int(y) >= rows:
                return False
            return not (mask is not None and mask[int(y), int(x)] > 127)
        keep[i] = decide(x, y)
        near[i] = any(decide(x + dx, y + dy) != keep[i] for dx in (-NEAR_KEEP_PX, NEAR_KEEP_PX) for dy in (-NEAR_KEEP_PX, NEAR_KEEP_PX))
    return keep, near


class RefTracker:
    """the bookkeeping of capi.KltTracker.step (feed_monocular :505-567 minus detection and the epipolar check) on the restatement"""

    def __init__(self, width, height, n_levels, win=15, dtype=np.float64):
        self.w, self.h, self.nl, self.win, self.T = width, height, n_levels, win, dtype
        self.pyr = None
        self.ids = np.zeros(0, dtype=np.int64)
        self.pts = np.zeros((0, 2), dtype=np.float32)
        self.near = np.zeros(0, dtype=bool)

    def add_points(self, ids, uv):
        self.ids = np.concatenate([self.ids, np.asarray(ids, dtype=np.int64).reshape(-1)])
        self.pts = np.concatenate([self.pts, np.asarray(uv, dtype=np.float32).reshape(-1, 2)])

    def step(self, img, mask=None, hist="HISTOGRAM"):
        pyr = build_pyramid(img, self.nl, hist)
        prev, self.pyr = self.pyr, pyr
        if prev is None or len(self.ids) == 0:
            self.near = np.zeros(len(self.ids), dtype=bool)
            return self.ids.copy(), self.pts.copy()
        p, st, rep = lk_track(prev, pyr, self.pts, self.pts, self.win, self.T)
        p = p.astype(np.float32)
        keep, near = keep_rule(p, st, self.w, self.h, mask)
        self.near = rep["near"] | near   # of the points that went into this step, in their order
        self.tracked_ids = self.ids.copy()
        self.ids, self.pts = self.ids[keep], p[keep]
        return self.ids.copy(), self.pts.copy()
