"""Restatement (numpy) of the detection stage the device is held to: Grider_FAST::perform_griding (ov_core), cv::FAST with
non-maximum suppression, cv::cornerSubPix and TrackPlane::perform_detection_monocular (track_plane/TrackPlane.cpp:1173-1297).
Grider_FAST and OpenCV are not in the reference tree: everything but perform_detection_monocular is RECALLED from the published
form, not pinned.  Every recalled convention is named exactly once, as a field of CONV; a mutant flips one (mutant()).  The tie
rule of the selection (raster order) is this project's own: the reference leaves ties to std::sort.

The functions report the branches a run met (the dicts called `report`), so that the tests can show every rule exercised."""
import numpy as np

CONV = dict(
    strict_threshold=True,   # a circle pixel counts when p > v + t or p < v - t, both strict
    arc=9,                   # FAST-9/16: 9 contiguous pixels of the 16
    score_minus_one=True,    # the score is the largest t' the pixel is still a corner at: (largest arc minimum) - 1
    strict_nms=True,         # kept when strictly greater than all 8 neighbours
    nms_across=False,        # scores of the adjacent cell (and of the cell's untested border) are never consulted
    border=3,                # pixels at least 3 from every edge of the cell are tested
    tie_reverse=False,       # OUR rule: equal scores go in raster order (row, then column)
    mask_before=False,       # the mask is applied after the selection of K: a masked point uses up a slot
    k_plus_one=True,         # K = (int)(num_features / cells) + 1
    float_cell=False,        # cell sizes by integer division
    regrid=True,             # num_features < grid_x grid_y shrinks the grid
    half_win=5,              # cornerSubPix window (5, 5): 11 x 11
    weights=True,            # exp(-x^2) exp(-y^2), x = (j - 5) / 5
    eps_squared=True,        # |det| <= DBL_EPSILON^2 stops
    max_iters=20,            # COUNT 20
    revert=True,             # more than the half window from the start in x or y: the start is returned
    border_mode="replicate",  # getRectSubPix replicates the border
)
MUTANTS = {
    "non_strict_threshold": dict(strict_threshold=False), "arc_8": dict(arc=8), "arc_10": dict(arc=10),
    "score_without_minus_one": dict(score_minus_one=False), "non_strict_nms": dict(strict_nms=False),
    "nms_across_cell_edge": dict(nms_across=True), "border_2": dict(border=2), "border_4": dict(border=4),
    "ties_reverse_raster": dict(tie_reverse=True), "mask_before_selection": dict(mask_before=True),
    "k_without_plus_one": dict(k_plus_one=False), "float_cell_size": dict(float_cell=True), "no_regrid": dict(regrid=False),
    "window_5x5": dict(half_win=2), "no_weights": dict(weights=False), "eps_not_squared": dict(eps_squared=False),
    "iterations_19": dict(max_iters=19), "no_revert": dict(revert=False), "reflected_border": dict(border_mode="reflect"),
}
EPS_STEP2 = 1e-6   # EPS 0.001, squared
MAX_K = 256        # the entry's limit on points per cell (OVP_FAST_MAX_K)
MAX_CELLS = 4096
# the 16-pixel Bresenham circle of radius 3, clockwise from 12 o'clock: (dx, dy)
CIRCLE = [(0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1),
          (-2, -2), (-1, -3)]


def mutant(name):
    return dict(CONV, **MUTANTS[name])


def grid(cols, rows, num_features, grid_x, grid_y, conv=CONV):
    """the cells of perform_griding -> dict(grid_x, grid_y, K, x0 [ct_cols + 1], y0 [ct_rows + 1] cell edges, ct_cols, ct_rows,
    regridded) - None when a cell would be empty (size 0)"""
    regridded = False
    if conv["regrid"] and num_features < grid_x * grid_y:
        ratio = float(grid_x) / float(grid_y)
        grid_y = int(np.ceil(np.sqrt(num_features / ratio)))
        grid_x = int(np.ceil(grid_y * ratio))
        regridded = True
    K = int(num_features / float(grid_x * grid_y)) + (1 if conv["k_plus_one"] else 0)
    if conv["float_cell"]:
        sx, sy = cols / float(grid_x), rows / float(grid_y)
        if sx < 1 or sy < 1:
            return None
        ct_cols, ct_rows = grid_x, grid_y
        x0 = [int(np.floor(c * sx)) for c in range(ct_cols + 1)]
        y0 = [int(np.floor(r * sy)) for r in range(ct_rows + 1)]
    else:
        sx, sy = cols // grid_x, rows // grid_y
        if sx < 1 or sy < 1:
            return None
        ct_cols, ct_rows = cols // sx, rows // sy
        x0 = [c * sx for c in range(ct_cols + 1)]
        y0 = [r * sy for r in range(ct_rows + 1)]
    return dict(grid_x=grid_x, grid_y=grid_y, K=K, x0=x0, y0=y0, ct_cols=ct_cols, ct_rows=ct_rows, regridded=regridded,
                size_x=sx, size_y=sy)


def _arc_max(d, arc):
    """largest over the 16 arcs of `arc` of the arc's minimum of d [16, h, w] -> (value [h, w], the same over the arcs that do
    not wrap index 15 -> 0)"""
    best = nowrap = None
    for s in range(16):
        m = d[s]
        for k in range(1, arc):
            m = np.minimum(m, d[(s + k) & 15])
        best = m if best is None else np.maximum(best, m)
        if s + arc <= 16:
            nowrap = m if nowrap is None else np.maximum(nowrap, m)
    return best, nowrap


def _tested(g, cols, rows, border):
    """the pixels cv::FAST tests: at least `border` from every edge of their cell (the strips outside the cells: none)"""
    lo_x, hi_x = np.full(cols, 1, dtype=np.int64), np.zeros(cols, dtype=np.int64)
    for c in range(g["ct_cols"]):
        lo_x[g["x0"][c]:g["x0"][c + 1]], hi_x[g["x0"][c]:g["x0"][c + 1]] = g["x0"][c] + border, g["x0"][c + 1] - border
    lo_y, hi_y = np.full(rows, 1, dtype=np.int64), np.zeros(rows, dtype=np.int64)
    for r in range(g["ct_rows"]):
        lo_y[g["y0"][r]:g["y0"][r + 1]], hi_y[g["y0"][r]:g["y0"][r + 1]] = g["y0"][r] + border, g["y0"][r + 1] - border
    xs, ys = np.arange(cols), np.arange(rows)
    return ((ys >= lo_y) & (ys < hi_y))[:, None] & ((xs >= lo_x) & (xs < hi_x))[None, :]


def score_maps(img, g, threshold, conv=CONV):
    """(score [h, w] uint8, nms [h, w] uint8, report) of cv::FAST per cell, laid into the image"""
    img = np.asarray(img, dtype=np.uint8)
    rows, cols = img.shape
    v = img.astype(np.int32)
    pad = np.pad(v, 3, mode="edge")  # (a pixel whose circle leaves the image is never tested: the pad's values are not used)
    d = np.stack([pad[3 + dy:3 + dy + rows, 3 + dx:3 + dx + cols] - v for dx, dy in CIRCLE])
    arc = conv["arc"]
    bright, bright_nw = _arc_max(d, arc)
    dark, dark_nw = _arc_max(-d, arc)
    m = np.maximum(bright, dark)
    t = int(threshold)
    is_corner = (m > t) if conv["strict_threshold"] else (m >= t)
    raw = np.clip(m - 1 if conv["score_minus_one"] else m, 0, 255)
    tested = _tested(g, cols, rows, conv["border"])
    inside3 = np.zeros_like(tested)
    inside3[3:rows - 3, 3:cols - 3] = True          # (the border-of-2 mutant still cannot read outside the image)
    tested &= inside3
    score = np.where(tested & is_corner, raw, 0).astype(np.uint8)
    consult = np.where(inside3 & is_corner, raw, 0).astype(np.uint8) if conv["nms_across"] else score

    def suppress(sc, consulted, strict):
        p = np.pad(consulted.astype(np.int32), 1)
        nb = np.max(np.stack([p[1 + dy:1 + dy + rows, 1 + dx:1 + dx + cols] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy]), axis=0)
        s = sc.astype(np.int32)
        return np.where((s > nb) if strict else (s >= nb), sc, 0).astype(np.uint8) * (sc > 0)
    nms = suppress(score, consult, conv["strict_nms"])
    # ---- what this run met
    m8 = np.maximum(_arc_max(d, 8)[0], _arc_max(-d, 8)[0])
    kept = nms > 0
    lx_lo = np.zeros((rows, cols), dtype=bool)
    for c in range(g["ct_cols"]):
        for r in range(g["ct_rows"]):
            x0, x1, y0, y1 = g["x0"][c], g["x0"][c + 1], g["y0"][r], g["y0"][r + 1]
            b = conv["border"]
            if x1 - x0 >= 2 * b + 1 and y1 - y0 >= 2 * b + 1:
                lx_lo[y0 + b:y1 - b, [x0 + b, x1 - b - 1]] = True
                lx_lo[[y0 + b, y1 - b - 1], x0 + b:x1 - b] = True
    across = suppress(score, np.where(inside3 & is_corner, raw, 0).astype(np.uint8), True) > 0
    cw = np.diff(g["x0"]) if g["ct_cols"] else np.zeros(0)
    chh = np.diff(g["y0"]) if g["ct_rows"] else np.zeros(0)
    in_cells = np.zeros((rows, cols), dtype=bool)
    in_cells[:g["y0"][-1], :g["x0"][-1]] = True
    report = dict(
        bright_arc=bool((tested & (bright > t)).any()), dark_arc=bool((tested & (dark > t)).any()),
        wrapped_arc=bool((tested & is_corner & (np.maximum(bright_nw, dark_nw) <= t)).any()),
        exactly_8=bool((tested & (m <= t) & (m8 > t)).any()),
        diff_equals_t=bool((tested & (m == t)).any()) and t > 0,
        equal_neighbours_suppressed=bool(((score > 0) & ~(suppress(score, score, True) > 0) & (suppress(score, score, False) > 0)).any()),
        corner_next_to_border=bool((kept & lx_lo).any()),
        stronger_neighbour_in_next_cell=bool((kept & ~across).any()),
        cell_smaller_than_7=bool(len(cw) and len(chh) and (cw.min() < 7 or chh.min() < 7)),
        cell_exactly_7x7=bool(len(cw) and len(chh) and cw.min() == 7 and cw.max() == 7 and chh.min() == 7 and chh.max() == 7),
        ct_cols_above_grid_x=bool(g["ct_cols"] > g["grid_x"]),
        corner_in_leftover_strip=bool((inside3 & is_corner & ~in_cells).any()),
        regrid=bool(g["regridded"]),
    )
    return score, nms, report


def select(nms, g, mask=None, conv=CONV):
    """per-cell top-K of the suppressed map, in output order -> (xy [n, 2] int32, response [n] int32, cell [n] int32, report)"""
    xy, resp, cell = [], [], []
    tie = masked_slot = False
    K = g["K"]
    for r in range(g["ct_cols"] * g["ct_rows"]):
        c, q = r % g["ct_cols"], r // g["ct_cols"]
        x0, x1, y0, y1 = g["x0"][c], g["x0"][c + 1], g["y0"][q], g["y0"][q + 1]
        sub = nms[y0:y1, x0:x1]
        ys, xs = np.nonzero(sub)  # raster order
        if mask is not None and conv["mask_before"]:
            ok = ~(mask[ys + y0, xs + x0] > 127)
            ys, xs = ys[ok], xs[ok]
        sc = sub[ys, xs].astype(np.int64)
        idx = np.arange(len(sc))
        order = np.lexsort((-idx if conv["tie_reverse"] else idx, -sc))
        tie |= len(order) > K >= 1 and sc[order[K - 1]] == sc[order[K]]
        for i in order[:K]:
            x, y = int(xs[i] + x0), int(ys[i] + y0)
            if mask is not None and not conv["mask_before"] and mask[y, x] > 127:
                masked_slot |= len(order) > K
                continue
            xy.append((x, y)), resp.append(int(sc[i])), cell.append(r)
    return (np.array(xy, dtype=np.int32).reshape(-1, 2), np.array(resp, dtype=np.int32), np.array(cell, dtype=np.int32),
            dict(tie_at_kth=bool(tie), masked_point_uses_slot=bool(masked_slot)))


def subpix_weights(half_win=5, weighted=True):
    """the window's weights, float: exp(-x^2) per axis with x = (j - half) / half in float; the exponential is taken in double and
    rounded to float (one rounding: the same bits from every libm)"""
    x = (np.arange(2 * half_win + 1, dtype=np.float32) - np.float32(half_win)) / np.float32(half_win)
    w = np.exp(-(x * x).astype(np.float64)).astype(np.float32) if weighted else np.ones(2 * half_win + 1, dtype=np.float32)
    return w


def _patch(img, cx, cy, half, border_mode, T):
    """getRectSubPix of a (2 half + 3)^2 patch around (cx, cy) [n], bilinear, arithmetic in T -> [n, s, s]"""
    rows, cols = img.shape
    s = 2 * half + 3
    ox, oy = cx - T(half + 1), cy - T(half + 1)
    fx, fy = np.floor(ox), np.floor(oy)
    a, b = (ox - fx).astype(T), (oy - fy).astype(T)
    lim = 2.0 ** 30  # (a position that far out reads the border either way; keeps the integer conversion defined)
    ix = np.clip(np.nan_to_num(fx, nan=0.0), -lim, lim).astype(np.int64)
    iy = np.clip(np.nan_to_num(fy, nan=0.0), -lim, lim).astype(np.int64)
    k = np.arange(s)
    X, Y = ix[:, None, None] + k[None, None, :], iy[:, None, None] + k[None, :, None]

    def rd(X, Y):
        if border_mode == "replicate":
            return img[np.clip(Y, 0, rows - 1), np.clip(X, 0, cols - 1)].astype(T)

        def refl(i, n):
            if n == 1:
                return np.zeros_like(i)
            p = 2 * (n - 1)
            i = np.mod(i, p)
            return np.where(i >= n, p - i, i)
        return img[refl(Y, rows), refl(X, cols)].astype(T)
    a, b = a[:, None, None], b[:, None, None]
    one = T(1)
    w00, w01, w10, w11 = (one - a) * (one - b), a * (one - b), (one - a) * b, a * b
    return w00 * rd(X, Y) + w01 * rd(X + 1, Y) + w10 * rd(X, Y + 1) + w11 * rd(X + 1, Y + 1)


def corner_subpix(img, pts, conv=CONV, patch_dtype=np.float32, order="numpy"):
    """cv::cornerSubPix(img, pts, (5,5), (-1,-1), COUNT+EPS 20, 0.001) -> (pts [n, 2] float32, report).  patch_dtype: the arithmetic
    of the patch and its gradients (float32 is the stage's; float64 the variant the spread is measured against); order: "numpy"
    (pairwise) / "forward" / "reverse" summation of the five sums, which are double either way."""
    img = np.asarray(img, dtype=np.uint8)
    rows, cols = img.shape
    start = np.asarray(pts, dtype=np.float32).reshape(-1, 2)
    n = len(start)
    half = conv["half_win"]
    T = patch_dtype
    w1 = subpix_weights(half, conv["weights"])
    W = (w1[:, None] * w1[None, :]).astype(np.float32).astype(np.float64)
    k = np.arange(-half, half + 1, dtype=np.float64)
    PX, PY = np.meshgrid(k, k)
    cur = start.copy()
    live = np.ones(n, dtype=bool)
    iters = np.zeros(n, dtype=np.int32)
    last_step2 = np.full(n, np.inf)
    why = np.zeros(n, dtype=np.int32)  # 1 converged, 2 exhausted, 3 singular, 4 left the image
    det_floor = np.finfo(np.float64).eps ** (2 if conv["eps_squared"] else 1)

    def total(a):
        a = a.reshape(len(a), -1)
        if order == "numpy":
            return a.sum(axis=1)
        a = a if order == "forward" else a[:, ::-1]
        s = np.zeros(len(a))
        for j in range(a.shape[1]):
            s = s + a[:, j]
        return s
    for it in range(conv["max_iters"]):
        idx = np.nonzero(live)[0]
        if not len(idx):
            break
        c = cur[idx]
        P = _patch(img, c[:, 0].astype(T), c[:, 1].astype(T), half, conv["border_mode"], T)
        gx = (P[:, 1:-1, 2:] - P[:, 1:-1, :-2]).astype(np.float64)
        gy = (P[:, 2:, 1:-1] - P[:, :-2, 1:-1]).astype(np.float64)
        gxx, gxy, gyy = gx * gx * W, gx * gy * W, gy * gy * W
        a, b, cc = total(gxx), total(gxy), total(gyy)
        bb1, bb2 = total(gxx * PX + gxy * PY), total(gxy * PX + gyy * PY)
        det = a * cc - b * b
        sing = np.abs(det) <= det_floor
        with np.errstate(all="ignore"):
            scale = 1.0 / det
            nx = (c[:, 0].astype(np.float64) + cc * scale * bb1 - b * scale * bb2).astype(np.float32)
            ny = (c[:, 1].astype(np.float64) - b * scale * bb1 + a * scale * bb2).astype(np.float32)
            step2 = (nx.astype(np.float64) - c[:, 0]) ** 2 + (ny.astype(np.float64) - c[:, 1]) ** 2
        mv = ~sing
        why[idx[sing]] = 3
        live[idx[sing]] = False
        im = idx[mv]
        cur[im, 0], cur[im, 1] = nx[mv], ny[mv]
        iters[im] += 1
        last_step2[im] = step2[mv]
        with np.errstate(all="ignore"):
            left = ~((nx >= 0) & (nx < cols) & (ny >= 0) & (ny < rows)) & mv
        conv_ = (step2 <= EPS_STEP2) & mv & ~left
        why[idx[left]] = 4
        why[idx[conv_]] = 1
        live[idx[left | conv_]] = False
    why[live] = 2
    out = cur.copy()
    with np.errstate(all="ignore"):
        far = (np.abs(out[:, 0] - start[:, 0]) > half) | (np.abs(out[:, 1] - start[:, 1]) > half)
    far |= ~np.isfinite(out).all(axis=1)
    if conv["revert"]:
        out[far] = start[far]
    report = dict(converged=why == 1, exhausted=why == 2, singular=why == 3, left_image=why == 4, reverted=far, iters=iters,
                  last_step2=last_step2, unreverted=cur)
    return out, report


def detect_candidates(img, num_features, grid_x, grid_y, threshold, conv=CONV, mask=None, **subpix_kw):
    """perform_griding on an image: dict(grid, score, nms, xy, response, cell, refined, report) - mask None is what the device's
    entry computes (every selected candidate); with a mask the masked ones are gone, as Grider_FAST returns them"""
    img = np.asarray(img, dtype=np.uint8)
    rows, cols = img.shape
    g = grid(cols, rows, num_features, grid_x, grid_y, conv)
    if g is None:
        raise ValueError("a cell of size 0")
    score, nms, rep = score_maps(img, g, threshold, conv)
    xy, resp, cell, rep2 = select(nms, g, mask, conv)
    rep.update(rep2)
    if len(xy):
        refined, rep3 = corner_subpix(img, xy.astype(np.float32), conv, **subpix_kw)
    else:  # perform_griding returns before the refinement
        refined, rep3 = np.zeros((0, 2), dtype=np.float32), None
    return dict(grid=g, score=score, nms=nms, xy=xy, response=resp, cell=cell, refined=refined, report=rep, subpix=rep3)


# ---- perform_detection_monocular (:1173-1297; this part is the reference's own text, not recalled) ---------------------------------
def occupancy_walk(cols, rows, pts, ids, mask, opts):
    """:1176-1242 -> (kept pts [m, 2] f32, kept ids, occupancy [h_close, w_close] bool, mask_updated, report)"""
    mpd = int(opts["min_px_dist"])
    wc, hc = int(np.float32(cols) / np.float32(mpd)), int(np.float32(rows) / np.float32(mpd))
    sx, sy = np.float32(cols) / np.float32(opts["grid_x"]), np.float32(rows) / np.float32(opts["grid_y"])
    occ = np.zeros((max(hc, 0), max(wc, 0)), dtype=bool)
    mask = np.zeros((rows, cols), dtype=np.uint8) if mask is None else np.asarray(mask, dtype=np.uint8)
    upd = mask.copy()
    kp, ki = [], []
    rep = dict(edge=0, outside_close=0, outside_grid=0, occupied=0, masked=0, painted=0, not_painted=0)
    pts = np.asarray(pts, dtype=np.float32).reshape(-1, 2)
    for p, i in zip(pts, np.asarray(ids, dtype=np.int64).reshape(-1)):
        x, y = int(p[0]), int(p[1])
        if x < 10 or x >= cols - 10 or y < 10 or y >= rows - 10:
            rep["edge"] += 1
            continue
        xc, yc = int(p[0] / np.float32(mpd)), int(p[1] / np.float32(mpd))
        if xc < 0 or xc >= wc or yc < 0 or yc >= hc:
            rep["outside_close"] += 1
            continue
        xg, yg = int(np.floor(p[0] / sx)), int(np.floor(p[1] / sy))
        if xg < 0 or xg >= opts["grid_x"] or yg < 0 or yg >= opts["grid_y"]:
            rep["outside_grid"] += 1
            continue
        if occ[yc, xc]:
            rep["occupied"] += 1
            continue
        if mask[y, x] > 127:
            rep["masked"] += 1
            continue
        occ[yc, xc] = True
        if x - mpd >= 0 and x + mpd < cols and y - mpd >= 0 and y + mpd < rows:
            upd[y - mpd:y + mpd + 1, x - mpd:x + mpd + 1] = 255
            rep["painted"] += 1
        else:
            rep["not_painted"] += 1
        kp.append(p), ki.append(int(i))
    return np.array(kp, dtype=np.float32).reshape(-1, 2), np.array(ki, dtype=np.int64), occ, upd, rep


def enough(n_kept, num_features):
    """:1246-1249 the return when fewer than 5 % are missing"""
    return (num_features - n_kept) < num_features * (1.0 - 0.95)


def accept(cand_xy_int, cand_refined, occ, upd, opts, currid):
    """the mask test of Grider_FAST on the candidates (at their integer pixel, on the updated mask) and :1265-1296 on the refined
    positions, in order -> (pts [m, 2] f32, ids [m], currid).  Refining every candidate and dropping the masked ones afterwards is
    the reference's order's equal: the refinement is per point."""
    mpd = np.float32(opts["min_px_dist"])
    hc, wc = occ.shape
    pts, ids = [], []
    for (x, y), p in zip(np.asarray(cand_xy_int).reshape(-1, 2), np.asarray(cand_refined, dtype=np.float32).reshape(-1, 2)):
        if upd[y, x] > 127:
            continue
        xc, yc = int(p[0] / mpd), int(p[1] / mpd)
        if xc < 0 or xc >= wc or yc < 0 or yc >= hc or occ[yc, xc]:
            continue
        occ[yc, xc] = True
        currid += 1
        pts.append(p), ids.append(currid)
    return np.array(pts, dtype=np.float32).reshape(-1, 2), np.array(ids, dtype=np.int64), currid


def perform_detection(cols, rows, candidates, mask, pts, ids, opts, currid):
    """perform_detection_monocular with the candidates handed in: candidates(num_features, grid_x, grid_y, threshold) ->
    (xy_int, refined), called only behind the 5 % return.  -> (pts, ids, currid, detected: bool)"""
    kp, ki, occ, upd, _ = occupancy_walk(cols, rows, pts, ids, mask, opts)
    if enough(len(ki), opts["num_features"]):
        return kp, ki, currid, False
    xy_int, refined = candidates()
    np_, ni, currid = accept(xy_int, refined, occ, upd, opts, currid)
    return np.concatenate([kp, np_]), np.concatenate([ki, ni]), currid, True


def detect_on_image(img, mask, pts, ids, opts, currid=0, conv=CONV):
    """the whole stage on the CPU: the restatement's own candidates (mask-independent, as the device's) through the host logic; a
    `mask_before` mutant filters inside the selection, on the updated mask, as Grider_FAST would"""
    rows, cols = np.asarray(img).shape

    def cands_for(upd):
        d = detect_candidates(img, opts["num_features"], opts["grid_x"], opts["grid_y"], opts["threshold"], conv,
                              mask=upd if conv["mask_before"] else None)
        return d["xy"], d["refined"]
    kp, ki, occ, upd, _ = occupancy_walk(cols, rows, pts, ids, mask, opts)
    if enough(len(ki), opts["num_features"]):
        return kp, ki, currid
    xy_int, refined = cands_for(upd)
    np_, ni, currid = accept(xy_int, refined, occ, upd, opts, currid)
    return np.concatenate([kp, np_]), np.concatenate([ki, ni]), currid
