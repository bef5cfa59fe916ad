"""numpy restatement of the two intake options the device runs (k_clahe.h, k_klt.hip): cv::CLAHE::apply on 8-bit data
(track_plane/TrackPlane.cpp:66-70: createCLAHE(10.0, Size(8, 8))) and the cv::pyrDown to Size(cols / 2.0, rows / 2.0) of
downsample_cameras (core/VioManager.cpp:279-289).

UNPINNED: OpenCV is neither on the build machine nor in the reference tree.  Every convention below is recalled from OpenCV's
published clahe.cpp, not verified against a file; each is one flag of CONV so that someone with OpenCV at hand can correct one
line, and each has a mutant - the convention changed, nothing else - that the tests show the comparison catches.  float32 where
OpenCV computes in float (np.float32 operations round once each: no contraction), integers elsewhere."""
import numpy as np

import klt_ref

BINS = 256
MAX_TILES = 16
CONV = dict(
    pad_both=True,        # an axis that does not divide extends BOTH axes: a divisible axis grows by a whole `tiles`
    reflect101=True,      # the extension is BORDER_REFLECT_101 (the edge pixel is not repeated)
    clip_floor=True,      # clip = max((int)(clip_limit * tile_area / 256), 1)
    clip_truncate=True,   # ... truncated, not rounded
    residual_strided=True,  # the residual goes to bins 0, step, 2 step, .. with step = max(256 / residual, 1)
    lut_round=True,       # lut = saturate(rint(cumsum * lut_scale)): to nearest ...
    half_even=True,       # ... ties to even (the LUT and the blended pixel)
    half_offset=True,     # tile coordinate = x * (1 / tile_w) - 0.5
    weight_unclamped=True,  # the weight comes from the unclamped tile index; the clamp follows
    tile_from_extended=True,  # tile size = extended size / tiles
    halve_floor=True,     # downsample_cameras: destination (w / 2, h / 2), where a pyramid level has ((w + 1) / 2, (h + 1) / 2)
)
MUTANTS = {
    "pad_needed_axis_only": dict(pad_both=False), "reflect_not_101": dict(reflect101=False), "clip_without_floor": dict(clip_floor=False),
    "clip_rounded": dict(clip_truncate=False), "residual_first_bins": dict(residual_strided=False), "lut_truncated": dict(lut_round=False),
    "round_half_up": dict(half_even=False), "no_half_offset": dict(half_offset=False), "clamp_before_weight": dict(weight_unclamped=False),
    "tile_from_unpadded": dict(tile_from_extended=False), "halve_to_ceil": dict(halve_floor=False),
}
F = np.float32


def mutant(name):
    return dict(CONV, **MUTANTS[name])


def _reflect(i, n, conv):
    """the extension's source index of any i >= 0: reflect-101, or (mutant) reflect with the edge pixel repeated"""
    if conv["reflect101"]:
        return klt_ref.reflect101(i, n)
    i = np.mod(np.asarray(i, dtype=np.int64), 2 * n)
    return np.where(i >= n, 2 * n - 1 - i, i)


def _round(x, conv):
    """cv::saturate_cast<uchar>(float) before the saturation: to nearest, ties to even"""
    x = np.asarray(x, dtype=F)
    return np.rint(x) if conv["half_even"] else np.floor(x + F(0.5))


def geometry(cols, rows, tiles_x, tiles_y, clip_limit, conv=CONV):
    """-> dict(ext_w, ext_h, tile_w, tile_h, area, clip, lut_scale): clahe.cpp's extension, tile size and clip limit.  A limit of
    the area or above clips nothing and is held at the area (no bin exceeds it)."""
    ext_w, ext_h = cols, rows
    bad_x, bad_y = cols % tiles_x != 0, rows % tiles_y != 0
    if bad_x or bad_y:
        if conv["pad_both"] or bad_x:
            ext_w = cols + tiles_x - cols % tiles_x
        if conv["pad_both"] or bad_y:
            ext_h = rows + tiles_y - rows % tiles_y
    if conv["tile_from_extended"]:
        tile_w, tile_h = ext_w // tiles_x, ext_h // tiles_y
    else:
        tile_w, tile_h = max(cols // tiles_x, 1), max(rows // tiles_y, 1)
    area = tile_w * tile_h
    clip = 0
    if clip_limit > 0.0:
        v = float(clip_limit) * area / BINS
        c = int(v) if conv["clip_truncate"] else int(np.rint(v))
        clip = area if v >= area else (max(c, 1) if conv["clip_floor"] else c)
    return dict(ext_w=ext_w, ext_h=ext_h, tile_w=tile_w, tile_h=tile_h, area=area, clip=clip, lut_scale=F(255.0) / F(area))


def tile_histograms(img, tiles_x, tiles_y, g, conv=CONV):
    """[tiles_y, tiles_x, 256] int64: the histograms of the tiles of the extended image (never made on the device: the tile's
    pixels are read through the index map)"""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    rows, cols = img.shape
    ys = _reflect(np.arange(tiles_y * g["tile_h"]), rows, conv)
    xs = _reflect(np.arange(tiles_x * g["tile_w"]), cols, conv)
    ext = img[np.ix_(ys, xs)]
    h = np.zeros((tiles_y, tiles_x, BINS), dtype=np.int64)
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            t = ext[ty * g["tile_h"]:(ty + 1) * g["tile_h"], tx * g["tile_w"]:(tx + 1) * g["tile_w"]]
            h[ty, tx] = np.bincount(t.reshape(-1), minlength=BINS)
    return h


def clip_redistribute(hist, clip, conv=CONV, report=None):
    """one tile's histogram [256] under the clip limit: bins above it cut to it, excess / 256 to every bin, the residual to bins
    0, step, 2 step, ..."""
    h = np.asarray(hist, dtype=np.int64).copy()
    if clip <= 0:
        return h
    excess = int(np.maximum(h - clip, 0).sum())
    h = np.minimum(h, clip)
    batch = excess // BINS
    residual = excess - batch * BINS
    h += batch
    if report is not None:
        report.append((excess, residual))
    if residual:
        if conv["residual_strided"]:
            step = max(BINS // residual, 1)
            k = np.arange(residual) * step
            h[k[k < BINS]] += 1
        else:
            h[:residual] += 1
    return h


def lut_table(img, tiles_x=8, tiles_y=8, clip_limit=10.0, conv=CONV, report=None):
    """[tiles_y, tiles_x, 256] uint8: lut[i] = saturate(rint((float) cumsum[i] * lut_scale)), lut_scale = 255.0f / tile_area"""
    rows, cols = np.asarray(img).shape
    g = geometry(cols, rows, tiles_x, tiles_y, clip_limit, conv)
    hist = tile_histograms(img, tiles_x, tiles_y, g, conv)
    lut = np.zeros((tiles_y, tiles_x, BINS), dtype=np.uint8)
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            cum = np.cumsum(clip_redistribute(hist[ty, tx], g["clip"], conv, report))
            v = cum.astype(F) * g["lut_scale"]
            v = _round(v, conv) if conv["lut_round"] else np.floor(v)
            lut[ty, tx] = np.clip(v, 0, 255).astype(np.uint8)
    return lut


def axis_weights(n, tile, tiles, conv=CONV):
    """per coordinate of an axis: (t1, t2, a, a1) - the two tile indices, clamped, and the weights a (of t2) and a1 = 1 - a"""
    f = np.arange(n).astype(F) * (F(1.0) / F(tile))
    if conv["half_offset"]:
        f = f - F(0.5)
    t1 = np.floor(f).astype(np.int64)
    t2 = t1 + 1
    if not conv["weight_unclamped"]:
        t1 = np.maximum(t1, 0)
    a = (f - t1.astype(F)).astype(F)
    a1 = (F(1.0) - a).astype(F)
    return np.clip(t1, 0, tiles - 1), np.clip(t2, 0, tiles - 1), a, a1


def apply(img, lut, g, conv=CONV):
    """the blend of the four neighbouring tiles' LUTs: res = (l11 xa1 + l12 xa) ya1 + (l21 xa1 + l22 xa) ya in float, in this order,
    dst = saturate(rint(res))"""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    rows, cols = img.shape
    tiles_y, tiles_x = lut.shape[:2]
    tx1, tx2, xa, xa1 = axis_weights(cols, g["tile_w"], tiles_x, conv)
    ty1, ty2, ya, ya1 = axis_weights(rows, g["tile_h"], tiles_y, conv)
    L = lut.astype(F)
    v = img.astype(np.int64)
    Y1, Y2, X1, X2 = ty1[:, None], ty2[:, None], tx1[None, :], tx2[None, :]
    top = (L[Y1, X1, v] * xa1[None, :] + L[Y1, X2, v] * xa[None, :]).astype(F)
    bot = (L[Y2, X1, v] * xa1[None, :] + L[Y2, X2, v] * xa[None, :]).astype(F)
    res = ((top * ya1[:, None]).astype(F) + (bot * ya[:, None]).astype(F)).astype(F)
    return np.clip(_round(res, conv), 0, 255).astype(np.uint8)


def clahe(img, tiles_x=8, tiles_y=8, clip_limit=10.0, conv=CONV):
    """cv::CLAHE::apply -> (equalised image, LUT table [tiles_y, tiles_x, 256])"""
    rows, cols = np.asarray(img).shape
    g = geometry(cols, rows, tiles_x, tiles_y, clip_limit, conv)
    lut = lut_table(img, tiles_x, tiles_y, clip_limit, conv)
    return apply(img, lut, g, conv), lut


def halve(img, conv=CONV):
    """downsample_cameras: cv::pyrDown to (int)(cols / 2.0) x (int)(rows / 2.0) - the pyramid's taps, rounding and reflect-101"""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w = img.shape
    ho, wo = (h // 2, w // 2) if conv["halve_floor"] else ((h + 1) // 2, (w + 1) // 2)
    src = img.astype(np.int64)
    rows = np.zeros((h, wo), dtype=np.int64)
    for k, t in enumerate(klt_ref.PYR_TAPS):
        rows += t * src[:, klt_ref.reflect101(2 * np.arange(wo) + k - 2, w)]
    out = np.zeros((ho, wo), dtype=np.int64)
    for k, t in enumerate(klt_ref.PYR_TAPS):
        out += t * rows[klt_ref.reflect101(2 * np.arange(ho) + k - 2, h), :]
    return ((out + klt_ref.PYR_ROUND) >> klt_ref.PYR_SHIFT).astype(np.uint8)


def intake(img, n_levels, hist="CLAHE", downsample=False, tiles_x=8, tiles_y=8, clip_limit=10.0, conv=CONV):
    """what ovp_klt_feed_image_opts leaves in the current half -> (pyramid [n_levels], LUT table or None): halve, equalise, pyramid"""
    if downsample:
        img = halve(img, conv)
    lut = None
    if hist == "CLAHE":
        img, lut = clahe(img, tiles_x, tiles_y, clip_limit, conv)
    elif hist == "HISTOGRAM":
        img = klt_ref.equalize_hist(img)
    elif hist != "NONE":
        raise ValueError(hist)
    pyr = [np.ascontiguousarray(img, dtype=np.uint8)]
    for _ in range(n_levels - 1):
        pyr.append(klt_ref.pyr_down(pyr[-1]))
    return pyr, lut
