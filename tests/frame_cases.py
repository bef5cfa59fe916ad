"""Cases for the fused hand-over of a frame's tracks (ovp_klt_match_frame): the planted three-frame sequence, the compaction edges
(sizes at the wave and chunk boundaries of k_klt_keep_append, keep patterns shaped by the image mask), the slot-order scenario, and
a numpy restatement of the survivor / slot plan (ov_plane_frame_plan.h) for the CPU test."""
import functools

import numpy as np

import klt_cases

PLANTED_SHIFTS = [(0, 5), (6, 0), (-5, -5)]
EDGE_SIZES = (1, 9, 10, 63, 64, 65, 1023, 1024, 1025, 4096)
PATTERNS = ("all", "none", "first", "last", "every_second", "chunk_dropped")
STAMPS = (10.0, 10.05, 10.1)


def camera(width, height):
    """the radtan camera of the sequence's tests: ("radtan", intrinsics [8])"""
    return "radtan", [0.9 * width, 0.9 * width, 0.5 * (width - 1), 0.5 * (height - 1), 0.0, 0.0, 0.0, 0.0]


def epipolar_opts(width, height):
    return dict(camera=camera(width, height), max_iters=64, seed=3)


@functools.lru_cache(maxsize=None)
def planted_sequence():
    """klt_cases.sequence() with three wrong tracks planted as tests/test_epipolar_gpu.py plants them: around three of its points
    the patch of frame 0 is pasted into frame 1 away from where the scene's motion (4 px to the right) takes it, by PLANTED_SHIFTS
    -> (sequence, frames, the planted ids)"""
    q = klt_cases.sequence()
    frames = [f.copy() for f in q["frames"]]
    pick = [i for i, (x, y) in enumerate(q["pts"][:12]) if 16 <= y <= 45 and 12 <= x <= 44][:3]
    assert len(pick) == 3
    for i, (dx, dy) in zip(pick, PLANTED_SHIFTS):
        x, y = int(round(q["pts"][i][0])), int(round(q["pts"][i][1]))
        frames[1][y - 10 + dy:y + 11 + dy, x - 10 + 4 + dx:x + 11 + 4 + dx] = q["frames"][0][y - 10:y + 11, x - 10:x + 11]
    return q, frames, q["ids"][pick]


def edge_points(n):
    """n points of the sequence's textured first frame, one per pixel (so that the image mask can name each of them alone), at the
    pixel's centre: with the same image fed twice the KLT leaves each where it is, half a pixel from every pixel border
    -> (ids [n] int64, pts [n, 2] f32)"""
    x0, x1, y0, y1 = 8, 88, 6, 58      # 80 x 52 = 4160 pixels, away from the border
    assert n <= (x1 - x0) * (y1 - y0)
    k = np.arange(n)
    pts = np.stack([x0 + k % (x1 - x0) + 0.5, y0 + k // (x1 - x0) + 0.5], axis=-1).astype(np.float32)
    return 5000 + 3 * k.astype(np.int64), pts


def pattern(name, n):
    """the intended keep vector [n] bool"""
    k = np.arange(n)
    if name == "all":
        return np.ones(n, dtype=bool)
    if name == "none":
        return np.zeros(n, dtype=bool)
    if name == "first":
        return k == 0
    if name == "last":
        return k == n - 1
    if name == "every_second":
        return k % 2 == 0
    if name == "chunk_dropped":        # the second chunk of 1024 where there is one, else the first (everything below 1025)
        c = 1 if n > 1024 else 0
        return ~((k >= 1024 * c) & (k < 1024 * (c + 1)))
    raise KeyError(name)


def mask_of(name, n, pts, width, height):
    """the image mask that shapes the pattern: 255 at the pixel of every point that is to go ("none": 255 everywhere)"""
    if name == "none":
        return np.full((height, width), 255, dtype=np.uint8)
    m = np.zeros((height, width), dtype=np.uint8)
    gone = ~pattern(name, n)
    m[pts[gone, 1].astype(np.int64), pts[gone, 0].astype(np.int64)] = 255
    return m


def slot_order_case():
    """max_slots 8, max_meas 4.  Ids 1..6 are appended (slots 0..5: the free list is a stack with slot 0 on top), 2, 3 and 5 are
    marked and cleaned up, which pushes their slots 1, 2, 4 back in ascending id - the stack now hands out 4, 2, 1, 6, 7: out of
    order.  Then a frame interleaves the known ids 1, 4, 6 with the fresh ids 11..15; the fresh 12 and 14 and the known 4 are masked
    out.  -> dict(S, M, first_ids, marked, frame_ids, frame_keep)"""
    return dict(S=8, M=4, first_ids=np.arange(1, 7, dtype=np.int64), marked=np.array([2, 5, 3], dtype=np.int64),
                frame_ids=np.array([11, 1, 12, 4, 13, 14, 6, 15], dtype=np.int64),
                frame_keep=np.array([1, 1, 0, 0, 1, 0, 1, 1], dtype=bool))


def plan_reference(keep, fresh, slot, free_slots):
    """numpy restatement of ov_plane::frame_plan: the survivors in order; a known id keeps its slot, the k-th fresh survivor takes
    free_slots[k] -> (kept_index int32, slot int32, n_fresh_kept)"""
    keep, fresh = np.asarray(keep, dtype=bool), np.asarray(fresh, dtype=bool)
    idx = np.flatnonzero(keep).astype(np.int32)
    rank = np.cumsum(keep & fresh) - 1                 # inclusive count - 1: the exclusive rank of a fresh survivor
    out = np.asarray(slot, dtype=np.int32)[idx].copy()
    f = fresh[idx]
    out[f] = np.asarray(free_slots, dtype=np.int32)[rank[idx][f]]
    return idx, out, int((keep & fresh).sum())
