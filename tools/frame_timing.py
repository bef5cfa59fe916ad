"""Timing of the fused hand-over of a frame's tracks (ovp_klt_match_frame: k_klt_track, the epipolar kernels, k_klt_keep_append in
one enqueue) against the unfused sequence of existing entries (ovp_klt_track + ovp_klt_epipolar + the keep rule on the host +
ovp_featdb_append), on the same tree in the same run.

    python tools/frame_timing.py [--reps 20] [--out profiles/frame_timing.json]

752 x 480, six levels, window 15 (the 12 px translation scene of tests/klt_cases.py), 150 and 500 points on a jittered grid, a
mask rectangle, the epipolar check on (max_iters 1000) and off.  Both images are fed once; what is timed is the hand-over alone,
on the host clock, the database reset (host only) outside the clock.  Per configuration seven windows; inside a window the arms
alternate call by call (fused, unfused, fused, ..); a window's figure per arm is the median over its repetitions, the reported one
the median of the seven with their spread (min, max).  Then, in a pass of its own with the timer on, the event time around
k_klt_keep_append.  Both arms go through the Python binding: the unfused one carries three ctypes wrappers and the keep rule in
numpy where the fused one carries one wrapper, so part of any difference is binding overhead and not the device's or the bus's.
Without the check the unfused sequence still needs uv_norm for the database and gets it from ovp_klt_epipolar with one hypothesis
(what KltTracker.step(database=) does): its RANSAC kernels run on one hypothesis, the fused entry runs k_epi_undistort alone.
The scene is one plane: the check's models are those of a degenerate configuration, and the figures say what the stages cost,
nothing about what they keep."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _spread(v):
    v = np.asarray(v, float)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_timing.json"))
    a = ap.parse_args()
    import klt_cases
    from ov_plane_amd import capi
    from ov_plane_amd.build import source_tree_hash

    sc = klt_cases.scene("trans12_752x480", levels=6)
    w, h = sc.width, sc.height
    f = 0.9 * w
    cam = ("radtan", [f, f, 0.5 * (w - 1), 0.5 * (h - 1), 0.0, 0.0, 0.0, 0.0])
    mask = np.zeros((h, w), dtype=np.uint8)
    mask[200:280, 300:420] = 255
    ctx = capi.Context(64, 4, 8)
    kt = capi.KltTracker(ctx, w, h, 6, klt_cases.WIN, 1024)
    db = capi.FeatureDatabase(ctx, 1024, 8)
    kt.feed_image(sc.img0)
    kt.feed_image(sc.img1)
    res = dict(source_hash=source_tree_hash(), reps=a.reps, windows=7, width=w, height=h, levels=6, win=klt_cases.WIN, max_iters=1000, rows=[])

    def fused(pts, ids, epi, check):
        return kt.match_frame(pts, ids, 1.0, mask, epi, check=check, database=db)["keep"]

    def unfused(pts, ids, epi, check):
        p, st = kt.track(pts, pts)
        e = kt.epipolar(pts, p, st, **epi)
        if check:
            st = e["mask"]
        x, y = p[:, 0], p[:, 1]
        xi, yi = np.clip(x, 0, w - 1).astype(np.int64), np.clip(y, 0, h - 1).astype(np.int64)
        keep = (st != 0) & ~(x < 0) & ~(y < 0) & (np.trunc(x) < w) & (np.trunc(y) < h) & ~(mask[yi, xi] > 127)
        db.update_feature(1.0, ids[keep], p[keep], e["uvn1"][keep])
        return keep

    for n in (150, 500):
        pts = klt_cases._grid_points(np.random.default_rng(900 + n), w, h, n, 30)
        ids = np.arange(n, dtype=np.int64)
        for check in (True, False):
            epi = dict(camera=cam, max_iters=1000 if check else 1, seed=7)
            arms = {"fused": fused, "unfused": unfused}
            t = {k: [] for k in arms}
            keeps = {}
            for _ in range(7):
                one = {k: [] for k in arms}
                for _ in range(a.reps):
                    for arm, fn in arms.items():
                        db.reset()
                        ctx.sync()
                        t0 = time.perf_counter()
                        keeps[arm] = fn(pts, ids, epi, check)
                        ctx.sync()   # (the append of the unfused sequence does not wait: the clock stops when the table is written)
                        one[arm].append(1e3 * (time.perf_counter() - t0))
                for arm in arms:
                    t[arm].append(np.median(one[arm]))
            kt.timer(True)
            k = []
            for _ in range(7 * a.reps):
                db.reset()
                fused(pts, ids, epi, check)
                k.append(kt.kernel_ms()["keep_append"])
            kt.timer(False)
            row = dict(n=n, check=check, kept=int(keeps["fused"].sum()), same_keep=bool(np.array_equal(keeps["fused"], keeps["unfused"])),
                       fused_host_ms=_spread(t["fused"]), unfused_host_ms=_spread(t["unfused"]), k_klt_keep_append_ms=_spread(k))
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
    db.close()
    kt.close()
    ctx.close()
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
