"""Timing of the detector (ovp_klt_detect: k_fast_score_nms, k_fast_select, k_fast_subpix) and of the tracker's loop with it.

    python tools/fast_timing.py [--reps 20] [--out profiles/fast_timing.json]

752 x 480 (the 12 px translation scene of tests/klt_cases.py, equalised) at the three shipped configurations (sim: 250 points,
20 x 20, threshold 15; EuRoC: 200, 12 x 12, 15; rpng_plane: 200, 12 x 12, 30).  Per configuration seven windows; inside a window
the arms are interleaved: the host clock of the entry with the timer off (one enqueue, one wait), and the event times around the
three kernels with the timer on.  A window's figure is the median over its repetitions, the reported one the median of the seven
with their spread (min, max).  Then KltTracker.step over the same two-image sequence, seeded with every second point of a detection on
the first image, with detect off (tracking alone) against detect on (the top-up on the previous half, which with half of the
points missing really detects - recorded as step_on_detected and step_on_points_added - then tracking of the larger set),
interleaved in the same way.  There is
no CPU comparator on either machine (no OpenCV): nothing here says how the stage compares with the reference's."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CONFIGS = {"sim": dict(num_features=250, grid_x=20, grid_y=20, threshold=15, min_px_dist=15),
           "euroc_mav": dict(num_features=200, grid_x=12, grid_y=12, threshold=15, min_px_dist=15),
           "rpng_plane": dict(num_features=200, grid_x=12, grid_y=12, threshold=30, min_px_dist=20)}


def _spread(v):
    v = np.asarray(v, float)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fast_timing.json"))
    a = ap.parse_args()
    import klt_cases
    from ov_plane_amd import capi
    from ov_plane_amd.build import source_tree_hash

    sc = klt_cases.scene("trans12_752x480")
    ctx = capi.Context(64, 4, 8)
    res = dict(source_hash=source_tree_hash(), scene=sc.name, width=sc.width, height=sc.height, levels=sc.levels, win=klt_cases.WIN,
               reps=a.reps, windows=7, configs=[])
    for name, det in CONFIGS.items():
        kt = capi.KltTracker(ctx, sc.width, sc.height, sc.levels, klt_cases.WIN, 1024, detector=det)
        kt.feed_image(sc.img0)
        ctx.sync()
        entry, k_score, k_sel, k_sub = [], [], [], []
        n = 0
        for w in range(7):
            for arm in ("host", "kernel"):
                kt.timer(arm == "kernel")
                e, s1, s2, s3 = [], [], [], []
                for r in range(a.reps):
                    n = len(kt.detect_candidates(0)["xy"])
                    e.append(kt.last_detect_ms)
                    if arm == "kernel":
                        m = kt.kernel_ms()
                        s1.append(m["score_nms"]), s2.append(m["select"]), s3.append(m["subpix"])
                if arm == "host":
                    entry.append(np.median(e))
                else:
                    k_score.append(np.median(s1)), k_sel.append(np.median(s2)), k_sub.append(np.median(s3))
        kt.timer(False)
        # the loop: a caller's seed against the tracker's own top-up.  The seed is every second point of a detection on the first
        # image: with half of num_features missing the top-up of `detect on` passes the 5 % return and really detects
        # (last_detected and the number of points it adds are recorded); `detect off` tracks the same seed
        full_pts, full_ids = kt.detect(0)
        seed_pts, seed_ids = full_pts[::2], full_ids[::2]
        off, on = [], []
        detected, topped = True, 0
        for w in range(7):
            for arm in ("off", "on"):
                t = []
                for r in range(a.reps):
                    kt.reset()
                    kt.feed_image(sc.img0)
                    kt.add_points(seed_ids, seed_pts)
                    ctx.sync()
                    t0 = time.perf_counter()
                    kt.step(sc.img1, detect=(arm == "on"))
                    t.append(1e3 * (time.perf_counter() - t0))
                    if arm == "on":
                        detected &= bool(kt.last_detected)
                        topped = int(len(kt.last_topped[0]) - len(seed_ids))
                (off if arm == "off" else on).append(np.median(t))
        kt.close()
        res["configs"].append(dict(config=name, detector=det, candidates=n, seeded=int(len(seed_ids)), step_on_detected=bool(detected),
                                   step_on_points_added=topped, detect_entry_host_ms=_spread(entry),
                                   k_fast_score_nms_ms=_spread(k_score), k_fast_select_ms=_spread(k_sel), k_fast_subpix_ms=_spread(k_sub),
                                   step_detect_off_host_ms=_spread(off), step_detect_on_host_ms=_spread(on)))
        print(json.dumps(res["configs"][-1]), flush=True)
        with open(a.out, "w") as fh:  # (after every configuration: a run that is cut short keeps what it has)
            json.dump(res, fh, indent=1)
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
