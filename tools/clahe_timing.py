"""Timing of the intake options (ovp_klt_feed_image_opts: histogram_method CLAHE, downsample_cameras).

    python tools/clahe_timing.py [--reps 20] [--out profiles/clahe_timing.json]

752 x 480, six levels, on the 12 px translation scene of tests/klt_cases.py.  Seven windows; inside a window the arms are
interleaved.  Arms: the feed with CLAHE against the same call with HISTOGRAM, and the feed of a 1504 x 960 image with downsample
(under HISTOGRAM) against the feed of the same image halved beforehand (752 x 480).  Per arm the host clock of the C call with the
timer off (the call does not wait for the device, so a stream synchronisation in front of it keeps the previous call's work out of
its figure), the host clock of call + synchronisation (what a caller that needs the image waits for), and, in a run of its own,
the event times around the halving, the equalisation as a whole, k_clahe_lut and k_clahe_apply each, and the pyramid launches
together with the timer on (the events add a stream synchronisation per entry).  A window's figure is the median over its
repetitions, the reported one the median of the seven with their spread (min, max).  There is no CPU comparator on either machine
(no OpenCV): nothing here says how the stage compares with the reference's."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clahe_timing.json"))
    a = ap.parse_args()
    import klt_cases
    from ov_plane_amd import capi
    from ov_plane_amd.build import source_tree_hash

    sc = klt_cases.scene("trans12_752x480")
    big = klt_cases.render(klt_cases.texture(2 * sc.width, 2 * sc.height, 13, cell=10.0), 2 * sc.width, 2 * sc.height)
    ctx = capi.Context(64, 4, 8)
    kt = capi.KltTracker(ctx, sc.width, sc.height, sc.levels, klt_cases.WIN, 16)
    small = kt.halve(big)
    arms = {
        "clahe": (sc.img0, capi.intake_defaults(hist_method="CLAHE")),
        "histogram": (sc.img0, capi.intake_defaults(hist_method="HISTOGRAM")),
        "downsample_1504x960": (big, capi.intake_defaults(hist_method="HISTOGRAM", downsample=1)),
        "prehalved_752x480": (small, capi.intake_defaults(hist_method="HISTOGRAM")),
    }
    keys = ("call_host_ms", "call_and_sync_host_ms", "halve_ms", "equalize_ms", "k_clahe_lut_ms", "k_clahe_apply_ms", "pyramid_launches_ms")
    win = {name: {k: [] for k in keys} for name in arms}
    for name, (img, o) in arms.items():  # warm-up: code objects, the full-size buffers
        for _ in range(3):
            kt.feed_image_opts(img, o)
        ctx.sync()
    for w in range(7):
        for mode in ("host", "kernel"):
            kt.timer(mode == "kernel")
            rep = {name: {k: [] for k in keys} for name in arms}
            for r in range(a.reps):
                for name, (img, o) in arms.items():
                    ctx.sync()
                    t0 = time.perf_counter()
                    kt.feed_image_opts(img, o)
                    ctx.sync()
                    both = 1e3 * (time.perf_counter() - t0)
                    if mode == "host":
                        rep[name]["call_host_ms"].append(kt.last_feed_ms), rep[name]["call_and_sync_host_ms"].append(both)
                    else:
                        m = kt.kernel_ms()
                        for k, src in (("halve_ms", "halve"), ("equalize_ms", "equalize"), ("k_clahe_lut_ms", "clahe_lut"),
                                       ("k_clahe_apply_ms", "clahe_apply"), ("pyramid_launches_ms", "pyramid")):
                            rep[name][k].append(m[src])
            for name in arms:
                for k in keys:
                    if rep[name][k]:
                        win[name][k].append(np.median(rep[name][k]))
    kt.close()
    ctx.close()
    res = dict(source_hash=source_tree_hash(), scene=sc.name, width=sc.width, height=sc.height, levels=sc.levels, reps=a.reps, windows=7,
               tiles=[8, 8], clip=10.0, arms={name: {k: _spread(v) for k, v in win[name].items()} for name in arms})
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
