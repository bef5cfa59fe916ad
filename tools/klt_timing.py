"""Timing of the image front end (ovp_klt_feed_image, ovp_klt_track: equalisation, image pyramid, pyramidal Lucas-Kanade).

    python tools/klt_timing.py [--reps 20] [--out profiles/klt_timing.json]

752 x 480, six levels, window 15, 150 and 500 points on the 12 px translation scene of tests/klt_cases.py.  Per size seven windows;
inside a window the arms are interleaved: the host clock of feed_image and of track with the timer off (the C calls alone; feed_image
does not wait for the device, so a stream synchronisation in front of it keeps the previous call's work out of its figure), and, in
a run of its own, the event times around the equalise kernels, the pyramid launches together and k_klt_track with the timer on
(the events add a stream synchronisation per entry).  A window's figure is the median over its repetitions, the reported one the
median of the seven with their spread (min, max).  Also the mean iteration count per level.  There is no CPU comparator on either
machine (no OpenCV): nothing here says how the stage compares with the reference's."""
import argparse
import json
import os
import sys

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "klt_timing.json"))
    a = ap.parse_args()
    import klt_cases
    from ov_plane_amd import capi
    from ov_plane_amd.build import source_tree_hash

    sc = klt_cases.scene("trans12_752x480")
    rng = np.random.default_rng(77)
    ctx = capi.Context(64, 4, 8)
    res = dict(source_hash=source_tree_hash(), scene=sc.name, width=sc.width, height=sc.height, levels=sc.levels, win=klt_cases.WIN,
               reps=a.reps, windows=7, sizes=[])
    for n in (150, 500):
        pts = np.stack([rng.uniform(12, sc.width - 24, n), rng.uniform(12, sc.height - 12, n)], 1).astype(np.float32)
        kt = capi.KltTracker(ctx, sc.width, sc.height, sc.levels, klt_cases.WIN, 512)
        feed, track, k_eq, k_pyr, k_trk = [], [], [], [], []
        iters = status = None
        for w in range(7):
            for arm in ("host", "kernel"):
                kt.timer(arm == "kernel")
                f, t, e, p, k = [], [], [], [], []
                for r in range(a.reps):
                    kt.feed_image(sc.img0)
                    ctx.sync()
                    kt.feed_image(sc.img1)
                    f.append(kt.last_feed_ms)
                    if arm == "kernel":
                        m = kt.kernel_ms()
                        e.append(m["equalize"]), p.append(m["pyramid"])
                    ctx.sync()
                    _, status = kt.track(pts)
                    t.append(kt.last_track_ms)
                    if arm == "kernel":
                        k.append(kt.kernel_ms()["track"])
                if arm == "host":
                    feed.append(np.median(f)), track.append(np.median(t))
                else:
                    k_eq.append(np.median(e)), k_pyr.append(np.median(p)), k_trk.append(np.median(k))
            iters = kt.iters(n)
        kt.close()
        res["sizes"].append(dict(points=n, status_1=int(status.sum()), feed_image_host_ms=_spread(feed), track_host_ms=_spread(track),
                                 equalize_kernels_ms=_spread(k_eq), pyramid_launches_ms=_spread(k_pyr), k_klt_track_ms=_spread(k_trk),
                                 mean_iterations_per_level=[float(x) for x in iters.mean(axis=0)]))
        print(json.dumps(res["sizes"][-1]), flush=True)
        with open(a.out, "w") as fh:  # (after every size: a run that is cut short keeps what it has)
            json.dump(res, fh, indent=1)
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
