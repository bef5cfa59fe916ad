"""Timing of the epipolar check (ovp_klt_epipolar: k_epi_undistort, k_epi_models, k_epi_count, k_epi_select) and of the tracker's
step with it.

    python tools/epipolar_timing.py [--reps 20] [--out profiles/epipolar_timing.json]

n = 150 and 300 synthetic points (tests/epi_cases.py: 30 % outliers, projected through the project's radtan INTRINSICS so that the
undistortion runs too), max_iters 1000.  Per size seven windows; inside a window the arms are interleaved: the host clock of the
entry with the timer off (one upload, one enqueue, one wait), and the event times around the four kernels with the timer on.  A
window's figure is the median over its repetitions, the reported one the median of the seven with their spread (min, max).  Then
KltTracker.step at 752 x 480 (the 12 px translation scene of tests/klt_cases.py, its own points) with the check off against on,
interleaved in the same way.  The scene is one plane, so the check's models there are those of a degenerate configuration: the
step figures say what the stage costs in the loop, nothing about what it keeps.  There is no CPU comparator on either machine (no
OpenCV): nothing here says how the stage compares with the reference's."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KERNELS = ("epi_undistort", "epi_models", "epi_count", "epi_select")


def _spread(v):
    v = np.asarray(v, float)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "epipolar_timing.json"))
    a = ap.parse_args()
    import epi_cases
    import klt_cases
    from ov_plane_amd import capi, synth
    from ov_plane_amd.build import source_tree_hash

    ctx = capi.Context(64, 4, 8)
    cam = ("radtan", synth.INTRINSICS)
    res = dict(source_hash=source_tree_hash(), reps=a.reps, windows=7, max_iters=1000, sizes=[])
    kt = capi.KltTracker(ctx, 64, 48, 1, 15, 512)
    for n in (150, 300):
        sc = epi_cases.scene(n, 40 + n, outliers=0.3)
        px = [np.stack(synth.radtan_distort(p[:, 0].astype(np.float64), p[:, 1].astype(np.float64), synth.INTRINSICS), axis=1).astype(np.float32)
              for p in (sc["pts0"], sc["pts1"])]
        entry, ker = [], {k: [] for k in KERNELS}
        r = None
        for w in range(7):
            for arm in ("host", "kernel"):
                kt.timer(arm == "kernel")
                e, s = [], {k: [] for k in KERNELS}
                for _ in range(a.reps):
                    r = kt.epipolar(px[0], px[1], camera=cam, max_iters=1000, seed=7)
                    e.append(kt.last_epipolar_ms)
                    if arm == "kernel":
                        m = kt.kernel_ms()
                        for k in KERNELS:
                            s[k].append(m[k])
                if arm == "host":
                    entry.append(np.median(e))
                else:
                    for k in KERNELS:
                        ker[k].append(np.median(s[k]))
        kt.timer(False)
        row = dict(n=n, inliers=int(r["count"]), planted_inliers=int(sc["planted"].sum()), stop=r["stop"], entry_host_ms=_spread(entry))
        row.update({"k_%s_ms" % k: _spread(v) for k, v in ker.items()})
        res["sizes"].append(row)
        print(json.dumps(row), flush=True)
    kt.close()
    sc = klt_cases.scene("trans12_752x480")
    f = 0.9 * sc.width
    epi = dict(camera=("radtan", [f, f, 0.5 * (sc.width - 1), 0.5 * (sc.height - 1), 0.0, 0.0, 0.0, 0.0]), max_iters=1000, seed=7)
    kt = capi.KltTracker(ctx, sc.width, sc.height, sc.levels, klt_cases.WIN, 1024)
    ids = np.arange(len(sc.pts))
    off, on, kept = [], [], {}
    for w in range(7):
        for arm in ("off", "on"):
            t = []
            for _ in range(a.reps):
                kt.reset()
                kt.feed_image(sc.img0)
                kt.add_points(ids, sc.pts)
                ctx.sync()
                t0 = time.perf_counter()
                out = kt.step(sc.img1, epipolar=(epi if arm == "on" else None))
                t.append(1e3 * (time.perf_counter() - t0))
                kept[arm] = int(len(out[0]))
            (off if arm == "off" else on).append(np.median(t))
    kt.close()
    res["step"] = dict(scene=sc.name, width=sc.width, height=sc.height, levels=sc.levels, win=klt_cases.WIN, points=int(len(ids)),
                       kept_off=kept["off"], kept_on=kept["on"], step_check_off_host_ms=_spread(off), step_check_on_host_ms=_spread(on))
    print(json.dumps(res["step"]), flush=True)
    ctx.close()
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
