"""bench.py's headline step (config 3) and its config-2 step with two builds of libovplane_hip.so in ONE process, in interleaved
windows: this checkout's and the one OVP_LIB_AB names (the build of the commit in front), as tools/plane_loop_ab_timing.py does for
the plane loop.  For a change of the point update's host code that must not cost anything.
    OVP_LIB_AB=path/to/parent/libovplane_hip.so python tools/point_update_ab_timing.py --out profiles/point_update_refactor_timing.json

Per window `reps` steps of bench.py's StepRunner; per build and workload the median of `windows` window means and their spread
(min .. max), the two builds interleaved window by window.  From ovp_host_timing: the point update's host clocks per call (enqueue:
entry -> second half enqueued, wait: for the published results).
Condition per figure: this <= other + the other's own window-to-window spread (max - min)."""
import argparse
import gc
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

FIGURES = ("step_ms", "point_enqueue_ms", "point_wait_ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--windows", type=int, default=7)
    a = ap.parse_args()
    other = os.environ.pop("OVP_LIB_AB", None)
    if not other:
        sys.exit("OVP_LIB_AB: the library to compare against")
    import torch

    import bench
    from ov_plane_amd import capi
    from ov_plane_amd.build import source_tree_hash
    from plane_loop_ab_timing import second_binding, stat

    capi_ab = second_binding(os.path.abspath(other))
    out = dict(what="bench.py's StepRunner step at config 3 (the headline) and config 2 with this checkout's library and with the one "
                    "in front of it in one process, interleaved windows (tools/point_update_ab_timing.py); ms; host clocks of the "
                    "point update per call from ovp_host_timing; condition per figure: this.median <= other.median + (other.max - "
                    "other.min)",
               source_tree_hash=source_tree_hash(), other_library=os.path.basename(os.path.dirname(os.path.abspath(other))) + "/" +
               os.path.basename(other), reps=a.reps, windows=a.windows, workloads={})
    ok = True
    for wname in ("config3", "config2"):
        sc = bench.make_workload(wname)
        runs = {"this": bench.StepRunner(capi, torch, sc, 0), "other": bench.StepRunner(capi_ab, torch, sc, 0)}
        rows = {k: {f: [] for f in FIGURES} for k in runs}

        def window(name, reps):
            run = runs[name]
            with torch.cuda.stream(run.stream):
                run.ctx.host_timing(reset=True)
                ts, _ = bench.run_block(run.step, reps)
                acc = run.ctx.host_timing(reset=True)
            rows[name]["step_ms"].append(1e3 * float(np.mean(ts)))
            for f in ("point_enqueue_ms", "point_wait_ms"):
                rows[name][f].append(acc[f] / acc["point_calls"])

        for name in runs:
            window(name, 150)  # (a fresh device runs its first steps at ramping clocks)
        for name in runs:
            for f in FIGURES:
                rows[name][f].clear()
        gc.collect()
        gc.disable()
        for _ in range(a.windows):
            for name in ("this", "other"):
                window(name, a.reps)
        gc.enable()
        figs = out["workloads"][wname] = {}
        for f in FIGURES:
            t, o = stat(rows["this"][f]), stat(rows["other"][f])
            spread = o["max"] - o["min"]
            fine = bool(t["median"] <= o["median"] + spread)
            ok &= fine
            figs[f] = dict(this=t, other=o, other_spread=round(spread, 5), within=fine)
            print(wname, f, json.dumps(figs[f]))
        for r in runs.values():
            r.close()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
    if not ok:
        print("A FIGURE OF THIS BUILD IS ABOVE THE OTHER BUILD'S BY MORE THAN ITS SPREAD")
        sys.exit(1)


if __name__ == "__main__":
    main()
