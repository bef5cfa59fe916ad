"""The config-3 step of bench.py with two builds of libovplane_hip.so in ONE process, in interleaved windows: this checkout's and the
one OVP_LIB_AB names (the build of the commit in front).  For a change that must not cost anything.
    OVP_LIB_AB=path/to/parent/libovplane_hip.so python tools/plane_loop_ab_timing.py --out profiles/plane_loop_refactor_timing.json

Per window `reps` steps of bench.py's StepRunner (restore of the prior, uploads, plane loop, point update, results); per build the
median of `windows` window means and their spread (min .. max), the two builds interleaved window by window.  From ovp_host_timing:
the plane entry's host clocks per call (entry -> first launch, entry -> last enqueue, wait).  The plane loop's device time comes
from a second set of windows with the loop's event pair on (plane_kernel_timer 2: events cost microseconds, they stay out of the
step's windows).
Condition per figure: this <= other + the other's own window-to-window spread (max - min)."""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIGURES = ("step_ms", "plane_loop_device_ms", "plane_pre_ms", "plane_enqueue_ms", "plane_wait_ms")


def second_binding(path):
    """ov_plane_amd.capi once more as a module of its own, bound to the library at `path`."""
    from ov_plane_amd import capi

    spec = importlib.util.spec_from_file_location("ov_plane_amd.capi_ab", capi.__file__)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    mod.LIB_PATH = path
    return mod


def stat(v):
    return dict(median=round(float(np.median(v)), 5), min=round(float(min(v)), 5), max=round(float(max(v)), 5))


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

    sc = bench.make_workload("config3")
    runs = {"this": bench.StepRunner(capi, torch, sc, 0), "other": bench.StepRunner(second_binding(os.path.abspath(other)), torch, sc, 0)}
    rows = {k: {f: [] for f in FIGURES} for k in runs}

    def window(name, reps, device_clock):
        run = runs[name]
        with torch.cuda.stream(run.stream):
            run.ctx.plane_kernel_timer(enable=2 if device_clock else 0, reset=True)
            run.ctx.host_timing(reset=True)
            ts, _ = bench.run_block(run.step, reps)
            acc = run.ctx.host_timing(reset=True)
            run.ctx.plane_kernel_timer(enable=0, reset=False)
        if device_clock:
            rows[name]["plane_loop_device_ms"].append(acc["plane_loop_device_ms"] / acc["plane_calls"])
        else:
            rows[name]["step_ms"].append(1e3 * float(np.mean(ts)))
            for f in ("plane_pre_ms", "plane_enqueue_ms", "plane_wait_ms"):
                rows[name][f].append(acc[f] / acc["plane_calls"])

    import gc

    for name in runs:
        window(name, 150, False)  # (a fresh device runs its first steps at ramping clocks)
    for name in runs:
        for f in FIGURES:
            rows[name][f].clear()
    gc.collect()
    gc.disable()
    for device_clock, reps in ((False, a.reps), (True, max(5, a.reps // 2))):
        for _ in range(a.windows):
            for name in ("this", "other"):
                window(name, reps, device_clock)
    gc.enable()
    out = dict(what="config-3 step (bench.py StepRunner) with this checkout's library and with the one in front of it in one process, "
                    "interleaved windows (tools/plane_loop_ab_timing.py); ms; host clocks of the plane entry per call from "
                    "ovp_host_timing; condition per figure: this.median <= other.median + (other.max - other.min)",
               source_tree_hash=source_tree_hash(), other_library=os.path.basename(os.path.dirname(os.path.abspath(other))) + "/" +
               os.path.basename(other), reps=a.reps, windows=a.windows, figures={})
    ok = True
    for f in FIGURES:
        t, o = stat(rows["this"][f]), stat(rows["other"][f])
        spread = o["max"] - o["min"]
        fine = bool(t["median"] <= o["median"] + spread)
        ok &= fine
        out["figures"][f] = dict(this=t, other=o, other_spread=round(spread, 5), within=fine)
        print(f, json.dumps(out["figures"][f]))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
    for r in runs.values():
        r.close()
    if not ok:
        print("A FIGURE OF THIS BUILD IS ABOVE THE OTHER BUILD'S BY MORE THAN ITS SPREAD")
        sys.exit(1)


if __name__ == "__main__":
    main()
