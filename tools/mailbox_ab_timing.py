"""Two builds of libovplane_hip.so in ONE process, in interleaved windows, by the method of tools/plane_loop_ab_timing.py: this
checkout's and the one OVP_LIB_AB names (the build of the commit in front).  For a change of the result handshake that must not
cost anything.
    OVP_LIB_AB=path/to/parent/libovplane_hip.so python tools/mailbox_ab_timing.py --out profiles/mailbox_refactor_timing.json

Figures (ms; per build the median of `windows` window means, the two builds interleaved window by window):
  step_ms, plane_pre_ms / plane_enqueue_ms / plane_wait_ms   the config-3 step of bench.py's StepRunner and the plane entry's host
                                                              clocks per call (ovp_host_timing)
  slam_update_ms, slam_delayed_init_ms, cov_propagate_ms     host clock around the call (inputs uploaded before it, outside the clock)
                                                              at the session's sizes (tools/session_timing.py: 11 clones, 25 landmarks)
Condition per figure: this.median <= other.median + (other.max - other.min)."""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

STEP = ("step_ms", "plane_pre_ms", "plane_enqueue_ms", "plane_wait_ms")
ENTRIES = ("slam_update_ms", "slam_delayed_init_ms", "cov_propagate_ms")


class Entries:
    """the three small entries on a context of one build"""

    def __init__(self, capi):
        from ov_plane_amd.synth import make_scene, make_slam_scene

        self.capi = capi
        self.slam = make_slam_scene(C=11, n_slam=25, seed=6)
        self.cand = make_scene(C=11, F=4, seed=8, ragged=True, chi2_mult=0.6)
        self.ctx = capi.Context(max(self.slam.N, self.cand.N) + 12, 11, 32)
        self.Phi = np.eye(15) + 1e-3 * np.random.default_rng(0).standard_normal((15, 15))
        self.Q = 1e-6 * np.eye(15)

    def window(self, reps):
        capi, ctx, t = self.capi, self.ctx, {k: 0.0 for k in ENTRIES}
        for _ in range(reps):
            for name, sc in (("slam_update_ms", self.slam), ("slam_delayed_init_ms", self.cand), ("cov_propagate_ms", self.slam)):
                ctx.cov_upload(sc.P)
                ctx.state_upload(sc)
                ctx.sync()
                o = capi.opts_from_scene(sc)
                t0 = time.perf_counter()
                if name == "slam_update_ms":
                    ctx.slam_update(o, sc.uv, sc.clone_idx, sc.n_meas, sc.p_FinG, sc.p_FinG_fej, sc.lm_id)
                elif name == "slam_delayed_init_ms":
                    ctx.slam_delayed_init(o, sc.uv, sc.clone_idx, sc.n_meas, sc.p_FinG)
                else:
                    ctx.cov_propagate(0, [0], [15], self.Phi, self.Q)
                t[name] += time.perf_counter() - t0
        return {k: 1e3 * v / reps for k, v in t.items()}


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

    libs = {"this": capi, "other": second_binding(os.path.abspath(other))}
    sc = bench.make_workload("config3")
    runs = {k: bench.StepRunner(m, torch, sc, 0) for k, m in libs.items()}
    small = {k: Entries(m) for k, m in libs.items()}
    rows = {k: {f: [] for f in STEP + ENTRIES} for k in libs}

    def window(name, reps, keep=True):
        run = runs[name]
        with torch.cuda.stream(run.stream):
            run.ctx.host_timing(reset=True)
            ts, _ = bench.run_block(run.step, reps)
            acc = run.ctx.host_timing(reset=True)
        got = dict(step_ms=1e3 * float(np.mean(ts)), **{f: acc[f] / acc["plane_calls"] for f in STEP[1:]})
        got.update(small[name].window(reps))
        if keep:
            for f, v in got.items():
                rows[name][f].append(v)

    for name in libs:
        window(name, 150, keep=False)  # (a fresh device runs its first steps at ramping clocks)
    gc.collect()
    gc.disable()
    for _ in range(a.windows):
        for name in ("this", "other"):
            window(name, a.reps)
    gc.enable()
    out = dict(what="this checkout's library and the one in front of it in one process, interleaved windows (tools/mailbox_ab_timing.py); "
                    "ms; condition per figure: this.median <= other.median + (other.max - other.min)",
               source_tree_hash=source_tree_hash(), other_library=os.path.basename(os.path.dirname(os.path.abspath(other))) + "/" +
               os.path.basename(other), reps=a.reps, windows=a.windows, figures={})
    ok = True
    for f in STEP + ENTRIES:
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
    for s in small.values():
        s.ctx.close()
    if not ok:
        print("A FIGURE OF THIS BUILD IS ABOVE THE OTHER BUILD'S BY MORE THAN ITS SPREAD")
        sys.exit(1)


if __name__ == "__main__":
    main()
