"""Times ovp_plane_init and ovp_plane_init_general of two builds of libovplane_hip.so in ONE process, in interleaved windows: this
checkout's and the one OVP_LIB_AB names (the build of the commit in front), as tools/plane_loop_ab_timing.py does for the plane loop.
    OVP_LIB_AB=path/to/parent/libovplane_hip.so python tools/plane_init_timing.py --out profiles/plane_init_retire_timing.json

C = 11 with 2 and with 4 planes of 13 features outside the state, const_init_chi2 = 1e9 (every plane is initialised).  A window is
`reps` calls of one entry of one build; the four (build, entry) pairs take turns window by window, seven windows each; reported are
the medians of the window means and their spread (min .. max).  Host clock = the entry; device clock = HIP events around the loop
(ovp_host_timing; 0 for an entry that has no loop to put events around).  Every call re-uploads covariance and tables outside the
clock.
Condition per entry: this.median <= other.median + (other.max - other.min)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from plane_loop_ab_timing import second_binding  # noqa: E402  (tools/ is the script's directory)

ENTRIES = ("plane_init", "plane_init_general")


def stat(v):
    return dict(median_ms=round(float(np.median(v)), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=7)
    a = ap.parse_args()
    other = os.environ.pop("OVP_LIB_AB", None)
    if not other:
        sys.exit("OVP_LIB_AB: the library to compare against")
    from ov_plane_amd import capi
    from ov_plane_amd.build import source_tree_hash
    from ov_plane_amd.synth import make_scene

    builds = {"this": capi, "other": second_binding(os.path.abspath(other))}
    rows, ok = [], True
    for n_planes in (2, 4):
        sc = make_scene(C=11, F=8 + 13 * n_planes, seed=7, n_planes=n_planes, feats_per_plane=13, planes_in_state_frac=0.0,
                        chi2_mult=1.0)
        ctxs = {}
        for name, mod in builds.items():
            ctxs[name] = mod.Context(sc.N + 3 * n_planes, sc.C, sc.F)
            ctxs[name].plane_kernel_timer(2, True)

        def call(build, entry):
            ctx, o = ctxs[build], builds[build].opts_from_scene(sc)
            ctx.cov_upload(sc.P)
            ctx.state_upload(sc)
            ctx.batch_upload_scene(sc)
            ctx.sync()
            ctx.host_timing(reset=True)
            t0 = time.perf_counter()
            r = getattr(ctx, entry)(o, sc.plane_id, sc.cp, 5.0, 1e9)
            t = (time.perf_counter() - t0) * 1e3
            assert r["ok"].all()
            return t, ctx.host_timing()["plane_loop_device_ms"]

        pairs = [(b, e) for b in builds for e in ENTRIES]
        acc = {p: ([], []) for p in pairs}
        for p in pairs:
            call(*p), call(*p)
        for _ in range(a.windows):
            for p in pairs:
                ts = [call(*p) for _ in range(a.reps)]
                acc[p][0].append(float(np.mean([t[0] for t in ts])))
                acc[p][1].append(float(np.mean([t[1] for t in ts])))
        row = dict(scene="C=11, %d planes x 13 features, N=%d" % (n_planes, sc.N))
        for e in ENTRIES:
            t, o = stat(acc[("this", e)][0]), stat(acc[("other", e)][0])
            spread = round(o["max_ms"] - o["min_ms"], 4)
            fine = bool(t["median_ms"] <= o["median_ms"] + spread)
            ok &= fine
            row["ovp_" + e] = dict(host_call=dict(this=t, other=o, other_spread_ms=spread, within=fine),
                                   device_loop=dict(this=stat(acc[("this", e)][1]), other=stat(acc[("other", e)][1])))
        rows.append(row)
        print(json.dumps(row))
        for ctx in ctxs.values():
            ctx.close()
    out = dict(what="ovp_plane_init and ovp_plane_init_general with this checkout's library and with the one in front of it in one "
                    "process, interleaved windows (tools/plane_init_timing.py); median of window means, spread = min .. max of the "
                    "windows; condition per entry: this.median <= other.median + (other.max - other.min)",
               source_tree_hash=source_tree_hash(), other_library=os.path.basename(os.path.dirname(os.path.abspath(other))) + "/" +
               os.path.basename(other), reps=a.reps, windows=a.windows, rows=rows)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
    if not ok:
        print("AN ENTRY OF THIS BUILD IS ABOVE THE OTHER BUILD'S BY MORE THAN ITS SPREAD")
        sys.exit(1)


if __name__ == "__main__":
    main()
