"""Times ovp_plane_init against ovp_plane_init_general on the same scenes and writes a JSON record under profiles/.
    python tools/plane_init_timing.py --out profiles/plane_init_general_timing.json

C = 11 with 2 and with 4 planes of 13 features outside the state, const_init_chi2 = 1e9 (every plane is initialised).  Both
entries run in ONE process, interleaved: a window is `reps` calls of one entry, then `reps` of the other, seven windows; reported
are the medians of the window means and their spread.  Host clock = the entry; device clock = HIP events around the loop
(ovp_host_timing, the new entry only: ovp_plane_init synchronises per plane and has no loop to put events around).
Every call re-uploads covariance and tables outside the clock.  Also recorded: the plane_chi2 differences the GPU tests take
their bounds from (tests/test_plane_init_general_gpu.py)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stat(v):
    return dict(median_ms=round(float(np.median(v)), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=7)
    a = ap.parse_args()
    from ov_plane_amd import capi
    from ov_plane_amd.build import source_tree_hash
    from ov_plane_amd.synth import make_scene

    rows = []
    for n_planes in (2, 4):
        sc = make_scene(C=11, F=8 + 13 * n_planes, seed=7, n_planes=n_planes, feats_per_plane=13, planes_in_state_frac=0.0,
                        chi2_mult=1.0)
        o = capi.opts_from_scene(sc)
        ctx = capi.Context(sc.N + 3 * n_planes, sc.C, sc.F)
        ctx.plane_kernel_timer(2, True)

        def call(entry):
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

        acc = {"plane_init": ([], []), "plane_init_general": ([], [])}
        for e in acc:
            call(e), call(e)
        for _ in range(a.windows):
            for e in acc:
                ts = [call(e) for _ in range(a.reps)]
                acc[e][0].append(float(np.mean([t[0] for t in ts])))
                acc[e][1].append(float(np.mean([t[1] for t in ts])))
        rows.append(dict(scene="C=11, %d planes x 13 features, N=%d" % (n_planes, sc.N),
                         ovp_plane_init=dict(host_call=stat(acc["plane_init"][0])),
                         ovp_plane_init_general=dict(host_call=stat(acc["plane_init_general"][0]),
                                                     device_loop=stat(acc["plane_init_general"][1]))))
        print(json.dumps(rows[-1]))
        ctx.close()
    out = dict(what="ovp_plane_init against ovp_plane_init_general (tools/plane_init_timing.py), interleaved windows in one process; "
                    "median of window means, spread = min .. max of the windows",
               source_tree_hash=source_tree_hash(), reps=a.reps, windows=a.windows, rows=rows,
               synchronisations_per_call=dict(ovp_plane_init="1 + 2 per plane that reaches the gate (1 when it is rejected)",
                                              ovp_plane_init_general="1 (2 above 288 columns: the push-through's)"),
               launches_per_call=dict(ovp_plane_init="per plane: 3 blocking copies in front, chol(P), 16 kernels of the first-generation job, "
                                                     "2 result copies; accepted: 7 more kernels and 2 copies",
                                      ovp_plane_init_general="front: fill, chol(P), permutation; per plane: 6 of the loop + k_plane_init_keep; "
                                                             "back: covariance product (3), un-permutation, k_plane_init_solve, "
                                                             "k_plane_init_columns x 2, publication"))
    if a.out:
        prev = {}
        if os.path.exists(a.out):
            with open(a.out) as fh:
                prev = json.load(fh)
        for k in ("chi2_split_observed", "chi2_gate_scene"):
            if k in prev:
                out[k] = prev[k]
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
