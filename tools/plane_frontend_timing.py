"""Times the fused plane front end (ovp_plane_fit_refine) against the per-plane pairs of calls it replaces (ovp_plane_fitting +
ovp_plane_optimize for every plane) on the same problems, and writes a JSON record under profiles/.
    python tools/plane_frontend_timing.py --out profiles/plane_frontend_timing.json

Two frames: P = 4 planes seen from C = 11 clones (the session shape) and P = 20 planes (the plane count of config 3), stereo
tracks, free planes with outliers and an in-state plane among them.  Host clock of the calls (what the caller waits for), after a
warm-up; `windows` windows of `reps` frames per variant, the two variants INTERLEAVED window by window in one process; per variant
the median of the window means and their spread (min .. max).  The pairs are fed the way the host mirror feeds them: the RANSAC
of a plane, then the refinement of its inliers with the poses looked up per observation (the pose table is taken from the fused
entry outside the clock; building the per-plane problems is outside the clock too, the ctypes binding of each call is inside it on
both sides).
Also: the host mirror's frame (UpdaterMSCKF::update through hostlib.run_msckf_update: triangulation, plane fit, plane loop, point
update, with the marshalling of the scene on both sides of the comparison) with StateOptions::gpu_fused_plane_fit off and on, on a
camera-0 scene of C = 10 with 4 planes of 20 features, interleaved in the same way.
Condition: fused <= sum of the pairs + the spread (max - min) of that sum."""
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
    from ov_plane_amd.synth import make_plane_frontend_scene
    from tests import plane_frontend_ref as R

    def frame(P, seed):
        kinds = [dict(n=14, outliers=2, stereo=5), dict(n=10, kind="fixed", n_slam=2, stereo=3), dict(n=12, stereo=4),
                 dict(n=16, stereo=6, cam1only=2, short=4)]
        return make_plane_frontend_scene(C=11, seed=seed, planes=[dict(kinds[k % 4]) for k in range(P)])

    rows = []
    for P, seed in ((4, 3), (20, 4)):
        sc = frame(P, seed)
        ctx = capi.Context(sc.N, sc.C, 4)
        ctx.state_upload(sc)
        ctx.cameras_upload(sc)
        args = R.fused_args(sc)
        ref = ctx.plane_fit_refine(**args)
        poses = ref["poses"]

        def fused():
            t0 = time.perf_counter()
            ctx.plane_fit_refine(**args)
            return (time.perf_counter() - t0) * 1e3

        def pairs():
            """The chain of tests/plane_frontend_ref.py over the device's per-plane calls; the clock runs inside the calls only."""
            t = [0.0]

            def fit(pts, mn, mc, var):
                t0 = time.perf_counter()
                o = ctx.plane_fitting([0, len(pts)], pts, mn, mc, var)
                t[0] += time.perf_counter() - t0
                return dict(ok=bool(o["ok"][0]), abcd=o["abcd"][0], inlier=o["inlier"])

            def opt(pb):
                t0 = time.perf_counter()
                o = ctx.plane_optimize([pb])[0]
                t[0] += time.perf_counter() - t0
                return o

            out = R.chain(sc, poses, fit, opt)
            assert (out["ok"] == ref["ok"]).all() and out["p_FinG"].tobytes() == ref["p_FinG"].tobytes()
            return t[0] * 1e3

        for _ in range(2):
            fused(), pairs()
        wf, wp = [], []
        for _ in range(a.windows):
            wf.append(float(np.mean([fused() for _ in range(a.reps)])))
            wp.append(float(np.mean([pairs() for _ in range(a.reps)])))
        sf, sp = stat(wf), stat(wp)
        spread = sp["max_ms"] - sp["min_ms"]
        rows.append(dict(scene="C=11, %d planes, %d features, %d observations" % (P, sc.F, int(sc.n_meas.sum())), planes=P,
                         planes_ok=int(ref["ok"].sum()), fused=sf, per_plane_pairs=sp, pairs_spread_ms=round(spread, 4),
                         fused_not_slower=bool(sf["median_ms"] <= sp["median_ms"] + spread)))
        print(json.dumps(rows[-1]))
        ctx.close()
    # host mirror: one frame of UpdaterMSCKF::update, option off / on
    from ov_plane_amd import hostlib
    from ov_plane_amd.build import build_host
    from ov_plane_amd.synth import make_scene

    build_host()
    scm = make_scene(C=10, F=150, seed=72, n_planes=4, feats_per_plane=20, chi2_mult=99999.0, px_noise=0.25, err_scale=0.05)
    fit = dict(min_feat=5, max_cond=200.0, variant=0)

    def frame_ms(on):
        t0 = time.perf_counter()
        hostlib.run_msckf_update(scm, triangulate=True, fit_planes=fit, fused_plane_fit=on)
        return (time.perf_counter() - t0) * 1e3

    for _ in range(2):
        frame_ms(False), frame_ms(True)
    w_off, w_on = [], []
    for _ in range(a.windows):
        w_off.append(float(np.mean([frame_ms(False) for _ in range(a.reps)])))
        w_on.append(float(np.mean([frame_ms(True) for _ in range(a.reps)])))
    host_frame = dict(scene="C=10, 150 features, 4 planes x 20, N=%d" % scm.N, per_plane=stat(w_off), fused=stat(w_on))
    print(json.dumps(dict(host_mirror_frame=host_frame)))
    out = dict(what="ovp_plane_fit_refine against the per-plane pairs ovp_plane_fitting + ovp_plane_optimize on the same problems "
                    "(tools/plane_frontend_timing.py); host clock of the C-ABI calls through ctypes, median of window means, spread = "
                    "min .. max of the windows; the pairs' figure includes the ctypes marshalling of plane_fitting / plane_optimize, "
                    "the fused figure that of plane_fit_refine",
               source_tree_hash=source_tree_hash(), reps=a.reps, windows=a.windows, rows=rows, host_mirror_frame=host_frame)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
    if not all(r["fused_not_slower"] for r in rows):
        print("FUSED ENTRY SLOWER THAN THE PAIRS IT REPLACES")
        sys.exit(1)


if __name__ == "__main__":
    main()
