"""Times the plane loop with and without general on-plane features (ovp_msckf_plane_update_general) and writes a JSON record
under profiles/.
    python tools/general_planes_timing.py --out profiles/general_planes_timing.json

One camera-0 scene of C = 11 with 4 planes of 12 features each, all of which fit the device batch, so that the SAME system can be
run three ways under forced accepts:
  (a) every on-plane feature in the batch (ovp_msckf_plane_update's enqueue: the new entry with no general feature on a plane)
  (b) four features of ONE plane moved to the general batch: that plane runs k_plane_feat_gen + k_plane_gen_pair in front of its
      assembly, and every plane of the call runs the camera-table commit behind k_chol2
  (c) every second on-plane feature moved (a handful per plane, all four planes)
and one long-track scene (C = 40, tracks of up to 40 views; the features above 32 views are general) against the same scene
without those features (what the loop did before).
Per variant: the loop on the device clock (HIP events around the whole loop, ovp_host_timing [7]) and the host clock of the call,
per call after a warm-up; `windows` windows of `reps` calls, the median of the window means and their spread (min .. max).
(b) - (a) on the device clock is one plane's extra kernel time plus the commits; nothing here is a promise of a figure.
Also recorded: the largest difference of plane_chi2 between (a) and (c) - the bound of
tests/test_general_planes_gpu.py::test_batch_and_general_features_are_one_system is 4 x the value seen on the first run."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def windows_of(fn, reps, windows, warmup=2):
    for _ in range(warmup):
        fn()
    dev, host = [], []
    for _ in range(windows):
        ts = [fn() for _ in range(reps)]
        dev.append(float(np.mean([t[0] for t in ts])))
        host.append(float(np.mean([t[1] for t in ts])))

    def stat(v):
        return dict(median_ms=round(float(np.median(v)), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4))

    return dict(device_loop=stat(dev), host_call=stat(host))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=7)
    a = ap.parse_args()
    from ov_plane_amd import capi
    from ov_plane_amd.build import source_tree_hash
    from ov_plane_amd.synth import make_long_plane_scene, make_scene

    def runner(sc, batch, gen):
        """One context per variant; every call re-uploads the covariance and the tables (outside the clock)."""
        o = capi.opts_from_scene(sc)
        force = np.ones(sc.cp.shape[0], dtype=np.uint8)
        W = min(32, sc.uv.shape[1])
        ctx = capi.Context(sc.N, sc.C, max(len(batch), 1))
        ctx.plane_kernel_timer(2, True)
        last = {}

        def call():
            ctx.cov_upload(sc.P)
            ctx.state_upload(sc)
            ctx.cameras_upload(sc)
            ctx.batch_upload(sc.uv[batch][:, :W], sc.clone_idx[batch][:, :W], sc.n_meas[batch], sc.p_FinG[batch])
            ctx.sync()
            ctx.host_timing(reset=True)
            t0 = time.perf_counter()
            r = ctx.plane_update_general(o, sc.plane_id[batch], sc.cp, sc.cp_fej, sc.plane_state_id, sc=sc, feats=gen,
                                         force_decision=force)
            t = (time.perf_counter() - t0) * 1e3
            last["chi2"] = r["chi2"].copy()
            return ctx.host_timing()["plane_loop_device_ms"], t

        return ctx, call, last

    rows = []
    sc = make_scene(C=11, F=60, seed=5, n_planes=4, feats_per_plane=12, chi2_mult=1.0, ragged=True)
    on = np.where(sc.plane_id > 0)[0]
    one_plane = on[sc.plane_id[on] == 1][:4]
    variants = [("a_all_in_batch", np.array([], dtype=np.int64)), ("b_four_general_on_one_plane", one_plane),
                ("c_every_second_general", on[::2])]
    chi2 = {}
    for name, gen in variants:
        batch = np.array([f for f in range(sc.F) if f not in set(gen.tolist())], dtype=np.int64)
        ctx, call, last = runner(sc, batch, gen)
        rec = windows_of(call, a.reps, a.windows)
        chi2[name] = last["chi2"]
        rows.append(dict(scene="C=11, 4 planes x 12 features, N=%d" % sc.N, variant=name, general_features=int(len(gen)), **rec))
        print(json.dumps(rows[-1]))
        ctx.close()
    med = {r["variant"]: r["device_loop"]["median_ms"] for r in rows}
    extra = dict(one_plane_extra_device_ms=round(med["b_four_general_on_one_plane"] - med["a_all_in_batch"], 4),
                 four_planes_extra_device_ms=round(med["c_every_second_general"] - med["a_all_in_batch"], 4),
                 plane_chi2_max_abs_diff_a_vs_c=float(np.abs(chi2["a_all_in_batch"] - chi2["c_every_second_general"]).max()),
                 plane_chi2=[float(v) for v in chi2["a_all_in_batch"]])
    print(json.dumps(extra))
    scl = make_long_plane_scene(C=40, n_planes=4, feats_per_plane=6, n_free=4, seed=1, chi2_mult=1.0)
    short = np.where(scl.n_meas <= 32)[0]
    long_ = np.where(scl.n_meas > 32)[0]
    for name, gen in (("long_tracks_left_out", np.array([], dtype=np.int64)), ("long_tracks_general", long_)):
        ctx, call, _ = runner(scl, short, gen)
        rec = windows_of(call, a.reps, a.windows)
        rows.append(dict(scene="C=40, 4 planes x 6 features, N=%d" % scl.N, variant=name, general_features=int(len(gen)),
                         general_on_planes=int((scl.plane_id[gen] > 0).sum()), **rec))
        print(json.dumps(rows[-1]))
        ctx.close()
    out = dict(what="plane loop with and without general on-plane features (tools/general_planes_timing.py); device clock = HIP events "
                    "around the loop, host clock = the call; median of window means, spread = min .. max of the windows",
               source_tree_hash=source_tree_hash(), reps=a.reps, windows=a.windows, rows=rows, **extra)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
