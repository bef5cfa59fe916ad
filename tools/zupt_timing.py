"""Host-clock timing of UpdaterZeroVelocity::try_update with StateOptions::gpu_zupt off against on, in the same run - run on the
GPU box.
usage: python tools/zupt_timing.py [--out profiles/zupt_timing.json] [--windows 7] [--frames 8]
  (i)   try_update through the harness (hostlib.run_zupt, C = 11; the harness state holds no landmarks: n = 96).  One harness call
        is one window: `frames` consecutive standing camera frames of one 400 Hz / 10 Hz window each (42 readings, 246 rows), all
        accepted, on one state; the first frame pays the context's first-use allocations and is reported apart, the window's figure
        is the median of the others.  The two arms alternate (off, on, off, on, ...); median, minimum and maximum over `windows`.
  (ii)  ovp_zupt_update alone through the C-ABI at the size the issue names - 11 clones and 25 landmarks, n = 171 - host clock from
        entry to return (the call waits for its result), accepted and rejected, and the three kernels on events (a run of its own:
        the events add a synchronisation)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stats(v, scale=1.0, nd=2):
    v = np.asarray(v, dtype=np.float64) * scale
    return dict(median=round(float(np.median(v)), nd), min=round(float(v.min()), nd), max=round(float(v.max()), nd))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    from ov_plane_amd.build import build_host, build_lib, source_tree_hash

    build_lib()
    build_host()
    from ov_plane_amd import capi, hostlib
    from ov_plane_amd.synth import PROP_OPTS, _cov, make_imu_scenario, make_scene, quat_2_rot, state_layout

    po = dict(PROP_OPTS)
    res = dict(source_tree=source_tree_hash())
    # ---- (i) ----
    sc = make_scene(C=11, F=4, seed=91)
    x, imu, _, _ = make_imu_scenario(5, t_state=100.0, t_off=0.004, stationary=True, n_cam=a.frames)
    stamps = [100.0 + 0.1 * (k + 1) for k in range(a.frames)]
    per = {False: [], True: []}
    first = {False: [], True: []}
    hostlib.run_zupt(sc, x, imu, 100.0, stamps, 0.004, po, gpu_zupt=True, timing=True)  # (code objects loaded, both routes)
    hostlib.run_zupt(sc, x, imu, 100.0, stamps, 0.004, po, gpu_zupt=False, timing=True)
    for _ in range(a.windows):
        for on in (False, True):
            out = hostlib.run_zupt(sc, x, imu, 100.0, stamps, 0.004, po, gpu_zupt=on, timing=True)
            assert out["accepted"].all(), out["accepted"]
            per[on].append(float(np.median(out["try_update_ms"][1:])))
            first[on].append(float(out["try_update_ms"][0]))
    res["try_update"] = dict(
        unit="us per try_update, host clock; one window = the median of %d consecutive accepted frames on one state (the first frame "
             "apart); median / min / max of %d interleaved windows" % (a.frames - 1, a.windows),
        state=dict(clones=11, landmarks=0, n=int(sc.N)), readings=42, rows=246,
        option_off=stats(per[False], 1e3), option_on=stats(per[True], 1e3),
        first_frame_option_off=stats(first[False], 1e3), first_frame_option_on=stats(first[True], 1e3))
    print(json.dumps(res["try_update"], indent=1), flush=True)
    # ---- (ii) ----
    ids = state_layout(11, n_slam=25)
    n = int(ids["N"])
    P = _cov(11, ids, np.random.default_rng(3))
    x1, imu1, t0, t1 = make_imu_scenario(5, t_state=100.0, t_off=0.004, stationary=True)
    k0, k1 = int(np.searchsorted(imu1[:, 0], t0)), int(np.searchsorted(imu1[:, 0], t1))
    sel = imu1[k0 - 1:k1 + 1]  # 42 readings around the window (the ends not interpolated: the arithmetic is the same)
    R = quat_2_rot(x1["q"])
    thr = capi.lib().ovp_chi2_quantile_095(6 * (len(sel) - 1))
    ctx = capi.Context(n + 8, 12, 8)
    abi = {}
    for name, kw in (("accepted", dict(disparity_passed=True)), ("rejected", dict(vel_ok=False))):
        ts = {False: [], True: []}
        kms = []
        for timed in (False, True):
            for w in range(a.windows):
                t_w = []
                for _ in range(a.reps):
                    ctx.cov_upload(P)
                    ctx_sync = capi.lib().ovp_sync(ctx.handle)
                    assert ctx_sync == 0
                    t_in = time.perf_counter()
                    out = ctx.zupt_update(sel, 0, R, R, x1["bg"], x1["ba"], po, thr, time_kernels=timed, **kw)
                    t_w.append(time.perf_counter() - t_in)
                    assert out["accepted"] == (name == "accepted")
                    if timed:
                        kms.append(out["kernel_ms"])
                ts[timed].append(float(np.median(t_w[5:])))
        kms = np.array(kms)
        abi[name] = dict(call_us=stats(ts[False], 1e6), call_us_with_events=stats(ts[True], 1e6),
                         kernel_us=dict(gate=stats(kms[:, 0], 1e3), rows=stats(kms[:, 1], 1e3), apply=stats(kms[:, 2], 1e3)))
    ctx.close()
    res["ovp_zupt_update"] = dict(
        unit="us; call: host clock around capi.Context.zupt_update (ctypes marshalling included), median / min / max over %d windows "
             "of the window's median over %d calls; kernels: events around each, every call of the timed run" % (a.windows, a.reps - 5),
        state=dict(clones=11, landmarks=25, n=n), readings=int(len(sel)), rows=6 * (len(sel) - 1), **abi)
    print(json.dumps(res["ovp_zupt_update"], indent=1), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
