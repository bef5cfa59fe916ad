"""Host-clock timing of Propagator::propagate_and_clone with StateOptions::gpu_propagate off against on, in the same run - run on
the GPU box.
usage: python tools/propagate_timing.py [--out profiles/propagate_timing.json] [--windows 7] [--reps 40]
  (i)   propagate_and_clone through the harness (hostlib.run_propagate, C = 11; the harness state holds no landmarks: n = 96), one
        400 Hz / 10 Hz window of 42 readings.  One harness call builds a state and times its one call, so every figure includes the
        first-use allocations of a fresh context; a window is the median of `reps` calls.  The two arms alternate (off, on, ...);
        median, minimum and maximum over `windows`.
  (ii)  ovp_propagate_and_clone alone through the C-ABI at n = 96 and at n = 171 (11 clones + 25 landmarks), host clock from entry
        to return (the call waits for its result) on a warm context, against the three calls ovp_cov_propagate + ovp_cov_clone +
        ovp_cov_augment_dt + ovp_sync fed with the entry's Phi, Q, last_w and v (the host integration NOT included in that arm);
        the entry's four steps on events in a run of its own (the events add a synchronisation).
  (iii) the session's `propagation` column (timing.txt, mean over frames 10.. of 120, C = 11, 25 landmarks) with the option off
        and on, alternating."""
import argparse
import json
import os
import sys
import tempfile
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
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--frames", type=int, default=120)
    a = ap.parse_args()
    from ov_plane_amd.build import build_host, build_lib, source_tree_hash

    build_lib()
    build_host()
    from ov_plane_amd import capi, closed_loop, hostlib
    from ov_plane_amd.sim import Simulator, synthetic_trajectory
    from ov_plane_amd.synth import PROP_OPTS, _cov, make_imu_scenario, make_scene, state_layout

    po = dict(PROP_OPTS)
    res = dict(source_tree=source_tree_hash())
    x, imu, t0, t1 = make_imu_scenario(5, t_state=100.0, t_off=0.004)
    # ---- (i) ----
    sc = make_scene(C=11, F=4, seed=91)
    per = {False: [], True: []}
    for on in (True, False):  # (code objects loaded, both routes)
        hostlib.run_propagate(sc, x, imu, 100.0, 100.1, 0.004, po, gpu_propagate=on, timing=True)
    for _ in range(a.windows):
        for on in (False, True):
            t_w = [hostlib.run_propagate(sc, x, imu, 100.0, 100.1, 0.004, po, gpu_propagate=on, timing=True)["propagate_ms"]
                   for _ in range(a.reps)]
            per[on].append(float(np.median(t_w)))
    res["propagate_and_clone"] = dict(
        unit="us per propagate_and_clone, host clock, on a state just built (first-use allocations of its context included); one "
             "window = the median of %d calls; median / min / max of %d interleaved windows" % (a.reps, a.windows),
        state=dict(clones=11, landmarks=0, n=int(sc.N)), readings=42,
        option_off=stats(per[False], 1e3), option_on=stats(per[True], 1e3))
    print(json.dumps(res["propagate_and_clone"], indent=1), flush=True)
    # ---- (ii) ----
    k0, k1 = int(np.searchsorted(imu[:, 0], t0)), int(np.searchsorted(imu[:, 0], t1))
    sel = imu[k0 - 1:k1 + 1]  # 42 readings around the window (the ends not interpolated: the arithmetic is the same)
    abi = {}
    for n_slam in (0, 25):
        ids = state_layout(11, n_slam=n_slam)
        n = int(ids["N"])
        P = _cov(11, ids, np.random.default_rng(3))
        dt_id = 15  # (the column behind the IMU block)
        ctx = capi.Context(n + 8, 12, 8)
        ts = {"entry": [], "entry_events": [], "three_calls": []}
        kms = []
        ctx.cov_upload(P)
        ref = ctx.propagate_and_clone(sel, 0, x, po, dt_id=dt_id)
        d = np.concatenate([ref["last_w"], ref["v"]])
        for w in range(a.windows):
            for arm in ("three_calls", "entry", "entry_events"):
                t_w = []
                for _ in range(a.reps):
                    ctx.cov_upload(P)
                    assert capi.lib().ovp_sync(ctx.handle) == 0
                    t_in = time.perf_counter()
                    if arm == "three_calls":
                        ctx.cov_propagate(0, [0], [15], ref["Phi"], ref["Q"])
                        ctx.cov_clone(0, 6)
                        ctx.cov_augment_dt(n, dt_id, d)
                        capi.lib().ovp_sync(ctx.handle)
                    else:
                        out = ctx.propagate_and_clone(sel, 0, x, po, dt_id=dt_id, time_kernels=arm == "entry_events")
                    t_w.append(time.perf_counter() - t_in)
                    if arm == "entry_events":
                        kms.append(out["kernel_ms"])
                ts[arm].append(float(np.median(t_w[5:])))
        ctx.close()
        kms = np.array(kms)
        abi["n%d" % n] = dict(state=dict(clones=11, landmarks=n_slam, n=n), entry_us=stats(ts["entry"], 1e6),
                              entry_us_with_events=stats(ts["entry_events"], 1e6), three_calls_us=stats(ts["three_calls"], 1e6),
                              kernel_us=dict(integrate=stats(kms[:, 0], 1e3), ekf_propagation=stats(kms[:, 1], 1e3),
                                             clone_dt=stats(kms[:, 2], 1e3), publish=stats(kms[:, 3], 1e3)))
    res["ovp_propagate_and_clone"] = dict(
        unit="us; host clock around the ctypes calls (marshalling included), median / min / max over %d windows of the window's "
             "median over %d calls; three_calls = ovp_cov_propagate + ovp_cov_clone + ovp_cov_augment_dt + ovp_sync WITHOUT the host "
             "integration that produces Phi, Q; kernels: events around each step, every call of the timed arm" % (a.windows, a.reps - 5),
        readings=int(len(sel)), form="sequential (the only one built)", **abi)
    print(json.dumps(res["ovp_propagate_and_clone"], indent=1), flush=True)
    # ---- (iii) ----
    col = {False: [], True: []}
    tot = {False: [], True: []}
    for _ in range(3):
        for on in (False, True):
            sim = Simulator(synthetic_trajectory(duration=30.0), num_pts=100, num_pts_plane=100)
            d_out = tempfile.mkdtemp()
            closed_loop.run_session(sim, n_frames=a.frames, C=11, max_slam=25, out_dir=d_out, gpu_propagate=on)
            with open(os.path.join(d_out, "timing.txt")) as f:
                head = [h.strip() for h in f.readline().lstrip("#").strip().split(",")]
                rows = np.array([[float(v) for v in ln.strip().split(",")] for ln in f if ln.strip()])
            col[on].append(float(np.mean(rows[10:, head.index("propagation")])))
            tot[on].append(float(np.mean(rows[10:, head.index("total")])))
    res["session"] = dict(unit="ms per frame, mean over frames 10.. of %d (C = 11, 25 landmarks); median / min / max of 3 interleaved "
                               "sessions per arm; the parent's figure for the option-off column: 0.1205 "
                               "(profiles/r06_final_session_timing.json)" % a.frames,
                          propagation_option_off=stats(col[False], 1e3, 4), propagation_option_on=stats(col[True], 1e3, 4),
                          total_option_off=stats(tot[False], 1e3, 4), total_option_on=stats(tot[True], 1e3, 4))
    print(json.dumps(res["session"], indent=1), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
