"""Times delayed initialisation of on-plane SLAM candidates: the device loop with plane rows (ovp_slam_delayed_init_planes,
StateOptions::gpu_dinit_planes) against the per-candidate host loop it replaces, and writes a JSON record under profiles/.
    python tools/dinit_planes_timing.py --out profiles/dinit_planes_timing.json

One mono scene of C = 11 (make_dinit_plane_scene, 3 planes in the state) with 10 and with 25 candidates, all on planes:
  (a) UpdaterSLAM::delayed_init through the host mirror, option off: the first plane candidate ends the device loop, everything takes
      delayed_init_host_loop (today's route)
  (b) the same with the option on: one device loop for the whole vector
  (c) ovp_slam_delayed_init_planes alone against ovp_slam_delayed_init on the same candidates stripped of their planes: what the extra
      m rows, the plane commit and the skipped second attempts cost
Host clock per call after a warm-up; `windows` windows of `reps` calls each, the median of the window means and their spread
(min .. max) are reported.  (a) and (b) include the same harness set-up (state construction, covariance upload); (c) times the
entry alone (context set-up outside the clock)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def windows_ms(fn, reps, windows, warmup=2):
    for _ in range(warmup):
        fn()
    means = []
    for _ in range(windows):
        ts = [fn() for _ in range(reps)]
        means.append(float(np.mean(ts)) * 1e3)
    return dict(median_ms=round(float(np.median(means)), 4), min_ms=round(min(means), 4), max_ms=round(max(means), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--once", action="store_true", help="one call of each device entry and nothing else (for a kernel trace)")
    a = ap.parse_args()
    from ov_plane_amd import capi, hostlib
    from ov_plane_amd.build import source_tree_hash
    from ov_plane_amd.synth import make_dinit_plane_scene

    rows = []
    for F in (10, 25):
        sc = make_dinit_plane_scene(C=11, F=F, n_planes=3, wrong_plane=0, outliers=0, seed=2, chi2_mult=2.0)
        o = capi.opts_from_scene(sc)
        cap = sc.N + 3 * sc.F

        def entry(planes):
            ctx = capi.Context(cap, sc.C, sc.F)
            ctx.cov_upload(sc.P)
            ctx.state_upload(sc)
            ctx.sync()
            t0 = time.perf_counter()
            if planes:
                r = ctx.slam_delayed_init_planes(o, sc.uv, sc.clone_idx, sc.n_meas, sc.p_FinG, plane_of_cand=sc.plane_id,
                                                 plane_state_id=sc.plane_state_id, cp=sc.cp, cp_fej=sc.cp_fej,
                                                 p_FinG_noplane=sc.p_FinG_noplane)
            else:
                r = ctx.slam_delayed_init(o, sc.uv, sc.clone_idx, sc.n_meas, sc.p_FinG)
            t = time.perf_counter() - t0
            ctx.close()
            entry.accepted = int(r["ok"].sum())
            return t

        def mirror(on):
            t0 = time.perf_counter()
            out = hostlib.run_updater(sc, "slam_delayed_init", state_planes=True, dinit_planes=on)
            mirror.route = out["route"]
            return time.perf_counter() - t0

        if a.once:
            entry(True)
            entry(False)
            continue
        c_pl = windows_ms(lambda: entry(True), a.reps, a.windows)
        acc_pl = entry.accepted
        c_free = windows_ms(lambda: entry(False), a.reps, a.windows)
        m_off = windows_ms(lambda: mirror(False), a.reps, a.windows)
        r_off = mirror.route
        m_on = windows_ms(lambda: mirror(True), a.reps, a.windows)
        r_on = mirror.route
        rows.append(dict(C=int(sc.C), candidates=int(sc.F), obs_per_candidate_max=int(sc.n_meas.max()), accepted_with_plane=acc_pl,
                         a_host_mirror_option_off=dict(m_off, route=r_off), b_host_mirror_option_on=dict(m_on, route=r_on),
                         a_minus_b_median_ms=round(m_off["median_ms"] - m_on["median_ms"], 4),
                         c_planes_entry=c_pl, c_plane_free_entry=c_free,
                         c_ratio=round(c_pl["median_ms"] / c_free["median_ms"], 3)))
        print(json.dumps(rows[-1]))
    if a.once:
        return
    rec = dict(what="delayed init of on-plane candidates: device loop with plane rows vs the per-candidate host loop "
                    "(tools/dinit_planes_timing.py); host clock, median of window means, spread = min .. max of the windows",
               source_tree_hash=source_tree_hash(), reps=a.reps, windows=a.windows, rows=rows)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
