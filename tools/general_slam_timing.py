"""Times the general SLAM entries against the host forms they replace, and writes a JSON record under profiles/.
    python tools/general_slam_timing.py --out profiles/general_slam_timing.json

update:       25 stereo landmarks (make_stereo_slam_scene, two in-state planes) at C = 11 and 20 - ovp_slam_update_general alone, and
              UpdaterSLAM::update through the host mirror with gpu_general_slam on (the entry) and off (update_dense: host Jacobians,
              a marginal covariance download per landmark, host gate, ovp_ekf_update)
delayed init: 10 stereo candidates at C = 16 - ovp_slam_delayed_init_general alone, and UpdaterSLAM::delayed_init with the option on
              (one device loop) and off (the per-candidate host loop)
Host clock per call, averaged; the host-mirror figures include the same harness set-up (state construction, covariance upload) on
both sides, reported separately as the difference of the two."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _clock(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e3


def stereo_candidates(C, F, seed):
    from ov_plane_amd.synth import make_stereo_scene

    return make_stereo_scene(C=C, F=F, seed=seed, stereo_frac=0.8, chi2_mult=1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    from ov_plane_amd import capi, hostlib
    from ov_plane_amd.build import source_tree_hash
    from ov_plane_amd.synth import make_stereo_slam_scene

    update_rows, init_rows = [], []
    for C in (11, 20):
        sc = make_stereo_slam_scene(C=C, n_slam=25, seed=11, n_planes=2, stereo_frac=1.0)
        pid = np.asarray(sc.plane_id, dtype=np.int64)
        sid = np.where(pid > 0, np.asarray(sc.plane_state_id)[np.maximum(pid, 1) - 1], -1).astype(np.int32)
        cp, cpf = np.asarray(sc.cp)[np.maximum(pid, 1) - 1], np.asarray(sc.cp_fej)[np.maximum(pid, 1) - 1]
        o = capi.opts_from_scene(sc)
        ctx = capi.Context(sc.N, sc.C, sc.F)
        ctx.state_upload(sc)
        ctx.cameras_upload(sc)

        def entry():
            ctx.cov_upload(sc.P)
            ctx.slam_update_general(o, sc.uv, sc.clone_idx, sc.cam_idx, sc.n_meas, sc.p_FinG, sc.p_FinG_fej, sc.lm_id, sid, cp, cpf)

        t_upload = _clock(lambda: ctx.cov_upload(sc.P), a.reps)
        t_entry = _clock(entry, a.reps) - t_upload
        ctx.close()
        t_on = _clock(lambda: hostlib.run_updater(sc, "slam_update", general_slam=True), max(3, a.reps // 4))
        t_off = _clock(lambda: hostlib.run_updater(sc, "slam_update"), max(3, a.reps // 4))
        update_rows.append(dict(C=C, landmarks=int(sc.F), new_obs_per_landmark_max=int(sc.n_meas.max()), general_entry_ms=round(t_entry, 4),
                                host_mirror_general_ms=round(t_on, 3), host_mirror_update_dense_ms=round(t_off, 3),
                                dense_minus_general_ms=round(t_off - t_on, 3)))
        print(update_rows[-1])
    sc = stereo_candidates(16, 10, 3)
    o = capi.opts_from_scene(sc)
    cap = sc.N + 3 * sc.F

    def dinit():
        ctx = capi.Context(cap, sc.C, sc.F)
        ctx.cov_upload(sc.P)
        ctx.state_upload(sc)
        ctx.cameras_upload(sc)
        t0 = time.perf_counter()
        ctx.slam_delayed_init_general(o, sc.uv, sc.clone_idx, sc.cam_idx, sc.n_meas, sc.p_FinG)
        t = time.perf_counter() - t0
        ctx.close()
        return t

    dinit()
    t_entry = float(np.mean([dinit() for _ in range(max(3, a.reps // 4))])) * 1e3
    t_on = _clock(lambda: hostlib.run_updater(sc, "slam_delayed_init", general_slam=True), max(3, a.reps // 4))
    t_off = _clock(lambda: hostlib.run_updater(sc, "slam_delayed_init"), max(3, a.reps // 4))
    init_rows.append(dict(C=int(sc.C), candidates=int(sc.F), obs_per_candidate_max=int(sc.n_meas.max()), general_entry_ms=round(t_entry, 4),
                          host_mirror_device_loop_ms=round(t_on, 3), host_mirror_per_candidate_loop_ms=round(t_off, 3),
                          host_loop_minus_device_loop_ms=round(t_off - t_on, 3)))
    print(init_rows[-1])
    rec = dict(what="general SLAM entries vs the host forms (see tools/general_slam_timing.py); host clock per call, averaged",
               source_tree_hash=source_tree_hash(), update=update_rows, delayed_init=init_rows)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
