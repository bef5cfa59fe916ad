"""Host-clock timing of the batched retirement against the one-by-one route, in the same run - run on the GPU box.
usage: python tools/retire_timing.py [--out profiles/retire_timing.json] [--reps 30] [--windows 7]
State: 11 clones, 25 landmarks, 4 planes (n = 183).  Every figure is the median over `windows` interleaved windows (old route, new
route, old, new, ...) of the window's median over `reps` calls; a call is timed from its first entry to the end of ovp_sync, the
covariance is uploaded again (untimed) in front of every call.
  (i)   retiring 1, 5 and 10 landmarks: ovp_cov_marginalize_many against the loop of ovp_cov_marginalize
  (ii)  one merge + two pruned planes, three merges + two pruned landmarks: ovp_planes_merge_retire against the host mirror's
        sequence per pair (ovp_cov_marginal, the 3 x 3 gate on the host, ovp_ekf_update, ovp_cov_marginalize) and a
        ovp_cov_marginalize per pruned variable
  (iii) a 40-frame session in which planes merge (tests/test_retire_host_gpu.py's scene) with StateOptions::gpu_batched_retire on and
        off: every column of timing.txt, mean over the frames, in ms"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CHI2_095_3 = 7.814727903251179


def interleaved(arms, windows, reps):
    """arms: {name: (prepare, call)} -> {name: median over windows of the window's median call time, in us}"""
    per = {k: [] for k in arms}
    for _ in range(windows):
        for name, (prepare, call) in arms.items():
            ts = []
            for _ in range(reps):
                prepare()
                t0 = time.perf_counter()
                call()
                ts.append(time.perf_counter() - t0)
            per[name].append(float(np.median(ts)))
    return {k: round(float(np.median(v)) * 1e6, 2) for k, v in per.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--session-windows", type=int, default=7)
    a = ap.parse_args()
    from ov_plane_amd.build import build_host, build_lib

    build_lib()
    build_host()
    from ov_plane_amd import capi, closed_loop
    from ov_plane_amd.sim import Simulator, synthetic_trajectory
    from ov_plane_amd.synth import _cov, state_layout

    ids = state_layout(11, n_slam=25, n_planes_in_state=4)
    N = int(ids["N"])
    P = _cov(11, ids, np.random.default_rng(3))
    pa, pb, pc, pd = (int(x) for x in ids["planes"])
    for o in (pb, pc, pd):  # re-detections of plane A: 0.9 x its error plus a part of their own, so that the merges are accepted
        P[o:o + 3, :] = 0.9 * P[pa:pa + 3, :]
        P[:, o:o + 3] = 0.9 * P[:, pa:pa + 3]
    for o in (pb, pc, pd):
        for q in (pb, pc, pd):
            P[o:o + 3, q:q + 3] = 0.81 * P[pa:pa + 3, pa:pa + 3] + (1e-5 * np.eye(3) if o == q else 0.0)
    assert np.linalg.eigvalsh(P).min() > 0
    cpA = np.array([2.0, 0.3, 0.1])
    cps = {pa: cpA, pb: cpA + [4e-4, -3e-4, 2e-4], pc: cpA + [-2e-4, 3e-4, 1e-4], pd: cpA + [1e-4, 2e-4, -3e-4]}
    ctx = capi.Context(N + 8, 12, 8)

    def prepare():
        ctx.cov_upload(P)

    res = dict(unit="us per call, host clock from entry to the end of ovp_sync; median of %d interleaved windows of %d calls" % (
        a.windows, a.reps), state=dict(clones=11, landmarks=25, planes=4, n=N))
    # ---- (i) ----
    slam = [int(x) for x in ids["slam"]]
    res["retire_landmarks"] = {}
    for k in (1, 5, 10):
        sel = slam[1:2 * k:2]  # every second landmark

        def loop(sel=sel):
            for i in sorted(sel, reverse=True):
                ctx.cov_marginalize(i, 3)
            ctx.sync()

        def many(sel=sel):
            ctx.cov_marginalize_many(sel, [3] * len(sel))
            ctx.sync()

        res["retire_landmarks"][str(k)] = interleaved(dict(loop_of_marginalize=(prepare, loop), marginalize_many=(prepare, many)),
                                                      a.windows, a.reps)
    # ---- (ii) ----
    sigma = 0.001

    def mirror(pairs, prunes):
        """the host mirror's present sequence (StateHelper::merge_planes_and_marginalize with the option off), columns renumbered as
        the variables leave"""
        gone = []
        shift = lambda c: c - 3 * sum(1 for g in gone if g < c)  # noqa: E731
        cp = {c: v.copy() for c, v in cps.items()}
        n_acc = 0
        for cn, co in pairs:
            jn, jo = shift(cn), shift(co)
            Pm = ctx.cov_marginal([jn, jo], [3, 3])
            wc = 1.0 / sigma
            H = np.hstack([wc * np.eye(3), -wc * np.eye(3)])
            r = wc * (0.0 - (cp[cn] - cp[co]))
            S = H @ Pm @ H.T + np.eye(3)
            y = np.linalg.solve(np.linalg.cholesky(S), r)
            dot = float(np.dot(cp[cn] / np.linalg.norm(cp[cn]), cp[co] / np.linalg.norm(cp[co])))
            if float(y @ y) < CHI2_095_3 and np.degrees(np.arccos(dot)) < 1.0:
                dx, _ = ctx.ekf_update(H, np.r_[jn:jn + 3, jo:jo + 3], r)
                for c in cp:
                    if c not in gone:
                        cp[c] = cp[c] + dx[shift(c):shift(c) + 3]
                n_acc += 1
            ctx.cov_marginalize(jo, 3)
            gone.append(co)
        for c in prunes:
            ctx.cov_marginalize(shift(c), 3)
            gone.append(c)
        ctx.sync()
        return n_acc

    def batched(pairs, prunes):
        cols = sorted({c for p in pairs for c in p}, key=lambda c: [q for p in pairs for q in p].index(c))
        out = ctx.planes_merge_retire([p[0] for p in pairs], [p[1] for p in pairs], cols, [cps[c] for c in cols], sigma, 1.0, 1.0,
                                      [p[1] for p in pairs] + list(prunes), [3] * (len(pairs) + len(prunes)))
        ctx.sync()
        return int(out["accepted"].sum())

    res["merge_and_prune"] = {}
    for name, pairs, prunes in (("1_merge_2_pruned_planes", [(pa, pb)], [pc, pd]),
                                ("3_merges_2_pruned_landmarks", [(pa, pb), (pa, pc), (pa, pd)], [slam[3], slam[11]])):
        prepare()
        n_old = mirror(pairs, prunes)
        P_old = ctx.cov_download()
        prepare()
        n_new = batched(pairs, prunes)
        P_new = ctx.cov_download()
        d = np.sqrt(np.abs(np.diag(P_old)))
        r = interleaved(dict(mirror_sequence=(prepare, lambda: mirror(pairs, prunes)),
                             planes_merge_retire=(prepare, lambda: batched(pairs, prunes))), a.windows, a.reps)
        r.update(accepted_old=n_old, accepted_new=n_new, normalised_dP=float((np.abs(P_new - P_old) / np.outer(d, d)).max()))
        res["merge_and_prune"][name] = r
    ctx.close()
    # ---- (iii) ----
    cols = {False: [], True: []}
    head = None
    for _ in range(a.session_windows):
        for on in (False, True):
            sim = Simulator(synthetic_trajectory(duration=20.0), num_pts=60, num_pts_plane=300)
            d = tempfile.mkdtemp()
            closed_loop.run_session(sim, n_frames=40, C=8, planes=2, max_slam=10, split_planes_until=24, forget_planes_at=32,
                                    batched_retire=on, out_dir=d)
            with open(os.path.join(d, "timing.txt")) as f:
                head = [h.strip() for h in f.readline().lstrip("#").strip().split(",")]
                rows = np.array([[float(x) for x in ln.strip().split(",")] for ln in f if ln.strip()])
            cols[on].append(rows[5:].mean(axis=0))
    res["session"] = dict(unit="ms per frame, mean over frames 5.. of a 40-frame session, median of %d interleaved runs" % a.session_windows,
                          **{("batched_retire_on" if on else "batched_retire_off"):
                             {h: round(float(np.median([c[i] for c in cols[on]])) * 1e3, 4) for i, h in enumerate(head) if i > 0}
                             for on in (False, True)})
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
