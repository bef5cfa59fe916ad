"""Timing of the active-tracks stage (ovp_active_tracks_update, VioManager::retriangulate_active_tracks on the device).

    python tools/active_tracks_timing.py [--frames 12] [--session-frames 10] [--out profiles/active_tracks_timing.json]

Three sizes: 250, 500 and 1000 tracked points of one camera, 50 of them SLAM landmarks of the state (half global, half anchored).
Per size, seven windows; inside a window the arms are interleaved - the entry's host clock with the timer off (the C call alone,
and the Python binding's update() around it, which also builds the two dicts), the kernel's event time with it on (the events add a stream synchronisation per frame), and the plane detector's first call
(ovp_plane_detect_triangulate, the same arithmetic per point) on the same points for comparison.  A window's figure is the median
over its frames from the fifth on (every point is solved from there), the reported one the median of the seven with their spread
(min, max).  Then the session's `re-tri & marg` column of timing.txt with StateOptions::gpu_active_tracks on against off (off is
the column's former content: marginalisation only), interleaved in the same way on the simulator's room with num_pts +
num_pts_plane = the size and max_slam = 50."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _rot(axis, ang):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)


def scene(n, n_frames, n_slam=50, seed=0):
    """n points 2 - 3.5 m in front of a camera that moves sideways, seen by a pinhole camera 0; the last n_slam are landmarks"""
    n -= n_slam
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy, w, h = 458.0, 457.0, 367.0, 248.0, 752, 480
    R_ItoC, p_IinC = _rot([0.2, -0.5, 1.0], 0.31), np.array([0.05, -0.02, 0.01])
    pts = np.stack([rng.uniform(-1.4, 1.4, n + n_slam), rng.uniform(-0.9, 0.9, n + n_slam), rng.uniform(2.0, 3.5, n + n_slam)], 1)
    ids = np.arange(n + n_slam, dtype=np.int64)
    poses = [(_rot([0, 1, 0], 0.01 * k), np.array([0.12 * k, 0.01 * k, 0.02 * k])) for k in range(n_frames)]  # R_GtoC, p_CinG
    slam_rel = np.arange(n_slam) % 2 == 1
    aRc, apc = poses[0]
    aR, ap = R_ItoC.T @ aRc, apc + aRc.T @ p_IinC            # the anchor clone: the first frame's IMU pose
    xyz = np.where(slam_rel[:, None], (pts[n:] - apc) @ aRc.T, pts[n:])
    frames = []
    for Rc, pc in poses:
        q = (pts - pc) @ Rc.T
        uv = (np.stack([fx * q[:, 0] / q[:, 2] + cx, fy * q[:, 1] / q[:, 2] + cy], 1) + 0.05 * rng.standard_normal((len(pts), 2))).astype(np.float32)
        uvn = np.stack([(uv[:, 0] - cx) / fx, (uv[:, 1] - cy) / fy], 1).astype(np.float32).astype(np.float64)
        frames.append(dict(cam_idx=np.zeros(len(ids), np.int32), ids=ids, uv=uv, uv_norm=uvn, R_GtoC=Rc[None], p_CinG=pc[None],
                           R_ItoC0=R_ItoC, p_IinC0=p_IinC, R_GtoI=R_ItoC.T @ Rc, p_IinG=pc + Rc.T @ p_IinC, width=w, height=h,
                           slam_ids=ids[n:], slam_xyz=xyz, slam_relative=slam_rel,
                           slam_anchor=(np.tile(aR, (n_slam, 1, 1)), np.tile(ap, (n_slam, 1)), np.tile(R_ItoC, (n_slam, 1, 1)),
                                        np.tile(p_IinC, (n_slam, 1)))))
    return frames


def _spread(v):
    v = np.asarray(v, float)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


_RECORDED = {}


def session_column(n, n_frames, on):
    """median of the `re-tri & marg` column (milliseconds) over the frames of one session run.  The simulator's frames of a size
    are drawn once and replayed for every run of that size (drawing them is seconds of Python and no part of what is measured)."""
    from ov_plane_amd import closed_loop
    from ov_plane_amd.sim import Simulator, synthetic_trajectory

    if n not in _RECORDED:
        sim = Simulator(synthetic_trajectory(duration=20.0), num_pts=n // 2, num_pts_plane=n // 2)
        _RECORDED[n] = (sim, closed_loop.collect(sim, 8 + 1 + n_frames))
    sim, recorded = _RECORDED[n]
    collect, closed_loop.collect = closed_loop.collect, lambda s, k: recorded
    try:
        with tempfile.TemporaryDirectory() as d:
            r = closed_loop.run_session(sim, n_frames=n_frames, C=8, max_slam=50, out_dir=d, active_tracks=on, feed_plane_tracks=True)
            rows = [ln.strip().split(",") for ln in open(os.path.join(d, "timing.txt")) if not ln.startswith("#")]
    finally:
        closed_loop.collect = collect
    col = np.array([float(x[-2]) for x in rows])[4:]
    pts = float(np.mean(r["active_per_frame"][4:, 0])) if on else None
    return 1e3 * float(np.median(col)), pts, int(r["counts"][:, 4].max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--session-frames", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "active_tracks_timing.json"))
    a = ap.parse_args()
    from ov_plane_amd import capi
    from ov_plane_amd.build import build_host, source_tree_hash

    build_host()
    ctx = capi.Context(64, 4, 8)
    res = dict(source_hash=source_tree_hash(), frames=a.frames, session_frames=a.session_frames, windows=7, n_slam=50, sizes=[])
    for n in (250, 500, 1000):
        frames = scene(n, a.frames)
        host, bind, kern, det_host, det_kern, ses_on, ses_off = [], [], [], [], [], [], []
        n_pos = n_lm = pts_on = None
        for w in range(7):
            for arm in ("entry", "kernel", "detector", "detector_kernel"):
                rows, brow = [], []
                if arm in ("entry", "kernel"):
                    at = capi.ActiveTracks(ctx)
                    at.timer(arm == "kernel")
                    for fr in frames:
                        t0 = time.perf_counter()
                        out = at.update(**fr)
                        t1 = time.perf_counter()
                        rows.append(at.kernel_ms() if arm == "kernel" else at.last_call_ms)
                        brow.append(1e3 * (t1 - t0))
                    n_pos = len(out["posinG"])
                    at.close()
                    if arm == "entry":
                        bind.append(np.median(brow[4:]))
                else:
                    det = capi.PlaneDetector(ctx)
                    det.timer(arm == "detector_kernel")
                    for fr in frames:
                        t0 = time.perf_counter()
                        det.triangulate(fr["ids"][:n], fr["uv"][:n], fr["uv_norm"][:n], fr["R_GtoC"][0], fr["p_CinG"][0])
                        t1 = time.perf_counter()
                        rows.append(float(det.kernel_ms()[0]) if arm == "detector_kernel" else 1e3 * (t1 - t0))
                    det.close()
                dict(entry=host, kernel=kern, detector=det_host, detector_kernel=det_kern)[arm].append(np.median(rows[4:]))
            for on in (True, False):
                ms, pts, n_lm_w = session_column(n, a.session_frames, on)
                (ses_on if on else ses_off).append(ms)
                if on:
                    pts_on, n_lm = pts, n_lm_w
        res["sizes"].append(dict(points=n, landmarks=50, positions_last_frame=n_pos,
                                 entry_host_ms=_spread(host), python_update_ms=_spread(bind), k_active_tracks_ms=_spread(kern),
                                 detector_first_call_host_ms=_spread(det_host), k_det_triangulate_ms=_spread(det_kern),
                                 session=dict(num_pts=n // 2, num_pts_plane=n // 2, max_slam=50, landmarks_in_state_max=n_lm,
                                              positions_per_frame_mean=pts_on, retri_and_marg_ms_on=_spread(ses_on),
                                              retri_and_marg_ms_off=_spread(ses_off))))
        print(json.dumps(res["sizes"][-1]), flush=True)
        with open(a.out, "w") as f:  # (after every size: a run that is cut short keeps what it has)
            json.dump(res, f, indent=1)
    ctx.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
