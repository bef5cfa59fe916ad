"""Timing of the plane detection stage (ovp_plane_detect_triangulate / ovp_plane_detect_planes) on the simulator's six-plane room,
and the label purity of the detected map against the simulator's point-to-plane truth.

    python tools/plane_detect_timing.py [--frames 40] [--out profiles/plane_detect_timing.json]

Two sizes (the simulator's num_pts + num_pts_plane = 125 + 125 and 250 + 250).  Per size: seven windows, each the whole frame
sequence on a fresh detector; a window's figure is the median over its frames, the reported one the median of the seven.  Host
clock of the two entries with the timer off; per-kernel GPU times in a separate pass with the events on (they add a stream
synchronisation per publication).  Purity = features whose detected plane's majority truth label is their own / features mapped,
over all frames; recorded, not asserted.  True camera poses are used, so the figures are the stage's alone."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scene(n_each, n_frames):
    from ov_plane_amd import closed_loop
    from ov_plane_amd.sim import P_IINC, R_ITOC, Simulator, synthetic_trajectory
    from ov_plane_amd.synth import quat_2_rot

    sim = Simulator(synthetic_trajectory(duration=20.0), num_pts=n_each, num_pts_plane=n_each)
    _, frames, plane_of = closed_loop.collect(sim, n_frames)
    out = []
    for t, seen in frames:
        gt = sim.get_state(t + sim.params["calib_camimu_dt"])
        R = R_ITOC @ quat_2_rot(gt["q"])
        p = gt["p"] - R.T @ P_IINC
        ids = np.array(sorted(seen), dtype=np.int64)
        uv = np.array([seen[int(f)] for f in ids], dtype=np.float32).reshape(-1, 2)
        xn, yn = closed_loop.radtan_undistort(uv[:, 0], uv[:, 1], sim.intr)
        out.append((ids, uv, np.stack([xn, yn], 1).astype(np.float32).astype(np.float64), R, p))
    return out, plane_of


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plane_detect_timing.json"))
    a = ap.parse_args()
    from ov_plane_amd import capi
    from ov_plane_amd.build import source_tree_hash

    ctx = capi.Context(64, 4, 8)
    res = dict(source_hash=source_tree_hash(), frames=a.frames, windows=7, sizes=[])
    for n_each in (125, 250):
        frames, plane_of = scene(n_each, a.frames)
        host, kern = [], []
        maps = None
        for timed in (False, True):
            for w in range(7):
                det = capi.PlaneDetector(ctx)
                det.timer(timed)
                rows, maps_w = [], []
                for ids, uv, uvn, R, p in frames:
                    t0 = time.perf_counter()
                    det.triangulate(ids, uv, uvn, R, p)
                    t1 = time.perf_counter()
                    det.planes()
                    t2 = time.perf_counter()
                    rows.append(list(det.kernel_ms()) if timed else [1e3 * (t1 - t0), 1e3 * (t2 - t1)])
                    maps_w.append(det.feature2plane())
                det.close()
                rows = np.array(rows)[4:]  # (the first frames hold no position yet: nothing behind the triangulation runs)
                (kern if timed else host).append(np.median(rows, axis=0))
                assert maps is None or maps == maps_w  # the windows agree: the stage is deterministic
                maps = maps_w
        agree = total = 0
        for m in maps:
            by_plane = {}
            for f, pl in m.items():
                by_plane.setdefault(pl, []).append(plane_of.get(int(f), -1) if hasattr(plane_of, "get") else plane_of[int(f)])
            for labels in by_plane.values():
                vals, cnt = np.unique(labels, return_counts=True)
                agree += int(cnt.max()) if vals[cnt.argmax()] > 0 else 0
                total += len(labels)
        h, k = np.median(host, axis=0), np.median(kern, axis=0)
        res["sizes"].append(dict(num_pts=n_each, num_pts_plane=n_each, points_per_frame_mean=float(np.mean([len(f[0]) for f in frames])),
                                 host_ms=dict(triangulate=float(h[0]), planes=float(h[1]), frame=float(h[0] + h[1])),
                                 kernel_ms=dict(k_det_triangulate=float(k[0]), k_det_tri_normals_and_vertex_norms=float(k[1]),
                                                k_det_match=float(k[2]), k_det_spatial_filter=float(k[3])),
                                 mapped_features_mean=float(np.mean([len(m) for m in maps])),
                                 planes_last_frame=len(set(maps[-1].values())),
                                 label_purity=(agree / total if total else None), mapped_total=total))
    # the filter kernel alone, on constructed planes (most frames of the room have no plane large enough for it)
    rng = np.random.default_rng(0)
    det = capi.PlaneDetector(ctx)
    det.timer(True)
    res["k_det_spatial_filter_ms"] = {}
    for n in (40, 300, 1024):
        xy = rng.uniform(0, 2.0, (n, 2))
        P = np.column_stack([xy, 2 * xy[:, 0] + 1])
        ms = []
        for w in range(7):
            one = []
            for rep in range(20):
                det.spatial_filter([P])
                one.append(float(det.kernel_ms()[3]))
            ms.append(np.median(one))
        res["k_det_spatial_filter_ms"]["one_plane_of_%d" % n] = float(np.median(ms))
    det.close()
    ctx.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
