"""Timing of the device Delaunay triangulation (k_det_delaunay) against the host's, in the same run on the same machine.

    python tools/plane_delaunay_timing.py [--frames 40] [--out profiles/plane_delaunay_timing.json]

(a) ovp_delaunay (host) against ovp_delaunay_device on the host clock, at 250, 500 and 1024 random pixels of a 752 x 480 image, and
    the kernel's own time from events (a separate pass: the events add a stream synchronisation);
(b) a detector frame (both calls) with the device triangulation off and on, at 250 and 500 points of the simulator's room;
(c) the per-frame time of the session test's scene (0.05 px, 200 planar points, detected planes) with the option off and on.
Seven windows per figure, the two arms interleaved inside every window; a window's figure is its median, the reported one the
median of the seven.  Nothing is asserted but that both arms give the same triangles / maps."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

WINDOWS = 7


def entries(capi, ctx, det):
    out = []
    for n in (250, 500, 1024):
        rng = np.random.default_rng(n)
        xy = np.stack([rng.uniform(0, 752, n), rng.uniform(0, 480, n)], 1).astype(np.float32)
        assert np.array_equal(capi.delaunay(xy), capi.delaunay_device(ctx, xy))
        host, dev, kern = [], [], []
        for w in range(WINDOWS):
            h, d = [], []
            for rep in range(10):
                t0 = time.perf_counter()
                capi.delaunay(xy)
                t1 = time.perf_counter()
                capi.delaunay_device(ctx, xy)
                t2 = time.perf_counter()
                h.append(1e3 * (t1 - t0)), d.append(1e3 * (t2 - t1))
            host.append(np.median(h)), dev.append(np.median(d))
        det.timer(True)
        for w in range(WINDOWS):
            k = []
            for rep in range(10):
                capi.delaunay_device(ctx, xy)
                k.append(float(det.delaunay_ms()[1]))
            kern.append(np.median(k))
        det.timer(False)
        out.append(dict(points=n, triangles=int(len(capi.delaunay(xy))), host_ms=float(np.median(host)), device_entry_ms=float(np.median(dev)),
                        k_det_delaunay_ms=float(np.median(kern))))
    return out


def detector_frames(capi, ctx, n_frames):
    from plane_detect_timing import scene

    out = []
    for n_each in (125, 250):
        frames, _ = scene(n_each, n_frames)
        arms = {False: [], True: []}
        kern = []
        maps = {}
        for w in range(WINDOWS):
            for on in (False, True):
                det = capi.PlaneDetector(ctx)
                det.set_device_delaunay(on)
                rows, maps_w = [], []
                for ids, uv, uvn, R, p in frames:
                    t0 = time.perf_counter()
                    det.triangulate(ids, uv, uvn, R, p)
                    t1 = time.perf_counter()
                    det.planes()
                    t2 = time.perf_counter()
                    rows.append([1e3 * (t1 - t0), 1e3 * (t2 - t1)])
                    maps_w.append(det.feature2plane())
                    assert det.tris_info()["source"] == ("device" if on else "host")
                det.close()
                arms[on].append(np.median(np.array(rows)[4:], axis=0))
                assert maps.setdefault("m", maps_w) == maps_w  # both arms, every window: the same maps
        det = capi.PlaneDetector(ctx)
        det.set_device_delaunay(True)
        det.timer(True)
        verts = []
        for ids, uv, uvn, R, p in frames:
            det.triangulate(ids, uv, uvn, R, p)
            det.planes()
            kern.append(float(det.delaunay_ms()[0]))
            verts.append(det.tris_info()["vertices"])
        det.close()
        off, on = np.median(arms[False], axis=0), np.median(arms[True], axis=0)
        out.append(dict(num_pts=n_each, num_pts_plane=n_each, points_per_frame_mean=float(np.mean([len(f[0]) for f in frames])),
                        vertices_per_frame_mean=float(np.mean(verts[4:])),
                        host_delaunay=dict(triangulate_ms=float(off[0]), planes_ms=float(off[1]), frame_ms=float(off.sum())),
                        device_delaunay=dict(triangulate_ms=float(on[0]), planes_ms=float(on[1]), frame_ms=float(on.sum())),
                        k_det_delaunay_ms=float(np.median(kern[4:]))))
    return out


def session(n_frames):
    from ov_plane_amd import closed_loop
    from ov_plane_amd.build import build_host
    from ov_plane_amd.sim import Simulator, synthetic_trajectory

    build_host()
    arms = {False: [], True: []}
    for w in range(WINDOWS):
        for on in (False, True):
            sim = Simulator(synthetic_trajectory(duration=20.0), num_pts=60, num_pts_plane=200, sigma_pix=0.05)
            t0 = time.perf_counter()
            r = closed_loop.run_session(sim, n_frames=n_frames, C=8, planes=2, detect_planes=True, device_delaunay=on)
            arms[on].append(1e3 * (time.perf_counter() - t0) / n_frames)
            assert arms.setdefault("traj", r["traj"].tobytes()) == r["traj"].tobytes()
    return dict(frames=n_frames, note="whole run_session call / frames: simulator bookkeeping in Python included on both arms",
                host_delaunay_ms_per_frame=float(np.median(arms[False])), device_delaunay_ms_per_frame=float(np.median(arms[True])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plane_delaunay_timing.json"))
    a = ap.parse_args()
    from ov_plane_amd import capi
    from ov_plane_amd.build import source_tree_hash

    ctx = capi.Context(64, 4, 8)
    det = capi.PlaneDetector(ctx)
    res = dict(source_hash=source_tree_hash(), windows=WINDOWS, entries=entries(capi, ctx, det))
    det.close()
    res["detector_frames"] = detector_frames(capi, ctx, a.frames)
    ctx.close()
    res["session"] = session(a.frames)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
