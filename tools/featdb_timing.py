"""Timing of the device feature database (ovp_featdb_*) against the path it replaces, in one run on one tree.

    python tools/featdb_timing.py [--reps 5] [--out profiles/featdb_timing.json]

Two sizes: BASELINE config 3's point batch (2000 features, 30 clones) and the session's (150 features, 11 clones), synthetic scenes
of ov_plane_amd.synth.  Seven windows; inside a window the arms are interleaved.  A repetition rebuilds the table (reset, one append
per clone time) and then runs, each between two stream synchronisations on the host clock:
  append           one frame's observations (the median over the repetition's frames)
  classify         the class table of every live feature (upload, launch, publication, wait)
  gather           the batch of every feature, bound - behind a classify over the SAME clone times, so that the gather's argument
                   check reads the cleaned counts that classify left (the cached case)
  gather_tri       gather + ovp_featdb_triangulate, cached: the device arm of a caller that classifies first
  gather_search / gather_tri_search   the same two behind a classify over OTHER clone times (untimed), so that the check searches
                   the host's shadow of every time stamp: what StateOptions::gpu_featdb pays as it is wired, where no classify
                   precedes the gather
  upload_tri       ovp_batch_upload + ovp_triangulate with a host uv_norm on the SAME batch, already packed at the batch's own
                   pitch (its longest track, as pack_features does): the comparator - the path the option replaces minus its host
                   packing loop, which is C++ in the mirror and is not timed here, so the comparator is flattered by that much
  cleanup          cleanup_measurements at a time below every observation: the full scan, nothing dropped
In a pass of its own with the timer on (events around the kernel, a stream synchronisation behind it): the kernels of append,
classify, gather, triangulate (behind the database's entry) and cleanup.  A window's figure is the median over its repetitions, the
reported one the median of the seven with their spread (min, max)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _spread(v):
    v = np.asarray(v, float)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def _frames(sc):
    """per clone time: ids, uv, uv_norm of the features that saw it, from the scene's batch"""
    uvn = np.asarray(sc.uv_norm, dtype=np.float32)
    out = []
    for c in range(sc.C):
        f, k = np.nonzero((sc.clone_idx == c) & (np.arange(sc.clone_idx.shape[1])[None, :] < sc.n_meas[:, None]))
        out.append((1000.0 + 0.05 * c, (f + 1).astype(np.int64), np.ascontiguousarray(sc.uv[f, k], dtype=np.float32),
                    np.ascontiguousarray(uvn[f, k])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "featdb_timing.json"))
    a = ap.parse_args()
    from ov_plane_amd import capi
    from ov_plane_amd.build import source_tree_hash
    from ov_plane_amd.synth import make_scene

    sizes = {"config3_2000x30": dict(C=30, F=2000), "session_150x11": dict(C=11, F=150)}
    keys = ("append", "classify", "gather", "gather_tri", "gather_search", "gather_tri_search", "upload_tri", "cleanup")
    kkeys = ("k_append", "k_classify", "k_gather", "k_triangulate", "k_cleanup")
    L = capi.lib()
    res = dict(source_hash=source_tree_hash(), reps=a.reps, windows=7, unit="ms", sizes={})
    world = {}
    for name, s in sizes.items():
        sc = make_scene(C=s["C"], F=s["F"], seed=21)
        ctx = capi.Context(sc.N, sc.C, sc.F)
        ctx.cov_upload(sc.P)
        ctx.state_upload(sc)
        db = capi.FeatureDatabase(ctx, max(sc.F, 1), 32)
        M = int(sc.n_meas.max())   # the comparator's pitch: the batch's longest track
        uv = np.zeros((sc.F, M, 2), np.float32)
        uvn = np.zeros((sc.F, M, 2), np.float32)
        ci = np.full((sc.F, M), -1, np.int32)
        uv[:], uvn[:], ci[:] = sc.uv[:, :M], np.asarray(sc.uv_norm, np.float32)[:, :M], sc.clone_idx[:, :M]
        world[name] = dict(sc=sc, ctx=ctx, db=db, frames=_frames(sc), ids=np.arange(1, sc.F + 1, dtype=np.int64),
                           times=[1000.0 + 0.05 * c for c in range(sc.C)], packed=(uv, ci, np.asarray(sc.n_meas, np.int32), np.zeros((sc.F, 3)), uvn),
                           win={k: [] for k in keys + kkeys})

    def clock(ctx, fn):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        return 1e3 * (time.perf_counter() - t0)

    def rep(wd, timed):
        ctx, db, r = wd["ctx"], wd["db"], {}
        L.ovp_featdb_debug(ctx.handle, b"timer", 1 if timed else 0, None, 0)
        kms = lambda: float(db._debug(b"time", np.float32, 1)[0])  # noqa: E731
        db.reset()
        ap_, k_ap = [], []
        for t, ids, uv, uvn in wd["frames"]:
            ap_.append(clock(ctx, lambda: db.update_feature(t, ids, uv, uvn)))
            k_ap.append(kms() if timed else 0.0)
        r["append"], r["k_append"] = np.median(ap_), np.median(k_ap)
        ts = wd["times"]
        r["classify"] = clock(ctx, lambda: db.classify(ts, ts[-1], ts[0], len(ts) - 1, True))
        r["k_classify"] = kms() if timed else 0.0
        r["gather"] = clock(ctx, lambda: db.gather(wd["ids"], ts))
        r["k_gather"] = kms() if timed else 0.0

        def dev():
            db.gather(wd["ids"], ts)
            return db.triangulate()

        def host():
            uv, ci, nm, p0, uvn = wd["packed"]
            ctx.batch_upload(uv, ci, nm, p0)
            return ctx.triangulate(uvn)
        r["gather_tri"] = clock(ctx, dev)
        r["k_triangulate"] = kms() if timed else 0.0
        db.classify(ts[1:], ts[-1], ts[1], len(ts) - 1, True)   # other clone times: the counts it leaves are not the gather's
        r["gather_search"] = clock(ctx, lambda: db.gather(wd["ids"], ts))
        r["gather_tri_search"] = clock(ctx, dev)
        r["upload_tri"] = clock(ctx, host)
        r["cleanup"] = clock(ctx, lambda: db.cleanup(False, 0.0))
        r["k_cleanup"] = kms() if timed else 0.0
        return r

    for wd in world.values():   # warm-up: code objects, and the two arms agree
        rep(wd, False)
        wd["db"].gather(wd["ids"], wd["times"])
        d = wd["db"].triangulate()
        uv, ci, nm, p0, uvn = wd["packed"]
        wd["ctx"].batch_upload(uv, ci, nm, p0)
        h = wd["ctx"].triangulate(uvn)
        assert d["p_FinG"].tobytes() == h["p_FinG"].tobytes() and d["ok"].tobytes() == h["ok"].tobytes()
    for _ in range(7):
        for timed in (False, True):
            acc = {name: [] for name in world}
            for _r in range(a.reps):
                for name, wd in world.items():
                    acc[name].append(rep(wd, timed))
            for name, wd in world.items():
                for k in (kkeys if timed else keys):
                    wd["win"][k].append(np.median([r[k] for r in acc[name]]))
    for name, wd in world.items():
        res["sizes"][name] = dict(features=int(wd["sc"].F), clones=int(wd["sc"].C), observations=int(wd["sc"].n_meas.sum()),
                                  arms={k: _spread(v) for k, v in wd["win"].items()})
        wd["db"].close()
        wd["ctx"].close()
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
