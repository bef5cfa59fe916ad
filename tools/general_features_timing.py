"""Times ovp_msckf_general_features against ovp_msckf_dense_blocks (host-built blocks, host gate) on the same features of a stereo
scene (half the features seen by both cameras), and writes a JSON record under profiles/.
    python tools/general_features_timing.py --out profiles/general_features_timing.json"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    from oracle import np_ref as R
    from ov_plane_amd import capi
    from ov_plane_amd.build import source_tree_hash
    from ov_plane_amd.synth import make_stereo_scene

    rows = []
    for C in (11, 20):
        sc = make_stereo_scene(C=C, F=80, seed=5, chi2_mult=1.0, stereo_frac=0.5)
        gen = np.arange(sc.n_stereo)
        o = capi.opts_from_scene(sc)
        ctx = capi.Context(sc.N, sc.C, sc.F)
        ctx.cov_upload(sc.P)
        ctx.state_upload(sc)
        ctx.cameras_upload(sc)
        ctx.msckf_general_features(o, sc, gen)
        t0 = time.perf_counter()
        for _ in range(a.reps):
            ctx.msckf_general_features(o, sc, gen)
        t_gen = (time.perf_counter() - t0) / a.reps * 1e3
        # the dense side channel: rows + projection on the host (numpy here, Eigen in the host mirror), marginal + gate in the entry
        t0 = time.perf_counter()
        for _ in range(3):
            blocks = []
            for f in gen:
                H_f, H_x, res, order = R.feature_jacobian_full(sc, int(f))
                Q, _ = np.linalg.qr(H_f, mode="complete")
                N = Q[:, 3:]
                blocks.append((N.T @ H_x, R.order_cols(order), N.T @ res))
        t_rows = (time.perf_counter() - t0) / 3 * 1e3
        ctx.msckf_dense_blocks(1.0, blocks)
        t0 = time.perf_counter()
        for _ in range(a.reps):
            ctx.msckf_dense_blocks(1.0, blocks)
        t_dense = (time.perf_counter() - t0) / a.reps * 1e3
        rows.append(dict(C=C, features=int(len(gen)), meas_per_feature=int(2 * C), general_entry_ms=round(t_gen, 4),
                         dense_blocks_entry_ms=round(t_dense, 4), numpy_rows_ms=round(t_rows, 3)))
        print(rows[-1])
        ctx.close()
    rec = dict(what="ovp_msckf_general_features vs ovp_msckf_dense_blocks on the stereo features of make_stereo_scene(F=80, "
                    "stereo_frac=0.5); host clock per call, averaged; the dense entry's time excludes building the rows",
               source_tree_hash=source_tree_hash(), rows=rows)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
