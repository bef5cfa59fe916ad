"""sha256 per route of the point update (csrc/ovp_point_plan.h) over the raw bytes of what the C-ABI returns - dx, accepted, chi2 and
the covariance afterwards - for ovp_msckf_update, for the staged triple (ovp_msckf_build_gate_gram_async ->
ovp_ekf_update_from_gram_async -> ovp_msckf_fetch_results) and for ovp_ekf_update's information form.  Two builds of
libovplane_hip.so that compute the same bits print the same list (the second one selected with OVP_LIB_AB, as
tools/plane_loop_digest.py does):
    python tools/point_update_digest.py --out a.json
    OVP_LIB_AB=path/to/other/libovplane_hip.so python tools/point_update_digest.py --out b.json
    python tools/point_update_digest.py --merge a.json b.json --out profiles/point_update_refactor_digests.json
The scenes are those of tests/test_point_routes_gpu.py and the switches of tests/test_gpu_parity.py: side stream, workgroup 0, no
reversed order, no boost on an exact stochastic clone (the semi-definite retry), 31 observations, the sub-state at N = 300, the
global fallback at N = 330 with every column pending, a pending dense pair, an index range, a frame behind a plane loop."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

KEYS = ("dx", "accepted", "chi2", "P")


def digest(out):
    h = hashlib.sha256()
    for k in KEYS:
        if k in out:
            h.update(k.encode() + b"\0" + np.ascontiguousarray(out[k]).tobytes())
    return h.hexdigest()


def stochastic_clone(sc):
    """the prior every frame of a running filter sees: the newest clone an exact copy of the IMU pose"""
    b = sc.ids["clones"][-1]
    idx = np.arange(sc.N)
    idx[b:b + 6] = np.arange(0, 6)
    sc["P"] = sc.P[np.ix_(idx, idx)]
    return sc


def point(capi, sc, staged, planes=False, rng=None, dense=False):
    """One point update on a fresh context: upload, (plane loop,) call or staged triple, download."""
    ctx = capi.Context(sc.N, sc.C, sc.F)
    ctx.cov_upload(sc.P)
    ctx.state_upload(sc)
    ctx.batch_upload_scene(sc)
    o = capi.opts_from_scene(sc)
    if planes:
        ctx.plane_update(o, sc.plane_id, sc.cp, sc.cp_fej, sc.plane_state_id)
        o.chi2_multiplier = 1.0
        o.skip_plane_used = 1
    if rng is not None:
        ctx.batch_set_range(*rng)
    if dense:  # one 3 x 9 block on the IMU's columns 3..8 and the landmark behind the clones: in front of the batch's first column
        g = np.random.default_rng(5)
        cols = np.r_[3:9, int(sc.ids["slam"][0]) + np.arange(3)].astype(np.int32)
        ctx.msckf_dense_blocks(1e9, [(g.standard_normal((3, 9)) * 5.0, cols, g.standard_normal(3) * 1e-3)])
    if staged:
        ctx.build_gate_gram_async(o)
        ctx.ekf_update_from_gram_async()
        out = ctx.fetch_results(raise_on_error=False)
    else:
        out = ctx.msckf_update(o, raise_on_error=False)
    try:
        out["route"] = ctx.debug_read("point_route", (8,), dtype=np.int32).tolist()
    except capi.OvpError:  # (a build from before the read-back)
        out["route"] = None
    out["P"] = ctx.cov_download()
    ctx.close()
    return out


def routes(capi):
    from ov_plane_amd.synth import make_scene
    from plane_loop_digest import env

    small = dict(C=9, F=80, seed=75, chi2_mult=1.0)
    slam = dict(C=7, F=90, seed=64, ragged=True, chi2_mult=1.0, n_slam=5)
    for staged in (False, True):
        tag = "staged/" if staged else "update/"
        yield tag + "side_stream", point(capi, make_scene(**small), staged)
        with env(OVP_OVERLAP_MODE="3"):
            yield tag + "workgroup_0", point(capi, make_scene(**small), staged)
        yield tag + "landmarks_behind", point(capi, make_scene(**slam), staged)
        with env(OVP_POINT_NO_FLIP="1"):
            yield tag + "no_flip", point(capi, make_scene(**slam), staged)
        yield tag + "stochastic_clone", point(capi, stochastic_clone(make_scene(**small)), staged)
        with env(OVP_POINT_NO_BOOST="1"):
            yield tag + "stochastic_clone_semidefinite_retry", point(capi, stochastic_clone(make_scene(**small)), staged)
        yield tag + "one_wave_31_observations", point(capi, make_scene(C=31, F=12, seed=23, chi2_mult=1.0), staged)
        yield tag + "sub_state_n300", point(capi, make_scene(C=30, F=48, seed=91, n_slam=30, chi2_mult=1.0), staged)
        yield tag + "many_features", point(capi, make_scene(C=12, F=2100, seed=76, ragged=True, min_meas=3, chi2_mult=1.0), staged)
        yield tag + "index_range", point(capi, make_scene(**small), staged, rng=(13, 61))
        yield tag + "dense_pair", point(capi, make_scene(**slam), staged, dense=True)
        yield tag + "behind_plane_loop", point(capi, make_scene(C=12, F=260, seed=62, n_planes=5, feats_per_plane=30,
                                                                planes_in_state_frac=0.6, chi2_mult=99999.0), staged, planes=True)
    # ovp_ekf_update's information form: the tile path, the sub-state and the global fallback
    with env(OVP_EKF_INFO_FORM="1"):
        for name, kw, cols in (("tile", small, np.r_[16:30, 30:42]), ("sub_state_n300", dict(C=30, F=4, seed=91, n_slam=30), np.r_[16:30, 204:216, 290:293]),
                               ("global_n330", dict(C=30, F=4, seed=92, n_slam=40), np.arange(330))):
            sc = make_scene(**kw)
            g = np.random.default_rng(11)
            H = g.standard_normal((12, len(cols))) * 20.0
            ctx = capi.Context(sc.N, sc.C, 4)
            ctx.cov_upload(sc.P)
            dx, _ = ctx.ekf_update(H, cols.astype(np.int32), g.standard_normal(12))
            out = dict(dx=dx, P=ctx.cov_download(), route=None)
            ctx.close()
            yield "ekf_update_info_form/" + name, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge", nargs=2, default=None, metavar=("THIS", "OTHER"))
    a = ap.parse_args()
    if a.merge:
        recs = [json.load(open(p)) for p in a.merge]
        names = list(recs[0]["digests"])
        equal = {n: recs[0]["digests"][n] == recs[1]["digests"].get(n) for n in names}
        rec = dict(what="sha256 over the raw dx, accepted, chi2 and covariance of one point update per route (tools/point_update_digest.py), "
                        "this checkout's library and the one in front of it in the same visit",
                   this=recs[0], other=recs[1], equal=equal, all_equal=all(equal.values()) and set(names) == set(recs[1]["digests"]))
        print("all equal" if rec["all_equal"] else "DIGESTS DIFFER: %s" % [n for n in names if not equal[n]])
        if a.out:
            with open(a.out, "w") as fh:
                json.dump(rec, fh, indent=1)
        sys.exit(0 if rec["all_equal"] else 1)
    from ov_plane_amd import capi
    from ov_plane_amd.build import source_tree_hash

    rec = dict(library=os.path.relpath(capi.LIB_PATH, ROOT), source_tree_hash_of_this_checkout=source_tree_hash(), digests={}, routes={})
    for name, out in routes(capi):
        rec["digests"][name] = digest(out)
        if out.get("route") is not None:
            rec["routes"][name] = out["route"]
        print(name, rec["digests"][name], out.get("route"), "accepted %d" % int(np.sum(out.get("accepted", 0))))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
