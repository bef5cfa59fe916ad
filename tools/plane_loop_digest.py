"""sha256 per route into the plane loop over the raw bytes of what the C-ABI entry returns: ok, chi2, dof, dx, used, gen_used, the
covariance afterwards, and for ovp_plane_init also new_ids and cp.  Two builds of libovplane_hip.so that compute the same bits
print the same list (the second one selected with OVP_LIB_AB):
    python tools/plane_loop_digest.py --out a.json
    OVP_LIB_AB=path/to/other/libovplane_hip.so python tools/plane_loop_digest.py --out b.json
Fixed small scenes, one per route: the loop's own column order, the state's order (OVP_PL_NATURAL_ORDER), the marginal of the involved
columns (N = 300), SLAM landmarks on out-of-state planes, general features, a plane with general features only, the retry on a
positive semi-definite prior, forced decisions, the forced two-workgroup solve (OVP_C2_SPLIT), ovp_plane_init, a frame without
planes."""
import argparse
import contextlib
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEYS = ("ok", "chi2", "dof", "dx", "used", "gen_used", "P", "new_ids", "cp")


def digest(out):
    h = hashlib.sha256()
    for k in KEYS:
        if k in out:
            h.update(k.encode() + b"\0" + np.ascontiguousarray(out[k]).tobytes())
    return h.hexdigest()


@contextlib.contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def exact_clone_scene():
    """tests/test_gpu_parity.py::test_plane_loop_on_a_positive_semidefinite_prior, case exact_clone at N <= 287: the newest clone an
    exact copy of the one before it - chol(P) fails and the loop runs once more on the pivot-dropping factor."""
    from ov_plane_amd.synth import make_scene

    sc = make_scene(C=9, F=150, seed=43, n_planes=3, feats_per_plane=25, planes_in_state_frac=0.67, chi2_mult=99999.0)
    a, b = sc.ids["clones"][-2], sc.ids["clones"][-1]
    idx = np.arange(sc.N)
    idx[b:b + 6] = np.arange(a, a + 6)
    sc["P"] = sc.P[np.ix_(idx, idx)]
    for k in ("clone_q", "clone_p", "clone_q_fej", "clone_p_fej"):
        sc[k][-1] = sc[k][-2]
    return sc


def plain(capi, sc, init=False, **kw):
    """One plane entry on a fresh context: upload, call, download."""
    npl = sc.cp.shape[0]
    ctx = capi.Context(sc.N + (3 * npl if init else 0), sc.C, sc.F)
    ctx.cov_upload(sc.P)
    ctx.state_upload(sc)
    ctx.batch_upload_scene(sc)
    o = capi.opts_from_scene(sc)
    if init:
        out = ctx.plane_init(o, sc.plane_id, sc.cp, 5.0, 1e9)
    else:
        out = ctx.plane_update(o, sc.plane_id, sc.cp, sc.cp_fej, sc.plane_state_id, **kw)
    out["P"] = ctx.cov_download()
    ctx.close()
    return out


def routes(capi):
    from ov_plane_amd.synth import make_scene, make_stereo_plane_scene, slam_rows_on_planes
    from tests import general_planes_ref as R

    small = dict(C=8, F=90, seed=73, n_planes=3, feats_per_plane=15, chi2_mult=1.0)
    sc = make_scene(**small)
    yield "full_order", plain(capi, sc)
    with env(OVP_PL_NATURAL_ORDER="1"):
        yield "natural_order", plain(capi, sc)
    yield "forced_decisions", plain(capi, sc, force_decision=np.array([1, 0, 1], dtype=np.uint8))
    big = make_scene(C=30, F=300, seed=33, n_planes=6, feats_per_plane=40, planes_in_state_frac=0.5, n_slam=27, chi2_mult=1.0)
    assert big.N == 300
    yield "sub_state_n300", plain(capi, big)
    ss = make_scene(n_slam=3, ragged=True, **dict(small, chi2_mult=99999.0))
    yield "slam_on_out_of_state_plane", plain(capi, ss, slam=slam_rows_on_planes(ss, 3))
    force = np.array([1, 1], dtype=np.uint8)
    st = make_stereo_plane_scene(C=8, n_planes=2, feats_per_plane=10, n_free=4, seed=3, planes_in_state_frac=0.5, chi2_mult=1.0)
    for name, scene in (("general_features", st),
                        ("general_features_only", make_stereo_plane_scene(C=8, n_planes=2, feats_per_plane=8, n_free=4, seed=4,
                                                                          stereo_frac=1.0, planes_in_state_frac=0.5, chi2_mult=1.0))):
        out = R.run_general(capi, scene, force=force)
        out.pop("ctx").close()
        yield name, out
    psd = plain(capi, exact_clone_scene())
    assert psd["ok"].all()
    yield "semidefinite_retry", psd
    with env(OVP_C2_SPLIT="5"):
        yield "c2_split_forced", plain(capi, make_scene(C=30, F=360, seed=21, n_planes=6, feats_per_plane=40, planes_in_state_frac=0.5,
                                                        chi2_mult=1.0))
    si = make_scene(C=8, F=80, seed=16, n_planes=2, feats_per_plane=25, planes_in_state_frac=0.0, chi2_mult=1.0, ragged=True)
    yield "plane_init", plain(capi, si, init=True)
    none = make_scene(C=8, F=40, seed=7, chi2_mult=1.0)
    assert none.cp.shape[0] == 0
    yield "no_plane", plain(capi, none)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ov_plane_amd import capi
    from ov_plane_amd.build import source_tree_hash

    rec = dict(library=os.path.relpath(capi.LIB_PATH, ROOT), source_tree_hash_of_this_checkout=source_tree_hash(), digests={})
    for name, out in routes(capi):
        rec["digests"][name] = digest(out)
        print(name, rec["digests"][name], "accepted %d of %d" % (int(np.sum(out["ok"])), len(out["ok"])))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
