"""sha256 per branch of the two SLAM entries (csrc/ovp_api_slam.hip) and of ovp_ekf_update over the raw bytes of what the C-ABI
returns - the return code, every output array - and of the covariance afterwards.  Two builds of libovplane_hip.so that compute the
same bits print the same list (the second one selected with OVP_LIB_AB):
    python tools/slam_digest.py --out a.json
    OVP_LIB_AB=path/to/other/libovplane_hip.so python tools/slam_digest.py --out b.json
Fixed small scenes (at most 11 clones and 25 landmarks): ovp_slam_update with and without a state plane, with a host-built block,
at a row count that takes the S-form, in the information form (OVP_EKF_INFO_FORM=1), on a positive semi-definite prior;
ovp_slam_update_general on a stereo scene and on a camera-0 batch; the three delayed-init entries (a rejected candidate, general
rows, planes with an accepted A / a rejected A whose B is accepted / no plane, mono and stereo); ovp_ekf_update on both sides of
its S-form limit; one refused call of each entry followed by a valid one on the same context."""
import argparse
import contextlib
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEYS = ("rc", "dx", "status", "ok", "chi2", "new_id", "delta_init", "info", "P", "refused_rc")


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


def plane_args(sc):
    """per-landmark plane_state_id / cp / cp_fej of a SLAM scene (None without planes)"""
    if sc.cp.shape[0] == 0:
        return None, None, None
    pid = np.asarray(sc.plane_id, dtype=np.int64)
    slot = np.maximum(pid, 1) - 1
    sid = np.where(pid > 0, np.asarray(sc.plane_state_id)[slot], -1).astype(np.int32)
    return sid, np.asarray(sc.cp)[slot], np.asarray(sc.cp_fej)[slot]


def context(capi, sc, cap=None, cameras=False):
    ctx = capi.Context(sc.N if cap is None else cap, sc.C, sc.F)
    ctx.cov_upload(sc.P)
    ctx.state_upload(sc)
    if cameras:
        ctx.cameras_upload(sc)
    return ctx


def packed(out, ctx, **more):
    rec = {k: out[k] for k in KEYS if k in out and k != "info"}
    if "info" in out:
        i = out["info"]
        rec["info"] = np.array([i.n_rows, i.n_cols, i.n_accepted, i.not_spd, i.neg_diag], dtype=np.int64)
    rec["rc"] = np.array([out["rc"]], dtype=np.int64)
    rec["P"] = ctx.cov_download()
    rec.update(more)
    return rec


def update(capi, sc, ctx=None, cam_idx=None, planes=True, pre=None, lm_id=None):
    """one ovp_slam_update / ovp_slam_update_general, on a fresh context unless one is handed in"""
    own = ctx is None
    if own:
        ctx = context(capi, sc, cameras=cam_idx is not None)
    sid, cp, cpf = plane_args(sc) if planes else (None, None, None)
    a = (sc.n_meas, sc.p_FinG, sc.p_FinG_fej, sc.lm_id if lm_id is None else lm_id, sid, cp, cpf)
    o = capi.opts_from_scene(sc)
    if cam_idx is None:
        out = ctx.slam_update(o, sc.uv, sc.clone_idx, *a, pre=pre, raise_on_error=False)
    else:
        out = ctx.slam_update_general(o, sc.uv, sc.clone_idx, cam_idx, *a, pre=pre, raise_on_error=False)
    rec = packed(out, ctx)
    if own:
        ctx.close()
    return rec


def host_block(sc, l, seed):
    """a fixed dense block for landmark l: three rows over its first clone and the landmark"""
    rng = np.random.default_rng(seed)
    cols = np.r_[sc.ids["clones"][int(sc.clone_idx[l][0])] + np.arange(6), int(sc.lm_id[l]) + np.arange(3)]
    return rng.standard_normal((3, len(cols))), cols, 1e-2 * rng.standard_normal(3)


def semidefinite(sc):
    """the newest clone an exact copy of the one before it: chol(P) fails, the update ends in the S-form on the singular prior"""
    from ov_plane_amd.synth import Scene

    sc = Scene(sc)
    a, b = sc.ids["clones"][-2], sc.ids["clones"][-1]
    idx = np.arange(sc.N)
    idx[b:b + 6] = np.arange(a, a + 6)
    sc["P"] = sc.P[np.ix_(idx, idx)]
    return sc


def dinit(capi, sc, entry, ctx=None, n_meas=None, cam_idx=None, **over):
    """one delayed-init entry (`entry`: mono / general / planes), on a fresh context unless one is handed in"""
    from tests.dinit_planes_ref import plane_call_args

    own = ctx is None
    if own:
        ctx = context(capi, sc, cap=sc.N + 3 * sc.F, cameras="cam1" in sc)
    o = capi.opts_from_scene(sc)
    nm = sc.n_meas if n_meas is None else n_meas
    if entry == "mono":
        out = ctx.slam_delayed_init(o, sc.uv, sc.clone_idx, nm, sc.p_FinG, raise_on_error=False)
    elif entry == "general":
        out = ctx.slam_delayed_init_general(o, sc.uv, sc.clone_idx, sc.cam_idx if cam_idx is None else cam_idx, nm, sc.p_FinG,
                                            raise_on_error=False)
    else:
        kw = plane_call_args(sc, over.pop("with_planes", True))
        kw.update(over)
        out = ctx.slam_delayed_init_planes(o, sc.uv, sc.clone_idx, nm, sc.p_FinG, raise_on_error=False, **kw)
    rec = packed(out, ctx)
    if own:
        ctx.close()
    return rec


def dense(sc, rows, seed):
    rng = np.random.default_rng(seed)
    cols = np.r_[sc.ids["clones"][1] + np.arange(6), sc.ids["calib"] + np.arange(6)]
    return rng.standard_normal((rows, len(cols))), cols, 1e-3 * rng.standard_normal(rows)


def ekf(capi, sc, rows, ctx=None, bad_column=False):
    own = ctx is None
    if own:
        ctx = context(capi, sc)
    H, cols, r = dense(sc, rows, 3)
    if bad_column:
        cols = cols.copy()
        cols[0] = sc.N
    try:
        dx, info = ctx.ekf_update(H, cols, r)
        rec = dict(rc=np.array([0], dtype=np.int64), dx=dx, info=np.array([info.n_rows, info.n_cols], dtype=np.int64))
    except capi.OvpError as e:
        rec = dict(rc=np.array([e.code], dtype=np.int64))
    rec["P"] = ctx.cov_download()
    if own:
        ctx.close()
    return rec


def after_refusal(refused, valid):
    """the refused call's code (it must be one) beside the valid call that followed it on the same context"""
    assert int(refused["rc"][0]) != 0 and int(valid["rc"][0]) == 0
    return dict(valid, refused_rc=refused["rc"])


def cases(capi):
    from ov_plane_amd.synth import make_scene, make_slam_scene, make_stereo_slam_scene
    from tests.dinit_planes_ref import mono_scene, stereo_scene

    sl = make_slam_scene(C=11, n_slam=14, seed=4, n_planes=3, outliers=2, wrong_plane=3)
    assert 2 * int(sl.n_meas.sum()) > 80  # (more rows than the S-form takes)
    r = update(capi, sl)
    assert set(int(s) for s in r["status"]) == {0, 1, 2}
    yield "update_state_planes", r
    yield "update_no_plane", update(capi, sl, planes=False)
    yield "update_host_built_block", update(capi, sl, pre=[None, host_block(sl, 1, 5)] + [None] * (sl.F - 2))
    few = make_slam_scene(C=4, n_slam=4, seed=6)
    assert 2 * int(few.n_meas.sum()) <= 80
    yield "update_sform", update(capi, few)
    with env(OVP_EKF_INFO_FORM="1"):
        yield "update_information_form", update(capi, few)
    r = update(capi, semidefinite(sl))
    assert int(r["rc"][0]) == 0  # (chol(P) of the singular prior fails; only ekf_sform behind it returns 0 with P updated)
    yield "update_semidefinite_prior", r
    st = make_stereo_slam_scene(C=11, n_slam=14, seed=4, n_planes=3, outliers=2, wrong_plane=3, cam1_only=2, do_fej=False)
    yield "update_general_stereo", update(capi, st, cam_idx=st.cam_idx)
    yield "update_general_stereo_host_built_block", update(capi, st, cam_idx=st.cam_idx,
                                                           pre=[None, host_block(st, 1, 6)] + [None] * (st.F - 2))
    yield "update_general_camera0", update(capi, sl, cam_idx=np.zeros(sl.clone_idx.shape, np.int32))
    # delayed initialisation
    cand = make_scene(C=4, F=4, seed=9, ragged=True, chi2_mult=0.6)
    mono, stereo = mono_scene(), stereo_scene()
    yield "dinit_mono", dinit(capi, cand, "mono")
    r = dinit(capi, mono, "mono")
    assert r["ok"].any() and not r["ok"].all()  # (rejected candidates: the marginalisation tail runs)
    yield "dinit_mono_some_rejected", r
    yield "dinit_general", dinit(capi, stereo, "general")
    for name, sc in (("mono", mono), ("stereo", stereo)):
        r = dinit(capi, sc, "planes")
        assert set(int(s) for s in r["status"]) == {0, 1, 2}  # (rejected, A accepted, A rejected and B accepted)
        yield "dinit_planes_" + name, r
        slots = np.array(sc.plane_id, dtype=np.int32)
        slots[::2] = 0
        yield "dinit_planes_%s_some_without_plane" % name, dinit(capi, sc, "planes", plane_of_cand=slots)
        yield "dinit_planes_%s_null_planes" % name, dinit(capi, sc, "planes", with_planes=False)
    # ovp_ekf_update on both sides of its S-form limit (80 rows)
    pl = make_scene(C=4, F=16, seed=11, n_planes=2, feats_per_plane=5, planes_in_state_frac=0.5, chi2_mult=99999.0)
    yield "ekf_update_80_rows_sform", ekf(capi, pl, 80)
    yield "ekf_update_81_rows_information_form", ekf(capi, pl, 81)
    # a refused call of each entry, then a valid one on the same context
    ctx = context(capi, sl, cameras=True)
    bad_lm = np.array(sl.lm_id, dtype=np.int32)
    bad_lm[3] = sl.N
    yield "refused_then_update", after_refusal(update(capi, sl, ctx=ctx, lm_id=bad_lm), update(capi, sl, ctx=ctx))
    ctx.cov_upload(sl.P)
    cam0 = np.zeros(sl.clone_idx.shape, np.int32)
    yield "refused_then_update_general", after_refusal(update(capi, sl, ctx=ctx, cam_idx=cam0 + 7), update(capi, sl, ctx=ctx, cam_idx=cam0))
    ctx.close()
    short = np.array(cand.n_meas, dtype=np.int32)
    short[1] = 1
    ctx = context(capi, cand, cap=cand.N + 3 * cand.F)
    yield "refused_then_dinit_mono", after_refusal(dinit(capi, cand, "mono", ctx=ctx, n_meas=short), dinit(capi, cand, "mono", ctx=ctx))
    ctx.close()
    ctx = context(capi, stereo, cap=stereo.N + 3 * stereo.F, cameras=True)
    yield "refused_then_dinit_general", after_refusal(dinit(capi, stereo, "general", ctx=ctx, cam_idx=np.asarray(stereo.cam_idx) + 2),
                                                      dinit(capi, stereo, "general", ctx=ctx))
    ctx.close()
    ctx = context(capi, mono, cap=mono.N + 3 * mono.F)
    beyond = np.array(mono.plane_id, dtype=np.int32)
    beyond[2] = mono.cp.shape[0] + 1
    yield "refused_then_dinit_planes", after_refusal(dinit(capi, mono, "planes", ctx=ctx, plane_of_cand=beyond),
                                                     dinit(capi, mono, "planes", ctx=ctx))
    ctx.close()
    ctx = context(capi, pl)
    yield "refused_then_ekf_update", after_refusal(ekf(capi, pl, 12, ctx=ctx, bad_column=True), ekf(capi, pl, 12, ctx=ctx))
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ov_plane_amd import capi
    from ov_plane_amd.build import source_tree_hash

    rec = dict(library=os.path.relpath(capi.LIB_PATH, ROOT), source_tree_hash_of_this_checkout=source_tree_hash(), digests={})
    for name, out in cases(capi):
        rec["digests"][name] = digest(out)
        print(name, rec["digests"][name], "rc %d" % int(out["rc"][0]))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
