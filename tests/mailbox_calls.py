"""One small fixed call per entry point that returns its results through a pinned mailbox (csrc/ovp_mailbox.h), each on a context
it is handed: it uploads what it needs itself, so its results depend on nothing an earlier call left in the context - except, if
the handshake were wrong, on what that call left in the pinned block.  Every function returns {name: array}; tests/test_mailbox_gpu.py
compares a sequence on one context with fresh contexts, tools/mailbox_digest.py hashes the same calls for two builds."""
import numpy as np

from ov_plane_amd.synth import make_scene, make_slam_scene

N_MAX, C_MAX, F_MAX = 160, 4, 40


def _planes(n_planes, F=16, feats_per_plane=5, seed=11):
    return make_scene(C=4, F=F, seed=seed, n_planes=n_planes, feats_per_plane=feats_per_plane, planes_in_state_frac=0.5,
                      chi2_mult=99999.0)


SCENES = {}


def scene(name):
    """built once, never modified"""
    if name not in SCENES:
        SCENES[name] = {"planes2": lambda: _planes(2), "planes1": lambda: _planes(1),
                        "planes_big": lambda: _planes(4, F=40, feats_per_plane=9, seed=12),
                        "slam": lambda: make_slam_scene(C=4, n_slam=10, seed=6),
                        "cand": lambda: make_scene(C=4, F=3, seed=8, ragged=True, chi2_mult=0.6),
                        "cand4": lambda: make_scene(C=4, F=4, seed=9, ragged=True, chi2_mult=0.6)}[name]()
        assert SCENES[name].N <= N_MAX - 12 and SCENES[name].F <= F_MAX
    return SCENES[name]


def new_context(capi):
    return capi.Context(N_MAX, C_MAX, F_MAX)


def _load(ctx, sc, batch=True):
    ctx.cov_upload(sc.P)
    ctx.state_upload(sc)
    if batch:
        ctx.batch_upload_scene(sc)


def plane_loop(capi, ctx, name="planes2"):
    sc = scene(name)
    _load(ctx, sc)
    out = ctx.plane_update(capi.opts_from_scene(sc), sc.plane_id, sc.cp, sc.cp_fej, sc.plane_state_id)
    assert out["rc"] == 0 and out["ok"].any()
    return dict(dx=out["dx"], ok=out["ok"], chi2=out["chi2"], dof=out["dof"], used=out["used"], P=ctx.cov_download())


def plane_loop_one(capi, ctx):
    return plane_loop(capi, ctx, "planes1")


def plane_loop_big(capi, ctx):
    return plane_loop(capi, ctx, "planes_big")


def slam_update(capi, ctx):
    sc = scene("slam")
    _load(ctx, sc, batch=False)
    out = ctx.slam_update(capi.opts_from_scene(sc), sc.uv, sc.clone_idx, sc.n_meas, sc.p_FinG, sc.p_FinG_fej, sc.lm_id)
    assert out["status"].any()
    return dict(dx=out["dx"], status=out["status"], chi2=out["chi2"], P=ctx.cov_download(),
                info=np.array([out["info"].n_rows, out["info"].n_cols, out["info"].n_accepted]))


def _dense(sc, rows, seed):
    rng = np.random.default_rng(seed)
    cols = np.r_[sc.ids["clones"][1] + np.arange(6), sc.ids["calib"] + np.arange(6)]
    return rng.standard_normal((rows, len(cols))), cols, 1e-3 * rng.standard_normal(rows)


def ekf_update(capi, ctx, rows=12):
    """rows = 12: the covariance form; rows = 96 (more than 80): the information form"""
    sc = scene("planes2")
    _load(ctx, sc, batch=False)
    H, cols, r = _dense(sc, rows, 3)
    dx, info = ctx.ekf_update(H, cols, r)
    return dict(dx=dx, P=ctx.cov_download(), info=np.array([info.n_rows, info.n_cols]))


def ekf_update_info_form(capi, ctx):
    return ekf_update(capi, ctx, rows=96)


def cov_initialize(capi, ctx):
    sc = scene("planes2")
    _load(ctx, sc, batch=False)
    rng = np.random.default_rng(4)
    Hu, cols, r = _dense(sc, 9, 4)
    Hx = rng.standard_normal((3, len(cols)))
    HLi = np.linalg.inv(rng.standard_normal((3, 3)) + 3.0 * np.eye(3))
    ok, chi2, dx = ctx.cov_initialize(Hx, Hu, cols, HLi, np.eye(3), r, 1.0, 1e9)
    assert ok
    return dict(ok=np.array([ok]), chi2=np.array([chi2]), dx=dx, P=ctx.cov_download())


def cov_propagate(capi, ctx):
    sc = scene("planes2")
    _load(ctx, sc, batch=False)
    Phi = np.eye(15) + 1e-3 * np.random.default_rng(0).standard_normal((15, 15))
    neg = ctx.cov_propagate(0, [0], [15], Phi, 1e-6 * np.eye(15))
    return dict(neg=np.array([neg]), P=ctx.cov_download())


def point_update_async(capi, ctx):
    """the staged point update: ovp_msckf_build_gate_gram_async -> ovp_ekf_update_from_gram_async -> ovp_msckf_fetch_results"""
    sc = scene("planes2")
    _load(ctx, sc)
    ctx.build_gate_gram_async(capi.opts_from_scene(sc))
    ctx.ekf_update_from_gram_async()
    out = ctx.fetch_results()
    assert out["accepted"].any()
    return dict(dx=out["dx"], accepted=out["accepted"], chi2=out["chi2"], P=ctx.cov_download())


def point_update(capi, ctx):
    sc = scene("planes2")
    _load(ctx, sc)
    out = ctx.msckf_update(capi.opts_from_scene(sc))
    return dict(dx=out["dx"], accepted=out["accepted"], chi2=out["chi2"], P=ctx.cov_download())


def slam_delayed_init(capi, ctx, name="cand"):
    sc = scene(name)
    _load(ctx, sc, batch=False)
    out = ctx.slam_delayed_init(capi.opts_from_scene(sc), sc.uv, sc.clone_idx, sc.n_meas, sc.p_FinG)
    return dict(ok=out["ok"], chi2=out["chi2"], new_id=out["new_id"], delta_init=out["delta_init"], dx=out["dx"], P=ctx.cov_download())


def slam_delayed_init_four(capi, ctx):
    return slam_delayed_init(capi, ctx, "cand4")


def detector_frames():
    """two walls of 16 points and 8 points off them over 8 frames: five frames of history with all 40 points, then a frame of 12
    points of one wall, one of all 40 (28 of them new again: they have no estimate yet) and one of the 12; the restatement
    (tests/plane_detect_ref.py) finds planes in each of the three"""
    import plane_detect_ref as ref

    frames = ref.two_wall_scene(2, n_wall=16, n_off=8, n_frames=8)
    few = np.arange(12)
    cut = lambda fr: (fr[0][few], fr[1][few], fr[2][few], fr[3], fr[4])
    return frames[:5], [cut(frames[5]), frames[6], cut(frames[7])]


def detector_frame(det, frame):
    """one frame through the detector -> everything it gives back"""
    ids = frame[0]
    has, pf = det.triangulate(*frame)
    det.planes()
    m = det.feature2plane()
    feats = [det.feature(int(f)) for f in ids]
    return dict(has=has, accepted=det.accepted, p=pf, map=np.array(sorted(m.items()), dtype=np.int64).reshape(-1, 2),
                filter=det.filter_rows(), avg=np.array([d["avg_norm"] for d in feats]),
                normals=np.concatenate([d["normals"].ravel() for d in feats]),
                count=np.array([d["count"] for d in feats]))
