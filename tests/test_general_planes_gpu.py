"""GPU tests of ovp_msckf_plane_update_general: the plane loop with the on-plane features the device batch cannot carry (tracks
above 32 views, observations of a second camera) stacked behind the batch's.

References: ovo_msckf_plane_update (any track length, camera 0) and the sequential numpy reference tests/general_planes_ref.py
(any camera; pinned against the oracle in tests/test_general_planes_cpu.py).  Bounds: those of the plane-loop parity tests of
tests/test_gpu_parity.py for the same quantities - |d state| < 1e-6, covariance 1e-4 correlation-normalised, rows of the gate and
consumed features equal.  The loops run under the reference's own accept / reject sequence (force_decision), so that every plane
takes part in the comparison."""
import numpy as np
import pytest

from tests import general_planes_ref as R
from ov_plane_amd.synth import make_long_plane_scene, make_scene, make_stereo_plane_scene

pytestmark = pytest.mark.gpu
TOL_DX = 1e-6   # tests/test_gpu_parity.py
TOL_P = 1e-4

LONG = dict(C=40, n_planes=4, feats_per_plane=6, n_free=4, seed=1, chi2_mult=1.0)   # the oracle accepts planes 1-3 and rejects plane 4
# N = 300: the loop runs on the 284 involved columns; the oracle rejects plane 3
LONG_SUB = dict(C=44, n_planes=4, feats_per_plane=6, n_free=4, seed=3, chi2_mult=0.95)


def _state_err(sc, out, ref_state, ref_cp):
    st, cp = R.apply_plane_dx(sc, out["dx"], out["ok"])
    e = max(np.abs(st["clone_p"] - ref_state["clone_p"]).max(), np.abs(st["clone_q"] - ref_state["clone_q"]).max(),
            np.abs(st["calib_q"] - ref_state["calib_q"]).max(), np.abs(st["calib_p"] - ref_state["calib_p"]).max(),
            np.abs(st["intr"] - ref_state["intr"]).max(), np.abs(cp - ref_cp).max())
    if "cam1" in st:
        for k in ("calib_q", "calib_p", "intr"):
            e = max(e, np.abs(st["cam1"][k] - ref_state["cam1"][k]).max())
    return float(e)


@pytest.mark.parametrize("kw", [LONG, LONG_SUB], ids=["n276", "n300_substate"])
def test_long_tracks_against_the_oracle(hiplib, oracle, kw):
    """At least 40 clones, planes in the state and outside it, on-plane tracks of up to C views beside ones the batch carries:
    per-plane dx (against the numpy reference, which the CPU test holds to the oracle), final state and P (against the oracle),
    rows of the gate and consumed features, every plane compared."""
    sc = make_long_plane_scene(**kw)
    on = sc.plane_id > 0
    assert ((sc.n_meas > 32) & on).sum() >= 4 and ((sc.n_meas <= 32) & on).sum() >= 4 and sc.n_meas.max() >= 40
    ref = oracle.msckf_plane_update(sc)
    assert ref["plane_ok"].any() and (~ref["plane_ok"]).any() and (ref["plane_rows"] > 0).all()
    npr = R.plane_loop_ref(sc, force=ref["plane_ok"], use_qr=True)
    out = R.run_general(hiplib, sc, force=ref["plane_ok"])
    assert len(out["gen"]) >= 4 and (sc.n_meas[out["gen"]] > 32).all()
    print("plane dx err", np.abs(out["dx"] - npr["dx"]).max(), "state err", _state_err(sc, out, ref, ref["cp"]), "relP",
          R.relP(out["P"], ref["P"]), "chi2", out["chi2"], ref["plane_chi2"])
    assert (out["ok"] == ref["plane_ok"]).all() and (out["dof"] == ref["plane_rows"]).all()
    assert (out["used_all"] == ref["used"]).all()
    assert out["gen_used"].any() and not out["gen_used"].all()
    assert np.abs(out["dx"] - npr["dx"]).max() < TOL_DX
    assert _state_err(sc, out, ref, ref["cp"]) < TOL_DX
    assert R.relP(out["P"], ref["P"]) < TOL_P
    out["ctx"].close()


def test_second_camera_two_plane_sequence(hiplib):
    """Stereo plane scene, both planes accepted: plane 2's rows are built at the calibration of camera 1 that plane 1's commit
    left.  Compared as a sequence against the numpy reference; a reference that does not correct camera 1 is told apart."""
    sc = make_stereo_plane_scene(C=8, n_planes=2, feats_per_plane=10, n_free=4, seed=3, planes_in_state_frac=0.5, chi2_mult=1.0)
    force = np.array([1, 1], dtype=np.uint8)
    npr = R.plane_loop_ref(sc, force=force)
    frozen = R.plane_loop_ref(sc, force=force, freeze_cam1=True)
    assert np.abs(frozen["dx"][1] - npr["dx"][1]).max() > 100 * TOL_DX   # the sequence does depend on camera 1's correction
    out = R.run_general(hiplib, sc, force=force)
    on_gen = sc.plane_id[out["gen"]]
    assert (on_gen == 1).sum() >= 2 and (on_gen == 2).sum() >= 2 and len(out["batch"]) > 0
    print("plane dx err", np.abs(out["dx"] - npr["dx"]).max(0).max(), "vs frozen", np.abs(out["dx"][1] - frozen["dx"][1]).max(),
          "state err", _state_err(sc, out, npr["state"], npr["cp"]), "relP", R.relP(out["P"], npr["P"]))
    assert out["ok"].all() and (out["dof"] == npr["plane_rows"]).all() and (out["used_all"] == npr["used"]).all()
    assert np.abs(out["dx"] - npr["dx"]).max() < TOL_DX
    assert _state_err(sc, out, npr["state"], npr["cp"]) < TOL_DX
    assert R.relP(out["P"], npr["P"]) < TOL_P
    # the tables of ovp_cameras_upload are what the caller gets by applying the returned dx in order
    _, cams = out["ctx"].camera_tables_download(2)
    from ov_plane_amd.synth import quat_2_rot
    assert np.abs(cams[1][:9].reshape(3, 3) - quat_2_rot(npr["state"]["cam1"]["calib_q"])).max() < TOL_DX
    assert np.abs(cams[1][9:12] - npr["state"]["cam1"]["calib_p"]).max() < TOL_DX
    assert np.abs(cams[1][12:20] - npr["state"]["cam1"]["intr"]).max() < TOL_DX
    assert np.abs(cams[0][12:20] - npr["state"]["intr"]).max() < TOL_DX
    out["ctx"].close()


# plane_chi2 of the same scene through the batch alone and with half of its on-plane features moved to the general batch: the
# largest difference seen on the first GPU run was CHI2_SPLIT_OBSERVED = 1.22e-6 on statistics of 70 .. 86
# (profiles/general_planes_timing.json); the bound is 4 x that, as tests/test_precision_gpu.py sets its bounds
CHI2_SPLIT_OBSERVED = 1.22e-6
ONE = dict(C=11, F=60, seed=5, n_planes=4, feats_per_plane=12, chi2_mult=1.0, ragged=True)


def test_batch_and_general_features_are_one_system(hiplib, oracle):
    """A camera-0 scene whose on-plane features all fit the batch, once through ovp_msckf_plane_update and once with half of them
    moved to the general batch: both agree with the oracle and with each other, the plane statistic included."""
    sc = make_scene(**ONE)
    ref = oracle.msckf_plane_update(sc)
    force = ref["plane_ok"].astype(np.uint8)
    ctx = hiplib.Context(sc.N, sc.C, sc.F)
    ctx.cov_upload(sc.P)
    ctx.state_upload(sc)
    ctx.batch_upload_scene(sc)
    a = ctx.plane_update(hiplib.opts_from_scene(sc), sc.plane_id, sc.cp, sc.cp_fej, sc.plane_state_id, force_decision=force)
    a["P"] = ctx.cov_download()
    ctx.close()
    on = np.where(sc.plane_id > 0)[0]
    b = R.run_general(hiplib, sc, force=force, move=on[::2])
    assert len(b["gen"]) == len(on[::2]) and (sc.n_meas[b["gen"]] <= 32).all()
    d_chi2 = float(np.abs(a["chi2"] - b["chi2"]).max())
    print("chi2 batch", a["chi2"], "chi2 split", b["chi2"], "oracle", ref["plane_chi2"], "max |d chi2|", d_chi2)
    print("dx a-b", np.abs(a["dx"] - b["dx"]).max(), "relP a-b", R.relP(b["P"], a["P"]), "relP b-oracle", R.relP(b["P"], ref["P"]))
    for o in (a, b):
        assert (o["ok"] == ref["plane_ok"]).all() and (o["dof"] == ref["plane_rows"]).all()
        assert _state_err(sc, o, ref, ref["cp"]) < TOL_DX
        assert R.relP(o["P"], ref["P"]) < TOL_P
    assert (b["used_all"] == ref["used"]).all() and (a["used"] == ref["used"]).all()
    assert np.abs(a["dx"] - b["dx"]).max() < TOL_DX
    assert R.relP(b["P"], a["P"]) < TOL_P
    assert d_chi2 <= 4.0 * CHI2_SPLIT_OBSERVED, d_chi2
    b["ctx"].close()


def test_long_track_keeps_its_plane_constraint(hiplib, oracle):
    """Semantic check against the previous behaviour: on-plane features of 40 views used to leave the plane loop (they went to the
    point update as plain points, their plane constraint lost).  Through the new entry the planes' dx and P move away from that
    result and onto the oracle's plane loop."""
    sc = make_long_plane_scene(**LONG)
    assert (sc.n_meas[sc.plane_id > 0] == 40).any()
    ref = oracle.msckf_plane_update(sc)
    force = ref["plane_ok"].astype(np.uint8)
    npr = R.plane_loop_ref(sc, force=force, use_qr=True)
    batch, gen = R.split_features(sc)
    # previous route: the plane loop sees the batch's features only
    ctx = hiplib.Context(sc.N, sc.C, len(batch))
    ctx.cov_upload(sc.P)
    ctx.state_upload(sc)
    ctx.batch_upload(sc.uv[batch][:, :32], sc.clone_idx[batch][:, :32], sc.n_meas[batch], sc.p_FinG[batch])
    old = ctx.plane_update(hiplib.opts_from_scene(sc), sc.plane_id[batch], sc.cp, sc.cp_fej, sc.plane_state_id, force_decision=force)
    old["P"] = ctx.cov_download()
    ctx.close()
    new = R.run_general(hiplib, sc, force=force)
    e_old_dx, e_new_dx = np.abs(old["dx"] - npr["dx"]).max(), np.abs(new["dx"] - npr["dx"]).max()
    e_old_P, e_new_P = R.relP(old["P"], ref["P"]), R.relP(new["P"], ref["P"])
    print("dx: old", e_old_dx, "new", e_new_dx, "| P: old", e_old_P, "new", e_new_P)
    assert e_new_dx < TOL_DX and e_new_P < TOL_P
    assert e_old_dx > 100 * TOL_DX and e_old_P > 10 * TOL_P
    assert np.abs(new["dx"] - old["dx"]).max() > 100 * TOL_DX
    new["ctx"].close()


def test_empty_general_batch_is_the_plain_loop_bit_for_bit(hiplib):
    sc = make_scene(C=11, F=160, seed=5, n_planes=4, feats_per_plane=25, chi2_mult=1.0)
    o = hiplib.opts_from_scene(sc)
    outs = []
    for variant in ("plain", "none", "off_plane"):
        ctx = hiplib.Context(sc.N, sc.C, sc.F)
        ctx.cov_upload(sc.P)
        ctx.state_upload(sc)
        ctx.cameras_upload(sc)
        ctx.batch_upload_scene(sc)
        if variant == "plain":
            r = ctx.plane_update(o, sc.plane_id, sc.cp, sc.cp_fej, sc.plane_state_id)
        elif variant == "none":
            r = ctx.plane_update_general(o, sc.plane_id, sc.cp, sc.cp_fej, sc.plane_state_id)
        else:  # a general batch none of whose features lies on a plane
            r = ctx.plane_update_general(o, sc.plane_id, sc.cp, sc.cp_fej, sc.plane_state_id, sc=sc, feats=[0, 1, 2], plane_of_gen=[0, 0, 0])
            assert not r["gen_used"].any()
        r["P"] = ctx.cov_download()
        outs.append(r)
        ctx.close()
    for r in outs[1:]:
        for k in ("dx", "chi2", "P", "ok", "dof", "used"):
            assert np.array_equal(np.asarray(r[k]), np.asarray(outs[0][k])), k


def test_two_runs_are_bit_identical(hiplib):
    sc = make_long_plane_scene(**LONG)
    a = R.run_general(hiplib, sc)
    b = R.run_general(hiplib, sc)
    for k in ("dx", "chi2", "P", "ok", "gen_used", "used"):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    a["ctx"].close()
    b["ctx"].close()


def test_limits_leave_everything_untouched(hiplib):
    """The limits of the general entries, checked on the host before anything is enqueued: OVP_E_CAPACITY above OVP_GEN_MAX_MEAS
    views, OVP_E_ARG for a camera without tables / a clone slot outside the tables / plane_of_gen outside the planes."""
    sc = make_scene(C=11, F=60, seed=5, n_planes=4, feats_per_plane=12, chi2_mult=1.0)
    o = hiplib.opts_from_scene(sc)
    ctx = hiplib.Context(sc.N, sc.C, sc.F)
    ctx.cov_upload(sc.P)
    ctx.state_upload(sc)
    ctx.cameras_upload(sc)
    ctx.batch_upload_scene(sc)
    P0, cams0 = ctx.cov_download(), np.concatenate([t.ravel() for t in ctx.camera_tables_download(1)])
    f = int(np.where(sc.plane_id > 0)[0][0])
    M = 70
    uv = np.zeros((1, M, 2), dtype=np.float32)
    ci = np.zeros((1, M), dtype=np.int32)
    cam = np.zeros((1, M), dtype=np.int32)
    pog = [int(sc.plane_id[f])]
    cases = [(dict(n_meas=[65]), "capacity"), (dict(n_meas=[5], cam=1), "arg"), (dict(n_meas=[5], clone=sc.C), "arg"),
             (dict(n_meas=[5], pog=[5]), "arg")]
    for kw, kind in cases:
        cam_k, ci_k = cam.copy(), ci.copy()
        cam_k[0, 0] = kw.get("cam", 0)
        ci_k[0, 0] = kw.get("clone", 0)
        r = ctx.plane_update_general(o, sc.plane_id, sc.cp, sc.cp_fej, sc.plane_state_id, uv=uv, clone_idx=ci_k, cam_idx=cam_k,
                                     n_meas=kw["n_meas"], p_FinG=sc.p_FinG[[f]], plane_of_gen=kw.get("pog", pog), raise_on_error=False)
        assert r["rc"] == (hiplib.OVP_E_CAPACITY if kind == "capacity" else hiplib.OVP_E_ARG), (kw, r["rc"])
        assert np.array_equal(ctx.cov_download(), P0)
        assert np.array_equal(np.concatenate([t.ravel() for t in ctx.camera_tables_download(1)]), cams0)
    # the context still works
    r = ctx.plane_update(o, sc.plane_id, sc.cp, sc.cp_fej, sc.plane_state_id)
    assert r["rc"] == 0
    ctx.close()


def test_host_mirror_routes_long_on_plane_tracks_through_the_loop(hiplib, oracle):
    """UpdaterMSCKF::update with StateOptions::gpu_general_planes: the on-plane features above 32 views stay in the plane loop, are
    flagged as used by their accepted planes and are not offered to the point update - the whole update then is the oracle's
    (plane loop over every on-plane feature, point loop on the rest).  With the option off the result is the previous one: such
    features are not consumed by their planes."""
    from ov_plane_amd.build import build_host

    build_host()
    from ov_plane_amd import hostlib
    from tests.test_gpu_parity import _oracle_full_update

    sc = make_long_plane_scene(C=40, n_planes=4, feats_per_plane=6, n_free=4, seed=1, chi2_mult=99999.0)
    long_on = (sc.n_meas > 32) & (sc.plane_id > 0)
    assert long_on.sum() >= 4
    ref = _oracle_full_update(oracle, sc)
    assert ref["used"][long_on].all()
    on = hostlib.run_msckf_update(sc, general_planes=True)
    print("host route: state err", np.abs(on["clone_p"] - ref["clone_p"]).max(), "relP", R.relP(on["P"], ref["P"]))
    assert (on["used"] == ref["used"]).all() and (on["kept"] == ref["kept"]).all() and on["deleted"].all()
    assert np.abs(on["clone_p"] - ref["clone_p"]).max() < TOL_DX and np.abs(on["clone_q"] - ref["clone_q"]).max() < TOL_DX
    assert np.abs(on["calib_p"] - ref["calib_p"]).max() < TOL_DX and np.abs(on["intr"] - ref["intr"]).max() < TOL_DX
    assert np.abs(on["cp_state"] - ref["cp"][sc.plane_in_state]).max() < TOL_DX
    assert R.relP(on["P"], ref["P"]) < TOL_P
    off, off2 = hostlib.run_msckf_update(sc), hostlib.run_msckf_update(sc, general_planes=False)
    # (a plane outside the state that is left with fewer than four features does not run at all: its short tracks stay unused too)
    assert not off["used"][long_on].any() and off["used"].any() and not off["used"][sc.plane_id == 0].any()
    assert off["used"].sum() < on["used"].sum()
    for k in ("P", "clone_q", "clone_p", "intr", "used", "kept"):
        assert np.array_equal(off[k], off2[k]), k
    assert R.relP(off["P"], ref["P"]) > 10 * TOL_P


def _only_camera1(sc, plane):
    """The scene with the features of `plane` (1-based) reduced to camera 1's observations."""
    from ov_plane_amd.synth import Scene

    out = Scene(sc)
    for k in ("uv", "clone_idx", "cam_idx", "n_meas", "uv_norm"):
        out[k] = sc[k].copy()
    for f in np.where(sc.plane_id == plane)[0]:
        m = int(sc.n_meas[f])
        sel = np.where(sc.cam_idx[f, :m] == 1)[0]
        assert 2 <= len(sel) < m
        for k in ("uv", "clone_idx", "cam_idx", "uv_norm"):
            out[k][f, :len(sel)] = sc[k][f, sel]
        out["clone_idx"][f, len(sel):] = -1
        out["cam_idx"][f, len(sel):] = 0
        out["n_meas"][f] = len(sel)
    return out


@pytest.mark.parametrize("cam1_only_plane", [0, 1, 2], ids=["both_cameras", "in_state_plane_camera1", "out_of_state_plane_camera1"])
def test_planes_with_general_features_only(hiplib, cam1_only_plane):
    """Every on-plane feature is seen by both cameras, as on a stereo rig: no plane has a feature in the device batch, the loop's
    structured Gram is empty and the whole pair comes from the general rows.  One plane in the state, one outside.  Variants: one
    plane's features keep camera 1's observations only - camera 0's calibration columns are then not among that plane's involved
    columns, and the rows of the gate say so."""
    sc = make_stereo_plane_scene(C=8, n_planes=2, feats_per_plane=8, n_free=4, seed=4, stereo_frac=1.0, planes_in_state_frac=0.5,
                                 chi2_mult=1.0)
    assert sc.plane_state_id[0] >= 0 and sc.plane_state_id[1] < 0
    if cam1_only_plane:
        sc = _only_camera1(sc, cam1_only_plane)
    force = np.array([1, 1], dtype=np.uint8)
    npr = R.plane_loop_ref(sc, force=force)
    out = R.run_general(hiplib, sc, force=force)
    assert len(out["batch"]) == 0 and (sc.plane_id[out["gen"]] > 0).sum() == 16
    print("plane dx err", np.abs(out["dx"] - npr["dx"]).max(), "state err", _state_err(sc, out, npr["state"], npr["cp"]), "relP",
          R.relP(out["P"], npr["P"]), "dof", out["dof"], npr["plane_rows"], "chi2", out["chi2"], npr["plane_chi2"])
    assert out["ok"].all() and (out["dof"] == npr["plane_rows"]).all() and (out["used_all"] == npr["used"]).all()
    assert np.abs(out["dx"] - npr["dx"]).max() < TOL_DX
    assert _state_err(sc, out, npr["state"], npr["cp"]) < TOL_DX
    assert R.relP(out["P"], npr["P"]) < TOL_P
    out["ctx"].close()


def test_64_observation_stereo_tracks(hiplib):
    """The longest track the general entries take: 32 clones, every view by both cameras, 64 observations per on-plane feature
    (129 rows with the merged point-on-plane row), planes in the state and outside it, against the numpy reference."""
    sc = make_stereo_plane_scene(C=32, n_planes=2, feats_per_plane=5, n_free=2, seed=2, stereo_frac=1.0, planes_in_state_frac=0.5,
                                 chi2_mult=1.0)
    assert (sc.n_meas[sc.plane_id > 0] == 64).all()
    force = np.array([1, 1], dtype=np.uint8)
    npr = R.plane_loop_ref(sc, force=force, use_qr=True)
    out = R.run_general(hiplib, sc, force=force)
    print("plane dx err", np.abs(out["dx"] - npr["dx"]).max(), "state err", _state_err(sc, out, npr["state"], npr["cp"]), "relP",
          R.relP(out["P"], npr["P"]), "dof", out["dof"], npr["plane_rows"])
    assert out["ok"].all() and (out["dof"] == npr["plane_rows"]).all() and (out["used_all"] == npr["used"]).all()
    assert np.abs(out["dx"] - npr["dx"]).max() < TOL_DX
    assert _state_err(sc, out, npr["state"], npr["cp"]) < TOL_DX
    assert R.relP(out["P"], npr["P"]) < TOL_P
    out["ctx"].close()


def _exact_clone_scene():
    """The prior of tests/test_gpu_parity.py::test_plane_loop_on_a_positive_semidefinite_prior, case exact_clone below the
    factorization's limit: chol(P) fails and the loop runs once more on the pivot-dropping factor."""
    sc = make_scene(C=9, F=150, seed=43, n_planes=3, feats_per_plane=25, planes_in_state_frac=0.67, chi2_mult=99999.0)
    assert sc.N <= 287
    a, b = sc.ids["clones"][-2], sc.ids["clones"][-1]
    idx = np.arange(sc.N)
    idx[b:b + 6] = np.arange(a, a + 6)
    sc["P"] = sc.P[np.ix_(idx, idx)]
    for k in ("clone_q", "clone_p", "clone_q_fej", "clone_p_fej"):
        sc[k][-1] = sc[k][-2]
    assert np.linalg.eigvalsh(sc.P).min() < 1e-12 * np.linalg.eigvalsh(sc.P).max()
    return sc


def test_no_route_into_the_loop_leaves_anything_behind_for_the_next(hiplib, monkeypatch):
    """ONE context through every route into the plane loop, one after the other: general features in the loop's own column order,
    a plain call, the same in the state's order (OVP_PL_NATURAL_ORDER), a positive semi-definite prior (the retry), ovp_plane_init,
    the plain call again.  Covariance, state and batch are uploaded afresh before each call; every output of every step equals
    BIT FOR BIT what the same call gives on a fresh context of the same capacity."""
    stereo = make_stereo_plane_scene(C=8, n_planes=2, feats_per_plane=10, n_free=4, seed=3, planes_in_state_frac=0.5, chi2_mult=1.0)
    small = make_scene(C=8, F=90, seed=73, n_planes=3, feats_per_plane=15, chi2_mult=99999.0)
    psd = _exact_clone_scene()
    fresh_planes = make_scene(C=8, F=80, seed=16, n_planes=2, feats_per_plane=25, planes_in_state_frac=0.0, chi2_mult=1.0, ragged=True)
    cap = (max(s.N for s in (stereo, small, psd, fresh_planes)) + 6, 9, 150)

    def general(ctx):
        out = R.run_general(hiplib, stereo, force=np.array([1, 1], dtype=np.uint8), ctx=ctx)
        return {k: v for k, v in out.items() if k != "ctx"}

    def plain(sc, init=False):
        def run(ctx):
            ctx.cov_upload(sc.P)
            ctx.state_upload(sc)
            ctx.batch_upload_scene(sc)
            o = hiplib.opts_from_scene(sc)
            out = ctx.plane_init(o, sc.plane_id, sc.cp, 5.0, 1e9) if init else \
                ctx.plane_update(o, sc.plane_id, sc.cp, sc.cp_fej, sc.plane_state_id)
            out["P"] = ctx.cov_download()
            return out
        return run

    steps = [("general", general, False), ("plain", plain(small), False), ("natural_order", plain(small), True),
             ("semidefinite_retry", plain(psd), False), ("plane_init", plain(fresh_planes, init=True), False),
             ("plain_again", plain(small), False)]

    def run_step(ctx, fn, natural):
        if natural:
            monkeypatch.setenv("OVP_PL_NATURAL_ORDER", "1")
        else:
            monkeypatch.delenv("OVP_PL_NATURAL_ORDER", raising=False)
        try:
            return fn(ctx)
        finally:
            monkeypatch.delenv("OVP_PL_NATURAL_ORDER", raising=False)

    one = hiplib.Context(*cap)
    chained = [run_step(one, fn, natural) for _, fn, natural in steps]
    one.close()
    assert chained[0]["ok"].all() and chained[0]["gen_used"].any()
    assert chained[1]["ok"].any() and chained[3]["ok"].all() and chained[4]["ok"].all()
    assert np.array_equal(chained[4]["new_ids"], fresh_planes.N + 3 * np.arange(2))
    for (name, fn, natural), got in zip(steps, chained):
        ctx = hiplib.Context(*cap)
        want = run_step(ctx, fn, natural)
        ctx.close()
        for k in ("ok", "chi2", "dof", "dx", "used", "gen_used", "P", "new_ids", "cp"):
            assert (k in got) == (k in want)
            if k in want:
                assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), (name, k)
