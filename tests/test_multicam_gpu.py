"""The any-camera kernels with three and four cameras (tests/multicam.py).

  (1) the general point path (ovp_msckf_general_features: k_feat_gen, k_gen_pair) against the long-double truth of oracle/ld_ref.py
      with the pass rule of tests/test_precision_gpu.py: decisions equal np_ref.msckf_point_update_dense, chi2 and the information pair
      (read back through a point update on a batch that contributes nothing) within max(K e_f64, HEADROOM x OBSERVED) and under the
      family ceilings of that file; one update shared with the batch and ovp_triangulate_general on the mixed-lens scene;
  (2) slot indexing of the other any-camera entries: a two-camera scene of their own tests extended to four cameras, run with the
      tables as [c0, c1, c2, c3] and again as [c0, c2, c3, c1] with camera 1 relabelled 3.

Why the two slot orders are held to each other BIT FOR BIT in the SLAM update, both delayed inits, the plane fit and the active
tracks.  There a slot number enters the device code in two ways only:
as an address (cam_cal + 20 * cam, cam_fisheye[cam], cam_calib_id[cam], cam_intr_id[cam], poses + 12 * cam), which fetches the same
values from another place, and as the ORDER of the calibration blocks among a feature's local columns, which every entry builds by
walking the cameras of the feature in ascending slot order (the camera masks of ovp_api_slam.hip and k_slam_body.h, CalCols::col_of
per used camera in ovp_api_plane.hip / ovp_api_general.hip).  Relabelling {0, 1} as {0, 3} keeps that order, each table keeps its
own state columns, and the observations keep their order in every list: the rows, their column ids and every sum downstream are
the same operations on the same numbers.  The commits walk the uploaded tables one by one, each moved by its own columns of dx.
So nothing may differ, and a last-bit difference would mean that some slot number got into the arithmetic.

Not so in the plane loop and the plane initialisation (ovp_api_plane.hip): with general features the loop's own column order places
the calibration columns of EVERY uploaded camera, slot by slot (co.place(gen_calib_id[k]) / gen_intr_id[k] for k = 0 .. n_cams - 1),
so the rotated order factorizes the same matrix under a permutation of its last columns: other sums, rounding-level differences.
These two hold the orders to each other at the bound their own tests hold against the reference."""
import numpy as np
import pytest

from oracle import ld_ref, np_ref
from tests import multicam as mc
from tests.test_general_features_gpu import TOL_DX, TOL_P, chi2_table, fits_batch, relP, triangulate_general_np, upload_batch
from tests.test_precision_gpu import _check, _givens_pair

pytestmark = pytest.mark.gpu


def _bits(a, b):
    """Same type, shape and bytes (lists: entry by entry)."""
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_bits(x, y) for x, y in zip(a, b))
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _context(capi, sc, cap=None):
    ctx = capi.Context(sc.N if cap is None else cap, sc.C, sc.F)
    ctx.cov_upload(sc.P)
    ctx.state_upload(sc)
    ctx.cameras_upload(sc)
    return ctx


def _nothing_batch(ctx, sc):
    """Two features of one observation each: the point update drops them (UpdaterMSCKF.cpp:94-96), so the pair it assembles is the
    pending pair of the general entry alone."""
    ctx.batch_upload(sc.uv[:2, :1], np.zeros((2, 1), dtype=np.int32), np.ones(2, dtype=np.int32), sc.p_FinG[:2])


@pytest.fixture(scope="module")
def scenes():
    return {}


def _case(scenes, name):
    if name not in scenes:
        sc = mc.make_case(name)
        scenes[name] = (sc, np_ref.msckf_point_update_dense(sc, chi2_table()), ld_ref.point_pair(sc))
    return scenes[name]


# ---- (1) the general point path ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(mc.CASES))
def test_general_pair_and_chi2_against_long_double(hiplib, scenes, case):
    """k_feat_gen + k_gen_pair on every feature of the case, under the rule, K, HEADROOM and family ceilings of
    tests/test_precision_gpu.py (its _check, with this file's OBSERVED)."""
    capi = hiplib
    sc, ref, truth = _case(scenes, case)
    mc.check_case(case, sc)
    ctx = _context(capi, sc)
    o = capi.opts_from_scene(sc)
    acc, chi2, rc = ctx.msckf_general_features(o, sc)
    assert rc == 0
    _nothing_batch(ctx, sc)
    out = ctx.msckf_update(o)
    assert out["rc"] == 0 and not out["accepted"].any()
    ld_ = ((sc.N + 15) // 16) * 16
    Ab = ctx.debug_read("Ab", (sc.N + 1, ld_)).copy()
    ctx.close()
    A, b = Ab[:sc.N, :sc.N], Ab[sc.N, :sc.N]
    assert (acc == ref["accepted"]).all(), (np.where(acc != ref["accepted"])[0], chi2, ref["chi2"])
    mc.check_decisions(case, acc, sc)
    feats = np.where(acc)[0]
    tp = ld_ref.point_pair(sc, feats=feats, with_chi2=False)
    Ag, bg = _givens_pair(sc, feats)
    eA, eb = ld_ref.err_pair(A, b, tp["A"], tp["b"], tp["rr"])
    fA, fb = ld_ref.err_pair(Ag, bg, tp["A"], tp["b"], tp["rr"])
    # the pair lives on the accepted features' columns only: a write anywhere else (another camera's block) is an error of its own
    used = np.zeros(sc.N, dtype=bool)
    for f in feats:
        used[np_ref.order_cols(np_ref.feature_jacobian_full(sc, int(f))[3])] = True
    assert not A[~used].any() and not A[:, ~used].any() and not b[~used].any()
    _check([(case + " chi2", "chi2", ld_ref.err_chi2(chi2, truth["chi2"]), ld_ref.err_chi2(ref["chi2"], truth["chi2"])),
            (case + " A", "A", eA, fA), (case + " b", "b", eb, fb)], OBSERVED)


def test_one_update_with_the_batch_on_the_mixed_lens_scene(hiplib, scenes):
    """K4_mixed_lens: the camera-0 features of <= 32 views take the batch, all others the general entry; ONE update equal to the dense
    restatement at the project's tolerances, two runs bit for bit."""
    capi = hiplib
    sc, ref, _ = _case(scenes, "K4_mixed_lens")
    fit = fits_batch(sc)
    gen, bat = np.where(~fit)[0], np.where(fit)[0]
    assert len(bat) >= 3 and len(gen) >= 12
    o = capi.opts_from_scene(sc)
    ctx = _context(capi, sc)
    runs = []
    for _ in range(2):
        ctx.cov_upload(sc.P)
        acc_g, chi2_g, _ = ctx.msckf_general_features(o, sc, gen)
        upload_batch(ctx, sc, bat)
        out = ctx.msckf_update(o)
        runs.append((acc_g, chi2_g, out, ctx.cov_download()))
    ctx.close()
    (acc_g, chi2_g, out, P), (acc_2, chi2_2, out2, P2) = runs
    assert (acc_g == ref["accepted"][gen]).all() and (out["accepted"] == ref["accepted"][bat]).all()
    derr, perr = float(np.abs(out["dx"] - ref["dx"]).max()), relP(P, ref["P"])
    print("mixed lens, one update: max |dx err| %.3e, normalised |dP| %.3e" % (derr, perr))
    assert derr < TOL_DX and perr < TOL_P
    assert np.array_equal(out["dx"], out2["dx"]) and np.array_equal(P, P2) and np.array_equal(chi2_g, chi2_2) and (acc_g == acc_2).all()


def test_triangulation_over_four_cameras(hiplib, scenes):
    """ovp_triangulate_general on K4_mixed_lens (features of camera 3 alone, of {1, 2} alone, of all four; cameras 1 and 3
    equidistant - the normalised coordinates carry the lens) against triangulate_general_np at that test's bound (1e-6)."""
    capi = hiplib
    sc, _, _ = _case(scenes, "K4_mixed_lens")
    only3 = [f for f in range(sc.F) if mc.cameras_of(sc, f) == [3]]
    only12 = [f for f in range(sc.F) if mc.cameras_of(sc, f) == [1, 2]]
    assert len(only3) >= 3 and len(only12) >= 3
    ctx = _context(capi, sc)
    out = ctx.triangulate_general(sc)
    ctx.close()
    tri = [triangulate_general_np(sc, f) for f in range(sc.F)]
    ok_ref = np.array([t[0] for t in tri])
    p_ref = np.array([t[1] for t in tri])
    assert (out["ok"] == ok_ref).all() and ok_ref.sum() >= 0.9 * sc.F
    assert ok_ref[only3].all() and ok_ref[only12].all()
    err = np.abs(out["p_FinG"][ok_ref] - p_ref[ok_ref]).max(axis=1)
    print("triangulation over four cameras: max |p - p_ref| %.3e m (camera 3 only %.3e, cameras {1, 2} only %.3e)" % (
        err.max(), np.abs(out["p_FinG"][only3] - p_ref[only3]).max(), np.abs(out["p_FinG"][only12] - p_ref[only12]).max()))
    assert err.max() < 1e-6
    assert np.abs(out["p_FinG"][ok_ref] - sc.truth["p_f"][ok_ref]).max() < 0.5


# ---- (2) slot indexing of the other any-camera entries -------------------------------------------------------------------------
def _tables_after(sc, cams, dxs):
    """The 20-double device table of every camera of `cams` after Type::update with the corrections `dxs`, in order."""
    from ov_plane_amd.synth import quat_2_rot, quat_boxplus

    out = []
    for t in cams:
        q, p, intr = t["calib_q"].copy(), t["calib_p"].copy(), t["intr"].copy()
        for dx in dxs:
            q = quat_boxplus(q, dx[t["calib_id"]:t["calib_id"] + 3])
            p = p + dx[t["calib_id"] + 3:t["calib_id"] + 6]
            intr = intr + dx[t["intr_id"]:t["intr_id"] + 8]
        out.append(np.r_[quat_2_rot(q).ravel(), p, intr])
    return np.array(out)


def test_slam_update_general_slots(hiplib):
    """ovp_slam_update_general (k_slam_gate_gen) on the first scene of test_general_slam_gpu.UPDATE_SCENES, calibration estimated,
    extended to four cameras: statuses, counts, chi2, dx and P of the rotated order equal to the straight one's bit for bit (module
    docstring: k_slam_gate_gen places the calibration blocks by the popcount of the landmark's camera mask below the camera), and the
    straight one within that test's bounds of the dense reference of the two-camera scene on its columns (the appended columns
    carry no rows, so the update of the others does not depend on them)."""
    from tests import test_general_slam_gpu as S

    capi = hiplib
    sc0 = S.UPDATE_SCENES[0][1]()
    assert sc0.opts["do_calib_pose"] and sc0.opts["do_calib_intr"] and (sc0.cam_idx == 1).any()
    ref = S.slam_update_reference(sc0)
    scA = mc.add_cameras(sc0, 4)
    scB = mc.slots_rotated(scA)
    kw = S.plane_slam(sc0)
    outs = []
    for sc in (scA, scB):
        ctx = _context(capi, sc)
        out = ctx.slam_update_general(capi.opts_from_scene(sc), sc.uv, sc.clone_idx, sc.cam_idx, sc.n_meas, sc.p_FinG, sc.p_FinG_fej,
                                      sc.lm_id, kw["plane_state_id"], kw["cp"], kw["cp_fej"])
        outs.append((out, ctx.cov_download()))
        ctx.close()
    (a, Pa), (b, Pb) = outs
    N0 = sc0.N
    assert (a["status"] == ref["status"]).all() and (b["status"] == a["status"]).all()
    assert (a["status"] == 2).any() and (a["status"] == 0).any()
    assert a["info"].n_accepted == b["info"].n_accepted == int((ref["status"] > 0).sum())
    cs = max(1.0, np.abs(ref["chi2"]).max())
    assert np.abs(a["chi2"] - ref["chi2"]).max() <= 1e-9 * cs
    assert np.abs(a["dx"][:N0] - ref["dx"]).max() < S.TOL_DX and relP(Pa[:N0, :N0], ref["P"]) < S.TOL_P
    assert _bits(b["chi2"], a["chi2"]) and _bits(b["dx"], a["dx"]) and _bits(Pb, Pa)
    assert np.abs(a["dx"][N0:]).max() > 0  # (the unused cameras' columns move through their correlation with the clones)


def test_slam_delayed_init_general_slots(hiplib):
    """ovp_slam_delayed_init_general (k_dinit_rows_gen and the commit of every uploaded camera's table) on the candidates of
    test_general_slam_gpu's delayed-init test extended to four cameras, in both slot orders: decisions, ids, every candidate's
    correction and the final covariance equal bit for bit (module docstring: the host lays a candidate's calibration blocks out
    camera by camera in slot order, ccol[cam]), and the straight order within that test's bounds of its sequential reference on the
    two-camera scene's columns; the device tables read back: slot 3 of the rotated order is slot 1 of the straight one bit for bit,
    and every table, used or not, is its upload moved by its own columns of the returned corrections."""
    from tests import test_general_slam_gpu as S

    capi = hiplib
    sc0 = S.stereo_candidates()
    ref = S.delayed_init_reference(sc0)
    assert ref["ok"].sum() >= 6
    scA = mc.add_cameras(sc0, 4)
    scB = mc.slots_rotated(scA)
    outs = []
    for sc in (scA, scB):
        ctx = _context(capi, sc, cap=sc.N + 3 * sc.F)
        out = ctx.slam_delayed_init_general(capi.opts_from_scene(sc), sc.uv, sc.clone_idx, sc.cam_idx, sc.n_meas, sc.p_FinG)
        outs.append((out, ctx.cov_download(), ctx.camera_tables_download(4)))
        ctx.close()
    (a, Pa, (cal_a, gen_a)), (b, Pb, (cal_b, gen_b)) = outs
    N0, NA = sc0.N, scA.N
    keep = lambda n: np.r_[np.arange(N0), np.arange(NA, n)]  # the two-camera scene's columns and the new landmarks
    assert (a["ok"] == ref["ok"]).all() and (b["ok"] == a["ok"]).all()
    assert (a["new_id"] == np.where(ref["ok"], ref["new_id"] + (NA - N0), -1)).all() and (b["new_id"] == a["new_id"]).all()
    acc = np.where(ref["ok"])[0]
    assert np.abs(a["delta_init"][acc] - ref["delta_init"][acc]).max() < S.TOL_DX
    assert _bits(b["delta_init"], a["delta_init"])
    for l in acc:
        n = len(ref["dx"][l]) + (NA - N0)
        assert np.abs(a["dx"][l][:n][keep(n)] - ref["dx"][l]).max() < S.TOL_DX
        assert _bits(b["dx"][l], a["dx"][l]), l
    assert Pa.shape[0] == ref["P"].shape[0] + (NA - N0) == Pb.shape[0]
    assert relP(Pa[np.ix_(keep(Pa.shape[0]), keep(Pa.shape[0]))], ref["P"]) < S.TOL_P and _bits(Pb, Pa)
    ta = _tables_after(scA, scA.cams, [a["dx"][l] for l in acc])
    tb = _tables_after(scB, scB.cams, [b["dx"][l] for l in acc])
    t0 = _tables_after(scA, scA.cams, [])
    assert np.abs(gen_a - ta).max() < 1e-9 and np.abs(cal_a - ta[0]).max() < 1e-9
    assert np.abs(gen_b - tb).max() < 1e-9 and np.abs(cal_b - tb[0]).max() < 1e-9
    assert _bits(gen_b[[0, 3, 1, 2]], gen_a) and _bits(cal_b, cal_a)
    assert (np.abs(ta - t0).max(axis=1) > 1e-9).all()  # (every table did move, the unused cameras' too)


def test_slam_delayed_init_planes_slots(hiplib):
    """ovp_slam_delayed_init_planes through the general rows (k_dinit_rows_gen_pl and its commit) on the stereo scene of
    test_dinit_planes_gpu extended to four cameras, in both slot orders: statuses (all three occur), ids, chi2, corrections and
    covariance equal bit for bit (module docstring; the same host layout as the delayed init without planes), the straight order
    within that test's bounds of its sequential reference on the two-camera columns; camera tables as in
    test_slam_delayed_init_general_slots, and the plane table the same bits in both orders."""
    from tests import dinit_planes_ref as D
    from tests import test_dinit_planes_gpu as T

    capi = hiplib
    sc0 = D.stereo_scene()
    ref = D.delayed_init_planes_reference(sc0)
    assert set(int(s) for s in ref["status"]) == {0, 1, 2}
    scA = mc.add_cameras(sc0, 4)
    scB = mc.slots_rotated(scA)
    outs = []
    for sc in (scA, scB):
        ctx = T.new_context(capi, sc)
        out = T.run(capi, ctx, sc)
        outs.append((out, ctx.cov_download(), ctx.camera_tables_download(4), ctx.plane_table_download(sc.cp.shape[0])))
        ctx.close()
    (a, Pa, (cal_a, gen_a), pl_a), (b, Pb, (cal_b, gen_b), pl_b) = outs
    N0, NA = sc0.N, scA.N
    keep = lambda n: np.r_[np.arange(N0), np.arange(NA, n)]
    assert np.array_equal(a["status"], ref["status"]) and np.array_equal(b["status"], a["status"])
    assert np.array_equal(a["new_id"], np.where(ref["ok"], ref["new_id"] + (NA - N0), -1)) and np.array_equal(b["new_id"], a["new_id"])
    cs = max(1.0, np.abs(ref["chi2"]).max())
    assert np.abs(a["chi2"] - ref["chi2"]).max() <= 1e-6 * cs and _bits(b["chi2"], a["chi2"])
    acc = np.where(ref["ok"])[0]
    assert np.abs(a["delta_init"][acc] - ref["delta_init"][acc]).max() < D.TOL_DX
    assert _bits(b["delta_init"], a["delta_init"])
    for l in acc:
        n = len(ref["dx"][l]) + (NA - N0)
        assert np.abs(a["dx"][l][:n][keep(n)] - ref["dx"][l]).max() < D.TOL_DX, l
    assert _bits(b["dx"], a["dx"]) and np.abs(a["dx"][~ref["ok"]]).max() == 0.0
    assert Pa.shape[0] == ref["P"].shape[0] + (NA - N0) == Pb.shape[0]
    assert D.relP(Pa[np.ix_(keep(Pa.shape[0]), keep(Pa.shape[0]))], ref["P"]) < D.TOL_P and _bits(Pb, Pa)
    ta = _tables_after(scA, scA.cams, [a["dx"][l] for l in acc])
    tb = _tables_after(scB, scB.cams, [b["dx"][l] for l in acc])
    assert np.abs(gen_a - ta).max() < 1e-9 and np.abs(cal_a - ta[0]).max() < 1e-9
    assert np.abs(gen_b - tb).max() < 1e-9 and np.abs(cal_b - tb[0]).max() < 1e-9
    assert _bits(gen_b[[0, 3, 1, 2]], gen_a) and _bits(cal_b, cal_a)
    assert (np.abs(ta - _tables_after(scA, scA.cams, [])).max(axis=1) > 1e-9).all()
    assert _bits(pl_b[0], pl_a[0]) and _bits(pl_b[2], pl_a[2])


def test_plane_loop_general_slots(hiplib):
    """ovp_msckf_plane_update_general (k_plane_feat_gen, k_plane_gen_commit) on the two-plane stereo scene of
    test_general_planes_gpu.test_second_camera_two_plane_sequence extended to four cameras, both planes accepted, in both slot
    orders: decisions, rows and consumed features identical, per-plane dx and P within that test's bounds (its TOL_DX / TOL_P) of
    each other and of the sequential numpy reference on the two-camera columns, chi2 within 1e-6 of the largest; the tables of every
    uploaded camera after the commits are the upload moved by their own columns of the returned corrections, and slot 3 of the
    rotated order is slot 1 of the straight one.  No bit equality here: the loop's column order follows the slots (module docstring)."""
    from ov_plane_amd.synth import make_stereo_plane_scene
    from tests import general_planes_ref as R
    from tests.test_general_planes_gpu import TOL_DX as G_TOL_DX, TOL_P as G_TOL_P

    capi = hiplib
    sc0 = make_stereo_plane_scene(C=8, n_planes=2, feats_per_plane=10, n_free=4, seed=3, planes_in_state_frac=0.5, chi2_mult=1.0)
    force = np.array([1, 1], dtype=np.uint8)
    npr = R.plane_loop_ref(sc0, force=force)
    scA = mc.add_cameras(sc0, 4)
    scB = mc.slots_rotated(scA)
    a, b = (R.run_general(capi, sc, force=force) for sc in (scA, scB))
    tabs = [o["ctx"].camera_tables_download(4) for o in (a, b)]
    a["ctx"].close()
    b["ctx"].close()
    N0 = sc0.N
    assert np.array_equal(a["gen"], b["gen"]) and (sc0.plane_id[a["gen"]] > 0).sum() >= 4 and len(a["batch"]) > 0
    for o in (a, b):
        assert o["ok"].all() and (o["dof"] == npr["plane_rows"]).all() and (o["used_all"] == npr["used"]).all()
    assert np.abs(a["dx"][:, :N0] - npr["dx"]).max() < G_TOL_DX and R.relP(a["P"][:N0, :N0], npr["P"]) < G_TOL_P
    assert np.abs(b["dx"] - a["dx"]).max() < G_TOL_DX and R.relP(b["P"], a["P"]) < G_TOL_P
    assert np.abs(b["chi2"] - a["chi2"]).max() <= 1e-6 * max(1.0, np.abs(a["chi2"]).max())
    (cal_a, gen_a), (cal_b, gen_b) = tabs
    ta = _tables_after(scA, scA.cams, list(a["dx"]))
    tb = _tables_after(scB, scB.cams, list(b["dx"]))
    assert np.abs(gen_a - ta).max() < G_TOL_DX and np.abs(gen_b - tb).max() < G_TOL_DX
    assert np.abs(gen_b[[0, 3, 1, 2]] - gen_a).max() < G_TOL_DX
    assert (np.abs(ta - _tables_after(scA, scA.cams, [])).max(axis=1) > 1e-9).all()


def test_plane_init_general_slots(hiplib):
    """ovp_plane_init_general on the stereo scene of test_plane_init_general_gpu.test_second_camera extended to four cameras, in
    both slot orders: decisions, new ids, rows and consumed features identical, the state, closest points and covariance within
    that test's bounds (its TOL_DX / TOL_P) of each other and of the numpy reference on the two-camera columns and the new planes;
    camera tables as in test_plane_loop_general_slots.  No bit equality, for the plane loop's reason (module docstring)."""
    from ov_plane_amd.synth import make_stereo_plane_scene
    from tests import general_planes_ref as R
    from tests import plane_init_general_ref as I
    from tests.test_plane_init_general_gpu import TOL_DX as I_TOL_DX, TOL_P as I_TOL_P

    capi = hiplib
    sc0 = make_stereo_plane_scene(C=8, n_planes=2, feats_per_plane=10, planes_in_state_frac=0.0)
    npr = I.plane_init_ref(sc0, 5.0, 1e9)
    assert npr["plane_ok"].all()
    scA = mc.add_cameras(sc0, 4)
    scB = mc.slots_rotated(scA)
    a, b = (I.run_init_general(capi, sc) for sc in (scA, scB))
    tabs = [o["ctx"].camera_tables_download(4) for o in (a, b)]
    a["ctx"].close()
    b["ctx"].close()
    N0, NA = sc0.N, scA.N
    n = a["P"].shape[0]
    keep = np.r_[np.arange(N0), np.arange(NA, n)]
    for o in (a, b):
        assert (o["ok"] == npr["plane_ok"]).all() and (o["new_ids"] == npr["new_id"] + (NA - N0)).all()
        assert (o["dof"] == npr["plane_dof"]).all() and (o["used_all"] == npr["used"]).all()
    assert I.state_err(a["state"], npr["state"]) < I_TOL_DX and np.abs(a["cp_end"] - npr["cp"]).max() < I_TOL_DX
    assert n == npr["P"].shape[0] + (NA - N0) == b["P"].shape[0] and R.relP(a["P"][np.ix_(keep, keep)], npr["P"]) < I_TOL_P
    assert I.state_err(b["state"], a["state"]) < I_TOL_DX and np.abs(b["cp_end"] - a["cp_end"]).max() < I_TOL_DX
    assert np.abs(b["dx"] - a["dx"]).max() < I_TOL_DX and R.relP(b["P"], a["P"]) < I_TOL_P
    (cal_a, gen_a), (cal_b, gen_b) = tabs
    ta = _tables_after(scA, scA.cams, [a["dx"][k] for k in range(2)])
    tb = _tables_after(scB, scB.cams, [b["dx"][k] for k in range(2)])
    assert np.abs(gen_a - ta).max() < I_TOL_DX and np.abs(gen_b - tb).max() < I_TOL_DX
    assert np.abs(gen_b[[0, 3, 1, 2]] - gen_a).max() < I_TOL_DX
    assert (np.abs(ta - _tables_after(scA, scA.cams, [])).max(axis=1) > 1e-9).all()


def test_plane_fit_refine_slots(hiplib, oracle):
    """ovp_plane_fit_refine (k_planefit_poses) on a frame of synth.make_plane_frontend_scene as tests/test_plane_frontend_gpu.py
    builds them (a free plane with outliers, an in-state plane with SLAM constants, a plane that only camera 1's tracks can fit, a
    scatter the RANSAC refuses, a plane of three features), extended to four cameras, in both slot orders.  The pose table of
    all four slots against numpy at that file's 16 eps; slot 3 of the rotated order is slot 1 of the straight one and every
    output of the two orders is equal bit for bit (module docstring: k_planefit_poses computes pair (clone, cam) by one thread from
    cam_cal + 20 * cam, k_planefit_link copies an item's pose from poses[clone][cam], and the item lists follow the features'
    observation order); flags, kept sets and iteration counts equal to the oracle chain's and abcd / cp / p_FinG within that file's
    TOL of it, the chain reading the poses of slots 0 and 1."""
    from ov_plane_amd.synth import make_plane_frontend_scene
    from tests import plane_frontend_ref as PF
    from tests.test_plane_frontend_gpu import EPS, TOL

    sc0 = make_plane_frontend_scene(C=8, seed=1, planes=[
        dict(n=14, outliers=2, stereo=5), dict(n=10, kind="fixed", n_slam=2, stereo=3), dict(n=12, cam1only=8, short=4),
        dict(n=12, kind="scatter"), dict(n=3)])
    scA = mc.add_cameras(sc0, 4)
    scB = mc.slots_rotated(scA)
    assert (scA.cam_idx == 1).sum() >= 100 and (scB.cam_idx == 3).sum() == (scA.cam_idx == 1).sum() and not (scB.cam_idx == 1).any()
    outs = []
    for sc in (scA, scB):
        ctx = hiplib.Context(sc.N, sc.C, 4)
        ctx.state_upload(sc)
        ctx.cameras_upload(sc)
        outs.append(ctx.plane_fit_refine(**PF.fused_args(sc, n_cams=4)))
        ctx.close()
    a, b = outs
    for sc, o in ((scA, a), (scB, b)):
        ref_T = PF.pose_table(sc)
        assert o["poses"].shape == ref_T.shape == (sc.C, 4, 12)
        eR = np.abs(o["poses"][:, :, :9] - ref_T[:, :, :9]).max()
        eP = (np.abs(o["poses"][:, :, 9:] - ref_T[:, :, 9:]) / np.maximum(1.0, np.abs(ref_T[:, :, 9:]))).max()
        assert eR <= 16 * EPS and eP <= 16 * EPS, (eR, eP)
    # every slot holds another camera: a read from the wrong one is centimetres off, not a rounding difference
    Ta = a["poses"]
    assert min(np.abs(Ta[:, i, 9:] - Ta[:, j, 9:]).max() for i in range(4) for j in range(i)) > 0.05
    assert _bits(b["poses"][:, [0, 3, 1, 2]], Ta)
    for k in ("fit_ok", "abcd", "inlier", "ok", "iterations", "kept", "cp", "p_FinG"):
        assert _bits(b[k], a[k]), k
    ref = PF.chain(sc0, Ta[:, :2], oracle.plane_fitting, oracle.optimize_plane)
    assert list(ref["fit_ok"]) == [True, True, True, False, False] and ref["ok"][:3].all() and not ref["ok"][3:].any()
    lo, hi = int(sc0.feat_start[2]), int(sc0.feat_start[3])
    assert (ref["kept"][lo:hi] & sc0.sees_cam1[lo:hi]).sum() >= 6 and (ref["inlier"] & ~ref["kept"]).any()
    for k in ("fit_ok", "inlier", "ok", "iterations", "kept"):
        assert (a[k] == ref[k]).all(), k
    e = [float(np.abs(a[k] - ref[k]).max()) for k in ("abcd", "cp", "p_FinG")]
    print("plane fit and refinement over four slots: abcd / cp / p_FinG err against the oracle chain", e)
    assert max(e) < TOL


def test_active_tracks_slots(hiplib):
    """ovp_active_tracks_update on the two-camera scene of test_active_tracks_gpu.test_two_cameras with four camera poses per
    frame: as [c0, c1, c2, c3], and as [c0, c2, c3, c1] with camera 1's observations relabelled 3.  Who has a position and who
    has a uvd is identical in both orders and equal to the restatement's; positions and uvd of the two orders equal bit for bit
    (module docstring: the kernel reads an observation's pose at poses + 12 * o_cam[o] and sums a track's observations in the order
    of the input list, which the relabelling leaves alone) and within that test's 1e-9 (relative) of the restatement, every frame."""
    from tests import test_active_tracks_gpu as T

    ref = T.ref
    extra = {2: (ref._rot([1.0, 0.3, -0.2], 0.21), np.array([0.02, 0.09, -0.03])),
             3: (ref._rot([-0.4, 1.0, 0.5], -0.17) @ ref.CALIB[0][0], np.array([0.07, -0.06, 0.04]))}
    calib_a = {0: ref.CALIB[0], 1: ref.CALIB[1], 2: extra[2], 3: extra[3]}
    calib_b = {0: ref.CALIB[0], 1: extra[2], 2: extra[3], 3: ref.CALIB[1]}
    frames_a, frames_b = ref.stereo_scene(), ref.stereo_scene()
    for fr in frames_a:
        fr["calib"] = calib_a
    for fr in frames_b:
        fr["calib"] = calib_b
        fr["cams"] = [(3 if c == 1 else c, ids, uv, uvn) for c, ids, uv, uvn in fr["cams"]]
    expect, _ = ref.run_reference(ref.stereo_scene())
    exp_b, _ = ref.run_reference(frames_b)
    outs = []
    for frames in (frames_a, frames_b):
        ctx = hiplib.Context(64, 4, 8)
        at = hiplib.ActiveTracks(ctx)
        res = []
        for fr in frames:
            args = T._args(fr, {})
            poses = [ref.cam_pose(fr, c) for c in range(4)]
            args.update(R_GtoC=np.array([p[0] for p in poses]), p_CinG=np.array([p[1] for p in poses]))
            res.append(at.update(**args))
        at.close()
        ctx.close()
        outs.append(res)
    for k, (oa, ob, e, eb) in enumerate(zip(outs[0], outs[1], expect, exp_b)):
        assert sorted(oa["posinG"]) == sorted(ob["posinG"]) == sorted(e["posinG"]) == sorted(eb["posinG"]), k
        assert sorted(oa["uvd"]) == sorted(ob["uvd"]) == sorted(e["uvd"]) == sorted(eb["uvd"]), k
        assert list(oa["ids"]) == list(ob["ids"]) and np.array_equal(oa["flags"], ob["flags"]) and oa["n_feats"] == ob["n_feats"]
        for key in ("posinG", "uvd"):
            order = sorted(e[key])
            T._close([oa[key][f] for f in order], [e[key][f] for f in order], "frame %d %s, straight order" % (k, key))
            assert _bits([np.asarray(ob[key][f]) for f in order], [np.asarray(oa[key][f]) for f in order]), (k, key)
    assert len(expect[-1]["posinG"]) == 24 and all(f not in expect[-1]["uvd"] for f in range(8, 16))


# ---- bounds --------------------------------------------------------------------------------------------------------------------
# e_dev of the first MI355X run of test_general_pair_and_chi2_against_long_double (the rule and the ceilings are
# tests/test_precision_gpu.py's).  Read with them:
#  - A and b sit at the double Givens pair's own error (1e-15, ratio 1..4 for A, 4..20 for b): k_feat_gen's projector and k_gen_pair's
#    plain sums lose nothing the batch path's Gram does (A there: 1e-12..1e-9).  The two views in one clone (dof 1) and the
#    64-view feature (128 rows) are no worse than the rest.
#  - chi2 is 9..21 times the dense double restatement's error in every case (2e-14..7e-14 against 1e-15..4e-15): the bordered
#    Cholesky of the full 2m x 2m M = Pi B Pi + I against a solve on the 2m - 3 projected rows.  Four decades under the ceiling.
OBSERVED = {
    "K3 chi2": 7.3e-14, "K3 A": 1.3e-15, "K3 b": 2.7e-15,
    "K4_m64 chi2": 2.7e-14, "K4_m64 A": 2.2e-15, "K4_m64 b": 2.0e-15,
    "K4_pair_in_one_clone chi2": 1.9e-14, "K4_pair_in_one_clone A": 2.8e-15, "K4_pair_in_one_clone b": 3.1e-15,
    "K4_mixed_lens chi2": 2.6e-14, "K4_mixed_lens A": 2.1e-15, "K4_mixed_lens b": 1.8e-15,
    "K4_pose_only chi2": 2.1e-14, "K4_pose_only A": 1.2e-15, "K4_pose_only b": 3.0e-15,
    "K4_intr_only chi2": 2.0e-14, "K4_intr_only A": 2.0e-15, "K4_intr_only b": 4.1e-15,
    "K4_nofej_reject chi2": 4.3e-14, "K4_nofej_reject A": 1.5e-15, "K4_nofej_reject b": 2.8e-15,
}
