"""ovp_slam_delayed_init_planes on the device (csrc/k_dinit.hip k_dinit_rows_pl / k_dinit_rows_gen_pl, csrc/k_init.hip k_init_*_sk):
delayed initialisation of candidates that lie on planes of the state, the fallback without the plane decided on the device, the
planes' closest points committed between candidates.  The reference is the sequential numpy restatement of
tests/dinit_planes_ref.py; tolerances are the project's (dx 1e-6, normalised dP 1e-4, decisions identical)."""
import numpy as np
import pytest

from ov_plane_amd.synth import make_dinit_plane_scene, quat_boxplus
from tests.dinit_planes_ref import (TOL_DX, TOL_P, cam_table, delayed_init_planes_reference, mono_scene, plane_call_args, relP,
                                    stereo_scene)


def new_context(capi, sc, cap=None):
    ctx = capi.Context(sc.N + 3 * sc.F if cap is None else cap, sc.C, sc.F)
    ctx.cov_upload(sc.P)
    ctx.state_upload(sc)
    if "cam1" in sc:
        ctx.cameras_upload(sc)
    return ctx


def run(capi, ctx, sc, with_planes=True, **over):
    kw = plane_call_args(sc, with_planes)
    kw.update(over)
    return ctx.slam_delayed_init_planes(capi.opts_from_scene(sc), sc.uv, sc.clone_idx, sc.n_meas, sc.p_FinG, **kw)


def check_against(out, ref, ctx):
    assert np.array_equal(out["status"], ref["status"]), (out["status"], ref["status"])
    assert np.array_equal(out["new_id"], ref["new_id"])
    acc = np.where(ref["ok"])[0]
    assert np.abs(out["chi2"] - ref["chi2"]).max() <= 1e-6 * max(1.0, np.abs(ref["chi2"]).max())
    assert np.abs(out["delta_init"][acc] - ref["delta_init"][acc]).max() < TOL_DX
    for l in acc:
        n = len(ref["dx"][l])
        assert np.abs(out["dx"][l][:n] - ref["dx"][l]).max() < TOL_DX, l
    assert np.abs(out["dx"][~ref["ok"]]).max() == 0.0
    assert ctx.cov_size() == ref["P"].shape[0]
    assert relP(ctx.cov_download(), ref["P"]) < TOL_P


@pytest.mark.gpu
@pytest.mark.parametrize("do_fej", [True, False], ids=["fej", "nofej"])
def test_mono_plane_candidates_match_the_sequential_reference(hiplib, do_fej):
    """C = 11, 16 candidates on 3 in-state planes through camera 0's rows, calibration estimated: statuses (all three occur), ids,
    H_L^-1 res_init, every accepted correction, the final covariance and its size."""
    capi = hiplib
    sc = mono_scene(do_fej=do_fej)
    ref = delayed_init_planes_reference(sc)
    assert set(int(s) for s in ref["status"]) == {0, 1, 2}
    ctx = new_context(capi, sc)
    out = run(capi, ctx, sc)
    check_against(out, ref, ctx)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("do_fej", [True, False], ids=["fej", "nofej"])
def test_stereo_plane_candidates_match_the_sequential_reference(hiplib, do_fej):
    """The same through the general rows: a two-camera state, stereo tracks of up to 22 views, two candidates seen by camera 1 only."""
    capi = hiplib
    sc = stereo_scene(do_fej=do_fej)
    ref = delayed_init_planes_reference(sc)
    assert set(int(s) for s in ref["status"]) == {0, 1, 2}
    ctx = new_context(capi, sc)
    out = run(capi, ctx, sc)
    check_against(out, ref, ctx)
    ctx.close()


@pytest.mark.gpu
def test_commit_leaves_the_tables_the_caller_gets_from_the_returned_dx(hiplib):
    """After the call the device pose tables, camera tables and the plane table equal Type::update of the returned corrections in
    order (1e-9); at least one plane's closest point moved."""
    capi = hiplib
    sc = stereo_scene()
    ctx = new_context(capi, sc)
    out = run(capi, ctx, sc)
    cq, cpos, q0, p0, i0 = sc.clone_q.copy(), sc.clone_p.copy(), sc.calib_q.copy(), sc.calib_p.copy(), sc.intr.copy()
    c1, cp, ids = dict(sc.cam1), np.array(sc.cp, dtype=np.float64).copy(), sc.ids
    for l in np.where(out["ok"])[0]:
        dx = out["dx"][l]
        for i in range(sc.C):
            cid = ids["clones"][i]
            cq[i] = quat_boxplus(cq[i], dx[cid:cid + 3])
            cpos[i] = cpos[i] + dx[cid + 3:cid + 6]
        q0, p0, i0 = quat_boxplus(q0, dx[ids["calib"]:ids["calib"] + 3]), p0 + dx[ids["calib"] + 3:ids["calib"] + 6], i0 + dx[ids["intr"]:ids["intr"] + 8]
        c1 = dict(c1, calib_q=quat_boxplus(c1["calib_q"], dx[ids["calib1"]:ids["calib1"] + 3]),
                  calib_p=c1["calib_p"] + dx[ids["calib1"] + 3:ids["calib1"] + 6], intr=c1["intr"] + dx[ids["intr1"]:ids["intr1"] + 8])
        for k in range(cp.shape[0]):
            pid = int(sc.plane_state_id[k])
            cp[k] = cp[k] + dx[pid:pid + 3]
    dcp, dcpf, did = ctx.plane_table_download(cp.shape[0])
    assert np.array_equal(did, np.asarray(sc.plane_state_id, dtype=np.int64)) and np.array_equal(dcpf, sc.cp_fej)
    assert np.abs(dcp - cp).max() < 1e-9
    assert np.abs(dcp - sc.cp).max(axis=1).max() > 1e-9  # (a plane did move)
    cal, gen = ctx.camera_tables_download(2)
    t0, t1 = cam_table(q0, p0, i0), cam_table(c1["calib_q"], c1["calib_p"], c1["intr"])
    assert np.abs(cal - t0).max() < 1e-9 and np.abs(gen[0] - t0).max() < 1e-9 and np.abs(gen[1] - t1).max() < 1e-9
    # the pose tables: a plane-free candidate enqueued behind the loop is linearised at them - compare through the reference state
    ref = delayed_init_planes_reference(sc)
    assert np.abs(cpos - ref["state"]["clone_p"]).max() < TOL_DX and np.abs(cp - ref["state"]["cp"]).max() < TOL_DX
    ctx.close()


@pytest.mark.gpu
def test_without_planes_the_entry_is_the_old_loop_bit_for_bit(hiplib):
    """plane_of_cand all zero (and planes == NULL): status / chi2 / ids / delta_init / dx and the covariance are bit-identical to
    ovp_slam_delayed_init (camera 0's rows) and ovp_slam_delayed_init_general (general rows) on the same input."""
    capi = hiplib
    for sc, gen in ((mono_scene(), False), (stereo_scene(), True)):
        o = capi.opts_from_scene(sc)
        ctx = new_context(capi, sc)
        if gen:
            a = ctx.slam_delayed_init_general(o, sc.uv, sc.clone_idx, sc.cam_idx, sc.n_meas, sc.p_FinG)
        else:
            a = ctx.slam_delayed_init(o, sc.uv, sc.clone_idx, sc.n_meas, sc.p_FinG)
        Pa = ctx.cov_download()
        ctx.close()
        for variant in ("zero_slots", "null"):
            ctx = new_context(capi, sc)
            if variant == "zero_slots":
                b = run(capi, ctx, sc, plane_of_cand=np.zeros(sc.F, np.int32))
            else:
                b = run(capi, ctx, sc, with_planes=False)
            Pb = ctx.cov_download()
            ctx.close()
            assert np.array_equal(b["status"], a["ok"].astype(np.uint8)) and a["ok"].any() and not a["ok"].all()
            for k in ("chi2", "new_id", "delta_init", "dx"):
                assert np.array_equal(a[k], b[k]), (gen, variant, k)
            assert np.array_equal(Pa, Pb), (gen, variant)


@pytest.mark.gpu
def test_fallback_is_linearised_at_the_point_before_plane_refinement(hiplib):
    """p_FinG of the wrong-plane candidates moved by centimetres (as a refinement towards their plane would), p_FinG_noplane the
    original: their delta_init and dx match the reference that relinearises the second attempt at p_FinG_noplane and do not match
    the one that stays at p_FinG."""
    capi = hiplib
    sc = mono_scene()
    wp = np.arange(sc.wrong_plane)
    p = sc.p_FinG.copy()
    p[wp] += np.array([0.03, -0.02, 0.025])
    sc.update(p_FinG=p)
    assert np.abs(sc.p_FinG[wp] - sc.p_FinG_noplane[wp]).max() > 0.02
    ref = delayed_init_planes_reference(sc)
    other = delayed_init_planes_reference(sc, fallback_at_noplane=False)
    fb = wp[ref["status"][wp] == 2]
    assert len(fb) >= 2 and np.array_equal(ref["status"], other["status"])
    ctx = new_context(capi, sc)
    out = run(capi, ctx, sc)
    check_against(out, ref, ctx)
    ctx.close()
    for l in fb:
        n = len(ref["dx"][l])
        assert np.abs(out["delta_init"][l] - other["delta_init"][l]).max() > TOL_DX
        assert np.abs(out["dx"][l][:n] - other["dx"][l]).max() > TOL_DX


def long_candidate(sc, m):
    """The scene's arrays with candidate 0 stretched to m observations (one per clone, camera 0)."""
    M = max(int(sc.uv.shape[1]), m)
    uv = np.zeros((sc.F, M, 2), np.float32)
    ci = -np.ones((sc.F, M), np.int32)
    uv[:, : sc.uv.shape[1]], ci[:, : sc.uv.shape[1]] = sc.uv, sc.clone_idx
    tr = sc.truth
    from ov_plane_amd.synth import project_all, quat_2_rot

    uvt, _ = project_all(tr["p_f"][:1], tr["R"][:m], tr["p"][:m], quat_2_rot(sc.calib_q), sc.calib_p, sc.intr, False)
    uv[0, :m], ci[0, :m] = uvt[0].astype(np.float32), np.arange(m)
    nm = sc.n_meas.copy()
    nm[0] = m
    return uv, ci, nm


@pytest.mark.gpu
def test_runs_are_bit_identical_and_limits_touch_nothing(hiplib):
    """Two runs give identical bits.  A 28-observation plane candidate gives OVP_E_CAPACITY, every bad argument OVP_E_ARG, each
    with the covariance, its size and the device tables untouched; a 22-observation plane candidate with full calibration passes
    the capacity check (and a 23-observation one does not: the LDS of k_init_core binds)."""
    capi = hiplib
    sc = stereo_scene()
    outs = []
    for _ in range(2):
        ctx = new_context(capi, sc)
        r = run(capi, ctx, sc)
        outs.append((r, ctx.cov_download(), ctx.camera_tables_download(2), ctx.plane_table_download(3)))
        ctx.close()
    (a, Pa, ta, pa), (b, Pb, tb, pb) = outs
    assert a["ok"].any() and np.array_equal(Pa, Pb) and np.array_equal(pa[0], pb[0])
    for k in ("status", "chi2", "new_id", "delta_init", "dx"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(ta[0], tb[0]) and np.array_equal(ta[1], tb[1])

    # limits: a long-track mono scene (C = 30), candidate 0 on plane 1
    sc = make_dinit_plane_scene(C=30, F=4, n_planes=2, seed=1, chi2_mult=2.0)
    o = capi.opts_from_scene(sc)
    ctx = new_context(capi, sc)
    cal0 = ctx.debug_read("cal", (20,))

    def untouched():
        return ctx.cov_size() == sc.N and np.array_equal(ctx.cov_download(), sc.P) and np.array_equal(ctx.debug_read("cal", (20,)), cal0)

    kw = plane_call_args(sc)
    for m, want in ((28, capi.OVP_E_CAPACITY), (23, capi.OVP_E_CAPACITY)):
        uv, ci, nm = long_candidate(sc, m)
        r = ctx.slam_delayed_init_planes(o, uv, ci, nm, sc.p_FinG, raise_on_error=False, **kw)
        assert r["rc"] == want and untouched(), (m, r["rc"])
    bad = []
    poc = sc.plane_id.copy()
    poc[1] = 3
    bad.append(dict(kw, plane_of_cand=poc))
    poc = sc.plane_id.copy()
    poc[2] = -1
    bad.append(dict(kw, plane_of_cand=poc))
    sid = np.asarray(sc.plane_state_id).copy()
    sid[1] = sc.N - 2
    bad.append(dict(kw, plane_state_id=sid))
    sid = np.asarray(sc.plane_state_id).copy()
    sid[0] = -1
    bad.append(dict(kw, plane_state_id=sid))
    cpz = np.array(sc.cp).copy()
    cpz[1] = 0.0
    bad.append(dict(kw, cp=cpz))
    for k in bad:
        r = ctx.slam_delayed_init_planes(o, sc.uv, sc.clone_idx, sc.n_meas, sc.p_FinG, raise_on_error=False, **k)
        assert r["rc"] == capi.OVP_E_ARG and untouched()
    # 22 observations with all 14 calibration columns: inside every limit, the loop runs
    uv, ci, nm = long_candidate(sc, 22)
    r = ctx.slam_delayed_init_planes(o, uv, ci, nm, sc.p_FinG, raise_on_error=False, **kw)
    assert r["rc"] == 0 and ctx.cov_size() == sc.N + 3 * int(r["ok"].sum())
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("make", [mono_scene, stereo_scene], ids=["mono", "stereo"])
def test_host_mirror_keeps_plane_candidates_in_the_device_loop(hiplib, make):
    """UpdaterSLAM::delayed_init on a frame of candidates with planes in the state: with StateOptions::gpu_dinit_planes the whole
    vector takes the device loop (route 5), and the landmarks, _features_SLAM_to_PLANE, state values and covariance agree with the
    option off (the per-candidate host loop, route 4, as before this option existed)."""
    from ov_plane_amd import hostlib

    sc = make()
    wp = np.arange(sc.wrong_plane)
    p = sc.p_FinG.copy()
    p[wp] += np.array([0.03, -0.02, 0.025])  # (the fallback point differs from the first attempt's: both routes must use it)
    sc.update(p_FinG=p)
    gen = make is stereo_scene
    off = hostlib.run_updater(sc, "slam_delayed_init", state_planes=True, general_slam=gen)
    assert off["route"] == hostlib.ROUTE_HOST_LOOP
    on = hostlib.run_updater(sc, "slam_delayed_init", state_planes=True, general_slam=gen, dinit_planes=True)
    assert on["route"] == hostlib.ROUTE_DEVICE_PLANES == 5
    ref = delayed_init_planes_reference(sc)
    F = sc.F
    want = np.where(ref["status"] == 1, sc.plane_id, np.where(sc.plane_id > 0, 0, -1))
    for r in (on, off):
        assert np.array_equal(r["new_id"][:F], ref["new_id"]) and np.array_equal(r["slam_to_plane"][:F], want)
    ok = ref["ok"]
    assert set(int(v) for v in ref["status"]) == {0, 1, 2}
    assert np.abs(on["new_p"][:F][ok] - off["new_p"][:F][ok]).max() < TOL_DX
    lm = np.array([e[1] for e in ref["lm"]])
    assert np.abs(on["new_p"][:F][ok] - lm).max() < TOL_DX
    for k in ("clone_p", "calib_p", "intr", "cp"):
        assert np.abs(on[k] - off[k]).max() < TOL_DX, k
    assert np.abs(on["cp"] - ref["state"]["cp"]).max() < TOL_DX and np.abs(on["cp"] - sc.cp).max() > 1e-9
    assert on["n"] == off["n"] == ref["P"].shape[0] and relP(on["P"], off["P"]) < TOL_P and relP(on["P"], ref["P"]) < TOL_P
