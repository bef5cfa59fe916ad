"""ovp_zupt_update on the GPU (the zero-velocity update's gate and update in one device pass, k_zupt.hip) against
oracle.zupt_update, which selects its own readings - the entry is fed oracle.select_imu_readings of the same window; then the host
mirror's try_update and a session with StateOptions::gpu_zupt on.  Tolerances: the project's (dx 1e-6, P 1e-4 normalised, chi2
1e-8 max(1, chi2)); the differences seen are printed."""
import numpy as np
import pytest

import zupt_ref as Z

pytestmark = pytest.mark.gpu
TOL_DX, TOL_P = 1e-6, 1e-4


def relP(Pa, Pb):
    d = np.sqrt(np.abs(np.diag(Pb)))
    return float((np.abs(Pa - Pb) / np.outer(d, d)).max())


@pytest.fixture(scope="module")
def scenarios():
    return {True: Z.scenario(True), False: Z.scenario(False)}


@pytest.fixture(scope="module")
def ctx(hiplib):
    c = hiplib.Context(96, 4, 8)
    yield c
    c.close()


def call(hiplib, oracle, ctx, P, imu_id, scn, t0, t1, upload=True, readings=None, **over):
    """one ovp_zupt_update on P as the mirror would make it -> (out, covariance behind it)"""
    x, imu = scn[0], scn[1]
    sel = oracle.select_imu_readings(imu, t0, t1) if readings is None else readings
    R, Rj = Z.rotations(x, Z.PO["do_fej"])
    if upload:
        ctx.cov_upload(P)
    kw = dict(noise_mult=Z.NOISE_MULT, vel_ok=bool(np.linalg.norm(x["v"]) <= Z.MAX_VELOCITY), disparity_passed=False)
    kw.update(over)
    thr = hiplib.lib().ovp_chi2_quantile_095(6 * (len(sel) - 1))
    out = ctx.zupt_update(sel, imu_id, R, Rj, x["bg"], x["ba"], Z.PO, thr, **kw)
    return out, ctx.cov_download()


def check(out, Pd, ref, what):
    e_chi2 = abs(out["chi2"] - ref["chi2"]) / max(1.0, ref["chi2"])
    e_dx, e_P = float(np.abs(out["dx"] - ref["dx"]).max()), relP(Pd, ref["P"])
    print("%s: chi2 %.6g, rel |d chi2| %.1e, |d dx| %.1e, normalised |dP| %.1e" % (what, ref["chi2"], e_chi2, e_dx, e_P))
    assert out["accepted"] == ref["accepted"] and out["rows"] == ref["rows"]
    assert e_chi2 < 1e-8 and e_dx < TOL_DX and e_P < TOL_P
    assert np.array_equal(Pd, Pd.T)  # both triangles kept equal


@pytest.mark.parametrize("state,window", [("c6", "one"), ("c6", "two"), ("c6", "full"), ("c2", "full"), ("edge65", "full"),
                                          ("imu_at_20", "full")])
def test_shapes_against_the_oracle(hiplib, oracle, ctx, scenarios, state, window):
    """two readings; three with dt = 0.4 ms and 2.1 ms; a full 400 Hz window; make_scene(C=2); n = 65 (an edge tile); the IMU block
    at column 20.  Standing: accepted, and not a no-op."""
    scn = scenarios[True]
    P, imu_id = Z.states()[state]
    t0, t1 = {n: (a, b) for n, a, b in Z.windows(scn)}[window]
    ref = oracle.zupt_update(scn[0], Z.PO, P, scn[1], t0, t1, imu_id=imu_id)
    out, Pd = call(hiplib, oracle, ctx, P, imu_id, scn, t0, t1)
    assert ref["accepted"] and not out["neg_diag"]
    assert relP(P, ref["P"]) > 100 * TOL_P  # (every one of these updates moves P by far more than the tolerance)
    check(out, Pd, ref, "%s/%s" % (state, window))


def test_decisions(hiplib, oracle, ctx, scenarios):
    P, imu_id = Z.states()["c6"]
    still, moving = scenarios[True], scenarios[False]
    # moving: rejected, nothing touched
    ref = oracle.zupt_update(moving[0], Z.PO, P, moving[1], moving[2], moving[3])
    out, Pd = call(hiplib, oracle, ctx, P, imu_id, moving, moving[2], moving[3])
    assert not ref["accepted"] and not out["accepted"]
    assert abs(out["chi2"] - ref["chi2"]) < 1e-8 * ref["chi2"] and out["rows"] == ref["rows"]
    assert np.array_equal(Pd, P) and not out["dx"].any()
    # moving, but the tracks did not move: accepted whatever chi2 and the velocity say
    ref = oracle.zupt_update(moving[0], Z.PO, P, moving[1], moving[2], moving[3], disparity_passed=True)
    out, Pd = call(hiplib, oracle, ctx, P, imu_id, moving, moving[2], moving[3], disparity_passed=True)
    assert ref["accepted"]
    check(out, Pd, ref, "moving, disparity passed")
    # standing, but the velocity estimate is too large: rejected although chi2 passes
    ref = oracle.zupt_update(still[0], Z.PO, P, still[1], still[2], still[3])
    out, Pd = call(hiplib, oracle, ctx, P, imu_id, still, still[2], still[3], vel_ok=False)
    assert ref["accepted"] and not out["accepted"] and abs(out["chi2"] - ref["chi2"]) < 1e-8 * max(1.0, ref["chi2"])
    assert np.array_equal(Pd, P) and not out["dx"].any()
    xv = dict(still[0], v=np.array([0.0, 0.0, 2 * Z.MAX_VELOCITY]))
    assert not oracle.zupt_update(xv, Z.PO, P, still[1], still[2], still[3])["accepted"]


def test_two_calls_give_the_same_bits(hiplib, oracle, ctx, scenarios):
    scn = scenarios[True]
    P, imu_id = Z.states()["edge65"]
    a, Pa = call(hiplib, oracle, ctx, P, imu_id, scn, scn[2], scn[3])
    b, Pb = call(hiplib, oracle, ctx, P, imu_id, scn, scn[2], scn[3])
    assert a["accepted"] and b["accepted"]
    assert a["chi2"] == b["chi2"] and np.array_equal(a["dx"], b["dx"]) and np.array_equal(Pa, Pb)


def test_error_codes_leave_the_covariance_alone(hiplib, oracle, ctx, scenarios):
    scn = scenarios[True]
    P, imu_id = Z.states()["c6"]
    sel = oracle.select_imu_readings(scn[1], scn[2], scn[3])
    ctx.cov_upload(P)
    twice = sel.copy()
    twice[5, 0] = twice[4, 0]                                  # dt = 0
    back = sel.copy()
    back[[7, 8]] = back[[8, 7]]                                # dt < 0
    many = np.repeat(sel[:1], hiplib.OVP_ZUPT_MAX_READINGS + 1, axis=0)
    many[:, 0] += 1e-3 * np.arange(len(many))
    for readings, iid, code in ((sel[:1], imu_id, hiplib.OVP_E_ARG), (twice, imu_id, hiplib.OVP_E_ARG), (back, imu_id, hiplib.OVP_E_ARG),
                                (sel, len(P) - 14, hiplib.OVP_E_ARG), (sel, -1, hiplib.OVP_E_ARG), (many, imu_id, hiplib.OVP_E_CAPACITY)):
        with pytest.raises(hiplib.OvpError) as e:
            call(hiplib, oracle, ctx, P, iid, scn, None, None, upload=False, readings=readings)
        assert e.value.code == code
        assert np.array_equal(ctx.cov_download(), P)
    # exactly the limit goes through (and the context still works behind the refusals)
    out, _ = call(hiplib, oracle, ctx, P, imu_id, scn, None, None, upload=False, readings=many[:-1], disparity_passed=True)
    assert out["accepted"] and out["rows"] == 6 * (hiplib.OVP_ZUPT_MAX_READINGS - 1)


def test_kept_factor_is_dropped_on_acceptance_and_kept_on_rejection(hiplib, oracle, scenarios):
    """The plane loop leaves a factor of the resident covariance for the point update behind it.  An accepted zero-velocity update
    in between writes P, so the point update must factor the new P: it gives what a context gives that was handed that P by
    upload.  A rejected one touches nothing: the point update gives the bits it gives without the call."""
    from ov_plane_amd.synth import make_scene

    sc = make_scene(C=8, F=96, seed=11, ragged=True, n_planes=3, feats_per_plane=14, chi2_mult=99999.0)
    still, moving = scenarios[True], scenarios[False]

    def arm(zupt_scn, upload_P=None, **over):
        c = hiplib.Context(sc.N, sc.C, sc.F)
        try:
            c.cov_upload(sc.P)
            c.state_upload(sc)
            c.batch_upload_scene(sc)
            o = hiplib.opts_from_scene(sc)
            c.plane_update(o, sc.plane_id, sc.cp, sc.cp_fej, sc.plane_state_id)
            z, Pz = None, None
            if zupt_scn is not None:
                z, Pz = call(hiplib, oracle, c, None, 0, zupt_scn, zupt_scn[2], zupt_scn[3], upload=False, **over)
            if upload_P is not None:
                c.cov_upload(upload_P)
            o.chi2_multiplier = 1.0
            o.skip_plane_used = 1
            out = c.msckf_update(o)
            return z, Pz, out, c.cov_download()
        finally:
            c.close()

    z, Pz, out_a, Pa = arm(still, disparity_passed=True)
    assert z["accepted"]
    _, _, out_b, Pb = arm(None, upload_P=Pz)
    e_dx, e_P = float(np.abs(out_a["dx"] - out_b["dx"]).max()), relP(Pa, Pb)
    print("point update behind an accepted call vs behind an upload of its P: |d dx| %.1e, normalised |dP| %.1e" % (e_dx, e_P))
    assert (out_a["accepted"] == out_b["accepted"]).all() and out_a["accepted"].sum() > 0
    assert e_dx < 1e-9 and e_P < 1e-9  # the same arithmetic on the same bits; a factor of the P before the call is off by ~1e-2
    z, Pz, out_c, Pc = arm(moving)
    _, _, out_d, Pd = arm(None)
    assert not z["accepted"]
    assert np.array_equal(out_c["dx"], out_d["dx"]) and np.array_equal(Pc, Pd) and (out_c["accepted"] == out_d["accepted"]).all()


@pytest.fixture(scope="module")
def hostlib(hiplib):
    from ov_plane_amd.build import build_host

    build_host()
    from ov_plane_amd import hostlib

    return hostlib


@pytest.mark.parametrize("case", ["standing", "moving", "moving_low_disparity", "two_frames"])
def test_host_mirror_try_update_with_the_option_on(hiplib, hostlib, oracle, case):
    """The four cases of test_host_cpp_mirror_updater_zero_velocity (tests/test_gpu_parity.py) with StateOptions::gpu_zupt on:
    the same assertions."""
    from ov_plane_amd.synth import PROP_OPTS, make_imu_scenario, make_scene, quat_boxplus

    sc = make_scene(C=6, F=4, seed=91)
    po = dict(PROP_OPTS)
    t_off, t_state = 0.004, 100.0
    standing = case in ("standing", "two_frames")
    n_cam = 2 if case == "two_frames" else 1
    x, imu, t0, t1 = make_imu_scenario(5, t_state=t_state, t_off=t_off, stationary=standing, n_cam=n_cam)
    stamps = [t_state + 0.1 * (k + 1) for k in range(n_cam)]
    rng = np.random.default_rng(3)
    uv0 = rng.uniform(50, 700, (30, 2)).astype(np.float32)
    shift = 0.2 if case == "moving_low_disparity" else 6.0   # pixels between the two images
    uv1 = (uv0 + shift * np.array([0.6, 0.8])).astype(np.float32)
    out = hostlib.run_zupt(sc, x, imu, t_state, stamps, t_off, po, uv0=uv0, uv1=uv1, gpu_zupt=True)
    disparity_passed = case == "moving_low_disparity"
    ref = oracle.zupt_update(x, po, sc.P, imu, t0, t1, disparity_passed=disparity_passed)
    assert out["accepted"][0] == ref["accepted"] == (case != "moving")
    assert abs(out["chi2"][0] - ref["chi2"]) < 1e-8 * max(1.0, ref["chi2"])
    if not ref["accepted"]:
        assert out["timestamp"] == t_state and np.abs(out["P"] - sc.P).max() < 1e-15 and out["meas_at_t1"] == 30
        return
    dx, P, xr, dt_new = ref["dx"], ref["P"], x, t_off

    def _apply_imu_dx(xa, d):
        return dict(xa, q=quat_boxplus(xa["q"], d[0:3]), p=xa["p"] + d[3:6], v=xa["v"] + d[6:9], bg=xa["bg"] + d[9:12],
                    ba=xa["ba"] + d[12:15])

    xr = _apply_imu_dx(x, dx)
    dt_new = t_off + dx[15]
    if n_cam == 2:
        # second frame: time0 = previous camera time + the PREVIOUS offset, time1 = new camera time + the corrected offset
        ref2 = oracle.zupt_update(xr, po, P, imu, stamps[0] + t_off, stamps[1] + dt_new)
        assert ref2["accepted"] and out["accepted"][1]
        assert abs(out["chi2"][1] - ref2["chi2"]) < 1e-7 * max(1.0, ref2["chi2"])
        xr = _apply_imu_dx(xr, ref2["dx"])
        dt_new += ref2["dx"][15]
        P = ref2["P"]
        assert out["meas_at_t1"] == 0          # cleanup_measurements_exact(last_zupt_state_timestamp)
    else:
        assert out["meas_at_t1"] == 30
    assert out["timestamp"] == stamps[-1]
    x16 = np.concatenate([xr["q"], xr["p"], xr["v"], xr["bg"], xr["ba"]])
    e_x = float(np.abs(out["x16"] - x16).max())
    print("%s: |d x16| %.1e, normalised |dP| %.1e" % (case, e_x, relP(out["P"], P)))
    assert e_x < TOL_DX and abs(out["calib_dt"] - dt_new) < TOL_DX
    assert relP(out["P"], P) < TOL_P


def test_session_standing_start_with_the_option_on_and_off(hostlib):
    """48 frames of the session ZUPT test's scene (the platform stands still for its first seconds, then moves): the same frames
    are zero-velocity frames with StateOptions::gpu_zupt on and off, and the trajectories agree within TOL_DX."""
    from ov_plane_amd import closed_loop
    from ov_plane_amd.sim import Simulator, synthetic_trajectory

    def run(**kw):
        sim = Simulator(synthetic_trajectory(duration=30.0, pause=5.0), num_pts=100, num_pts_plane=100, sim_distance_threshold=-1.0)
        return closed_loop.run_session(sim, n_frames=48, C=11, max_slam=25, zupt={}, **kw)

    off, on = run(), run(gpu_zupt=True)
    z = off["zupt_frames"]
    n_still = int(z.sum())
    print("zero-velocity frames", np.nonzero(z)[0].tolist())
    assert 30 <= n_still < 48 and z[:n_still].all()          # the scene stands, then moves
    assert np.array_equal(on["zupt_frames"], z) and np.array_equal(on["counts"], off["counts"])
    e = float(np.abs(on["traj"] - off["traj"]).max())
    print("max |d x16| over the trajectory %.2e" % e)
    assert e < TOL_DX
