"""ovp_propagate_and_clone on the device against the long-double truth (tests/propagate_ref.py) in the derived bounds of
tests/propagate_cases.py, and the properties of the entry: symmetry, untouched elements, the exact clone, the jitter, the three
separate calls, run-to-run bits, refusals, the kept factor, the negative-diagonal verdict."""
import numpy as np
import pytest

import cov_bookkeeping_cases as B
import propagate_cases as PC
from precision_helpers import context_pool

pytestmark = pytest.mark.gpu
CASES = PC.cases()
RUNS = [(c, cap) for c in CASES for cap in PC.capacities(c["n"], c["clone"])]


@pytest.fixture(scope="module")
def pool(hiplib):
    yield from context_pool(hiplib)


def run(ctx, c, jitter=0.0):
    P, rd = PC.inputs(c)
    ctx.cov_clone_jitter(jitter)
    try:
        ctx.cov_upload(P)
        out = ctx.propagate_and_clone(rd, c["imu_id"], PC.imu_state(), PC.options(c), clone=bool(c["clone"]), dt_id=c["dt_id"])
        return out, ctx.cov_download()
    finally:
        ctx.cov_clone_jitter(0.0)


@pytest.mark.parametrize("c,cap", RUNS, ids=["%s_cap%d" % (c["name"], cap) for c, cap in RUNS])
def test_against_the_truth(pool, c, cap):
    ctx = pool(cap)
    P, rd = PC.inputs(c)
    n, imu = c["n"], c["imu_id"]
    out, Pd = run(ctx, c)
    r = PC.ratios(c, out, Pd)
    print("PROP %s %.3g" % (c["name"], PC.worst(r)), {k: "%.2g" % v for k, v in r.items()})
    assert not out["neg_diag"] and out["n_intervals"] == max(c["readings"] - 1, 0)
    assert out["clone_id"] == (n if c["clone"] else -1)
    assert ctx.cov_size() == n + (6 if c["clone"] else 0) == len(Pd)
    assert np.array_equal(Pd, Pd.T)
    keep = np.ones(len(Pd), bool)
    keep[imu:imu + 15] = False
    keep[n:] = False
    assert np.array_equal(Pd[np.ix_(keep, keep)], P[np.ix_(keep[:n], keep[:n])])
    if c["clone"] and c["dt_id"] < 0:  # the exact copy
        idx = np.concatenate([np.arange(n), imu + np.arange(6)])
        assert np.array_equal(Pd, Pd[:n, :n][np.ix_(idx, idx)])
    assert PC.worst(r) <= 1.0, r


@pytest.mark.parametrize("name", ["n21_r42_last_nodt", "n63_r42"])
def test_jittered_clone(pool, name):
    """with ovp_cov_clone_jitter set the new diagonal is as ovp_cov_clone leaves it: (1 + jitter) x the copied value, then (n63) the
    time-offset term on top - in the bounds of the jittered truth; without dt the rest of the new block is still the exact copy"""
    c = next(c for c in CASES if c["name"] == name)
    jit = 1e-7
    ctx = pool(c["n"] + 6)
    out, Pd = run(ctx, c, jitter=jit)
    r = PC.ratios(c, out, Pd, jitter=jit)
    print("PROP %s_jitter %.3g" % (name, PC.worst(r)))
    assert PC.worst(r) <= 1.0, r
    n, imu = c["n"], c["imu_id"]
    if c["dt_id"] < 0:
        src = Pd[imu:imu + 6, imu:imu + 6]
        new = Pd[n:, n:]
        assert np.array_equal(np.diag(new), np.diag(src) * (1.0 + jit))
        off = ~np.eye(6, dtype=bool)
        assert np.array_equal(new[off], src[off])
        # ... the same bits ovp_cov_clone leaves on the same propagated matrix
        ctx.cov_clone_jitter(jit)
        try:
            ctx.cov_upload(np.ascontiguousarray(Pd[:n, :n]))
            ctx.cov_clone(imu, 6)
            assert np.array_equal(ctx.cov_download(), Pd)
        finally:
            ctx.cov_clone_jitter(0.0)


@pytest.mark.parametrize("name", ["n21_r42_rk1_avg0_fej1", "n21_r42_rk0_avg1_fej0", "n64_r42", "n694_r42"])
def test_three_separate_calls_agree(pool, name):
    """ovp_cov_propagate + ovp_cov_clone + ovp_cov_augment_dt fed with the entry's own Phi, Q, last_w and v: both within one bound of
    the truth, so within two of each other"""
    c = next(c for c in CASES if c["name"] == name)
    ctx = pool(c["n"] + 6)
    P, _ = PC.inputs(c)
    n, imu = c["n"], c["imu_id"]
    out, Pd = run(ctx, c)
    ctx.cov_upload(P)
    assert ctx.cov_propagate(imu, [imu], [15], out["Phi"], out["Q"]) == 0
    ctx.cov_clone(imu, 6)
    if c["dt_id"] >= 0:
        ctx.cov_augment_dt(n, c["dt_id"], np.concatenate([out["last_w"], out["v"]]))
    P3 = ctx.cov_download()
    t, Pt, Bp = PC.truth(c)
    r1, r3 = PC._abs_ratio(Pd, Pt, Bp), PC._abs_ratio(P3, Pt, Bp)
    r13 = PC._abs_ratio(Pd, PC.LD(1) * P3, 2 * Bp)
    print("PROP %s_three_calls entry %.3g three %.3g between %.3g" % (name, r1, r3, r13))
    assert r1 <= 1.0 and r3 <= 1.0 and r13 <= 1.0


def test_two_runs_give_the_same_bits(pool):
    c = next(c for c in CASES if c["name"] == "n694_r4096")
    ctx = pool(700)
    a, Pa = run(ctx, c)
    b, Pb = run(ctx, c)
    for k in ("q", "p", "v", "last_w", "Phi", "Q"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(Pa, Pb)


def test_refusals_leave_everything_as_it_was(hiplib, pool):
    c = next(c for c in CASES if c["name"] == "n21_r42_rk1_avg0_fej1")
    P, rd = PC.inputs(c)
    x, po = PC.imu_state(), PC.options(c)

    def refused(ctx, code, readings=rd, imu_id=0, **kw):
        with pytest.raises(hiplib.OvpError) as e:
            ctx.propagate_and_clone(readings, imu_id, x, po, **kw)
        assert e.value.code == code, (e.value.code, code)
        assert ctx.cov_size() == 21 and np.array_equal(ctx.cov_download(), P)

    ctx = pool(27)
    ctx.cov_upload(P)
    refused(ctx, hiplib.OVP_E_ARG, imu_id=-1)
    refused(ctx, hiplib.OVP_E_ARG, imu_id=7)                      # imu_id + 15 > n
    refused(ctx, hiplib.OVP_E_ARG, dt_id=3)                       # inside the IMU block
    refused(ctx, hiplib.OVP_E_ARG, dt_id=21)                      # >= n
    bad = rd.copy()
    bad[5, 0] = bad[4, 0]
    refused(ctx, hiplib.OVP_E_ARG, readings=bad)                  # a non-increasing time stamp
    many = np.zeros((hiplib.OVP_PROP_MAX_READINGS + 1, 7))
    many[:, 0] = 100.0 + 1e-4 * np.arange(len(many))
    refused(ctx, hiplib.OVP_E_CAPACITY, readings=many)
    refused(ctx, hiplib.OVP_E_ARG, dt_id=-2)                      # below -1
    L = hiplib.lib()
    assert L.ovp_propagate_and_clone(ctx._h, None, None) == hiplib.OVP_E_ARG
    import ctypes as C

    zin, zout = hiplib.PropagateIn(), hiplib.PropagateOut()
    zin.n_readings, zin.readings, zin.imu_id, zin.dt_id, zin.clone = 3, None, 0, -1, 1  # readings announced, none given
    assert L.ovp_propagate_and_clone(ctx._h, C.byref(zin), C.byref(zout)) == hiplib.OVP_E_ARG
    assert L.ovp_propagate_and_clone(None, C.byref(zin), C.byref(zout)) == hiplib.OVP_E_ARG     # no context
    assert ctx.cov_size() == 21 and np.array_equal(ctx.cov_download(), P)
    small = pool(26)                                              # n + 6 > n_max
    small.cov_upload(P)
    refused(small, hiplib.OVP_E_CAPACITY, dt_id=20)
    out = small.propagate_and_clone(rd, 0, x, po, clone=False, dt_id=20)  # ... without the clone it fits
    assert out["clone_id"] == -1 and small.cov_size() == 21
    fresh = hiplib.Context(27, 2, 4)
    try:
        with pytest.raises(hiplib.OvpError) as e:
            fresh.propagate_and_clone(rd, 0, x, po)
        assert e.value.code == hiplib.OVP_E_STATE
    finally:
        fresh.close()


def test_negative_diagonal_verdict(pool):
    c = next(c for c in CASES if c["name"] == "n21_r42_rk1_avg0_fej1")
    P, rd = PC.inputs(c)
    ctx = pool(27)
    bad = P.copy()
    bad[:15, :] = 0.0
    bad[:, :15] = 0.0
    bad[:15, :15] = -1e-3 * np.eye(15)
    ctx.cov_upload(bad)
    out = ctx.propagate_and_clone(rd, 0, PC.imu_state(), PC.options(c), dt_id=20)
    assert out["neg_diag"] and ctx.cov_size() == 27 and out["n_intervals"] == 41 and out["clone_id"] == 21
    out, Pd = run(ctx, c)
    assert not out["neg_diag"] and PC.worst(PC.ratios(c, out, Pd)) <= 1.0


def test_kept_factor_is_dropped(hiplib):
    """The plane loop leaves a factor of the resident covariance for the point update behind it.  The call writes P, so the point
    update must factor the new P: it gives, bit for bit, what a context gives that was handed the call's P by upload."""
    from ov_plane_amd.synth import make_scene

    sc = make_scene(C=8, F=96, seed=11, ragged=True, n_planes=3, feats_per_plane=14, chi2_mult=99999.0)
    c = next(c for c in CASES if c["name"] == "n21_r42_rk1_avg0_fej1")
    _, rd = PC.inputs(c)

    def arm(propagate, upload_P=None, refuse=False):
        ctx = hiplib.Context(sc.N, sc.C, sc.F)
        try:
            ctx.cov_upload(sc.P)
            ctx.state_upload(sc)
            ctx.batch_upload_scene(sc)
            o = hiplib.opts_from_scene(sc)
            ctx.plane_update(o, sc.plane_id, sc.cp, sc.cp_fej, sc.plane_state_id)
            Pp = None
            if refuse:  # a refused call (dt_id inside the IMU block) leaves P and the kept factor as they are
                with pytest.raises(hiplib.OvpError):
                    ctx.propagate_and_clone(rd, 0, PC.imu_state(), PC.options(c), clone=False, dt_id=3)
            if propagate:
                out = ctx.propagate_and_clone(rd, 0, PC.imu_state(), PC.options(c), clone=False, dt_id=-1)
                assert not out["neg_diag"]
                Pp = ctx.cov_download()
            if upload_P is not None:
                ctx.cov_upload(upload_P)
            o.chi2_multiplier = 1.0
            o.skip_plane_used = 1
            res = ctx.msckf_update(o)
            return Pp, res, ctx.cov_download()
        finally:
            ctx.close()

    Pp, out_a, Pa = arm(True)
    _, out_b, Pb = arm(False, upload_P=Pp)
    assert (out_a["accepted"] == out_b["accepted"]).all() and out_a["accepted"].sum() > 0
    assert np.array_equal(out_a["dx"], out_b["dx"]) and np.array_equal(Pa, Pb)
    _, out_c, Pc = arm(False, refuse=True)
    _, out_d, Pd = arm(False)
    assert np.array_equal(out_c["dx"], out_d["dx"]) and np.array_equal(Pc, Pd) and (out_c["accepted"] == out_d["accepted"]).all()


@pytest.fixture(scope="module")
def hostlib(hiplib):
    from ov_plane_amd.build import build_host

    build_host()
    from ov_plane_amd import hostlib

    return hostlib


@pytest.mark.parametrize("mode", [dict(use_rk4=0, do_fej=0, imu_avg=1), dict(use_rk4=1, do_fej=1, imu_avg=0)],
                         ids=["discrete", "rk4"])
def test_host_mirror_with_the_option_on(hostlib, mode):
    """hostlib.run_propagate with StateOptions::gpu_propagate against the truth in the same bounds (the scene of
    test_host_cpp_mirror_propagator: C = 6, the IMU block first, the time offset at column 15), the clone registered at the end of
    the state and at the propagated time, value and first estimate both the propagated mean; with the option off the harness
    still sits in the same bounds."""
    import propagate_ref as PR
    from ov_plane_amd.synth import PROP_OPTS, make_imu_scenario, make_scene
    from oracle import np_ref

    sc = make_scene(C=6, F=4, seed=91)
    x, imu, t0, t1 = make_imu_scenario(7, t_state=100.0, dt_cam=0.1, t_off=0.004)
    po = dict(PROP_OPTS, **mode)
    sel = np_ref.select_imu_readings(imu, t0, t1)
    t = PR.integrate({k: x[k] for k in ("q", "p", "v", "bg", "ba", "q_fej", "p_fej", "v_fej")}, po, sel)
    Pt, Bp = PR.covariance(sc.P, 0, t, True, 15)
    for on in (True, False):
        out = hostlib.run_propagate(sc, x, imu, 100.0, 100.1, 0.004, po, gpu_propagate=on, timing=True)
        b = t["b"]
        r = dict(q=PC._abs_ratio(out["x16"][0:4], t["q"], b["q"]), p=PC._abs_ratio(out["x16"][4:7], t["p"], b["p"]),
                 v=PC._abs_ratio(out["x16"][7:10], t["v"], b["v"]), last_w=PC._abs_ratio(out["last_w"], t["last_w"], b["last_w"]),
                 Phi=PC._abs_ratio(out["Phi"], t["Phi"], b["Phi"]), Q=PC._abs_ratio(out["Q"], t["Q"], b["Q"]),
                 P=PC._abs_ratio(out["P"], Pt, Bp))
        print("PROP host_mirror_%s_option_%s %.3g" % ("rk4" if mode["use_rk4"] else "discrete", "on" if on else "off", PC.worst(r)), r)
        assert PC.worst(r) <= 1.0, r
        assert np.array_equal(out["x16"], out["x16_fej"]) and np.array_equal(out["new_clone"], out["x16"][:7])
        assert np.array_equal(out["x16"][10:], np.concatenate([x["bg"], x["ba"]]))
        assert out["new_clone_id"] == sc.N     # ovph_run_propagate looks the clone up at the propagated time
        if on:
            assert np.array_equal(out["P"], out["P"].T)


def test_session_with_the_option_on_and_off(hostlib):
    """40 frames of the scene of test_filter_session_with_slam_landmarks_planes_and_anchor_changes with 25 landmarks: the same
    clone, landmark and plane counts at every frame, positions within 1e-6 of the option-off arm's own position RMSE."""
    from ov_plane_amd import closed_loop
    from ov_plane_amd.sim import Simulator, synthetic_trajectory

    def run(**kw):
        sim = Simulator(synthetic_trajectory(duration=30.0), num_pts=100, num_pts_plane=100)
        return closed_loop.run_session(sim, n_frames=40, C=11, max_slam=25, **kw)

    off, on = run(), run(gpu_propagate=True)
    e = float(np.linalg.norm(on["traj"][:, 4:7] - off["traj"][:, 4:7], axis=1).max())
    print("PROP session max |d p| %.3g, option-off position RMSE %.3g, ratio %.3g" % (e, off["rmse_pos"], e / off["rmse_pos"]))
    differ = np.nonzero((on["counts"] != off["counts"]).any(axis=1))[0]
    assert differ.size == 0, ("frames whose counts differ", differ.tolist(), on["counts"][differ[:3]], off["counts"][differ[:3]])
    assert off["rmse_pos"] > 0 and e <= 1e-6 * off["rmse_pos"]
