"""The bounds of the propagate-and-clone tests, held against the double-precision reference chain on the CPU, and the boundary of
the new entry (tests/propagate_cases.py has the cases and the derivation, tests/propagate_ref.py the long-double truth)."""
import os
import re

import numpy as np
import pytest

import propagate_cases as PC
import propagate_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = PC.cases()


def oracle_summed(oracle, c):
    """oracle.propagate_summed on a stream that selects exactly the case's readings (one reading appended behind the window, so the
    selection's end-of-period branch takes the last one as it is)"""
    _, rd = PC.inputs(c)
    x = PC.imu_state()
    if len(rd) == 0:
        return dict(q=x["q"], p=x["p"], v=x["v"], last_w=np.zeros(3), Phi=np.eye(15), Q=np.zeros((15, 15)))
    tail = rd[-1].copy()
    tail[0] += 1e-3
    xs = dict(x, bg_fej=x["bg"], ba_fej=x["ba"])
    o = oracle.propagate_summed(xs, PC.options(c), np.vstack([rd, tail]), rd[0, 0], rd[-1, 0])
    assert o["n_sel"] == len(rd), (o["n_sel"], len(rd))
    return dict(q=o["x"]["q"], p=o["x"]["p"], v=o["x"]["v"], last_w=o["last_w"], Phi=o["Phi"], Q=o["Q"])


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_reference_chain_sits_inside_the_bounds(oracle, c):
    got, P = PC.chain(c, oracle_summed(oracle, c))
    r = PC.ratios(c, got, P)
    print("PROP_CPU", c["name"], {k: "%.3g" % v for k, v in r.items()})
    assert PC.worst(r) <= 1.0, r
    t, Pt, Bp = PC.truth(c)
    assert t["n_intervals"] == max(c["readings"] - 1, 0)
    n, imu = c["n"], c["imu_id"]
    keep = np.ones(len(Pt), bool)
    keep[imu:imu + 15] = False
    keep[n:] = False
    assert (Bp[np.ix_(keep, keep)] == 0).all() and (np.asarray(Pt, dtype=np.float64)[np.ix_(keep, keep)] == PC.inputs(c)[0][np.ix_(keep[:n], keep[:n])]).all()


@pytest.mark.parametrize("mutant", PC.MUTANTS)
def test_every_mutant_leaves_the_bounds(mutant):
    """in at least one case with more than one interval"""
    worst = 0.0
    for c in CASES:
        if c["readings"] < 3 or c["readings"] > 100 or not c["clone"] or c["dt_id"] < 0 or c["kind"] != "moving":
            continue
        s = PC.summed_double(c, mutant)
        got, P = PC.chain(c, s, mutant)
        worst = max(worst, PC.worst(PC.ratios(c, got, P)))
        if worst > 1.0:
            break
    assert worst > 1.0, (mutant, worst)
    # ... and the same chain without a fault sits inside
    c = next(c for c in CASES if c["name"] == "n21_r42_rk0_avg1_fej1")
    got, P = PC.chain(c, PC.summed_double(c))
    assert PC.worst(PC.ratios(c, got, P)) <= 1.0


def test_truth_phi_is_the_jacobian_of_its_own_mean_integration():
    """finite differences of the truth's discrete mean integration (JPL left-multiplicative error state) against its F, at the level
    test_oracle_pins.py holds the double restatement to"""
    from ov_plane_amd.synth import quat_boxplus, quat_multiply

    c = next(c for c in CASES if c["name"] == "n21_r3_rk0_avg0_fej0")
    _, rd = PC.inputs(c)
    x, o = PC.imu_state(), PC.options(c)
    f = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    xn, F, _ = PR.predict_and_compute(x, o, rd[1], rd[2])

    def perturb(e):
        y = dict(x)
        y["q"] = quat_boxplus(x["q"], e[0:3])
        y["p"], y["v"], y["bg"], y["ba"] = x["p"] + e[3:6], x["v"] + e[6:9], x["bg"] + e[9:12], x["ba"] + e[12:15]
        return y

    def err(y):
        qi = f(xn["q"]) * np.array([-1, -1, -1, 1.0])
        dq = quat_multiply(f(y["q"]), qi)
        return np.concatenate([2 * dq[:3] / dq[3], f(y["p"] - xn["p"]), f(y["v"] - xn["v"]), f(y["bg"] - xn["bg"]), f(y["ba"] - xn["ba"])])

    eps = 1e-6
    Ffd = np.zeros((15, 15))
    for k in range(15):
        e = np.zeros(15)
        e[k] = eps
        yp, _, _ = PR.predict_and_compute(perturb(e), o, rd[1], rd[2])
        ym, _, _ = PR.predict_and_compute(perturb(-e), o, rd[1], rd[2])
        Ffd[:, k] = (err(yp) - err(ym)) / (2 * eps)
    assert np.abs(f(F) - Ffd).max() < 2e-8


def test_truth_summed_phi_is_the_jacobian_of_the_whole_window():
    """the same finite differences through all 41 intervals of a window (discrete, plain form): the summed Phi of the truth, in the
    order Phi <- F Phi, is the Jacobian of the composed mean integration"""
    from ov_plane_amd.synth import quat_boxplus, quat_multiply

    c = next(c for c in CASES if c["name"] == "n21_r42_rk0_avg0_fej0")
    _, rd = PC.inputs(c)
    x, o = PC.imu_state(), PC.options(c)
    f = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    t0 = PR.integrate(x, o, rd)

    def end(e):
        y = dict(x)
        y["q"] = quat_boxplus(x["q"], e[0:3])
        y["p"], y["v"], y["bg"], y["ba"] = x["p"] + e[3:6], x["v"] + e[6:9], x["bg"] + e[9:12], x["ba"] + e[12:15]
        t = PR.integrate(y, o, rd)
        dq = quat_multiply(f(t["q"]), f(t0["q"]) * np.array([-1, -1, -1, 1.0]))
        return np.concatenate([2 * dq[:3] / dq[3], f(t["p"] - t0["p"]), f(t["v"] - t0["v"]), e[9:12], e[12:15]])

    eps = 1e-6
    Pfd = np.zeros((15, 15))
    for k in range(15):
        e = np.zeros(15)
        e[k] = eps
        Pfd[:, k] = (end(e) - end(-e)) / (2 * eps)
    assert np.abs(f(t0["Phi"]) - Pfd).max() < 2e-8 * max(1.0, np.abs(f(t0["Phi"])).max())


def test_option_and_harness_surface():
    """StateOptions::gpu_propagate exists, is off by default, and is reachable through the harness, hostlib and the session"""
    import inspect

    from ov_plane_amd.build import build_host

    build_host()
    from ov_plane_amd import closed_loop, hostlib

    L = hostlib.lib()
    assert hasattr(L, "ovph_run_propagate_opt") and hasattr(L, "ovph_run_propagate") and hasattr(L, "ovph_session_enable_gpu_propagate")
    assert inspect.signature(hostlib.run_propagate).parameters["gpu_propagate"].default is False
    assert inspect.signature(closed_loop.run_session).parameters["gpu_propagate"].default is False
    assert callable(hostlib.Session.enable_gpu_propagate)
    txt = open(os.path.join(ROOT, "ov_plane_amd", "csrc", "host", "ov_plane_host.h")).read()
    assert re.search(r"bool\s+gpu_propagate\s*=\s*false\s*;", txt)


def test_header_declares_and_library_exports_the_entry(hiplib):
    txt = open(os.path.join(ROOT, "include", "ovplane_hip.h")).read()
    assert re.search(r"int\s+ovp_propagate_and_clone\s*\(\s*ovp_ctx\s*\*", txt)
    assert "OVP_PROP_MAX_READINGS 4096" in txt
    assert hasattr(hiplib.lib(), "ovp_propagate_and_clone") and "ovp_propagate_and_clone" in hiplib.EXPORTS
    assert hiplib.OVP_PROP_MAX_READINGS == 4096
    import ctypes as C

    # the layouts the header gives on LP64: int, pointer, int, 26 doubles ...
    assert C.sizeof(hiplib.PropagateIn) == 8 + 8 + 8 + 8 * 26 + 8 * 5 + 4 * 6
    assert C.sizeof(hiplib.PropagateOut) == 8 * 13 + 4 * 3 + 4 + 8 * 450 + 4 * 4
