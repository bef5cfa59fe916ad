"""CPU checks of ovp_zupt_update (the zero-velocity update's gate and update in one device pass): the compressed form the kernels
compute (tests/zupt_ref.py) equals the oracle's stacked form on standing and moving windows of 1, 2 and 41 intervals, with and
without first-estimate Jacobians; the decisions the GPU tests rely on sit clear of their threshold; the entry is declared, exported
and bound, and the ctypes structs match the header."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import zupt_ref as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_DX, TOL_P = 1e-6, 1e-4


def relP(Pa, Pb):
    d = np.sqrt(np.abs(np.diag(Pb)))
    return float((np.abs(Pa - Pb) / np.outer(d, d)).max())


_IN = ("n_readings", "readings", "imu_id", "R_GtoI", "R_GtoI_jac", "b_g", "b_a", "gravity_mag", "sigma_w", "sigma_a", "sigma_wb",
       "sigma_ab", "zupt_noise_multiplier", "chi2_threshold", "vel_ok", "disparity_passed", "time_kernels")
_OUT = ("accepted", "rows", "chi2", "kernel_ms")
_LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "ovplane_hip.h"
int main(void) {
  printf("%%zu %%zu %%d", sizeof(ovp_zupt_in), sizeof(ovp_zupt_out), OVP_ZUPT_MAX_READINGS);
%s
  printf("\n");
  return 0;
}
""" % "\n".join(['  printf(" %%zu", offsetof(ovp_zupt_in, %s));' % f for f in _IN] +
                ['  printf(" %%zu", offsetof(ovp_zupt_out, %s));' % f for f in _OUT])


def test_entry_is_declared_exported_and_bound(hiplib):
    txt = open(os.path.join(ROOT, "include", "ovplane_hip.h")).read()
    assert re.search(r"\bint ovp_zupt_update\s*\(", txt) and "ovp_zupt_in" in txt and "ovp_zupt_out" in txt
    L = hiplib.lib()
    assert hasattr(L, "ovp_zupt_update") and "ovp_zupt_update" in hiplib.EXPORTS
    assert callable(hiplib.Context.zupt_update)
    assert L.ovp_zupt_update(None, None, None, None, None) == hiplib.OVP_E_ARG


def test_struct_mirrors_match_the_header(hiplib, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(_LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    want = [C.sizeof(hiplib.ZuptIn), C.sizeof(hiplib.ZuptOut), hiplib.OVP_ZUPT_MAX_READINGS]
    want += [getattr(hiplib.ZuptIn, f).offset for f in _IN] + [getattr(hiplib.ZuptOut, f).offset for f in _OUT]
    assert got == want
    assert [f for f, _ in hiplib.ZuptIn._fields_] == list(_IN) and [f for f, _ in hiplib.ZuptOut._fields_] == list(_OUT)


def test_host_mirror_exports_the_option_entries():
    from ov_plane_amd.build import build_host

    build_host()
    from ov_plane_amd import closed_loop, hostlib
    import inspect

    L = hostlib.lib()
    assert hasattr(L, "ovph_run_zupt_opt") and hasattr(L, "ovph_run_zupt") and hasattr(L, "ovph_session_enable_gpu_zupt")
    assert inspect.signature(hostlib.run_zupt).parameters["gpu_zupt"].default is False
    assert inspect.signature(closed_loop.run_session).parameters["gpu_zupt"].default is False
    assert callable(hostlib.Session.enable_gpu_zupt)


@pytest.mark.parametrize("do_fej", [True, False], ids=["fej", "nofej"])
@pytest.mark.parametrize("standing", [True, False], ids=["standing", "moving"])
def test_compressed_form_equals_the_oracles_stacked_form(oracle, hiplib, standing, do_fej):
    """1, 2 and 41 intervals (both ends of every window interpolated, the two-interval one with dt = 0.4 ms and 2.1 ms), with the
    override on so that the moving windows are updated too: chi2, dx and P of the compressed form against ovo_zupt_update."""
    po = dict(Z.PO, do_fej=do_fej)
    scn = Z.scenario(standing)
    x, imu = scn[0], scn[1]
    P, imu_id = Z.states()["c6"]
    R, Rj = Z.rotations(x, do_fej)
    seen = []
    for name, t0, t1 in Z.windows(scn):
        sel = oracle.select_imu_readings(imu, t0, t1)
        seen.append(len(sel) - 1)
        ref = oracle.zupt_update(x, po, P, imu, t0, t1, imu_id=imu_id, disparity_passed=True)
        got = Z.compressed(P, sel, imu_id, R, Rj, x["bg"], x["ba"], po)
        assert ref["accepted"] and got["spd"] and got["rows"] == ref["rows"] == 6 * (len(sel) - 1)
        e_chi2 = abs(got["chi2"] - ref["chi2"]) / max(1.0, ref["chi2"])
        e_dx = float(np.abs(got["dx"] - ref["dx"]).max())
        e_P = relP(got["P"], ref["P"])
        print("%s %s %s: %d intervals, chi2 %.6g, rel |d chi2| %.1e, |d dx| %.1e, normalised |dP| %.1e" % (
            "standing" if standing else "moving", "fej" if do_fej else "nofej", name, len(sel) - 1, ref["chi2"], e_chi2, e_dx, e_P))
        assert e_chi2 < 1e-8 and e_dx < TOL_DX and e_P < TOL_P
        assert np.abs(got["P"] - got["P"].T).max() <= 1e-15 * np.abs(got["P"]).max()
        if name == "two":
            dt = np.diff(sel[:, 0])
            assert dt.max() > 3 * dt.min() > 0
    assert seen == [1, 2, 41]
    if do_fej:  # the Jacobian's rotation matters: the value in its place moves dx by more than the tolerance's noise floor
        sel = oracle.select_imu_readings(imu, scn[2], scn[3])
        a = Z.compressed(P, sel, imu_id, R, Rj, x["bg"], x["ba"], po)
        b = Z.compressed(P, sel, imu_id, R, R, x["bg"], x["ba"], po)
        assert np.abs(a["dx"] - b["dx"]).max() > 1e-12


def test_gpu_cases_sit_clear_of_the_threshold(oracle, hiplib):
    """The decisions the GPU file asserts are not rounding's to make: on every state and window it uses, chi2 is at least 5 % from
    chi2_0.95(6 (n - 1)); standing windows pass, moving ones fail, and the velocity bound separates the two scenarios."""
    q95 = hiplib.lib().ovp_chi2_quantile_095
    for standing in (True, False):
        scn = Z.scenario(standing)
        x, imu = scn[0], scn[1]
        assert (np.linalg.norm(x["v"]) <= Z.MAX_VELOCITY) == standing
        R, Rj = Z.rotations(x, True)
        for sname, (P, imu_id) in Z.states().items():
            for wname, t0, t1 in Z.windows(scn):
                sel = oracle.select_imu_readings(imu, t0, t1)
                got = Z.compressed(P, sel, imu_id, R, Rj, x["bg"], x["ba"], Z.PO)
                thr = q95(got["rows"])
                assert abs(got["chi2"] - thr) > 0.05 * thr, (standing, sname, wname, got["chi2"], thr)
                if wname == "full":
                    assert (got["chi2"] <= thr) == standing, (sname, got["chi2"], thr)
                assert abs(got["chi2"] - Z.stacked_chi2(P, sel, imu_id, R, Rj, x["bg"], x["ba"], Z.PO)) < 1e-8 * max(1.0, got["chi2"])


def test_permuted_state_is_the_same_problem(oracle):
    """The IMU block at column 20: the oracle with imu_id = 20 on the permuted covariance gives the permuted result."""
    scn = Z.scenario(True)
    x, imu, t0, t1 = scn
    P0, _ = Z.states()["c6"]
    P1, imu_id = Z.states()["imu_at_20"]
    assert imu_id == 20 and np.array_equal(P1[20:35, 20:35], P0[:15, :15]) and np.array_equal(P1, P1.T)
    a = oracle.zupt_update(x, Z.PO, P0, imu, t0, t1)
    b = oracle.zupt_update(x, Z.PO, P1, imu, t0, t1, imu_id=20)
    assert a["accepted"] and b["accepted"] and abs(a["chi2"] - b["chi2"]) < 1e-9 * a["chi2"]
    assert np.abs(Z.permuted(a["P"], 20) - b["P"]).max() < 1e-12 * np.abs(a["P"]).max()
