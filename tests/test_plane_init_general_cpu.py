"""CPU tests of the plane initialisation over features of any camera: the sequential numpy reference
(tests/plane_init_general_ref.py) against oracle.plane_init on camera-0 scenes, the information-form tail the device evaluates
against that sequence, the capacity arithmetic and the binding."""
import ctypes as C

import numpy as np
import pytest

from tests import general_planes_ref as R
from tests import plane_init_general_ref as I
from ov_plane_amd.synth import make_scene

TOL_DX = 1e-6   # tests/test_gpu_parity.py
TOL_P = 1e-4

SCENES = [
    dict(C=8, F=80, seed=16, n_planes=2, feats_per_plane=25, planes_in_state_frac=0.0, chi2_mult=1.0, ragged=True),
    dict(C=11, F=140, seed=15, n_planes=3, feats_per_plane=30, planes_in_state_frac=0.0, chi2_mult=1.0),
]


@pytest.fixture(scope="module", params=SCENES, ids=["c8_ragged", "c11"])
def pinned(request, oracle):
    sc = make_scene(**request.param)
    return sc, oracle.plane_init(sc, const_init_multi=5.0, const_init_chi2=1e9), I.plane_init_ref(sc, 5.0, 1e9)


def test_numpy_reference_against_the_oracle(pinned):
    sc, ref, npr = pinned
    assert ref["plane_ok"].all()
    assert (npr["plane_ok"] == ref["plane_ok"]).all() and (npr["plane_dof"] == ref["plane_dof"]).all()
    assert (npr["new_id"] == ref["new_id"]).all() and (npr["used"] == ref["used"]).all()
    e = I.state_err(npr["state"], ref)
    print("state", e, "cp", np.abs(npr["cp"] - ref["cp"]).max(), "relP", R.relP(npr["P"], ref["P"]), "chi2", npr["plane_chi2"],
          ref["plane_chi2"])
    assert e < TOL_DX and np.abs(npr["cp"] - ref["cp"]).max() < TOL_DX
    assert npr["P"].shape == ref["P"].shape and R.relP(npr["P"], ref["P"]) < TOL_P


def test_tail_formulas_equal_the_sequence(pinned):
    """Cross block -P+ Z_k, plane blocks Z_j^T P+ Z_k + delta_jk Ecc_k^-1, d cp_k = Ecc_k^-1 (b_c,k - Ecx_k dx_k) and -Z_j^T dx_k for
    the earlier planes, on the systems the sequence linearised: the sequence's own covariance, closest points and corrections."""
    sc, ref, npr = pinned
    t = I.tail_form(sc, npr)
    print("relP", R.relP(t["P"], npr["P"]), "cp", np.abs(t["cp"] - npr["cp"]).max())
    assert R.relP(t["P"], npr["P"]) < TOL_P and R.relP(t["P"], ref["P"]) < TOL_P
    assert np.abs(t["cp"] - npr["cp"]).max() < TOL_DX and np.abs(t["cp"] - ref["cp"]).max() < TOL_DX
    for k, dx in t["dx"].items():
        assert np.abs(dx - npr["dx"][k][:sc.N]).max() < TOL_DX


def test_capacity_arithmetic():
    assert I.capacity_code(100, 106, 80, 2, 64) is None
    assert I.capacity_code(100, 105, 80, 2, 64) == "capacity"       # n + 3 * planes > n_state_max
    assert I.capacity_code(100, 106, 80, 2, 65) == "capacity"       # a general feature above OVP_GEN_MAX_MEAS
    assert I.capacity_code(300, 306, 287, 2, 10) is None            # a state above 288 columns runs on its involved columns
    assert I.capacity_code(300, 306, 288, 2, 10) == "capacity"
    # 34 clones and two cameras with all 14 calibration columns each: 204 + 28 involved columns
    assert I.capacity_code(260, 266, 6 * 34 + 2 * 14, 2, 34) is None
    from ov_plane_amd import capi
    assert capi.OVP_GEN_MAX_MEAS == I.OVP_GEN_MAX_MEAS


def test_symbol_and_argument_types():
    import os

    from ov_plane_amd import capi

    assert "ovp_plane_init_general" in capi.EXPORTS
    a = capi.lib().ovp_plane_init_general.argtypes
    assert len(a) == 16
    assert a[1] == C.POINTER(capi.UpdateOpts) and a[2] == C.POINTER(capi.PlaneBatch) and a[13] == C.POINTER(capi.GeneralBatch)
    assert a[3] == C.c_double and a[4] == C.c_double and a[6] == C.c_int
    assert callable(capi.Context.plane_init_general)
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(capi.__file__))), "include", "ovplane_hip.h")
    assert "int ovp_plane_init_general(" in open(header).read()


def test_host_mirror_has_the_option():
    from ov_plane_amd.build import build_host

    build_host()
    from ov_plane_amd import hostlib
    import inspect

    assert hostlib.carries_option("general_plane_init")
    assert "general_plane_init" in inspect.signature(hostlib.run_updater).parameters
