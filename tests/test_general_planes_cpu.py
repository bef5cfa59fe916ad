"""CPU tests of the general on-plane path of the plane loop: the new entry is exported, declared and bound, and the sequential
numpy reference the GPU tests use (tests/general_planes_ref.py) is held to ovo_msckf_plane_update on camera-0 scenes with tracks of
more than 32 views - the oracle takes any max_meas - before anything on the GPU is held to it."""
import ctypes
import os
import re

import numpy as np
import pytest

from ov_plane_amd.synth import make_long_plane_scene, make_stereo_plane_scene
from tests import general_planes_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_is_exported_declared_and_bound():
    from ov_plane_amd import capi
    from ov_plane_amd.build import build_lib

    lib = ctypes.CDLL(build_lib())
    assert hasattr(lib, "ovp_msckf_plane_update_general")
    hdr = open(os.path.join(ROOT, "include", "ovplane_hip.h")).read()
    m = re.search(r"int ovp_msckf_plane_update_general\(([^;]*)\);", hdr)
    assert m and "const ovp_general_batch *general" in m.group(1) and "plane_of_gen" in m.group(1) and "gen_used" in m.group(1)
    # the layouts the entry shares with the existing ones are untouched: 7 fields / 11 fields
    assert [f[0] for f in capi.GeneralBatch._fields_] == ["n_feats", "max_meas", "uv", "clone_idx", "cam_idx", "n_meas", "p_FinG"]
    assert len(capi.PlaneBatch._fields_) == 11
    assert hasattr(capi.Context, "plane_update_general")
    assert len(capi.lib().ovp_msckf_plane_update_general.argtypes) == 11
    src = open(os.path.join(ROOT, "ov_plane_amd", "csrc", "k_plane_feat_gen.hip")).read()
    assert "k_plane_feat_gen" in src and "build_plane_row" in src and "build_bearing_row" in src and "atomic" not in src.replace("no atomics", "")


def test_host_mirror_switch_is_exported_and_bound():
    import inspect

    from ov_plane_amd import hostlib
    from ov_plane_amd.build import build_host

    L = ctypes.CDLL(build_lib_host := build_host())
    assert build_lib_host and hostlib.carries_option("general_planes", L)
    assert "general_planes" in inspect.signature(hostlib.run_msckf_update).parameters
    hdr = open(os.path.join(ROOT, "ov_plane_amd", "csrc", "host", "ov_plane_host.h")).read()
    assert re.search(r"bool gpu_general_planes = false;", hdr)


def test_generators_give_long_tracks_and_a_second_camera():
    sc = make_long_plane_scene(C=40, n_planes=4, feats_per_plane=6, n_free=4, seed=1)
    on = sc.plane_id > 0
    assert sc.C >= 40 and ((sc.n_meas > 32) & on).sum() >= 4 and ((sc.n_meas <= 32) & on).sum() >= 4
    batch, gen = R.split_features(sc)
    assert (sc.n_meas[gen] > 32).all() and (sc.n_meas[batch] <= 32).all() and len(batch) + len(gen) == sc.F
    st = make_stereo_plane_scene(C=8, n_planes=2, feats_per_plane=10, n_free=4, seed=3, planes_in_state_frac=0.5)
    batch, gen = R.split_features(st)
    assert set(st.plane_id[gen]) >= {1, 2} and set(st.plane_id[batch]) >= {1, 2}
    assert all(st.cam_idx[f, : st.n_meas[f]].any() for f in gen) and not any(st.cam_idx[f, : st.n_meas[f]].any() for f in batch)


@pytest.mark.parametrize("kw", [
    dict(C=40, n_planes=4, feats_per_plane=6, n_free=4, seed=1, chi2_mult=1.0),    # the oracle accepts three planes, rejects one
    dict(C=40, n_planes=4, feats_per_plane=6, n_free=4, seed=0, chi2_mult=1.0),    # accepts all four
])
def test_numpy_reference_is_pinned_to_the_oracle_on_long_tracks(oracle, kw):
    """Tracks of 33 to 40 views, planes in the state and outside it: the numpy loop under the oracle's decisions reproduces the
    oracle's state and covariance to rounding (both are f64 Givens sweeps of the same systems), the rows of the gate and the
    consumed features exactly."""
    sc = make_long_plane_scene(**kw)
    assert (sc.n_meas[sc.plane_id > 0] > 32).sum() >= 4
    ref = oracle.msckf_plane_update(sc)
    if kw["seed"] == 1:
        assert ref["plane_ok"].any() and (~ref["plane_ok"]).any()
    for use_qr in (False, True):
        mine = R.plane_loop_ref(sc, force=ref["plane_ok"], use_qr=use_qr)
        assert (mine["plane_ok"] == ref["plane_ok"]).all() and (mine["plane_rows"] == ref["plane_rows"]).all()
        assert (mine["used"] == ref["used"]).all()
        assert R.relP(mine["P"], ref["P"]) < 1e-9
        for k in ("clone_q", "clone_p", "calib_q", "calib_p", "intr"):
            assert np.abs(mine["state"][k] - ref[k]).max() < 1e-10, k
        assert np.abs(mine["cp"] - ref["cp"]).max() < 1e-10
    # without the long tracks the loop computes something else: the comparison can tell
    batch, _ = R.split_features(sc)
    short = R.plane_loop_ref(sc, force=ref["plane_ok"], feats=batch, use_qr=True)
    assert R.relP(short["P"], ref["P"]) > 1e-3
