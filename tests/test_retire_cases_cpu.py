"""CPU checks around the batched retirement: the two entries are declared and exported, and the merge cases of
tests/retire_ref.py are what the GPU test needs them to be - chosen with the restatement alone, every decision at least 5 % in chi2
and 0.5 degrees in angle from its threshold, and the chain case sensitive to the dependency between its pairs."""
import ctypes as C
import os
import re

import numpy as np

import retire_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_entries_are_declared_exported_and_bound(hiplib):
    txt = open(os.path.join(ROOT, "include", "ovplane_hip.h")).read()
    L = hiplib.lib()
    for name in ("ovp_cov_marginalize_many", "ovp_planes_merge_retire"):
        assert re.search(r"\bint %s\s*\(" % name, txt), name
        assert hasattr(L, name) and name in hiplib.EXPORTS
    assert "ovp_plane_merge_in" in txt
    # ovp_plane_merge_in: int, 2 pointers, int, 2 pointers, 3 doubles, int, 2 pointers (LP64 padding behind each int)
    assert C.sizeof(hiplib.PlaneMergeIn) == 8 + 16 + 8 + 16 + 24 + 8 + 16
    assert hiplib.PlaneMergeIn.cp.offset == 40 and hiplib.PlaneMergeIn.n_retire.offset == 72


def test_cases_sit_clear_of_their_thresholds():
    P = R.small_state()
    assert P.shape == (R.N, R.N) and np.linalg.eigvalsh(P).min() > 0
    for name, kw in R.cases().items():
        ref = R.merge_ref(P, **kw)
        assert ref["accepted"].tolist() == R.EXPECTED[name], name
        for chi2, ang in zip(ref["chi2"], ref["angle_deg"]):
            assert abs(chi2 - ref["chi2_thr"]) >= 0.05 * ref["chi2_thr"], (name, chi2)
            assert abs(ang - kw["deg_max"]) >= 0.5, (name, ang)
    b = R.merge_ref(P, **R.cases()["b_chi2"])
    assert b["chi2"][0] >= 1.1 * b["chi2_thr"] and b["angle_deg"][0] < 0.5          # chi2 alone
    c = R.merge_ref(P, **R.cases()["c_angle"])
    assert c["chi2"][0] < 0.95 * c["chi2_thr"] and c["angle_deg"][0] >= 2.0          # the angle alone


def test_chain_case_fails_on_stale_values():
    """The second pair of the chain must see the first pair's closest point: with the value at entry instead the restatement's own
    answer moves by far more than the GPU test's tolerances."""
    P = R.small_state()
    kw = R.cases()["d_chain"]
    true, stale = R.merge_ref(P, **kw), R.merge_ref(P, stale_cp=True, **kw)
    assert abs(stale["chi2"][1] - true["chi2"][1]) > 1e-6 * true["chi2"][1]
    assert np.abs(stale["dx"][1] - true["dx"][1]).max() > 1e-6 * np.abs(true["dx"][1]).max()
    # ... and its covariance: pair 2 reads what pair 1 wrote
    first_only = R.merge_ref(P, **dict(kw, pairs=kw["pairs"][1:]))
    assert abs(first_only["chi2"][0] - true["chi2"][1]) > 1e-6 * true["chi2"][1]
