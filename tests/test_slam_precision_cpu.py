"""The bounds of tests/slam_precision_cases.py held on the CPU: a plain float64 model of every stage sits at ratio <= 1 on every case,
every fault of the model exceeds 1 on a named case, the statuses are the ones the cases intend, every truth chi2 keeps the gate
margin, and the geometry (H in LDS or in scratch, S-form or information form) is what each case claims."""
import numpy as np
import pytest

import slam_precision_cases as S
import slam_ref as R
from oracle import np_ref

CASES = S.cases()
BY_NAME = {c["name"]: c for c in CASES}


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_float64_model_is_inside_every_bound(c):
    r = S.ratios(c, S.model(c))
    print("SLAMPREC_MODEL", c["name"], " ".join("%s %.3g" % kv for kv in r.items()))
    assert max(r.values()) <= 1.0, r


# fault -> (case, stage) on which it must show
NAMED = {
    "rows_f32": ("m235_cal", "rows"),
    "lm_jac_at_value": ("m235_cal", "rows"),
    "plane_cols_lost": ("planes_outlier_between", "rows"),
    "no_identity_row": ("m123_nocal", "gate"),
    "fallback_all_rows": ("planes_outlier_between", "gate"),
    "chunk_last_col": ("m123_nocal", "gate"),
    "odd_last_col": ("m235_cal", "gate"),
    "m_not_zeroed": ("planes_outlier_between", "M"),
    "row0_plus_1": ("m235_cal", "rows"),
    "info_last_row_lost": ("rows81", "tail"),
}
TURNS_A_STATUS = ("fallback_all_rows",)  # these show as a status that differs from the truth's, in front of every stage


@pytest.mark.parametrize("fault", S.FAULTS)
def test_every_fault_exceeds_its_bound(fault):
    name, stage = NAMED[fault]
    c = BY_NAME[name]
    got = S.model(c, fault)
    if fault in TURNS_A_STATUS:
        assert [int(x) for x in got["status"]] != c["expect"]
        with pytest.raises(S.StatusDiffers):
            S.ratios(c, got)
        return
    r = S.ratios(c, got)
    print("SLAMPREC_FAULT", fault, name, " ".join("%s %.3g" % kv for kv in r.items()))
    assert r[stage] > 1.0, (fault, r)


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_statuses_margins_and_geometry(c):
    sc = S.scene(c)
    tr = S.truth_rows(c)
    gt = S.gate_truth(c, [(np.array(Hv, dtype=np.float64), np.array(rv, dtype=np.float64), None, None) for Hv, rv, _, _ in tr])
    assert [t["status"] for t in gt] == c["expect"]
    for t in gt:
        for chi2, thr in t["compared"]:
            assert abs(float(chi2) / thr - 1.0) > S.MARGIN, (c["name"], float(chi2), thr)
    m_total, gcols, h_in_lds, sform = S.geometry(c, sc)
    assert sform == (c["form"] == "s")
    if "h_in_lds" in c:
        assert h_in_lds == c["h_in_lds"]
    if c["name"] == "rows80":
        assert m_total == 80
    if c["name"] == "rows81":
        assert m_total == 81
    if c["name"] == "m30_h_in_scratch":
        assert m_total <= S.SFORM_ROWS and not S.init_fits(m_total, gcols)  # (the information form by LDS, not by rows)


def test_lds_switch_is_at_29_and_30_observations():
    """14 calibration columns, no plane: 2 m rows, 6 m + 17 columns"""
    assert S.gate_lds(58, 191, 1) <= S.GATE_LDS < S.gate_lds(60, 197, 1)
    assert S.gate_lds(60, 197, 0) <= S.GATE_LDS


def test_restated_rows_agree_with_np_ref():
    """slam_ref on floats against np_ref.feature_jacobian_full where np_ref can state the rows (no first estimate of the
    landmark's own: every scene with do_fej off), inside the rows' bound: radtan, equidistant, the two lenses in one call, and the
    point-on-plane row with the plane in the state.  np_ref associates its products differently (matrices formed, then multiplied):
    this is the check of the doubled count."""
    for name in ("nofej", "fisheye", "planes_outlier_between", "lens_mix"):
        c = dict(BY_NAME[name], name=name + "_nofej")
        sc = type(S.scene(BY_NAME[name]))(S.scene(BY_NAME[name]))
        sc["opts"] = dict(sc.opts, do_fej=False)
        S._SC[c["name"]] = sc
        sid, cp, cpf = S.plane_args(c, sc)
        for f, (Hv, rv, bH, br) in enumerate(S.truth_rows(c)):
            kw = dict(cp=cp[f], cp_fej=cpf[f], plane_state_id=int(sid[f]), planeid=1) if (sid is not None and sid[f] >= 0) else {}
            H_f, H_x, res, order = np_ref.feature_jacobian_full(sc, f, **kw)
            H = np.zeros((len(res), sc.N))
            H[:, np_ref.order_cols(order)] = H_x
            H[:, int(sc.lm_id[f]):int(sc.lm_id[f]) + 3] = H_f
            assert S.B.ratio(H, Hv, bH, -1) <= 1.0 and S.B.ratio(res, rv, br, -1) <= 1.0


def test_error_carrier_counts_a_cancellation_by_its_operands():
    a, b = R.E(1.0) + R.E(2.0 ** -30), R.E(1.0)
    d = a - b
    assert float(d.v) == 2.0 ** -30 and float(d.e) >= 1.0
