"""oracle/ld_ref.py, the extended-precision truth of tests/test_precision_gpu.py, pinned on its own: exact integer cases, and agreement
with the double-precision restatement (oracle/np_ref.py) to double rounding on synthetic scenes."""
from math import comb

import numpy as np
import pytest

from oracle import ld_ref, np_ref
from ov_plane_amd.synth import make_scene

LD = np.longdouble


def test_long_double_is_extended_precision():
    # the truth is only a truth with a 64-bit mantissa (x87 80-bit); a platform where long double is double must fail here,
    # not make every yardstick of the GPU tests compare double with double
    assert np.finfo(LD).nmant >= 63
    assert np.finfo(LD).eps < 1.1e-19


@pytest.mark.parametrize("n", [1, 4, 9, 14])
def test_pascal_matrix_has_its_exact_factor_and_inverse(n):
    """S_ij = C(i+j, i) = L L^T with L_ij = C(i, j) (lower Pascal), L^-1_ij = (-1)^(i-j) C(i, j): integers that the factorization
    and the solves must reproduce exactly up to n = 14 (entries < 2^63)."""
    L = np.array([[comb(i, j) for j in range(n)] for i in range(n)], dtype=LD)
    Li = np.array([[(-1) ** (i - j) * comb(i, j) if j <= i else 0 for j in range(n)] for i in range(n)], dtype=LD)
    S = np.array([[comb(i + j, i) for j in range(n)] for i in range(n)], dtype=LD)
    assert (ld_ref.chol(S) == L).all()
    assert (ld_ref.solve_lower(L, np.eye(n, dtype=LD)) == Li).all()
    assert (ld_ref.solve_upper(L.T, np.eye(n, dtype=LD)) == Li.T).all()
    if n <= 9:  # S^-1 = L^-T L^-1 has integer entries; the product stays exact while they are small
        assert (ld_ref.inv_spd(S) == Li.T @ Li).all()


def test_unimodular_and_bordered_systems_have_exact_solutions():
    """A unimodular L L^T (integer L, unit diagonal) and a bordered system [[S, c], [c^T, d]] whose solution is rational with a
    power-of-two denominator: both solved exactly, by the Cholesky solves and by the pivoting elimination."""
    rng = np.random.default_rng(3)
    n = 8
    L = np.tril(rng.integers(-3, 4, size=(n, n)), -1) + np.eye(n, dtype=np.int64)
    S = (L @ L.T).astype(LD)
    x = rng.integers(-20, 21, size=n).astype(LD)
    rhs = S @ x
    Lf = ld_ref.chol(S)
    assert (Lf == L.astype(LD)).all()
    assert (ld_ref.solve_upper(Lf.T, ld_ref.solve_lower(Lf, rhs)) == x).all()
    # (the pivoting elimination forms fractions on the way: exact to long-double rounding, not bit for bit)
    assert np.abs(ld_ref.solve(S, rhs) - x).max() <= 1e-15 * np.abs(x).max()
    # bordered: S^-1 is an integer matrix (det S = 1), the Schur complement d - c^T S^-1 c = 4, so the factor is integer with a
    # last pivot of 2 and the solution x with a last entry of 1/4 comes out exactly
    c = rng.integers(-5, 6, size=n).astype(LD)
    Si = ld_ref.inv_spd(S)
    assert (Si == np.round(Si)).all()
    d = c @ Si @ c + 4
    B = np.zeros((n + 1, n + 1), dtype=LD)
    B[:n, :n], B[:n, n], B[n, :n], B[n, n] = S, c, c, d
    xb = np.append(x, LD(0.25))
    Lb = ld_ref.chol(B)
    assert Lb[n, n] == 2 and (Lb == np.round(Lb)).all()
    assert (ld_ref.solve_upper(Lb.T, ld_ref.solve_lower(Lb, B @ xb)) == xb).all()


def test_projector_pair_equals_the_householder_and_the_givens_pair():
    """Hp^T Hp of the Householder basis (the truth's) against the projector identity (feature_pair, no basis at all) and against the
    reference's Givens basis in double (np_ref.nullspace_project_inplace): the pair does not depend on the basis.  Observed
    (relative to max |A_f|): Householder - Givens <= 2.6e-15, projector - Householder <= 3.3e-15 (a two-observation feature,
    where H_f^T H_f is least well conditioned; the projector is the one off there: Givens agrees with Householder)."""
    sc = make_scene(C=9, F=12, seed=5, ragged=True, min_meas=2)
    for f in range(sc.F):
        H_f, H_x, res, _ = np_ref.feature_jacobian_full(sc, f)
        A, b, rr = ld_ref.feature_pair(H_f, H_x, res)
        Hp, rp = ld_ref.nullspace_rows(H_f, H_x, res)
        s = max(float(np.abs(A).max()), 1.0)
        assert np.abs(Hp.T @ Hp - A).max() <= 3e-14 * s
        assert np.abs(Hp.T @ rp - b).max() <= 1e-18 * s * max(1.0, float(np.sqrt(rr)))
        assert abs(rp @ rp - rr) <= 1e-17 * max(1.0, float(rr))
        Hg, rg = np_ref.nullspace_project_inplace(H_f, H_x, res)
        assert Hg.shape[0] == Hp.shape[0] == H_x.shape[0] - 3
        assert np.abs(ld_ref.ld(Hg.T @ Hg) - Hp.T @ Hp).max() <= 2e-14 * s
        assert np.abs(ld_ref.ld(Hg.T @ rg) - Hp.T @ rp).max() <= 1e-14 * s * max(1.0, float(np.sqrt(rr)))


@pytest.mark.parametrize("kw", [
    dict(C=7, F=24, seed=31, chi2_mult=1.0),
    dict(C=5, F=20, seed=32, ragged=True, min_meas=2, chi2_mult=1.0),
    dict(C=6, F=16, seed=33, chi2_mult=1.0, fisheye=True, calib=False),
])
def test_point_update_in_long_double_rounds_to_the_double_restatement(kw):
    """point_pair + update_from_pair on the accepted set of np_ref.msckf_point_update == that update (Givens, compression, S-form
    EKFUpdate in double) to double rounding: chi2 of every feature, dx, P."""
    sc = make_scene(**kw)
    ref = np_ref.msckf_point_update(sc)
    acc = np.where(ref["accepted"])[0]
    assert 0 < len(acc)
    allp = ld_ref.point_pair(sc)
    assert (allp["dof"] == ref["rows"]).all()
    assert ld_ref.err_chi2(ref["chi2"], allp["chi2"]) < 1e-11
    pair = ld_ref.point_pair(sc, feats=acc, with_chi2=False)
    Pp, dx = ld_ref.update_from_pair(sc.P, pair["A"], pair["b"])
    assert ld_ref.err_state(ref["dx"], dx, Pp) < 1e-10
    assert ld_ref.rel_p(ref["P"], Pp) < 1e-11
    # the information form and the form without P^-1 are the same update
    Pi, dxi = ld_ref.update_from_pair_info(sc.P, pair["A"], pair["b"])
    assert ld_ref.rel_p(Pi, Pp) < 1e-15 and ld_ref.err_state(dxi, dx, Pp) < 1e-14
    # ... and the double-precision twin of update_from_pair lands within double rounding of it
    P64, dx64 = ld_ref.update_from_pair(sc.P, np.asarray(pair["A"], dtype=np.float64), np.asarray(pair["b"], dtype=np.float64),
                                        dtype=np.float64)
    assert ld_ref.rel_p(P64, Pp) < 1e-11 and ld_ref.err_state(dx64, dx, Pp) < 1e-10


def test_update_from_pair_on_an_exactly_singular_prior():
    """A clone that is an exact copy of another one (P singular): the form without P^-1 against np_ref's S-form EKFUpdate."""
    sc = make_scene(C=7, F=20, seed=34, chi2_mult=1.0)
    a, b_ = sc.ids["clones"][-2], sc.ids["clones"][-1]
    idx = np.arange(sc.N)
    idx[b_:b_ + 6] = np.arange(a, a + 6)
    sc["P"] = sc.P[np.ix_(idx, idx)]
    sc["clone_q"][-1], sc["clone_p"][-1] = sc["clone_q"][-2], sc["clone_p"][-2]
    sc["clone_q_fej"][-1], sc["clone_p_fej"][-1] = sc["clone_q_fej"][-2], sc["clone_p_fej"][-2]
    with pytest.raises(np.linalg.LinAlgError):
        ld_ref.chol(sc.P)
    ref = np_ref.msckf_point_update(sc)
    pair = ld_ref.point_pair(sc, feats=np.where(ref["accepted"])[0], with_chi2=False)
    Pp, dx = ld_ref.update_from_pair(sc.P, pair["A"], pair["b"])
    assert ld_ref.err_state(ref["dx"], dx, Pp) < 1e-9
    assert ld_ref.rel_p(ref["P"], Pp) < 1e-10


@pytest.mark.parametrize("rows", [1, 2, 9, 40])
def test_dense_ekf_update_rounds_to_the_double_restatement(rows):
    rng = np.random.default_rng(rows)
    sc = make_scene(C=6, F=4, seed=41)
    order = [(int(sc.ids["clones"][1]), 6), (int(sc.ids["calib"]), 6), (0, 3)]
    cols = np_ref.order_cols(order)
    H = rng.standard_normal((rows, len(cols))) * 30.0
    r = rng.standard_normal(rows)
    Pn, dxn = np_ref.ekf_update(sc.P, order, H, r)
    Pt, dxt = ld_ref.ekf_update_dense(sc.P, cols, H, r)
    assert ld_ref.err_state(dxn, dxt, Pt) < 1e-10
    assert ld_ref.rel_p(Pn, Pt) < 1e-10
    # the same measurement as a pair: A = H^T H, b = H^T r scattered into the state columns
    A = np.zeros((sc.N, sc.N), dtype=LD)
    bb = np.zeros(sc.N, dtype=LD)
    A[np.ix_(cols, cols)] = ld_ref.ld(H).T @ ld_ref.ld(H)
    bb[cols] = ld_ref.ld(H).T @ ld_ref.ld(r)
    Pp, dx = ld_ref.update_from_pair(sc.P, A, bb)
    assert ld_ref.rel_p(Pp, Pt) < 1e-15 and ld_ref.err_state(dx, dxt, Pt) < 1e-14


def test_pivot_dropping_update_equals_the_plain_one_on_an_exact_pair():
    """update_from_pair_dropping drops the directions the pair determines only to rounding (the IMU and dt columns no feature
    touches, the unobservable ones); on the long-double pair of an exact-clone scene it is update_from_pair to double rounding."""
    sc = make_scene(C=9, F=40, seed=41, chi2_mult=1.0)
    a, b_ = sc.ids["clones"][-2], sc.ids["clones"][-1]
    idx = np.arange(sc.N)
    idx[b_:b_ + 6] = np.arange(a, a + 6)
    sc["P"] = sc.P[np.ix_(idx, idx)]
    sc["clone_q"][-1], sc["clone_p"][-1] = sc["clone_q"][-2], sc["clone_p"][-2]
    sc["clone_q_fej"][-1], sc["clone_p_fej"][-1] = sc["clone_q_fej"][-2], sc["clone_p_fej"][-2]
    pair = ld_ref.point_pair(sc, with_chi2=False)
    Pt, dxt = ld_ref.update_from_pair(sc.P, pair["A"], pair["b"])
    Pd, dxd, dropped = ld_ref.update_from_pair_dropping(sc.P, pair["A"], pair["b"])
    assert set(range(16)) <= set(dropped)
    assert ld_ref.err_state(dxd, dxt, Pt) < 1e-11 and ld_ref.rel_p(Pd, Pt) < 1e-12


# ---- covariance bookkeeping: the restatements of tests/test_cov_bookkeeping_gpu.py, their bounds, and the mutations the bounds catch ----
import cov_bookkeeping_cases as B  # noqa: E402


def _embed(n, rows, block):
    F = np.eye(n, dtype=LD)
    F[rows, :] = 0
    F[rows, :] = block
    return F


@pytest.mark.parametrize("c", B.prop_cases(), ids=lambda c: c["name"])
def test_propagation_restatement_against_the_double_one_and_F_P_Ft(c):
    """ld_ref.ekf_propagation == np_ref.ekf_propagation to double rounding (inside the derived bound), == F P F^T + Q embedded in
    the state with F the identity whose rows [new_start, new_start + phi) are replaced by Phi scattered to the old columns, and its
    companion is the same computation on absolute values."""
    P, Phi, Q = B.prop_inputs(c)
    old, a, phi, n = B.flat(c["old"]), c["start"], c["phi"], c["n"]
    T, comp = ld_ref.ekf_propagation(P, a, old, Phi, Q)
    assert T.dtype == LD and comp.dtype == LD and (comp >= np.abs(T)).all()
    Pd = np_ref.ekf_propagation(P, a, phi, c["old"], Phi, Q)
    assert B.ratio(Pd, T, comp, B.prop_K(c)) <= 1.0
    touched = np.zeros((n, n), dtype=bool)
    touched[a:a + phi, :] = touched[:, a:a + phi] = True
    assert np.array_equal(np.asarray(T, dtype=np.float64)[~touched], P[~touched])
    # the independent definition: rows of F outside the block are the identity's; a repeated old column adds its Phi columns
    Fb = np.zeros((phi, n), dtype=LD)
    for k, col in enumerate(old):
        Fb[:, col] += ld_ref.ld(Phi[:, k])
    F = _embed(n, slice(a, a + phi), Fb)
    Qe = np.zeros((n, n), dtype=LD)
    Qe[a:a + phi, a:a + phi] = np.triu(ld_ref.ld(Q)) + np.triu(ld_ref.ld(Q), 1).T
    T2 = F @ ld_ref.ld(P) @ F.T + Qe
    assert np.abs(T2 - T).max() == 0 or (np.abs(T2 - T) <= 64 * np.finfo(LD).eps * (len(old) + 2) * comp).all()
    T3, comp3 = ld_ref.ekf_propagation(np.abs(P), a, old, np.abs(Phi), np.abs(Q))
    assert np.array_equal(T3, comp) and np.array_equal(comp3, comp)


@pytest.mark.parametrize("c", B.augment_cases(), ids=lambda c: c["name"])
def test_augment_dt_restatement_is_J_P_Jt(c):
    P, d = B.augment_inputs(c)
    n, p, t = c["n"], c["pose"], c["dt"]
    T, comp = ld_ref.augment_dt(P, p, t, d)
    J = np.eye(n, dtype=LD)
    J[p:p + 6, t] += ld_ref.ld(d)
    T2 = J @ ld_ref.ld(P) @ J.T
    assert (np.abs(T2 - T) <= 64 * np.finfo(LD).eps * comp).all()
    assert (np.abs(T - T.T) <= 64 * np.finfo(LD).eps * comp).all()  # symmetric in, symmetric out (to long-double rounding in the pose block)
    untouched = np.ones((n, n), dtype=bool)
    untouched[p:p + 6, :] = untouched[:, p:p + 6] = False
    assert np.array_equal(np.asarray(T, dtype=np.float64)[untouched], P[untouched])
    Ja = np.eye(n, dtype=LD)
    Ja[p:p + 6, t] += np.abs(ld_ref.ld(d))
    assert (np.abs(Ja @ np.abs(ld_ref.ld(P)) @ Ja.T - comp) <= 64 * np.finfo(LD).eps * comp).all()
    with pytest.raises(AssertionError):
        ld_ref.augment_dt(P, p, p + 2, d)


@pytest.mark.parametrize("c", B.init_cases(), ids=lambda c: c["name"])
def test_initialize_invertible_restatement_is_J_blkdiag_Jt(c):
    """The new variable is x_L = H_L^-1 (r - H_R x - n): its error is -H_L^-1 (H_R dx + n), so the grown covariance is
    J blkdiag(P, R) J^T with J = [[I, 0], [-H_L^-1 H_R (scattered), -H_L^-1]] and R the upper view."""
    P, H_R, H_Linv, R = B.init_inputs(c)
    n, k, cols = c["n"], c["k"], np.asarray(c["cols"])
    T, comp = ld_ref.initialize_invertible(P, cols, H_R, H_Linv, R)
    assert T.shape == (n + k, n + k) and (comp >= np.abs(T)).all()
    Hs = np.zeros((k, n), dtype=LD)
    Hs[:, cols] = ld_ref.ld(H_R)
    Hi = ld_ref.ld(H_Linv)
    J = np.zeros((n + k, n + k), dtype=LD)
    J[:n, :n] = np.eye(n, dtype=LD)
    J[n:, :n] = -Hi @ Hs
    J[n:, n:] = -Hi
    blk = np.zeros((n + k, n + k), dtype=LD)
    blk[:n, :n] = ld_ref.ld(P)
    blk[n:, n:] = np.triu(ld_ref.ld(R)) + np.triu(ld_ref.ld(R), 1).T
    T2 = J @ blk @ J.T
    assert (np.abs(T2 - T) <= 64 * np.finfo(LD).eps * (len(cols) + k) ** 2 * comp).all()
    assert np.array_equal(np.asarray(T[:n, :n], dtype=np.float64), P)


@pytest.mark.parametrize("k", [1, 3])
def test_initialize_invertible_restatement_against_the_oracle(oracle, k):
    """pyoracle.initialize(..., do_update=False) with as many rows as new columns is initialize_invertible behind a Givens rotation
    of the rows, which the appended block does not depend on when R is isotropic."""
    rng = np.random.default_rng(70 + k)
    sc = make_scene(C=4, F=4, seed=71)
    order = [(int(sc.ids["clones"][1]), 6), (int(sc.ids["calib"]), 6)]
    cols = np_ref.order_cols(order)
    H_R = rng.standard_normal((k, len(cols)))
    H_L = rng.standard_normal((k, k)) + 2 * np.eye(k)
    r_iso = 0.7
    ref = oracle.initialize(sc.P, order, H_R, H_L, rng.standard_normal(k), r_iso, 1e9, do_update=False)
    assert ref["P"].shape == (sc.N + k, sc.N + k)
    T, comp = ld_ref.initialize_invertible(sc.P, cols, H_R, np.linalg.inv(H_L), r_iso * np.eye(k))
    assert ld_ref.rel_p(ref["P"], T) < 1e-10


def _all_cases():
    for c in B.prop_cases():
        yield "prop", c
    for c in B.augment_cases():
        yield "augment", c
    for c in B.init_cases():
        yield "init", c


def _model_ratio(kind, c, **mut):
    if kind == "prop":
        P, Phi, Q = B.prop_inputs(c)
        old = B.flat(c["old"])
        T, comp = ld_ref.ekf_propagation(P, c["start"], old, Phi, Q)
        return B.ratio(B.prop_model(P, c["start"], old, Phi, Q, **mut), T, comp, B.prop_K(c))
    if kind == "augment":
        P, d = B.augment_inputs(c)
        T, comp = ld_ref.augment_dt(P, c["pose"], c["dt"], d)
        return B.ratio(B.augment_model(P, c["pose"], c["dt"], d, **mut), T, comp, B.augment_K(c))
    P, H_R, H_Linv, R = B.init_inputs(c)
    T, comp = ld_ref.initialize_invertible(P, c["cols"], H_R, H_Linv, R)
    return B.ratio(B.init_model(P, c["cols"], H_R, H_Linv, R, **mut), T, comp, B.init_K(c))


@pytest.mark.parametrize("kind,c", list(_all_cases()), ids=lambda v: v if isinstance(v, str) else v["name"])
def test_plain_float64_evaluation_stays_inside_the_bound(kind, c):
    """the bound alone rejects nothing correct: numpy in double, whatever order its products sum in"""
    r = _model_ratio(kind, c)
    print("BOOKKEEPING-CPU %s/%s %.3f" % (kind, c["name"], r))
    assert r <= 1.0


def test_jitter_bound_holds_in_float64():
    v = B.spd(40, 9).diagonal()
    T, comp = B.jitter_truth(v, 1e-11)
    assert B.ratio(v * (1.0 + 1e-11), T, comp, B.JITTER_K) <= 1.0
    assert B.ratio(v, T, comp, B.JITTER_K) > 1e3  # (the jitter itself is far outside rounding)


@pytest.mark.parametrize("kind,mut", [
    ("prop", dict(q_lower=True)), ("init", dict(r_lower=True)), ("augment", dict(stale_row=True)), ("prop", dict(phi_transposed=True)),
    ("prop", dict(skip=0)), ("init", dict(no_sign=True)), ("init", dict(hinv_plain=True))], ids=lambda v: v if isinstance(v, str) else next(iter(v)))
def test_the_bound_catches_each_mutated_model(kind, mut):
    """the lower triangle of Q or of R read, augment_dt's row step on the row dt from before the column step, Phi transposed, one
    old column skipped, the cross block without its sign, H_Linv not transposed: each leaves the bound in at least one case"""
    worst = 0.0
    for kd, c in _all_cases():
        if kd != kind or ("phi_transposed" in mut and c["phi"] != len(B.flat(c["old"]))):
            continue
        worst = max(worst, _model_ratio(kind, c, **mut))
    print("mutation %s: worst error / bound %.3g" % (mut, worst))
    assert worst > 1.0
