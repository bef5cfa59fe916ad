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


def _givens_split(H_f, H_x, res):
    """the reference's rotations (np_ref.nullspace_project_inplace) with the top rows kept: (H_L, H_R, res_L), (Hp, rp)"""
    H_f, H_x, res = H_f.copy(), H_x.copy(), res.copy().reshape(-1, 1)
    nf = H_f.shape[1]
    for n in range(nf):
        for m in range(H_f.shape[0] - 1, n, -1):
            c, s = np_ref.make_givens(H_f[m - 1, n], H_f[m, n])
            for M, c0 in ((H_f, n), (H_x, 0), (res, 0)):
                np_ref._rot2(M, m - 1, c, s, c0)
    return (np.triu(H_f[:nf]), H_x[:nf], res[:nf, 0]), (H_x[nf:], res[nf:, 0])


def test_householder_split_invariants_against_the_givens_split():
    """What ld_ref.householder_split names as independent of the basis, against the oracle's Givens split in double: H_L^-1 res_L,
    H_L^-1 H_R, P_LL, the cross block, the chi2 of the bottom rows, and dx / P+ of the update with them.  Tolerances: the double
    split's own rounding, 1e-12 relative to each quantity's largest element (kappa(H_L) of a 2- to 9-observation feature times
    a few hundred roundings)."""
    sc = make_scene(C=9, F=8, seed=5, ragged=True, min_meas=2)
    P = ld_ref.ld(sc.P)
    rel = lambda a, b: float(np.abs(ld_ref.ld(a) - b).max() / max(float(np.abs(b).max()), 1e-300))  # noqa: E731
    for f in range(sc.F):
        H_f, H_x, res, order = np_ref.feature_jacobian_full(sc, f)
        cols = np_ref.order_cols(order)
        (HL, HR, rL), (Hp, rp) = ld_ref.householder_split(H_f, H_x, res)
        (gL, gR, grL), (gp, grp) = _givens_split(H_f, H_x, res)
        assert np.abs(np.tril(HL, -1)).max() == 0 and HL.shape == (3, 3) and Hp.shape[0] == H_x.shape[0] - 3
        Hp2, rp2 = ld_ref.nullspace_rows(H_f, H_x, res)
        assert (Hp2 == Hp).all() and (rp2 == rp).all()
        Li, gLi = ld_ref.solve_upper(HL, np.eye(3, dtype=ld_ref.LD)), np.linalg.inv(gL)
        assert rel(gLi @ grL, Li @ rL) <= 1e-12 and rel(gLi @ gR, Li @ HR) <= 1e-12
        t, _ = ld_ref.initialize_invertible(P, cols, HR, Li, np.eye(3))
        g, _ = ld_ref.initialize_invertible(P, cols, gR, gLi, np.eye(3))
        n = sc.N
        assert rel(g[n:, n:], t[n:, n:]) <= 1e-12 and rel(g[:n, n:], t[:n, n:]) <= 1e-12
        if Hp.shape[0] == 0:
            continue
        chi2 = lambda H, r: (lambda y: y @ y)(ld_ref.solve_lower(ld_ref.chol(ld_ref.sym(  # noqa: E731
            ld_ref.ld(H) @ P[np.ix_(cols, cols)] @ ld_ref.ld(H).T + np.eye(len(r), dtype=ld_ref.LD))), ld_ref.ld(r)))
        assert abs(chi2(gp, grp) - chi2(Hp, rp)) <= 1e-12 * max(1.0, float(chi2(Hp, rp)))
        Pt, dxt = ld_ref.ekf_update_dense(P, cols, Hp, rp)
        Pg, dxg = ld_ref.ekf_update_dense(P, cols, gp, grp)
        assert rel(dxg, dxt) <= 1e-11 and ld_ref.rel_p(Pg, Pt) <= 1e-12


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


# ---- the zero-velocity update and the plane merge: the truths of tests/test_zupt_precision_gpu.py and tests/test_retire_precision_gpu.py,
# ---- their bounds, and the faulty models the bounds catch ----
import retire_cases as RC  # noqa: E402
import retire_ref as RR  # noqa: E402
import zupt_cases as ZC  # noqa: E402
import zupt_ref as ZR  # noqa: E402

EPS_LD = float(np.finfo(LD).eps)


def _zupt_args(c):
    P, rd, kw = ZC.inputs(c)
    x = ZC.imu_state()
    return (P, rd, c["imu_id"], x["R"], x["Rj"], x["bg"], x["ba"], ZR.PO, ZR.NOISE_MULT), kw


def _ld_ratio(got, truth, comp, K):
    """cov_bookkeeping_cases.ratio with the long-double unit roundoff 2^-64 in place of u: max |got - truth| / (K 2^-64 comp)"""
    err = np.abs(got - truth)
    bound = K * LD(EPS_LD / 2) * comp
    r = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, 1))
    return float(np.max(np.where((bound == 0) & (err > 0), np.inf, r)))


@pytest.mark.parametrize("c", [c for c in ZC.cases() if c["readings"] <= 258], ids=lambda c: c["name"])
def test_zupt_compressed_equals_the_stacked_system_in_long_double(c):
    """zupt_compressed == zupt_stacked (the reference's own 6 (n - 1)-row system, whitened, through ekf_update_dense) at long-double
    level, element by element on the companions of the compressed form, with the metric of cov_bookkeeping_cases.ratio at the
    long-double unit roundoff 2^-64 and K = 2 (ni + 6) roundings, no condition number: 7.6e-19 relative for two readings, 2.9e-17
    for 258.  The counts: each formulation sums ni terms per element and solves with 6 (or 6 ni, banded by construction) unknowns,
    hence ni + 6 each.  chi2: relative to itself.  P: against comp.P = |P'| + |Y| |Y|^T.  dx = Y z: against |Y| comp.z with
    comp.z = |L^-1| rhobar, not |Y| |z|: standing, rbar is what is left of readings and gravity that cancel to 1e-4 of their size,
    and z inherits the rounding of the operands (rhobar), in either formulation.
    The stacked system of 4096 readings has 24570 rows and is too large to factor here: at 4096 the compressed truth stands
    alone, held up by the 257 / 258-reading cases (the same code, the same strides) and by the double restatement below."""
    args, _ = _zupt_args(c)
    t, comp = ld_ref.zupt_compressed(*args)
    s = ld_ref.zupt_stacked(*args)
    ni = c["readings"] - 1
    K = 2 * (ni + 6)
    assert s["rows"] == t["rows"] == 6 * ni
    r = [_ld_ratio(s["chi2"], t["chi2"], t["chi2"], K), _ld_ratio(s["dx"], t["dx"], np.abs(t["Y"]) @ comp["z"], K),
         _ld_ratio(s["P"], t["P"], comp["P"], K)]
    print("ZUPT-LD %s: chi2 %.3f dx %.3f P %.3f of %d x 2^-64" % (c["name"], r[0], r[1], r[2], K))
    assert max(r) <= 1.0
    assert (comp["P"] >= np.abs(t["P"])).all() and t["P"].dtype == LD
    assert (np.abs(t["Y"]) @ comp["z"] >= np.abs(t["Y"]) @ np.abs(t["z"])).all()


@pytest.mark.parametrize("c", ZC.cases(), ids=lambda c: c["name"])
def test_zupt_cases_have_their_margin_and_the_double_restatements_stay_inside_the_bound(oracle, c):
    """Every gated case: the truth's chi2 outside thr (1 -+ 1e-9), the decision the case is named after.  Then zupt_ref.compressed,
    the model of zupt_cases.py without a fault and - up to 258 readings, where its stacked system is small enough - the C oracle's
    zupt_update through the derived bounds: ratio <= 1."""
    args, kw = _zupt_args(c)
    t, _, _ = ZC.truth(c)
    thr = ZC.threshold(c)
    assert abs(float(t["chi2"]) / thr - 1.0) > ZC.MARGIN
    acc = ZC.decision(c, float(t["chi2"]))
    assert acc == ZC.expected(c)
    assert (float(t["chi2"]) <= thr) == (c["kind"] in ("accept", "reject_vel"))
    ref = ZR.compressed(*args[:-1])
    m = ZC.model(c)
    assert ref["spd"] and m["accepted"] == acc
    for what, got in (("restatement", ref), ("model", m)):
        r = ZC.ratios(c, got["chi2"], got["dx"] if acc else None, got["P"] if acc else None)
        print("ZUPT-CPU %s %s %s" % (c["name"], what, " ".join("%.4f" % v for v in r)))
        assert max(r) <= 1.0
    # the C oracle selects its own readings: a stream with one more reading on either side gives the case's readings back
    # unchanged for their own first and last time stamp; its stacked system has 6 (n - 1) rows, so the 4096-reading cases stay out
    P, rd = args[0], args[1]
    if c["readings"] <= 258:
        pre, post = rd[:1].copy(), rd[-1:].copy()
        pre[0, 0] -= 2.5e-3
        post[0, 0] += 2.5e-3
        stream = np.vstack([pre, rd, post])
        assert np.array_equal(oracle.select_imu_readings(stream, rd[0, 0], rd[-1, 0]), rd)
        x = ZR.scenario(True)[0]
        if not kw["vel_ok"]:  # the oracle takes the velocity estimate and the limit, not the flag: an estimate over the limit
            x = dict(x, v=np.array([0.0, 0.0, 2 * ZR.MAX_VELOCITY]))
        o = oracle.zupt_update(x, ZR.PO, P, stream, rd[0, 0], rd[-1, 0], imu_id=c["imu_id"], disparity_passed=kw["disparity_passed"])
        assert o["accepted"] == acc and o["rows"] == t["rows"]
        r = ZC.ratios(c, o["chi2"], o["dx"] if acc else None, o["P"] if acc else None)
        print("ZUPT-CPU %s oracle %s" % (c["name"], " ".join("%.4f" % v for v in r)))
        assert max(r) <= 1.0


@pytest.mark.parametrize("fault", ZC.FAULTS)
def test_the_zupt_bound_catches_each_faulty_model(fault):
    """one fault each (zupt_cases.model): at least one case leaves the bound or flips its decision"""
    worst, flipped = 0.0, False
    for c in ZC.cases():
        t, _, _ = ZC.truth(c)
        acc = ZC.decision(c, float(t["chi2"]))
        m = ZC.model(c, fault)
        if m["accepted"] != acc:
            flipped = True
            continue
        worst = max(worst, max(ZC.ratios(c, m["chi2"], m["dx"] if acc else None, m["P"] if acc else None)))
    print("zupt fault %s: worst error / bound %.3g, decision flipped %s" % (fault, worst, flipped))
    assert worst > 1.0 or flipped


WELL_CONDITIONED = ["n63_behind_first_last", "n65_across64", "n129_chain_chi2", "n257_to_254"]


@pytest.mark.parametrize("name", WELL_CONDITIONED)
def test_plane_merge_equals_the_information_form(name):
    """every accepted pair of plane_merge against update_from_pair_info on A = H^T H, b = H^T res scattered into the state: the same
    update without S.  The covariances of these cases have a condition number of ~1e17 over their eight decades of scales, so the
    comparison runs on the correlation-scaled problem (D P D, D^-1 H: the same update, exactly, with D a diagonal of powers of two)."""
    c = RC.case(name)
    t, _, _ = RC.truth(name)
    n = c["n"]
    wc = 1 / LD(c["sigma"])
    steps = list(ld_ref.plane_merge_steps(c["P"], t))
    assert len(steps) == int(t["accepted"].sum())
    for j, (k, Pin, comp_P) in enumerate(steps):
        cn, co = c["pairs"][k]
        d = 2.0 ** -np.round(np.log2(np.sqrt(np.asarray(np.diag(Pin), dtype=np.float64))))
        D = ld_ref.ld(d)
        H = np.zeros((3, n), dtype=LD)
        H[:, cn:cn + 3] = wc * np.eye(3, dtype=LD)
        H[:, co:co + 3] = -wc * np.eye(3, dtype=LD)
        Hs = H / D[None, :]
        Pi, dxi = ld_ref.update_from_pair_info(Pin * np.outer(D, D), Hs.T @ Hs, Hs.T @ t["res"][k])
        Pn = steps[j + 1][1] if j + 1 < len(steps) else t["P"]
        if j + 1 == len(steps):  # the replay is ekf_update_dense's own expression: the last step lands on the truth's P, bit for bit
            assert np.array_equal(ld_ref.sym(Pin - t["W"][k] @ t["W"][k].T), t["P"])
        assert (comp_P >= np.abs(Pn)).all()
        e_P = ld_ref.rel_p(Pi / np.outer(D, D), Pn)
        e_dx = ld_ref.err_state(dxi / D, t["dx"][k], Pn)
        print("MERGE-LD %s pair %d: P %.1e dx %.1e" % (name, k, e_P, e_dx))
        assert e_P < 1e-15 and e_dx < 1e-14


@pytest.mark.parametrize("name", RC.names())
def test_merge_cases_have_their_margins_and_the_double_restatements_stay_inside_the_bound(name):
    """chi2 outside thr (1 -+ 1e-9) and the angle outside deg_max (1 -+ 1e-9) for every pair, the decisions the case is built for,
    the first-order angle bound in its range (delta << 1 - dot), the exactly parallel pair at dot = 1 and 0.0 degrees; then
    retire_ref.merge_ref and the model of retire_cases.py without a fault through the derived bounds: ratio <= 1."""
    c = RC.case(name)
    t, _, b = RC.truth(name)
    thr = float(t["chi2_thr"])
    assert t["accepted"].tolist() == RC.expected(c)
    for k, kind in enumerate(c["kinds"]):
        assert abs(float(t["chi2"][k]) / thr - 1.0) > RC.MARGIN and abs(float(t["angle_deg"][k]) / c["deg_max"] - 1.0) > RC.MARGIN
        assert (float(t["chi2"][k]) < thr) == (kind != "chi2") and (float(t["angle_deg"][k]) < c["deg_max"]) == (kind != "angle")
        if kind == "parallel":
            assert t["dot"][k] == 1 and t["angle_deg"][k] == 0 and b["angle"][k] == 0
        else:
            assert float(b["angle"][k]) * RC.U * np.pi / 180 * np.sqrt(float(1 - t["dot"][k] ** 2)) < 1e-3 * float(1 - t["dot"][k])
        if kind == "near":
            assert 0.5e-3 < float(t["angle_deg"][k]) < 2e-3
    ref = RR.merge_ref(c["P"], c["pairs"], c["plane_col"], c["cp"], c["sigma"], c["chi2_mult"], c["deg_max"], c["retire_ids"], c["retire_sizes"])
    m = RC.model(name)
    for what, got in (("restatement", ref), ("model", m)):
        assert got["accepted"].tolist() == t["accepted"].tolist()
        r = RC.ratios(name, got["chi2"], got["angle_deg"], got["dx"], got["P"])
        print("RETIRE-CPU %s %s %s" % (name, what, " ".join("%.4f" % v for v in r)))
        assert max(r) <= 1.0


@pytest.mark.parametrize("fault", RC.FAULTS)
def test_the_merge_bound_catches_each_faulty_model(fault):
    worst, flipped = 0.0, False
    for name in RC.names():
        t, _, _ = RC.truth(name)
        m = RC.model(name, fault)
        if m["accepted"].tolist() != t["accepted"].tolist():
            flipped = True
            continue
        worst = max(worst, max(RC.ratios(name, m["chi2"], m["angle_deg"], m["dx"], m["P"])))
    print("merge fault %s: worst error / bound %.3g, decision flipped %s" % (fault, worst, flipped))
    assert worst > 1.0 or flipped


def test_a_compaction_map_that_restarts_at_column_256_is_caught():
    """compact_model == compact_ref on every compaction case; with the restart it differs wherever n_out > 256 and something was
    removed in front of output column 256"""
    caught = 0
    for name, (n, ids, sizes) in RC.compact_cases().items():
        P = B.spd(n, 60 + n + len(ids))
        want = RR.compact_ref(P, ids, sizes)
        assert want.shape[0] == n - sum(sizes)
        assert np.array_equal(RC.compact_model(P, ids, sizes), want), name
        caught += not np.array_equal(RC.compact_model(P, ids, sizes, restart=True), want)
    assert caught >= 5
