"""Extended-precision restatement of the update algebra: the truth the device and the double-precision oracle are measured against.

Everything here computes in np.longdouble (x87 80-bit on x86-64: 64-bit mantissa, eps 1.08e-19).  Inputs may be double (the
Jacobians of np_ref.feature_jacobian_full, a covariance, a pair read back from the device): the answer is then the exact answer for
those inputs to ~1e-19 x the conditioning, and nothing is rounded to double before the end.  Nothing here depends on the basis a
kernel picks for the null space of a feature (no Givens): the pair and the per-feature chi2 come from a Householder basis of the left
null space of H_f (Hp^T Hp, Hp^T rp, |rp|^2 and chi2 do not depend on the choice).  The projector identity (feature_pair) states the
same pair without any basis; it loses ~cond(H_f^T H_f) x eps to cancellation on short tracks (3e-15 relative on a two-observation
feature), so it is the cross-check (tests/test_ld_ref_cpu.py), not the truth.

  chol / solve_lower / solve_upper / inv_spd / solve   the dense pieces (lower Cholesky, Gaussian elimination with pivoting)
  feature_pair                                         A_f = Hp^T Hp, b_f = Hp^T rp, |rp|^2 of one feature by the projector identity
  nullspace_rows                                       Hp, rp in a Householder basis of the left null space of H_f
  householder_split                                    the same reflections with the top part kept: (H_L, H_R, res_L) and (Hp, rp)
  point_pair                                           the information pair of a set of point features, per-feature chi2 and dof
  update_from_pair                                     P+ = (I + P A)^-1 P = (P^-1 + A)^-1, dx = P+ b (no P^-1: singular priors too)
  update_from_pair_dropping                            the same on the pivot-dropping factor of A (the device's S-form retry)
  ekf_update_dense                                     StateHelper::EKFUpdate (S-form, R = I) on the columns `cols`
  ekf_propagation / augment_dt / initialize_invertible the covariance bookkeeping (StateHelper), each with its absolute companion
  zupt_compressed / zupt_stacked                       the zero-velocity update: the compressed form ovp_zupt_update computes, and the
                                                       reference's stacked 6 (n - 1)-row system through ekf_update_dense
  plane_merge / plane_merge_steps                      StateHelper::merge_planes_and_marginalize's pairs in order, each through
                                                       ekf_update_dense, with the quantities the rounding bounds of the tests need;
                                                       the n x n companion of each accepted pair, replayed one at a time
  eigvals_sym                                          eigenvalues of a small symmetric matrix (Jacobi), for kappa of S
  err_state / rel_p / err_chi2 / err_pair              the error metrics of tests/test_precision_gpu.py
"""
from __future__ import annotations

import numpy as np

from oracle import np_ref

LD = np.longdouble


def ld(a):
    return np.asarray(a, dtype=LD)


def sym(A):
    return (A + A.T) / 2


# ---- dense pieces ------------------------------------------------------------------------------------------------------
def chol(A):
    """Lower L with L L^T = A (A symmetric positive definite); raises on a non-positive pivot."""
    A = ld(A)
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not v[0] > 0:
            raise np.linalg.LinAlgError("chol: pivot %d is %r" % (j, float(v[0])))
        L[j:, j] = v / np.sqrt(v[0])
    return L


def solve_lower(L, B):
    X = np.array(B, dtype=LD, copy=True)
    for i in range(L.shape[0]):
        X[i] = (X[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def solve_upper(U, B):
    X = np.array(B, dtype=LD, copy=True)
    for i in range(U.shape[0] - 1, -1, -1):
        X[i] = (X[i] - U[i, i + 1:] @ X[i + 1:]) / U[i, i]
    return X


def inv_spd(A):
    Li = solve_lower(chol(A), np.eye(A.shape[0], dtype=LD))
    return Li.T @ Li


def solve(M, B):
    """M^-1 B by Gaussian elimination with partial pivoting (M square, B a vector or a matrix with M.shape[0] rows)."""
    M = np.array(M, dtype=LD, copy=True)
    B = np.array(B, dtype=LD, copy=True)
    vec = B.ndim == 1
    if vec:
        B = B[:, None]
    n = M.shape[0]
    for k in range(n):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        if M[p, k] == 0:
            raise np.linalg.LinAlgError("solve: singular at column %d" % k)
        if p != k:
            M[[k, p]] = M[[p, k]]
            B[[k, p]] = B[[p, k]]
        f = M[k + 1:, k] / M[k, k]
        M[k + 1:, k:] -= np.outer(f, M[k, k:])
        B[k + 1:] -= np.outer(f, B[k])
    X = solve_upper(np.triu(M), B)
    return X[:, 0] if vec else X


# ---- one feature ---------------------------------------------------------------------------------------------------------
def feature_pair(H_f, H_x, res):
    """(A_f, b_f, rr_f) = (Hp^T Hp, Hp^T rp, |rp|^2) with [Hp | rp] the rows of [H_x | res] left after projecting out the columns of
    H_f, by the projector identity Hp^T Hp = H_x^T H_x - (H_f^T H_x)^T (H_f^T H_f)^-1 (H_f^T H_x) (the same for b and rr)."""
    Hf, Hx, r = ld(H_f), ld(H_x), ld(res)
    Gi = inv_spd(Hf.T @ Hf)
    FX, Fr = Hf.T @ Hx, Hf.T @ r
    A = Hx.T @ Hx - FX.T @ Gi @ FX
    b = Hx.T @ r - FX.T @ (Gi @ Fr)
    rr = r @ r - Fr @ (Gi @ Fr)
    return sym(A), b, rr


def householder_split(H_f, H_x, res):
    """((H_L, H_R, res_L), (Hp, rp)): [H_f | H_x | res] under the Householder reflections that make H_f upper triangular.  The top
    cols(H_f) rows are the system that initialises the feature (UpdaterHelper / StateHelper::initialize: H_L [nf, nf] upper
    triangular, H_R, res_L), the bottom rows are the update rows nullspace_rows returns.  The basis is one of many (the reference
    takes Givens rotations; any orthogonal Q = diag(Q1, Q2) in front of the two parts is as good).  These do NOT depend on it:
    H_L^-1 res_L and H_L^-1 H_R (Q1 cancels), hence the initial value's correction, P_LL = H_L^-1 (H_R P H_R^T + I) H_L^-T and the
    cross block -P H_R^T H_L^-T; Hp^T Hp, Hp^T rp and |rp|^2 (Q2 cancels), hence the chi2 of the bottom rows, dx and P+ of the
    update with them (tests/test_ld_ref_cpu.py holds each against the oracle's Givens split)."""
    nf = np.asarray(H_f).shape[1]
    Hf, Hx, r = _householder(H_f, H_x, res)
    return (np.triu(Hf[:nf]), Hx[:nf], r[:nf]), (Hx[nf:], r[nf:])


def nullspace_rows(H_f, H_x, res):
    """(Hp, rp): [H_x | res] in a Householder basis of the left null space of H_f (rows - cols(H_f) rows)."""
    nf = np.asarray(H_f).shape[1]
    _, Hx, r = _householder(H_f, H_x, res)
    return Hx[nf:], r[nf:]


def _householder(H_f, H_x, res):
    Hf, Hx, r = np.array(H_f, dtype=LD), np.array(H_x, dtype=LD), np.array(res, dtype=LD)
    nf = Hf.shape[1]
    for k in range(nf):
        x = Hf[k:, k]
        nx = np.sqrt(x @ x)
        v = x.copy()
        v[0] += nx if x[0] >= 0 else -nx
        vv = v @ v
        if vv == 0:
            continue
        Hf[k:] -= np.outer(v, (2 / vv) * (v @ Hf[k:]))
        Hx[k:] -= np.outer(v, (2 / vv) * (v @ Hx[k:]))
        r[k:] -= v * ((2 / vv) * (v @ r[k:]))
    return Hf, Hx, r


def point_pair(sc, feats=None, P=None, with_chi2=True):
    """The information pair A = sum_f Hp^T Hp, b = sum_f Hp^T rp of the point features `feats` of a scene, in state columns, and
    per feature (over `feats`, in that order) chi2 = rp^T (Hp P_f Hp^T + I)^-1 rp (P_f the marginal of P on the feature's columns;
    P defaults to the scene's) and dof = rows - 3.  Returns dict(A, b, rr, chi2, dof)."""
    feats = range(sc.F) if feats is None else [int(f) for f in feats]
    P = sc.P if P is None else P
    N = sc.N
    A = np.zeros((N, N), dtype=LD)
    b = np.zeros(N, dtype=LD)
    rr = LD(0)
    chi2, dof = [], []
    for f in feats:
        H_f, H_x, res, order = np_ref.feature_jacobian_full(sc, f)
        cols = np_ref.order_cols(order)
        Hp, rp = nullspace_rows(H_f, H_x, res)
        A[np.ix_(cols, cols)] += sym(Hp.T @ Hp)
        b[cols] += Hp.T @ rp
        rr += rp @ rp
        dof.append(Hp.shape[0])
        if with_chi2:
            S = Hp @ ld(P[np.ix_(cols, cols)]) @ Hp.T + np.eye(Hp.shape[0], dtype=LD)
            y = solve_lower(chol(sym(S)), rp)
            chi2.append(y @ y)
    return dict(A=A, b=b, rr=rr, chi2=np.array(chi2, dtype=LD), dof=np.array(dof, dtype=np.int64))


# ---- the EKF tail ----------------------------------------------------------------------------------------------------------
def update_from_pair(P, A, b, dtype=LD):
    """P+ = (P^-1 + A)^-1 = (I + P A)^-1 P and dx = P+ b.  The second form needs no P^-1, so it holds for priors that are only
    positive semi-definite (an exact clone, a clone of a clone): I + P A is regular for any P, A >= 0.  dtype=np.float64 is the same
    algebra in double through LAPACK (the yardstick of a careful double implementation)."""
    if dtype == np.float64:
        P, A, b = (np.asarray(x, dtype=np.float64) for x in (P, A, b))
        Pp = np.linalg.solve(np.eye(P.shape[0]) + P @ A, P)
    else:
        P, A, b = ld(P), ld(A), ld(b)
        Pp = solve(np.eye(P.shape[0], dtype=LD) + P @ A, P)
    Pp = sym(Pp)
    return Pp, Pp @ b


def chol_dropping(A, rel):
    """Lower L with L L^T = A except in the columns whose pivot falls to rel x max diag(A) or below: those are zero (dropped, not
    flagged).  The rule of the device's pivot-dropping factor (csrc/k_chol2.hip, piv_floor with floor_scale = max diag), in the
    natural column order.  Returns (L, dropped columns)."""
    A = ld(A)
    n = A.shape[0]
    L = np.zeros_like(A)
    floor = LD(rel) * np.abs(np.diag(A)).max()
    dropped = []
    for j in range(n):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not v[0] > floor:
            dropped.append(j)
            continue
        L[j:, j] = v / np.sqrt(v[0])
    return L, dropped


def update_from_pair_dropping(P, A, b, rel=1e-13):
    """The update the device's S-form retry (ekf_sform, behind a failed chol(P)) intends: H := La^T with La the pivot-dropping factor
    of A (chol_dropping), P+ = P - P La (I + La^T P La)^-1 La^T P, dx = P+ b.  It differs from update_from_pair by the information
    in the dropped directions only: pivots at or below rel x max diag(A), i.e. rounding noise of the pair."""
    P = ld(P)
    La, dropped = chol_dropping(A, rel)
    W = P @ La
    Pp = sym(P - W @ solve(np.eye(P.shape[0], dtype=LD) + La.T @ W, W.T))
    return Pp, Pp @ ld(b), dropped


def update_from_pair_info(P, A, b):
    """The information form (P^-1 + A)^-1 of the same update, for positive definite priors."""
    Pp = sym(inv_spd(sym(inv_spd(ld(P)) + ld(A))))
    return Pp, Pp @ ld(b)


def ekf_update_dense(P, cols, H, r):
    """StateHelper::EKFUpdate with R = I (state/StateHelper.cpp:121-202), S-form: M = P[:, cols] H^T, S = H P[cols, cols] H^T + I,
    P+ = P - M S^-1 M^T, dx = M S^-1 r."""
    P, H, r = ld(P), ld(H), ld(r)
    cols = np.asarray(cols, dtype=np.int64)
    M = P[:, cols] @ H.T
    S = sym(H @ P[np.ix_(cols, cols)] @ H.T + np.eye(H.shape[0], dtype=LD))
    L = chol(S)
    W = solve_lower(L, M.T)  # L^-1 M^T
    y = solve_lower(L, r)
    return sym(P - W.T @ W), W.T @ y


# ---- covariance bookkeeping ------------------------------------------------------------------------------------------------
# Each returns (truth, companion).  The companion is the same expression with |.| of every operand, element by element (so every
# sign of the expression becomes a plus): the quantity the rounding bound of a sum of products is a multiple of.  An element the
# operation only copies has the companion |P_ij|.
def _upper_view(M):
    return np.triu(M) + np.triu(M, 1).T


def _propagation(P, new_start, old, Phi, Q):
    phi = Phi.shape[0]
    CPT = P[:, old] @ Phi.T                      # Cov * Phi^T over the old columns            (n x phi)
    PCP = Phi @ CPT[old, :] + _upper_view(Q)     # Phi * Cov * Phi^T + Q.selfadjointView<Upper>
    Pn = P.copy()
    s = slice(new_start, new_start + phi)
    Pn[s, :] = CPT.T
    Pn[:, s] = CPT
    Pn[s, s] = PCP
    return Pn


def ekf_propagation(P, new_start, old_cols, Phi, Q):
    """StateHelper::EKFPropagation (state/StateHelper.cpp:41-119) with the old variables flattened to their state columns
    `old_cols` (any order, repeats allowed; Phi [phi x len(old_cols)] in that order): the rows and columns [new_start,
    new_start + phi) become Phi P[old, :] and its transpose, the block Phi P[old, old] Phi^T + Q.selfadjointView<Upper>."""
    old = np.asarray(old_cols, dtype=np.int64)
    P, Phi, Q = ld(P), ld(Phi), ld(Q)
    assert Phi.shape[1] == len(old) and Q.shape == (Phi.shape[0], Phi.shape[0])
    return _propagation(P, new_start, old, Phi, Q), _propagation(np.abs(P), new_start, old, np.abs(Phi), np.abs(Q))


def _augment_dt(P, pose_id, dt_id, d):
    Pn = P.copy()
    Pn[:, pose_id:pose_id + 6] += np.outer(Pn[:, dt_id], d)   # Cov.block(0, pose, n, 6) += Cov.col(dt) d^T
    Pn[pose_id:pose_id + 6, :] += np.outer(d, Pn[dt_id, :])   # Cov.block(pose, 0, 6, n) += d Cov.row(dt), the row after step one
    return Pn


def augment_dt(P, pose_id, dt_id, d):
    """StateHelper::augment_clone's time-offset Jacobian on a clone already in the state: the column step, then the row step on
    the row dt the column step left.  dt_id must lie outside [pose_id, pose_id + 6)."""
    assert not pose_id <= dt_id < pose_id + 6
    P, d = ld(P), ld(d).reshape(6)
    return _augment_dt(P, pose_id, dt_id, d), _augment_dt(np.abs(P), pose_id, dt_id, np.abs(d))


def _initialize_invertible(P, cols, H_R, H_Linv, R, sign):
    n, k = P.shape[0], H_R.shape[0]
    M_a = P[:, cols] @ H_R.T                                   # P H^T                                     (n x k)
    M = _upper_view(H_R @ M_a[cols, :] + R)                    # (H_R P H_R^T + R).selfadjointView<Upper>
    Pn = np.zeros((n + k, n + k), dtype=P.dtype)
    Pn[:n, :n] = P
    Pn[n:, n:] = H_Linv @ M @ H_Linv.T
    Pn[:n, n:] = sign * (M_a @ H_Linv.T)
    Pn[n:, :n] = Pn[:n, n:].T
    return Pn


def initialize_invertible(P, cols, H_R, H_Linv, R):
    """StateHelper::initialize_invertible (state/StateHelper.cpp:520-573) on the state columns `cols` (H_R [k x len(cols)] in that
    order, H_Linv and R [k x k]): the covariance with the k new columns appended, P_LL = H_L^-1 M H_L^-T with the upper view of
    M = H_R P[cols, cols] H_R^T + R, cross block -P[:, cols] H_R^T H_L^-T."""
    cols = np.asarray(cols, dtype=np.int64)
    P, H_R, H_Linv, R = ld(P), ld(H_R), ld(H_Linv), ld(R)
    assert H_R.shape[1] == len(cols) and H_Linv.shape == R.shape == (H_R.shape[0], H_R.shape[0])
    return (_initialize_invertible(P, cols, H_R, H_Linv, R, -1),
            _initialize_invertible(np.abs(P), cols, np.abs(H_R), np.abs(H_Linv), np.abs(R), 1))


# ---- the zero-velocity update ----------------------------------------------------------------------------------------------
# (update/UpdaterZeroVelocity.cpp:119-265; include/ovplane_hip.h has the algebra of the compressed form)
def _zupt_cols(imu_id):
    return int(imu_id) + np.array([0, 1, 2, 9, 10, 11, 12, 13, 14], dtype=np.int64)  # theta | b_g | b_a


def _zupt_parts(sel, R, Rj, bg, ba, po, noise_mult):
    """dt [ni], r [ni, 6] (the residual of an interval is that of its first reading), rho [ni, 6] (|.| of every operand of r), the
    weights D [6], the per-second bias noise q [6] and H0 [6, 9]"""
    sel = ld(sel)
    g = np.array([0, 0, po["gravity_mag"]], dtype=LD)
    Rg, Rjg = ld(R) @ g, ld(Rj) @ g
    bg, ba = ld(bg), ld(ba)
    dt = np.diff(sel[:, 0])
    r = -np.concatenate([sel[:-1, 1:4] - bg, sel[:-1, 4:7] - ba - Rg], axis=1)
    rho = np.concatenate([np.abs(sel[:-1, 1:4]) + np.abs(bg), np.abs(sel[:-1, 4:7]) + np.abs(ba) + np.abs(Rg)], axis=1)
    m = LD(noise_mult)
    D = np.concatenate([np.full(3, 1 / (m * LD(po["sigma_w"]) ** 2)), np.full(3, 1 / (m * LD(po["sigma_a"]) ** 2))])
    q = np.concatenate([np.full(3, LD(po["sigma_wb"])), np.full(3, LD(po["sigma_ab"]))])  # sigmas, not squares (:184-186)
    S3 = np.array([[0, -Rjg[2], Rjg[1]], [Rjg[2], 0, -Rjg[0]], [-Rjg[1], Rjg[0], 0]], dtype=LD)
    H0 = np.zeros((6, 9), dtype=LD)
    H0[0:3, 3:6] = -np.eye(3, dtype=LD)
    H0[3:6, 0:3] = -S3
    H0[3:6, 6:9] = -np.eye(3, dtype=LD)
    return dt, r, rho, D, q, H0


def eigvals_sym(S):
    """The eigenvalues of a small symmetric matrix in long double, ascending, by cyclic Jacobi rotations (numpy's eigvalsh has no
    long-double path)."""
    A = np.array(S, dtype=LD, copy=True)
    n = A.shape[0]
    for _ in range(60):
        off = np.sqrt(((A - np.diag(np.diag(A))) ** 2).sum())
        if off <= np.finfo(LD).eps * np.abs(np.diag(A)).max():
            break
        for p in range(n - 1):
            for q in range(p + 1, n):
                if A[p, q] == 0:
                    continue
                theta = (A[q, q] - A[p, p]) / (2 * A[p, q])
                t = (1 if theta >= 0 else -1) / (np.abs(theta) + np.sqrt(theta * theta + 1))
                c = 1 / np.sqrt(t * t + 1)
                J = np.eye(n, dtype=LD)
                J[p, p] = J[q, q] = c
                J[p, q], J[q, p] = t * c, -t * c
                A = sym(J.T @ A @ J)
    return np.sort(np.diag(A))


def _cond2(S):
    """(2-norm condition number, smallest eigenvalue, largest) of a small SPD matrix: computed in long double (eigvals_sym), then
    rounded to double"""
    w = eigvals_sym(S)
    return float(w[-1] / w[0]), float(w[0]), float(w[-1])


def zupt_compressed(P, sel, imu_id, R, Rj, bg, ba, po, noise_mult):
    """The algebra of tests/zupt_ref.py::compressed: T = sum dt_i, rbar = sum dt_i r_i / T, the scatter about rbar, P' = P + Q_bias
    on the bias diagonal, Sbar = H0 P'_ss H0^T + (T D)^-1 = L L^T, z = L^-1 rbar, chi2 = scatter + |z|^2, Y = P'_{:,s} H0^T L^-T,
    dx = Y z, P+ = P' - Y Y^T.  No inverse is formed: Y comes from a triangular solve.  Returns (truth, companion):
      truth      dict(chi2, rows, dx, P, kappa, ...) with kappa the 2-norm condition number of Sbar rounded to double, and the
                 intermediate values the derivation of a bound refers to: T, rbar, scatter, z, Y, Pp (= P'), Sbar, lam_min, lam_max, Tq (= diag Q_bias)
      companion  dict(P = |P'| + |Y| |Y|^T element by element; rbar = sum dt_i rho_i / T with rho_i the |.| of the operands of r_i;
                 scatter_lin = sum dt_i D |r_i - rbar| (rho_i + rbar's), scatter_sq = sum dt_i D (rho_i + rbar's)^2: what an error
                 of r_i - rbar is multiplied by; Sbar = |H0| |P'_ss| |H0|^T + (T D)^-1; SbarT = its part that is a multiple of the summed
                 T: (T D)^-1 + |H0| Q_bias |H0|^T; M = |P'_{:,s}| |H0|^T [n, 6]; z = |L^-1| rbar's companion [6], which is what z is
                 conditioned by when rbar is a small difference of readings and gravity: L^-1 here is a companion only, no truth
                 value passes through it)"""
    P = ld(P)
    dt, r, rho, D, q, H0 = _zupt_parts(sel, R, Rj, bg, ba, po, noise_mult)
    T = dt.sum()
    rbar = (dt[:, None] * r).sum(axis=0) / T
    rhobar = (dt[:, None] * rho).sum(axis=0) / T
    e = r - rbar
    scatter = (dt[:, None] * e * e * D).sum()
    s = _zupt_cols(imu_id)
    Pp = P.copy()
    Pp[s[3:], s[3:]] += T * q
    Rbar = np.diag(1 / (T * D))
    Sbar = sym(H0 @ Pp[np.ix_(s, s)] @ H0.T + Rbar)
    L = chol(Sbar)
    z = solve_lower(L, rbar)
    M = Pp[:, s] @ H0.T                     # [n, 6]
    Y = solve_lower(L, M.T).T               # M L^-T
    kappa, lam_min, lam_max = _cond2(Sbar)
    truth = dict(chi2=scatter + z @ z, rows=6 * len(dt), dx=Y @ z, P=sym(Pp - Y @ Y.T), kappa=kappa, T=T, rbar=rbar, scatter=scatter,
                 z=z, Y=Y, Pp=Pp, Sbar=Sbar, lam_min=lam_min, lam_max=lam_max, Tq=T * q)
    w = rho + rhobar
    comp = dict(P=np.abs(Pp) + np.abs(Y) @ np.abs(Y).T, rbar=rhobar, scatter_lin=(dt[:, None] * D * np.abs(e) * w).sum(),
                scatter_sq=(dt[:, None] * D * w * w).sum(), Sbar=np.abs(H0) @ np.abs(Pp[np.ix_(s, s)]) @ np.abs(H0).T + Rbar,
                M=np.abs(Pp[:, s]) @ np.abs(H0).T, z=np.abs(solve_lower(L, np.eye(6, dtype=LD))) @ rhobar, SbarT=Rbar + np.abs(H0[:, 3:]) @ np.diag(T * q) @ np.abs(H0[:, 3:]).T)
    return truth, comp


def zupt_stacked(P, sel, imu_id, R, Rj, bg, ba, po, noise_mult):
    """The reference's own system: 6 rows per interval, H = H0 over [theta, b_g, b_a], noise noise_mult sigma^2 / dt_i, whitened
    row by row with sqrt(dt_i D) so that R = I, on P + Q_bias, through ekf_update_dense; chi2 = res^T S^-1 res of the whitened
    rows.  Returns dict(chi2, rows, dx, P)."""
    P = ld(P)
    dt, r, _, D, q, H0 = _zupt_parts(sel, R, Rj, bg, ba, po, noise_mult)
    s = _zupt_cols(imu_id)
    Pp = P.copy()
    Pp[s[3:], s[3:]] += dt.sum() * q
    w = np.sqrt(dt[:, None] * D[None, :])                  # [ni, 6]
    H = (w[:, :, None] * H0[None, :, :]).reshape(-1, 9)
    res = (w * r).reshape(-1)
    Pn, dx = ekf_update_dense(Pp, s, H, res)
    S = sym(H @ Pp[np.ix_(s, s)] @ H.T + np.eye(H.shape[0], dtype=LD))
    y = solve_lower(chol(S), res)
    return dict(chi2=y @ y, rows=H.shape[0], dx=dx, P=Pn)


# ---- the plane merge -------------------------------------------------------------------------------------------------------
def plane_merge(P, pairs, plane_col, cp, sigma, chi2_mult, deg_max, chi2_095_3=7.814727903251179):
    """StateHelper::merge_planes_and_marginalize's pairs (state/StateHelper.cpp:693-734), in order: for the pair (new, old) the
    angle of the two closest points' directions, H = [I, -I] / sigma over [new..new+3, old..old+3], res = (0 - (cp_new - cp_old)) /
    sigma, chi2 = res^T S^-1 res, the decision chi2 < chi2_mult chi2_095(3) and angle < deg_max, and on acceptance
    ekf_update_dense on the P the pair before left and cp += dx for every plane of the table.  Returns (truth, companion):
      truth      dict(accepted [np], chi2, angle_deg, dot, dx [np, n], P (un-compacted), cp (as the last pair left them), and per
                 pair the small values a bound refers to: S, kappa, lam_min, lam_max, y (= L^-1 res), res, cp_new, cp_old, and
                 W (= M L^-T [n, 3]; None for a rejected pair))
      companion  per pair dict(M = (|P_in[:, new]| + |P_in[:, old]|) / sigma [n, 3], S = (|P_nn| + |P_no| + |P_on| + |P_oo|) /
                 sigma^2 + I), P_in the P the pair read.  The n x n companion |P_in| + |W| |W|^T of an accepted pair is not kept per
                 pair (64 pairs at n = 399 would hold 160 MB): plane_merge_steps replays P_in and yields it pair by pair."""
    P = ld(P).copy()
    n = P.shape[0]
    wc = 1 / LD(sigma)
    thr = LD(chi2_mult) * LD(chi2_095_3)
    cur = {int(c): ld(v).copy() for c, v in zip(plane_col, np.reshape(np.asarray(cp, dtype=np.float64), (-1, 3)))}
    H = np.hstack([wc * np.eye(3, dtype=LD), -wc * np.eye(3, dtype=LD)])
    keys = ("accepted", "chi2", "angle_deg", "dot", "S", "kappa", "lam_min", "lam_max", "y", "res", "W", "cp_new", "cp_old", "dx")
    t = {k: [] for k in keys}
    comps = []
    for cn, co in pairs:
        cn, co = int(cn), int(co)
        c1, c0 = cur[cn], cur[co]
        dot = (c1 / np.sqrt(c1 @ c1)) @ (c0 / np.sqrt(c0 @ c0))
        with np.errstate(invalid="ignore"):
            angle = (LD(180) / np.arccos(LD(-1))) * np.arccos(dot)  # (a dot product rounded above 1 is NaN here as in :701, and a rejection)
        idx = np.r_[cn:cn + 3, co:co + 3]
        res = wc * (0 - (c1 - c0))
        S = sym(H @ P[np.ix_(idx, idx)] @ H.T + np.eye(3, dtype=LD))
        L = chol(S)
        y = solve_lower(L, res)
        chi2 = y @ y
        ok = bool(chi2 < thr and angle < LD(deg_max))
        kappa, lam_min, lam_max = _cond2(S)
        An, Ao = np.abs(P[:, cn:cn + 3]), np.abs(P[:, co:co + 3])
        comps.append(dict(M=wc * (An + Ao), S=wc * wc * (An[cn:cn + 3] + Ao[cn:cn + 3] + An[co:co + 3] + Ao[co:co + 3]) + np.eye(3, dtype=LD)))
        W, dx = None, np.zeros(n, dtype=LD)
        if ok:
            W = solve_lower(L, (P[:, idx] @ H.T).T).T
            P, dx = ekf_update_dense(P, idx, H, res)
            for c in cur:
                cur[c] = cur[c] + dx[c:c + 3]
        for k, v in zip(keys, (ok, chi2, angle, dot, S, kappa, lam_min, lam_max, y, res, W, c1.copy(), c0.copy(), dx)):
            t[k].append(v)
    truth = dict(t, accepted=np.array(t["accepted"], dtype=bool), chi2=np.array(t["chi2"], dtype=LD), angle_deg=np.array(t["angle_deg"], dtype=LD),
                 dx=np.array(t["dx"], dtype=LD).reshape(-1, n), P=P, cp=cur, chi2_thr=thr)
    return truth, comps


def plane_merge_steps(P, truth):
    """For every accepted pair k of a plane_merge truth on P, in order: (k, P_in, |P_in| + |W| |W|^T), P_in the covariance the pair
    read and the second the companion of its step.  P_in is replayed as sym(P_in - W W^T), the expression ekf_update_dense
    evaluates (bit for bit: the last one equals truth["P"])."""
    P = ld(P).copy()
    for k, W in enumerate(truth["W"]):
        if W is None:
            continue
        yield k, P, np.abs(P) + np.abs(W) @ np.abs(W).T
        P = sym(P - W @ W.T)


# ---- error metrics ---------------------------------------------------------------------------------------------------------
def _scale(d):
    d = np.sqrt(np.abs(np.asarray(d, dtype=np.float64)))
    d[d == 0] = 1.0
    return d


def err_state(dx, dx_true, P_true):
    """max_i |dx_i - dx_true_i| / sqrt(P+_true_ii): the state error in standard deviations of the updated state."""
    return float((np.abs(np.asarray(dx, dtype=LD) - ld(dx_true)) / _scale(np.diag(P_true))).max())


def rel_p(P, P_true):
    """max_ij |P_ij - P_true_ij| / sqrt(P_true_ii P_true_jj) (correlation-normalised, as the parity tests measure it)."""
    d = _scale(np.diag(P_true))
    return float((np.abs(np.asarray(P, dtype=LD) - ld(P_true)) / np.outer(d, d)).max())


def rel_diag(P, P_true, cols):
    """max_{i in cols} |P_ii - P_true_ii| / P_true_ii: the diagonal alone, in units of itself."""
    cols = np.asarray(cols, dtype=np.int64)
    d = np.abs(np.diag(ld(P_true))[cols])
    return float((np.abs(np.diag(np.asarray(P, dtype=LD))[cols] - np.diag(ld(P_true))[cols]) / np.where(d > 0, d, 1)).max())


def err_chi2(c, c_true):
    """max_f |chi2_f - chi2_true_f| / max(1, chi2_true_f)."""
    c_true = ld(c_true)
    return float((np.abs(np.asarray(c, dtype=LD) - c_true) / np.maximum(1, np.abs(c_true))).max())


def err_pair(A, b, A_true, b_true, rr_true):
    """Pair errors on their natural scales: (max_ij |dA_ij| / sqrt(A_ii A_jj), max_i |db_i| / sqrt(A_ii rr)) with the truth's
    diagonal and residual energy (|b_i| <= sqrt(A_ii rr) by Cauchy-Schwarz)."""
    d = _scale(np.diag(A_true))
    eA = float((np.abs(np.asarray(A, dtype=LD) - ld(A_true)) / np.outer(d, d)).max())
    eb = float((np.abs(np.asarray(b, dtype=LD) - ld(b_true)) / (d * np.sqrt(max(float(rr_true), 1e-300)))).max())
    return eA, eb
