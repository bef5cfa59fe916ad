"""The cases, rounding bounds and plain float64 models of the covariance bookkeeping tests (tests/test_cov_bookkeeping_gpu.py on the
device, tests/test_ld_ref_cpu.py for the bounds themselves).

Every expected value is either a copy or a short sum of products.  For a sum the bound is the standard one of a dot product:
an element whose terms pass through at most K roundings (products, additions, fused or not, in any order) differs from the exact
value by at most gamma_K x companion, gamma_K = K u / (1 - K u) with u = 2^-53 and the companion the same expression with |.| of
every operand (oracle/ld_ref.py returns it).  (K + 2) u covers gamma_K for every K here (K u < 1e-12) and the rounding of the
long-double truth (2^-64 relative).  K is counted per element below; nothing is taken from a run of the code under test."""
import numpy as np

from oracle import ld_ref

U = 2.0 ** -53
STATE_SIZES = (15, 16, 17, 129, 257, 700)  # ld = n and ld > n, the 128- and 256-thread block edges, the cap (OVP_LDG_CAP = 704)


def capacities(n):
    """n_max = n and n_max > n (700 is the largest context there is)"""
    return (n,) if n >= 700 else (n, n + 5)


def spd(n, seed):
    """A symmetric positive definite matrix, exactly symmetric, whose standard deviations spread over eight decades (a uniform
    scale lets an error in a small block disappear under a global maximum)."""
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((n, n + 3))
    A = G @ G.T / (n + 3)
    A = (A + A.T) / 2 + 0.5 * np.eye(n)
    s = 10.0 ** rng.uniform(-4.0, 4.0, n)
    return np.outer(s, s) * A


def flat(old):
    """[(id, size), ...] -> state columns, in that order"""
    return np.array([i + k for i, sz in old for k in range(sz)], dtype=np.int64)


def ratio(got, truth, comp, K):
    """max over the elements of |got - truth| / ((K + 2) u companion); K a number or an array.  An element with a zero bound must
    be exact (inf otherwise)."""
    err = np.abs(np.asarray(got, dtype=ld_ref.LD) - truth)
    bound = (np.asarray(K, dtype=ld_ref.LD) + 2) * ld_ref.LD(U) * comp
    r = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, 1))
    r = np.where((bound == 0) & (err > 0), np.inf, r)
    return float(np.max(r)) if r.size else 0.0


# ---- propagation ---------------------------------------------------------------------------------------------------------
def prop_cases():
    """dict(name, n, start, phi, old [(id, size)], seed[, qdiag]) - Q always has differing triangles.
    front / middle / very end; phi 1, 3, 15, 64; one old variable; the anchor change (phi = 3 at the end; landmark, two clones and
    the calibration out of ascending order); an old column listed twice; old columns with and without the new block."""
    cases = []
    for n in STATE_SIZES:  # every size: three columns at the very end, old variables unsorted, the block among them
        cases.append(dict(name="end3_n%d" % n, n=n, start=n - 3, phi=3, old=[(n - 3, 3), (6, 6), (0, 6)]))
    cases += [
        dict(name="whole15", n=15, start=0, phi=15, old=[(0, 15)]),                      # front and end at once, one old variable
        dict(name="front15", n=17, start=0, phi=15, old=[(0, 15)]),
        dict(name="front15_n700", n=700, start=0, phi=15, old=[(0, 15)]),
        dict(name="middle1", n=16, start=7, phi=1, old=[(7, 1)]),
        dict(name="middle3", n=129, start=60, phi=3, old=[(60, 3), (10, 6)]),
        dict(name="middle15_wide", n=257, start=100, phi=15, old=[(100, 15), (200, 57), (0, 64)]),
        dict(name="end64", n=257, start=193, phi=64, old=[(193, 64)]),
        dict(name="end64_n700", n=700, start=636, phi=64, old=[(636, 64), (0, 15)]),
        dict(name="anchor_change", n=129, start=126, phi=3, old=[(126, 3), (42, 6), (30, 6), (16, 6)]),
        dict(name="anchor_change_n700", n=700, start=697, phi=3, old=[(697, 3), (42, 6), (30, 6), (16, 6)]),
        dict(name="twice", n=129, start=100, phi=3, old=[(5, 3), (100, 3), (5, 3)]),
        dict(name="without_block", n=257, start=254, phi=3, old=[(0, 15)]),
        dict(name="without_block_middle", n=17, start=8, phi=3, old=[(12, 5), (0, 6)]),
    ]
    for i, c in enumerate(cases):
        c["seed"] = 100 + i
    return cases


def prop_inputs(c, qdiag=None):
    """(P, Phi, Q) of a case.  Q = a symmetric part on the scale of the block plus a different strictly lower triangle (read by
    nobody); qdiag replaces Q[0, 0] (a large negative value drives that diagonal element of the block negative)."""
    rng = np.random.default_rng(c["seed"])
    n, phi = c["n"], c["phi"]
    P = spd(n, c["seed"])
    nold = len(flat(c["old"]))
    Phi = rng.standard_normal((phi, nold)) * 10.0 ** rng.uniform(-2, 2, (1, nold))
    s = np.sqrt(np.diag(P)[c["start"]:c["start"] + phi])
    Qh = rng.standard_normal((phi, phi))
    Q = np.outer(s, s) * (Qh @ Qh.T) * 1e-2
    Q = np.triu(Q) + np.tril(rng.standard_normal((phi, phi)) * s.max() ** 2, -1)
    if qdiag is not None:
        Q[0, 0] = qdiag
    return P, Phi, Q


def prop_K(c):
    """Roundings per element.  Strip element (r outside the block): one dot product over the nold old columns, K = nold.  Block
    element: a dot product over nold terms plus Q (nold + 1) whose operands are strip values that carry nold roundings already:
    2 nold + 1, the issue's 2 nold + 2.  Every other element is a copy: K irrelevant (checked for equality)."""
    n, a, phi = c["n"], c["start"], c["phi"]
    nold = len(flat(c["old"]))
    K = np.zeros((n, n))
    K[a:a + phi, :] = nold
    K[:, a:a + phi] = nold
    K[a:a + phi, a:a + phi] = 2 * nold + 2
    return K


def prop_model(P, start, old, Phi, Q, q_lower=False, phi_transposed=False, skip=None):
    """EKFPropagation in plain float64 numpy; the flags are the mutations the bound has to catch."""
    old = np.asarray(old)
    if phi_transposed:
        Phi = Phi.T
    if skip is not None:
        Phi = Phi.copy()
        Phi[:, skip] = 0.0
    phi = Phi.shape[0]
    Qs = np.tril(Q) + np.tril(Q, -1).T if q_lower else np.triu(Q) + np.triu(Q, 1).T
    CPT = P[:, old] @ Phi.T
    PCP = Phi @ CPT[old, :] + Qs
    Pn = P.copy()
    Pn[start:start + phi, :] = CPT.T
    Pn[:, start:start + phi] = CPT
    Pn[start:start + phi, start:start + phi] = PCP
    return Pn


# ---- augment_dt ----------------------------------------------------------------------------------------------------------
def augment_cases():
    """dict(name, n, pose, dt, seed): the pose in front of dt and behind it, n 23 / 129 / 300, pose or dt at the last columns"""
    cases = [
        dict(name="behind_n23", n=23, pose=17, dt=15),
        dict(name="front_n23", n=23, pose=0, dt=22),
        dict(name="behind_n129", n=129, pose=123, dt=15),
        dict(name="front_n129", n=129, pose=30, dt=128),
        dict(name="behind_n300", n=300, pose=294, dt=15),
        dict(name="front_n300", n=300, pose=250, dt=256),
    ]
    for i, c in enumerate(cases):
        c["seed"] = 300 + i
    return cases


def augment_inputs(c):
    rng = np.random.default_rng(c["seed"])
    P = spd(c["n"], c["seed"])
    s = np.sqrt(np.diag(P))
    d = rng.standard_normal(6) * s[c["pose"]:c["pose"] + 6] / s[c["dt"]]  # a velocity: pose units per unit of dt
    return P, d


def augment_K(c):
    """Column step: P[r][pose+j] + P[r][dt] d_j, a product and an addition, K = 2; the row step the same on the pose rows, K = 2.
    In the 6 x 6 pose block the row step adds d_k x (row dt after the column step): the term P[dt][dt] d_j d_k passes through a
    product, an addition, a product and an addition, K = 4 (the issue's figure).  Everything else is untouched."""
    n, p = c["n"], c["pose"]
    K = np.zeros((n, n))
    K[:, p:p + 6] = 2
    K[p:p + 6, :] = 2
    K[p:p + 6, p:p + 6] = 4
    return K


def augment_model(P, pose, dt, d, stale_row=False):
    Pn = P.copy()
    row_before = Pn[dt, :].copy()
    Pn[:, pose:pose + 6] += np.outer(Pn[:, dt], d)
    Pn[pose:pose + 6, :] += np.outer(d, row_before if stale_row else Pn[dt, :])
    return Pn


# ---- initialize_invertible -------------------------------------------------------------------------------------------------
def init_cases():
    """dict(name, n, k, cols, ld, seed): k 1 / 3 / 6, columns non-contiguous and out of order, n 20 / 257 / 300, ld > k; R always
    has differing triangles"""
    cases = [
        dict(name="k1_n20", n=20, k=1, cols=[7, 2, 19, 11], ld=1),
        dict(name="k3_n20", n=20, k=3, cols=[16, 17, 18, 3, 4, 5, 0], ld=5),
        dict(name="k6_n20", n=20, k=6, cols=list(range(14, 20)) + list(range(0, 6)), ld=6),
        dict(name="k3_n257", n=257, k=3, cols=[256, 128, 127, 0, 200, 201, 202, 64, 65], ld=3),
        dict(name="k6_n257", n=257, k=6, cols=list(range(250, 256)) + [30, 31, 32, 33, 34, 35, 16, 17, 18, 19, 20, 21, 256], ld=8),
        dict(name="k1_n300", n=300, k=1, cols=[299, 0, 150], ld=4),
        dict(name="k6_n300", n=300, k=6, cols=list(range(294, 300)) + list(range(100, 106)) + list(range(16, 22)), ld=6),
    ]
    for i, c in enumerate(cases):
        c["seed"] = 500 + i
    return cases


def init_inputs(c):
    """(P, H_R, H_Linv, R): R = a symmetric positive part in its upper triangle, a different strictly lower one"""
    rng = np.random.default_rng(c["seed"])
    n, k, cols = c["n"], c["k"], np.asarray(c["cols"])
    P = spd(n, c["seed"])
    s = np.sqrt(np.diag(P))[cols]
    H_R = rng.standard_normal((k, len(cols))) / s[None, :]            # rows of order one in measurement units
    H_Linv = np.linalg.inv(rng.standard_normal((k, k)) + 2.0 * np.eye(k)) * 10.0 ** rng.uniform(-1, 1, (k, 1))
    Rh = rng.standard_normal((k, k))
    R = np.triu(Rh @ Rh.T + np.eye(k)) + np.tril(rng.standard_normal((k, k)) * 5.0, -1)
    return P, H_R, H_Linv, R


def init_K(c):
    """Cross block: M_a[r] is a dot product over the cols columns (cols roundings), then a dot product over k with H_Linv (k): the
    issue's cols + k + 2.  New block: M = H_R M_a[cols] + R (cols + 1 on operands that carry cols), then H_Linv M H_Linv^T as a
    sum of k^2 terms of two products each: the issue's 2 cols + k^2 + 3.  The old n x n block is untouched."""
    n, k, nc = c["n"], c["k"], len(c["cols"])
    K = np.zeros((n + k, n + k))
    K[:n, n:] = nc + k + 2
    K[n:, :n] = nc + k + 2
    K[n:, n:] = 2 * nc + k * k + 3
    return K


def init_model(P, cols, H_R, H_Linv, R, r_lower=False, no_sign=False, hinv_plain=False):
    cols = np.asarray(cols)
    n, k = P.shape[0], H_R.shape[0]
    M_a = P[:, cols] @ H_R.T
    M = H_R @ M_a[cols, :] + R
    M = np.tril(M) + np.tril(M, -1).T if r_lower else np.triu(M) + np.triu(M, 1).T
    Hl, Hr = (H_Linv.T, H_Linv) if hinv_plain else (H_Linv, H_Linv.T)
    Pn = np.zeros((n + k, n + k))
    Pn[:n, :n] = P
    Pn[n:, n:] = Hl @ M @ Hr
    Pn[:n, n:] = (1.0 if no_sign else -1.0) * (M_a @ Hr)
    Pn[n:, :n] = Pn[:n, n:].T
    return Pn


# ---- the jittered diagonal of a clone ------------------------------------------------------------------------------------------
def jitter_truth(v, jitter):
    """v (1 + jitter) and its companion; K = 2: the rounding of 1 + jitter and the product"""
    v = ld_ref.ld(v)
    return v * (1 + ld_ref.LD(jitter)), np.abs(v) * (1 + ld_ref.LD(jitter))


JITTER_K = 2
