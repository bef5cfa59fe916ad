"""The cases, derived rounding bounds and plain float64 models of the zero-velocity precision tests
(tests/test_zupt_precision_gpu.py on the device, tests/test_ld_ref_cpu.py for the bounds themselves).  The truth is
oracle/ld_ref.py::zupt_compressed; the metric is cov_bookkeeping_cases.ratio, element by element, a case passes at ratio <= 1.

The bounds.  u = 2^-53, ni = intervals, every count is of roundings of the device's arithmetic (k_zupt.hip and the parameter block
ovp_zupt_update stages), fused or not, in any order; + 2 on every count covers gamma_K versus K u and the truth's own rounding, as in
cov_bookkeeping_cases.py.  Nothing is taken from a run of the code under test.

  r_i       a gyro component is one subtraction, an accelerometer component (m - b_a) - R g with R g a rounded product: 3 roundings,
            each relative to an operand no larger than rho_i = |m| + |b| + |R g|:                                |d r_i| <= 3 u rho_i
  rbar      (sum dt_i r_i) / T: ni fused additions relative to sum dt_i |r_i| <= sum dt_i rho_i, the inputs' 3, T's own ni (dt_i
            is exact: neighbouring time stamps), the division:                          |d rbar| <= (2 ni + 4) u rhobar =: d_rbar
  scatter   e_i = r_i - rbar carries 3 + (2 ni + 4) + 1 roundings relative to w_i = rho_i + rhobar, so e_i^2 is off by
            2 |e_i| eps_i + eps_i^2 with eps_i = (2 ni + 8) u w_i; the sum itself is an ordinary dot product of ni terms whose
            factors carry 3 (the chain of three squares) + 2 (the two weights) + 3 (D = 1 / (mult sigma^2) on the host) roundings:
            |d scatter| <= (ni + 8) u scatter + 2 (2 ni + 8) u scatter_lin + ((2 ni + 8) u)^2 scatter_sq
  Sbar      two nested 9-term sums (18), the addition of Q_bias on a bias diagonal (1) and of Rbar (1): 20 u comp.Sbar.  The parts
            that are multiples of the summed T carry its ni roundings as well: Q_bias = T q (ni + 1), Rbar = 1 / (T D) (ni + 3 + 2):
            (ni + 5) u comp.SbarT.  In the 2-norm (<= Frobenius), with the factorization's backward error gamma_7 |L| |L|^T, whose
            norm is <= trace(Sbar) <= 6 lam_max:
            |d Sbar|_2 <= eps_S lam_max,  eps_S = ((20 |comp.Sbar|_F + (ni + 5) |comp.SbarT|_F) / lam_max + 42) u
  z, |z|^2  z = L^-1 rbar.  A perturbation dS of Sbar moves L^-1 by L^-1 dL L^-1 with |L^-1 dL|_F <= |L^-1 dS L^-T|_F <= sqrt(6) eps_S
            kappa (first order; kappa = lam_max / lam_min); the substitution's backward error gamma_6 |L| adds |L^-1| |L| <= 6
            sqrt(kappa) <= 6 kappa times 6 u; the error of rbar enters through |L^-1|_2 = lam_min^-1/2:
            |d z|_2 <= |d_rbar|_2 / sqrt(lam_min) + (sqrt(6) eps_S + 36 u) kappa |z|_2 =: dz;  |d z^T z| <= 2 |z| dz + dz^2 + 8 u |z|^2
  chi2      the two parts and their sum:                                          |d chi2| <= d scatter + d |z|^2 + 2 u chi2
  Y         The device forms Li = L^-1 explicitly, column by column, then G = H0^T Li^T and Y = P'_{:,s} G.  Each column of Li
            solves (L + dL_c) x = e_c with |dL_c| <= gamma_6 |L|, so Li = (I + F) L^-1 with |F| <= gamma_6 |L^-1| |L| |L^-1| |L| and
            |F|_2 <= 6 u (6 sqrt(kappa))^2 = 216 u kappa: the explicit inverse costs a constant, NOT a second factor of kappa, because
            Y is only ever used as Y Y^T and Y z, where L^-T (I + F)^T (I + F) L^-1 perturbs Sbar^-1 the way dS does.  The sums
            of G (6 terms) and Y (9 terms) are within 15 u of |P'_{:,s}| |H0|^T |Li|^T, row i of which is at most
            sqrt(6) |comp.M_i|_2 / sqrt(lam_min) =: c_i in norm; the addition of Q_bias on a bias row is one more, and its T q
            brings (ni + 1) u T q_i |G|_2 <= (ni + 1) u T q_i sqrt(6 / lam_min) =: t_i.  With a_i = |Y_i|_2:
            |d Y_i|_2 <= phi a_i + 16 u c_i + t_i =: d_i,  phi = (sqrt(6) eps_S + 216 u) kappa
  dx        dx_i = Y_i . z (6 fused terms):                          |d dx_i| <= d_i |z| + a_i dz + d_i dz + 8 u a_i |z|
  P+        P'_ij - Y_i . Y_j: the difference, the addition of Q_bias and the 6-term product sum are within 9 u of comp.P = |P'| +
            |Y| |Y|^T, a bias diagonal carries (ni + 1) u T q_i more; the errors of Y enter norm-wise, so the kappa part multiplies
            a_i a_j >= (|Y| |Y|^T)_ij:              |d P+_ij| <= 9 u comp.P_ij (+ (ni + 1) u T q_i) + d_i a_j + a_i d_j + d_i d_j
A rejected call is held to the chi2 bound, a covariance equal to the input bit for bit and a zero dx."""
import numpy as np

import cov_bookkeeping_cases as B
import zupt_ref as Z
from precision_helpers import capacities, spd_with  # noqa: F401
from oracle import ld_ref, np_ref

LD = ld_ref.LD
U = B.U
SIZES = (15, 16, 17, 65, 129, 257, 700)
MARGIN = 1e-9  # the truth's chi2 of a gated case lies outside thr (1 -+ MARGIN)


_IMU_SCALES = []


def imu_scales():
    """standard deviations of the 15 IMU columns of the covariance the parity tests use (make_scene(...).P)"""
    if not _IMU_SCALES:
        from ov_plane_amd.synth import make_scene

        _IMU_SCALES.append(np.sqrt(np.diag(make_scene(C=2, F=4, seed=91).P)[:15]).copy())
    return _IMU_SCALES[0]


def cases():
    """dict(name, n, imu_id, readings, kind, seed).  kind: accept (standing, chi2 passes) | reject_chi2 (moving) | reject_vel
    (standing, vel_ok = False) | forced (moving, disparity_passed).  Every size with imu_id 0 or n - 15 (both at n = 15), one block
    across column 64 and one across row 64 of the row blocks (imu_id = 57 at n = 129, 50 at n = 65); 257 / 258 readings on either
    side of one interval per thread of the gate, 4096 the limit, 3 readings with dt = 40 us and 4.1 ms."""
    cs = [
        dict(name="n15_r2_accept", n=15, imu_id=0, readings=2, kind="accept"),
        dict(name="n16_r3_unequal_accept", n=16, imu_id=1, readings=3, kind="accept"),
        dict(name="n17_r42_reject_chi2", n=17, imu_id=0, readings=42, kind="reject_chi2"),
        dict(name="n17_r42_forced", n=17, imu_id=2, readings=42, kind="forced"),
        dict(name="n65_r42_reject_vel", n=65, imu_id=50, readings=42, kind="reject_vel"),
        dict(name="n65_r258_accept", n=65, imu_id=50, readings=258, kind="accept"),
        dict(name="n129_r257_across64_accept", n=129, imu_id=57, readings=257, kind="accept"),
        dict(name="n129_r258_end_forced", n=129, imu_id=114, readings=258, kind="forced"),
        dict(name="n257_r258_front_accept", n=257, imu_id=0, readings=258, kind="accept"),
        dict(name="n257_r257_end_reject_chi2", n=257, imu_id=242, readings=257, kind="reject_chi2"),
        dict(name="n257_r42_end_accept", n=257, imu_id=242, readings=42, kind="accept"),
        dict(name="n700_r4096_end_accept", n=700, imu_id=685, readings=4096, kind="accept"),
        dict(name="n700_r42_front_forced", n=700, imu_id=0, readings=42, kind="forced"),
        dict(name="n700_r4096_front_reject_chi2", n=700, imu_id=0, readings=4096, kind="reject_chi2"),
    ]
    for i, c in enumerate(cs):
        c["seed"] = 700 + i
    return cs


_X = {}


def imu_state():
    """the IMU estimate of zupt_ref.scenario (standing): rotation, its first estimate, the biases"""
    if not _X:
        x = Z.scenario(True)[0]
        R, Rj = Z.rotations(x, Z.PO["do_fej"])
        _X.update(R=R, Rj=Rj, bg=np.array(x["bg"]), ba=np.array(x["ba"]))
    return _X


def make_readings(count, moving, seed):
    """[count, 7] rows (t, w, a): time stamps near 100 s, 400 Hz with +-40 % jitter (count = 3: 40 us and 4.1 ms); standing: bias +
    gravity + sensor noise; moving: a slow sine on top, as make_imu_scenario has it"""
    rng = np.random.default_rng(seed)
    x = imu_state()
    dt = 2.5e-3 * (1.0 + 0.4 * rng.uniform(-1.0, 1.0, count - 1))
    if count == 3:
        dt = np.array([4.0e-5, 4.1e-3])
    t = 100.004 + np.concatenate([[0.0], np.cumsum(dt)])
    rd = np.zeros((count, 7))
    rd[:, 0] = t
    amp = 1.0 if moving else 0.0
    ph = rng.uniform(0, 2 * np.pi, 6)
    for k in range(3):
        rd[:, 1 + k] = amp * 0.35 * np.sin(2 * np.pi * 0.7 * (t - t[0]) + ph[k]) + x["bg"][k]
        rd[:, 4 + k] = amp * 0.6 * np.sin(2 * np.pi * 1.1 * (t - t[0]) + ph[3 + k]) + x["ba"][k]
    rd[:, 4:7] += x["R"] @ np.array([0.0, 0.0, Z.PO["gravity_mag"]])
    rd[:, 1:4] += 1.7e-4 * np.sqrt(400.0) * rng.standard_normal((count, 3))
    rd[:, 4:7] += 2.0e-3 * np.sqrt(400.0) * rng.standard_normal((count, 3))
    assert (np.diff(rd[:, 0]) > 0).all()
    return rd


_INPUTS = {}


def inputs(c):
    """(P, readings, keyword arguments of the decision) of a case; P: spd_with the IMU columns at the parity scene's scales"""
    if c["name"] not in _INPUTS:
        P = spd_with(c["n"], c["seed"], c["imu_id"] + np.arange(15), imu_scales())
        rd = make_readings(c["readings"], c["kind"] in ("reject_chi2", "forced"), c["seed"])
        kw = dict(vel_ok=c["kind"] != "reject_vel", disparity_passed=c["kind"] == "forced")
        _INPUTS[c["name"]] = (P, rd, kw)
    return _INPUTS[c["name"]]


def threshold(c):
    return np_ref.chi2_095(6 * (c["readings"] - 1))


def expected(c):
    return c["kind"] in ("accept", "forced")


_TRUTH = {}


def truth(c):
    """(truth, companion, bounds) of a case, computed once"""
    if c["name"] not in _TRUTH:
        P, rd, _ = inputs(c)
        x = imu_state()
        t, comp = ld_ref.zupt_compressed(P, rd, c["imu_id"], x["R"], x["Rj"], x["bg"], x["ba"], Z.PO, Z.NOISE_MULT)
        _TRUTH[c["name"]] = (t, comp, bounds(c, t, comp))
    return _TRUTH[c["name"]]


def decision(c, chi2):
    _, _, kw = inputs(c)
    return bool(kw["disparity_passed"] or (chi2 <= threshold(c) and kw["vel_ok"]))


def bounds(c, t, comp):
    """dict(chi2, dx [n], P [n, n]): the weighted companions W of the module docstring, in units of u: a value passes when
    ratio(got, truth, W, -1) = max |got - truth| / (u W) <= 1"""
    u = LD(U)
    ni = c["readings"] - 1
    n = c["n"]
    kappa, lam_min, lam_max = LD(t["kappa"]), LD(t["lam_min"]), LD(t["lam_max"])
    nz = np.sqrt(t["z"] @ t["z"])
    d_rbar = (2 * ni + 4 + 2) * u * comp["rbar"]
    ke = (2 * ni + 8 + 2) * u
    d_scatter = (ni + 8 + 2) * u * t["scatter"] + 2 * ke * comp["scatter_lin"] + ke * ke * comp["scatter_sq"]
    fro = lambda A: np.sqrt((A ** 2).sum())  # noqa: E731
    eps_S = (((20 + 2) * fro(comp["Sbar"]) + (ni + 5 + 2) * fro(comp["SbarT"])) / lam_max + 42) * u
    dz = np.sqrt(d_rbar @ d_rbar) / np.sqrt(lam_min) + (np.sqrt(LD(6)) * eps_S + 36 * u) * kappa * nz
    d_zz = 2 * nz * dz + dz * dz + (8 + 2) * u * nz * nz
    b_chi2 = d_scatter + d_zz + (2 + 2) * u * t["chi2"]
    phi = (np.sqrt(LD(6)) * eps_S + 216 * u) * kappa
    a = np.sqrt((t["Y"] ** 2).sum(axis=1))
    cn = np.sqrt(LD(6)) * np.sqrt((comp["M"] ** 2).sum(axis=1)) / np.sqrt(lam_min)
    bias = c["imu_id"] + np.arange(9, 15)
    tq = np.zeros(n, dtype=LD)
    tq[bias] = (ni + 1 + 2) * u * t["Tq"]
    d = phi * a + (16 + 2) * u * cn + tq * np.sqrt(LD(6) / lam_min)
    b_dx = d * nz + a * dz + d * dz + (8 + 2) * u * a * nz
    b_P = (9 + 2) * u * comp["P"] + np.diag(tq) + np.outer(d, a) + np.outer(a, d) + np.outer(d, d)
    return dict(chi2=b_chi2 / u, dx=b_dx / u, P=b_P / u)


def ratios(c, chi2, dx, P):
    """(chi2, dx, P) error / bound of an accepted result; of a rejected one pass dx = P = None"""
    t, _, b = truth(c)
    r = [B.ratio(np.array([chi2]), np.array([t["chi2"]]), np.array([b["chi2"]]), -1)]
    if dx is not None:
        r += [B.ratio(dx, t["dx"], b["dx"], -1), B.ratio(P, t["P"], b["P"], -1)]
    return r


# ---- the plain float64 model and its faults ----------------------------------------------------------------------------------
FAULTS = ("q_missing", "q_squared", "mirror_stale", "tile_row", "drop_rbar", "drop_scatter")


def model(c, fault=None):
    """The compressed update in plain float64, as the kernels split it (gate, rows, tiles of 16 x 16), with one fault:
    q_missing     Q_bias missing on the first bias diagonal element (in the tiles' own addition)
    q_squared     Q_bias = T sigma^2 instead of T sigma
    mirror_stale  the mirror image of lower tile (1, 0) keeps the input's values
    tile_row      the tiles b >= 120 of the row-by-row numbering take the rows of Y one tile row up
    drop_rbar     intervals >= 256 missing from T and rbar
    drop_scatter  intervals >= 256 missing from the scatter
    Returns dict(accepted, chi2, dx, P)."""
    from ov_plane_amd.synth import skew

    P, rd, kw = inputs(c)
    x, po = imu_state(), Z.PO
    n, imu_id = c["n"], c["imu_id"]
    dt = np.diff(rd[:, 0])
    g = np.array([0.0, 0.0, po["gravity_mag"]])
    r = -np.concatenate([rd[:-1, 1:4] - x["bg"], rd[:-1, 4:7] - x["ba"] - x["R"] @ g], axis=1)
    T = dt.sum()
    first = slice(0, 256)
    if fault == "drop_rbar":
        T = dt[first].sum()
        rbar = (dt[first, None] * r[first]).sum(axis=0) / T
    else:
        rbar = (dt[:, None] * r).sum(axis=0) / T
    D = np.concatenate([np.full(3, 1.0 / (Z.NOISE_MULT * po["sigma_w"] ** 2)), np.full(3, 1.0 / (Z.NOISE_MULT * po["sigma_a"] ** 2))])
    terms = dt[:, None] * (r - rbar) ** 2 * D
    scatter = float(terms[first].sum() if fault == "drop_scatter" else terms.sum())
    sig = np.concatenate([np.full(3, po["sigma_wb"]), np.full(3, po["sigma_ab"])])
    q = T * (sig ** 2 if fault == "q_squared" else sig)
    s = Z.imu_cols(imu_id)
    Pp = P.copy()
    Pp[s[3:], s[3:]] += q
    H0 = np.zeros((6, 9))
    H0[0:3, 3:6] = -np.eye(3)
    H0[3:6, 0:3] = -skew(x["Rj"] @ g)
    H0[3:6, 6:9] = -np.eye(3)
    Sbar = H0 @ Pp[np.ix_(s, s)] @ H0.T + np.diag(1.0 / (T * D))
    L = np.linalg.cholesky(Sbar)
    z = np.linalg.solve(L, rbar)
    chi2 = scatter + float(z @ z)
    acc = bool(kw["disparity_passed"] or (chi2 <= threshold(c) and kw["vel_ok"]))
    if not acc:
        return dict(accepted=False, chi2=chi2, dx=np.zeros(n), P=P.copy())
    Y = Pp[:, s] @ (H0.T @ np.linalg.inv(L).T)
    Pq = Pp.copy()
    if fault == "q_missing":
        Pq[s[3], s[3]] = P[s[3], s[3]]
    out = Pq - Y @ Y.T
    if fault == "tile_row":
        nt = (n + 15) // 16
        b = 0
        for bi in range(nt):
            for bj in range(bi + 1):
                if b >= 120:
                    i0, j0 = 16 * bi, 16 * bj
                    rows = np.arange(i0, min(i0 + 16, n))
                    cols = np.arange(j0, min(j0 + 16, n))
                    blk = Pq[np.ix_(rows, cols)] - Y[rows - 16] @ Y[cols].T
                    out[np.ix_(rows, cols)] = blk
                    out[np.ix_(cols, rows)] = blk.T
                b += 1
    if fault == "mirror_stale" and n > 16:
        rows, cols = np.arange(16, min(32, n)), np.arange(0, 16)
        out[np.ix_(cols, rows)] = P[np.ix_(cols, rows)]
    return dict(accepted=True, chi2=chi2, dx=Y @ z, P=out)
