"""The cases, derived rounding bounds and mutants of the propagate-and-clone tests (tests/test_propagate_cpu.py for the bounds
themselves, tests/test_propagate_gpu.py on the device).  The truth is tests/propagate_ref.py (long double); the metric is
|got - truth| / bound, element by element, a case passes at ratio <= 1.

The bounds.  u = 2^-53.  Every count is of roundings of a double-precision evaluation of the reference's formulas (k_propagate.hip,
the host mirror and the C oracle alike), fused or not, in any order.  Nothing is taken from a run of the code under test.  The
allowances of the device math library are SINCOS_ULPS = 2 ulp for sin and cos and SQRT_ULPS = 1 ulp for sqrt and a division, with
1 ulp <= 2 u |value|.  Vector errors are carried in the 2-norm, matrix errors element by element; a 2-norm bound of a vector (a
Frobenius bound of a matrix) bounds each of its elements.  The inputs (readings, IMU state, densities) are exact doubles.

Per interval, from the errors eq, ev, ep of the mean the interval starts from (zero for the first; the first estimates carry the
same errors from the second interval on, and none in the first):
  dt        a difference of two time stamps: 1 rounding.   w_hat, a_hat: one subtraction each, |d w| <= u |w|.
  R         R(q) is quadratic in q: |dR|_F <= (4 sqrt3 + 4 sqrt2 + 4) |dq| <= 17 eq for |q| <= 1; its own arithmetic rounds each
            diagonal element 6 times and each other one 3 times on terms <= 2: |.|_F <= 13 u; 60 u is allowed.   R_err = 17 eq + 60 u
  discrete  w = (w1 + w2) / 2: |dw| <= 2 u max|w_i|; |w|: the norm is 1-Lipschitz, its sum of squares and root cost 4 u |w|;
            theta = |w| dt / 2 three more; c0 = cos, s = sin: e_theta + 4 u |value|; c1 = s / |w|: e_s / |w| + |c1| e_|w| / |w| +
            2 u |c1| (the small-angle branch c0 = 1, c1 = dt / 2 costs u dt).  q' = M q with M = c0 I + c1 Omega(w), |M|_2 =
            sqrt(c0^2 + c1^2 |w|^2) = mu: e_raw = mu eq + (e_c0 + e_c1 |w| + |c1| e_w) |q| + 16 u (|c0| + 2 |c1| |w|) [8 roundings
            per component, 4 components].  The normalisation is a projection: first-order it does not expand the error; its own
            arithmetic costs 8 u:                                                              eq' = e_raw / |raw| + 8 u
            v' = v + R^T a dt - g dt: ev' = ev + dt (R_err |a| + e_a + 15 u |a|) + 4 u (|v| + |a| dt + g dt)
            p' likewise with dt ev, dt^2 / 2 of the R^T a term and 6 roundings on the sum of magnitudes.
  RK4       kappa = max|w| dt / 2 (< 0.1 asserted).  The four stages' k_q carry a = dt e_ws / 2 + 8 u kappa (e_ws = 5 u (|w1| +
            |w2|): the interpolated rate) and kappa x the error of the stage's dq, which is the previous k_q's plus 10 u; the
            recursion stays below 1.12 (a + 10 u kappa).  The final dq: e_dq = dt e_ws + 40 u kappa + 16 u; q' = dq (x) q keeps the
            2-norm: eq' = eq + e_dq + 24 u.  Each k_v = (R_s^T a_s - g) dt with R_s off by R_err(eq + e_dq + 34 u):
            e_kv = dt (R_s_err max|a| + e_as + 15 u max|a|) + 3 u dt (max|a| + g); ev' = ev + e_kv + 6 u (|v| + (max|a| + g) dt);
            ep' = ep + dt (ev + e_kv + 4 u (..)) + 6 u (|p| + dt (..)).
  F         Jr = Jl(w1 dt): the argument carries 3 u theta; s I: 10 u; (1 - s) a a^T: 10 u (the cancellation is absolute);
            c S(a) with c = (1 - cos theta) / theta: 6 u / theta - the reference's own formula loses that much:
            E_J = e_phi + 12 u + 6 u / theta (the identity below 1e-6 is exact).  Plain form: Rth = exp(-w1 dt): 2 e_phi + 12 u +
            10 u theta; RT = R^T: R_err(eq); V = RT skew(a dt), P = RT skew(a dt^2) / 2 as 3 x 3 products: 3 (EA Bmax + Amax EB) +
            15 u Amax Bmax per element.  FEJ form: Rth = R(q') R(q_fej)^T: 17 (eq' + eq_fej) + 130 u; av = v' - v_fej + g dt:
            ev' + ev_fej + 3 u (..); ap likewise with 6; V = skew(av) RT, P = skew(ap) RT as products.  The scaled blocks add the
            roundings of their scale (dt: 2, dt^2 / 2: 3, the p-v block dt I: 1).
  Qd        qc = sigma^2 / dt or sigma^2 dt: 3 roundings; (G qc) G^T has at most three terms of two products: with the
            symmetrisation 13 u on the companion |G| qc |G|^T, plus the blocks' own errors (E_G taken from E_F).
  Phi, Q    running: E_Phi' = |F| E_Phi + E_F |Phi| + E_F E_Phi + 13 u |F| |Phi| (a row of F has at most 12 non-zeros);
            T = F Q the same; T2 = T F^T + Qd: 14 u on |T| |F|^T + |Qd|; the mean of T2 and its transpose one more.
            The bounds grow with the interval count through this recursion.  Q must be symmetric to the bit (a zero bound).
  last_w    one subtraction.
The covariance: EKFPropagation's strips are 15-term sums (K = 15) of P and Phi, the block 2 x 15 + 2, on the companion
oracle/ld_ref.py returns, plus |P| E_Phi^T (and E_Phi |P| |Phi|^T + ... + E_Q in the block); the clone copies values and bounds;
the time-offset term adds K = 2 (4 in the new block) and the errors of dnc_dt = [last_w ; v]; a jittered diagonal 2 more.  K + 2
on every count and a factor 1 + 1e-6 on the carried errors cover gamma_K against K u and the second-order terms.  An element with
neither index in the IMU block or the new block has a zero bound: it must equal the input bit for bit."""
import numpy as np

import cov_bookkeeping_cases as B
import propagate_ref as R
from precision_helpers import spd_with
from oracle import ld_ref

LD = ld_ref.LD
COMBOS = [(rk4, avg, fej) for rk4 in (0, 1) for avg in (0, 1) for fej in (0, 1)]


def imu_scales():
    import zupt_cases

    return zupt_cases.imu_scales()


def capacities(n, clone):
    """n_max = exactly what the call needs and room to spare (700 is the largest context there is)"""
    need = n + (6 if clone else 0)
    return (need,) if need >= 700 else (need, need + 5)


def cases():
    """dict(name, n, imu_id, dt_id, readings, rk4, avg, fej, clone, kind, seed).  Readings 0, 1, 2, 3, 42 and 4096 (the kernel reads
    a reading where it needs it: there is no staging granularity to step over); one window whose every gyro reading equals the bias
    (the small-angle branches); all eight option combinations at 3 and at 42 readings; n = 16 (IMU + dt), 21 with the IMU block
    first and last, the clone across the 16- and 64-row borders (58, 63, 64), 694 -> 700; dt_id none, in front of and behind the
    IMU block; clone = 0."""
    # (k_prop_integrate reads each reading from global memory at the interval that needs it.  If the readings are ever staged in LDS
    #  in chunks, or the intervals combined over a tree, add a case one above each chunk / leaf count here, as zupt_cases.py has
    #  257 / 258.)
    cs = []
    for nr in (3, 42):
        for rk4, avg, fej in COMBOS:
            cs.append(dict(name="n21_r%d_rk%d_avg%d_fej%d" % (nr, rk4, avg, fej), n=21, imu_id=0 if fej else 6, dt_id=20 if fej else 0,
                           readings=nr, rk4=rk4, avg=avg, fej=fej))
    cs += [
        dict(name="n16_r0", n=16, imu_id=0, dt_id=15, readings=0, rk4=1, avg=0, fej=1),
        dict(name="n16_r1", n=16, imu_id=1, dt_id=0, readings=1, rk4=1, avg=0, fej=1),
        dict(name="n16_r2", n=16, imu_id=0, dt_id=15, readings=2, rk4=0, avg=1, fej=0),
        dict(name="n21_r42_small_angle", n=21, imu_id=0, dt_id=17, readings=42, rk4=0, avg=1, fej=0, kind="bias"),
        dict(name="n21_r42_small_angle_rk4", n=21, imu_id=6, dt_id=3, readings=42, rk4=1, avg=0, fej=1, kind="bias"),
        dict(name="n21_r42_last_nodt", n=21, imu_id=6, dt_id=-1, readings=42, rk4=1, avg=0, fej=1),
        dict(name="n21_r42_noclone", n=21, imu_id=0, dt_id=20, readings=42, rk4=1, avg=0, fej=1, clone=0),
        dict(name="n58_r42", n=58, imu_id=0, dt_id=21, readings=42, rk4=1, avg=0, fej=1),
        dict(name="n63_r42", n=63, imu_id=40, dt_id=2, readings=42, rk4=0, avg=0, fej=1),
        dict(name="n64_r3", n=64, imu_id=49, dt_id=-1, readings=3, rk4=1, avg=1, fej=0),
        dict(name="n64_r42", n=64, imu_id=0, dt_id=63, readings=42, rk4=1, avg=0, fej=1),
        dict(name="n694_r42", n=694, imu_id=0, dt_id=21, readings=42, rk4=1, avg=0, fej=1),
        dict(name="n694_r4096", n=694, imu_id=679, dt_id=5, readings=4096, rk4=0, avg=1, fej=1),
        dict(name="n64_r4096_rk4", n=64, imu_id=0, dt_id=15, readings=4096, rk4=1, avg=0, fej=0),
    ]
    for i, c in enumerate(cs):
        c.setdefault("clone", 1)
        c.setdefault("kind", "moving")
        c["seed"] = 900 + i
    return cs


def options(c):
    from ov_plane_amd.synth import PROP_OPTS

    return dict(PROP_OPTS, use_rk4=c["rk4"], imu_avg=c["avg"], do_fej=c["fej"])


_X = {}


def imu_state():
    """the IMU estimate of the zero-velocity scenario (moving): value, biases and distinct first estimates"""
    if not _X:
        import zupt_ref

        x = zupt_ref.scenario(False)[0]
        _X.update({k: np.array(x[k], dtype=np.float64) for k in ("q", "p", "v", "bg", "ba", "q_fej", "p_fej", "v_fej")})
    return _X


def make_readings(count, kind, seed):
    """[count, 7] rows (t, w, a): time stamps near 100 s, 400 Hz with +-40 % jitter (count = 3: 40 us and 4.1 ms; 4096: 50 us
    steps, a window of 0.2 s); a slow sine on bias + gravity + sensor noise; kind "bias": every gyro reading equals b_g exactly"""
    rng = np.random.default_rng(seed)
    x = imu_state()
    if count == 0:
        return np.zeros((0, 7))
    step = 5.0e-5 if count > 1000 else 2.5e-3
    dt = step * (1.0 + 0.4 * rng.uniform(-1.0, 1.0, max(count - 1, 0)))
    if count == 3:
        dt = np.array([4.0e-5, 4.1e-3])
    t = 100.004 + np.concatenate([[0.0], np.cumsum(dt)])
    rd = np.zeros((count, 7))
    rd[:, 0] = t
    ph = rng.uniform(0, 2 * np.pi, 6)
    from ov_plane_amd.synth import quat_2_rot

    Rg = quat_2_rot(x["q"]) @ np.array([0.0, 0.0, 9.81])
    for k in range(3):
        rd[:, 1 + k] = 0.35 * np.sin(2 * np.pi * 0.7 * (t - t[0]) + ph[k]) + x["bg"][k]
        rd[:, 4 + k] = 0.6 * np.sin(2 * np.pi * 1.1 * (t - t[0]) + ph[3 + k]) + x["ba"][k] + Rg[k]
    rd[:, 1:4] += 1.7e-4 * np.sqrt(400.0) * rng.standard_normal((count, 3))
    rd[:, 4:7] += 2.0e-3 * np.sqrt(400.0) * rng.standard_normal((count, 3))
    if kind == "bias":
        rd[:, 1:4] = x["bg"]
    assert count < 2 or (np.diff(rd[:, 0]) > 0).all()
    return rd


_INPUTS, _TRUTH = {}, {}


def inputs(c):
    """(P, readings) of a case; P: spd_with the IMU columns at the parity scene's scales, the others over eight decades"""
    if c["name"] not in _INPUTS:
        P = spd_with(c["n"], c["seed"], c["imu_id"] + np.arange(15), imu_scales())
        _INPUTS[c["name"]] = (P, make_readings(c["readings"], c["kind"], c["seed"]))
    return _INPUTS[c["name"]]


def truth(c, jitter=0.0):
    """(t, P_truth, P_bound) of a case, computed once: t = propagate_ref.integrate (values and bounds)"""
    key = (c["name"], jitter)
    if key not in _TRUTH:
        P, rd = inputs(c)
        k0 = (c["name"], 0.0)
        t = _TRUTH[k0][0] if k0 in _TRUTH else R.integrate(imu_state(), options(c), rd)
        Pt, Bp = R.covariance(P, c["imu_id"], t, bool(c["clone"]), c["dt_id"], jitter)
        _TRUTH[key] = (t, Pt, Bp)
    return _TRUTH[key]


def _abs_ratio(got, tr, bound):
    """max |got - truth| / bound; an element with a zero bound must be exact (inf otherwise)"""
    err = np.abs(np.asarray(got, dtype=LD) - tr)
    bound = np.broadcast_to(np.asarray(bound, dtype=LD), err.shape)
    r = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, 1))
    r = np.where((bound == 0) & (err > 0), np.inf, r)
    return float(np.max(r)) if r.size else 0.0


def ratios(c, got, P=None, jitter=0.0):
    """error / bound of a result got = dict(q, p, v, last_w, Phi, Q) and (optionally) the covariance: dict(q, p, v, last_w, Phi, Q,
    Qsym[, P]).  Qsym: the antisymmetric part of Q against a zero bound."""
    t, Pt, Bp = truth(c, jitter)
    b = t["b"]
    Q = np.asarray(got["Q"])
    r = dict(q=_abs_ratio(got["q"], t["q"], b["q"]), p=_abs_ratio(got["p"], t["p"], b["p"]), v=_abs_ratio(got["v"], t["v"], b["v"]),
             last_w=_abs_ratio(got["last_w"], t["last_w"], b["last_w"]), Phi=_abs_ratio(got["Phi"], t["Phi"], b["Phi"]),
             Q=_abs_ratio(Q, t["Q"], b["Q"]), Qsym=0.0 if (Q == Q.T).all() else np.inf)
    if P is not None:
        r["P"] = _abs_ratio(P, Pt, Bp)
    return r


def worst(r):
    return max(r.values())


# ---- the double-precision chain and its mutants --------------------------------------------------------------------------------
MUTANTS = ("drop_interval", "avg_flipped", "no_sym", "float32", "old_velocity", "rows_only")


def chain(c, summed, mutant=None):
    """EKFPropagation -> copy -> time-offset term in plain float64 (oracle.np_ref) on a summed result dict(x | q p v, Phi, Q, last_w),
    with one fault:
      float32       Phi, Q rounded to float32
      old_velocity  dnc_dt built from the velocity the window started from
      rows_only     the time-offset term applied to the rows only
    (drop_interval, avg_flipped, no_sym live in the integration: see summed_double).  Returns (got, P)."""
    from oracle import np_ref

    P, _ = inputs(c)
    n, imu = c["n"], c["imu_id"]
    Phi, Q = np.array(summed["Phi"], dtype=np.float64), np.array(summed["Q"], dtype=np.float64)
    if mutant == "float32":
        Phi, Q = Phi.astype(np.float32).astype(np.float64), Q.astype(np.float32).astype(np.float64)
    got = dict(q=summed["q"], p=summed["p"], v=summed["v"], last_w=summed["last_w"], Phi=Phi, Q=Q)
    order = [(imu, 15)]
    Pn = np_ref.ekf_propagation(P, imu, 15, order, Phi, Q)
    if c["clone"]:
        idx = np.concatenate([np.arange(n), imu + np.arange(6)])
        Pn = Pn[np.ix_(idx, idx)].copy()
        if c["dt_id"] >= 0:
            v = imu_state()["v"] if mutant == "old_velocity" else np.asarray(summed["v"], dtype=np.float64)
            d = np.concatenate([np.asarray(summed["last_w"], dtype=np.float64), v])
            if mutant != "rows_only":
                Pn[:, n:n + 6] += np.outer(Pn[:, c["dt_id"]], d)
            Pn[n:n + 6, :] += np.outer(d, Pn[c["dt_id"], :])
    return got, Pn


def summed_double(c, mutant=None):
    """the summed result of a case in double precision with a fault of the integration (the truth's own loop, rounded to double at
    the end - a fault moves the value by many orders of magnitude more than that rounding):
      drop_interval  the middle interval missing;  avg_flipped  imu_avg the other way;  no_sym  neither symmetrisation"""
    _, rd = inputs(c)
    po = options(c)
    if mutant == "avg_flipped":
        po["imu_avg"] = 0 if po["imu_avg"] else 1
    t = R.integrate(imu_state(), po, rd, mutate=mutant if mutant in ("drop_interval", "no_sym") else None)
    f = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    return dict(q=f(t["q"]), p=f(t["p"]), v=f(t["v"]), last_w=f(t["last_w"]), Phi=f(t["Phi"]), Q=f(t["Q"]))
