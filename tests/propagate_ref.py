"""Long-double truth of ovp_propagate_and_clone (Propagator::propagate_and_clone behind its preamble): predict_and_compute in all
eight option combinations, the summed Phi and Q, last_w, then oracle/ld_ref.py's EKFPropagation, the exact copy of the pose block
and the time-offset term.  Everything computes in np.longdouble from double inputs; nothing is rounded to double before the end.

integrate() carries, beside every truth value, a bound on the rounding error of a double-precision evaluation of the same formulas
(the derivation is in tests/propagate_cases.py); the bounds are absolute and already hold the factor u = 2^-53."""
import numpy as np

from oracle import ld_ref

LD = np.longdouble
U = LD(2.0) ** -53
SINCOS_ULPS = 2   # device library: sin, cos within 2 ulp, 1 ulp <= 2 u |value|
SQRT_ULPS = 1     # sqrt (and a division) within 1 ulp
S4 = 2 * SINCOS_ULPS * U   # relative allowance of one sin / cos
TH, PP, VV, BG, BA = slice(0, 3), slice(3, 6), slice(6, 9), slice(9, 12), slice(12, 15)


def ld(a):
    return np.asarray(a, dtype=LD)


def skew(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=LD)


def norm(v):
    return np.sqrt((ld(v) ** 2).sum())


def q2R(q):
    x, y, z, w = q
    a = 2 * w * w - 1
    return np.array([[a + 2 * x * x, 2 * w * z + 2 * x * y, -2 * w * y + 2 * x * z],
                     [-2 * w * z + 2 * y * x, a + 2 * y * y, 2 * w * x + 2 * y * z],
                     [2 * w * y + 2 * z * x, -2 * w * x + 2 * z * y, a + 2 * z * z]], dtype=LD)


def quatnorm(q):
    assert abs(q[3]) > 1e-3, "a scalar part this close to zero makes the sign flip a coin toss"
    q = -q if q[3] < 0 else q
    return q / norm(q)


def omega_times(w, q):
    return np.array([w[2] * q[1] - w[1] * q[2] + w[0] * q[3], -w[2] * q[0] + w[0] * q[2] + w[1] * q[3],
                     w[1] * q[0] - w[0] * q[1] + w[2] * q[3], -w[0] * q[0] - w[1] * q[1] - w[2] * q[2]], dtype=LD)


def quat_mul(q, p):
    x, y, z, w = q
    return quatnorm(np.array([w * p[0] + z * p[1] - y * p[2] + x * p[3], -z * p[0] + w * p[1] + x * p[2] + y * p[3],
                              y * p[0] - x * p[1] + w * p[2] + z * p[3], -x * p[0] - y * p[1] - z * p[2] + w * p[3]], dtype=LD))


def _clear_of(th, limit):
    assert th == 0 or abs(float(th) / limit - 1.0) > 1e-6, "an angle on a branch threshold"


def exp_so3(w):
    S = skew(w)
    th = norm(w)
    _clear_of(th, 1e-7)
    A = LD(1) if th < 1e-7 else np.sin(th) / th
    B = LD(0.5) if th < 1e-7 else (1 - np.cos(th)) / (th * th)
    return np.eye(3, dtype=LD) + A * S + B * (S @ S)


def jl_so3(w):
    th = norm(w)
    _clear_of(th, 1e-6)
    if th < 1e-6:
        return np.eye(3, dtype=LD)
    a = w / th
    s, c = np.sin(th) / th, (1 - np.cos(th)) / th
    return s * np.eye(3, dtype=LD) + (1 - s) * np.outer(a, a) + c * skew(a)


def predict_mean(x, po, dt, w1, a1, w2, a2):
    """Propagator::predict_mean_discrete / predict_mean_rk4 (:456-602).  Returns (q, v, p)."""
    g = np.array([0, 0, po["gravity_mag"]], dtype=LD)
    q0, p0, v0 = x["q"], x["p"], x["v"]
    if not po["use_rk4"]:
        w, a = ((w1 + w2) / 2, (a1 + a2) / 2) if po["imu_avg"] else (w1, a1)
        wn = norm(w)
        assert wn == 0 or wn > 1e-15
        c0 = np.cos(wn * dt / 2) if wn > 1e-20 else LD(1)
        c1 = np.sin(wn * dt / 2) / wn if wn > 1e-20 else dt / 2
        Rta = q2R(q0).T @ a
        return quatnorm(c0 * q0 + c1 * omega_times(w, q0)), v0 + Rta * dt - g * dt, p0 + v0 * dt + Rta * dt * dt / 2 - g * dt * dt / 2
    wal, aj = (w2 - w1) / dt, (a2 - a1) / dt
    dq0 = np.array([0, 0, 0, 1], dtype=LD)
    kq, kp, kv = [], [], []
    w, a = w1, a1
    for s, frac in enumerate((LD(0), LD(0.5), LD(0.5), LD(1))):
        if s in (1, 3):
            w, a = w + wal * dt / 2, a + aj * dt / 2
        dq = quatnorm(dq0 + frac * kq[-1]) if s else dq0
        vs = v0 + frac * kv[-1] if s else v0
        R = q2R(quat_mul(dq, q0))
        kq.append(omega_times(w, dq) * dt / 2)
        kp.append(vs * dt)
        kv.append((R.T @ a - g) * dt)
    c = (LD(1) / 6, LD(1) / 3, LD(1) / 3, LD(1) / 6)
    dq = quatnorm(dq0 + sum(ci * k for ci, k in zip(c, kq)))
    return quat_mul(dq, q0), v0 + sum(ci * k for ci, k in zip(c, kv)), p0 + sum(ci * k for ci, k in zip(c, kp))


def blocks_of(x, po, dt, w1, a1, nq, nv, npos):
    """the 3 x 3 blocks of F (Propagator.cpp:379-432): dict(Rth, RJ, RT, Vth [F[v, th] = -Vth], Pth [F[p, th] = pscale Pth],
    pscale, Jr, av, ap)"""
    g = np.array([0, 0, po["gravity_mag"]], dtype=LD)
    Jr = jl_so3(w1 * dt)   # Jr(-w dt) = Jl(w dt)
    if po["do_fej"]:
        RT = q2R(x["q_fej"]).T
        Rth = q2R(nq) @ RT
        av = nv - x["v_fej"] + g * dt
        ap = npos - x["p_fej"] - x["v_fej"] * dt + g * dt * dt / 2
        Vth, Pth, ps = skew(av) @ RT, skew(ap) @ RT, LD(-1)
    else:
        RT = q2R(x["q"]).T
        Rth = exp_so3(-w1 * dt)
        av, ap = a1 * dt, a1 * dt * dt
        Vth, Pth, ps = RT @ skew(av), RT @ skew(ap), LD(-0.5)
    return dict(Rth=Rth, RJ=Rth @ Jr, RT=RT, Vth=Vth, Pth=Pth, pscale=ps, Jr=Jr, av=av, ap=ap)


def assemble(b, dt, po):
    """(F, G, qc) from the blocks"""
    F, G = np.zeros((15, 15), dtype=LD), np.zeros((15, 12), dtype=LD)
    I = np.eye(3, dtype=LD)
    F[TH, TH], F[TH, BG] = b["Rth"], -dt * b["RJ"]
    F[VV, TH], F[VV, BA] = -b["Vth"], -dt * b["RT"]
    F[PP, TH], F[PP, BA], F[PP, VV] = b["pscale"] * b["Pth"], -dt * dt / 2 * b["RT"], dt * I
    F[BG, BG] = F[BA, BA] = F[VV, VV] = F[PP, PP] = I
    G[TH, 0:3], G[VV, 3:6], G[PP, 3:6], G[BG, 6:9], G[BA, 9:12] = F[TH, BG], F[VV, BA], F[PP, BA], I, I
    qc = np.repeat(ld([LD(po["sigma_w"]) ** 2 / dt, LD(po["sigma_a"]) ** 2 / dt, LD(po["sigma_wb"]) ** 2 * dt,
                       LD(po["sigma_ab"]) ** 2 * dt]), 3)
    return F, G, qc


def predict_and_compute(x, po, minus, plus):
    """Propagator::predict_and_compute (:343-454) in long double.  Returns (x_new, F, Qd)."""
    minus, plus = ld(minus), ld(plus)
    x = {k: ld(v) for k, v in x.items()}
    dt = plus[0] - minus[0]
    w1, a1, w2, a2 = minus[1:4] - x["bg"], minus[4:7] - x["ba"], plus[1:4] - x["bg"], plus[4:7] - x["ba"]
    nq, nv, npos = predict_mean(x, po, dt, w1, a1, w2, a2)
    F, G, qc = assemble(blocks_of(x, po, dt, w1, a1, nq, nv, npos), dt, po)
    Qd = (G * qc) @ G.T
    xn = dict(x, q=nq, p=npos, v=nv, q_fej=nq, p_fej=npos, v_fej=nv)
    return xn, F, (Qd + Qd.T) / 2


def _prod_err(EA, Amax, EB, Bmax):
    """element bound of the error of a 3 x 3 product A B (3 products, 2 additions per element) whose factors carry EA, EB"""
    return 3 * (EA * Bmax + Amax * EB) + 3 * EA * EB + 15 * U * Amax * Bmax


def _R_err(eq):
    """R(q) of a quaternion off by eq in the 2-norm (propagate_cases.py, 'R')"""
    return 17 * eq + 60 * U


def integrate(x, po, rd, mutate=None):
    """The window's readings rd [n, 7] through predict_and_compute, Phi <- F Phi, Q <- 1/2 ((F Q F^T + Qd) + (.)^T), and last_w.
    Returns dict(q, p, v, Phi, Q, last_w, n_intervals) and under "b" the absolute rounding bounds dict(q, p, v [scalars: 2-norm of
    the vector's error], Phi, Q [15 x 15], last_w [3]).  mutate: None | "drop_interval" | "no_sym" (the test's mutants that live
    in this loop; they change the VALUE returned, the bounds are not meaningful then)."""
    rd = ld(np.asarray(rd, dtype=np.float64).reshape(-1, 7))
    x = {k: ld(v) for k, v in x.items()}
    nr = len(rd)
    Phi, Q = np.eye(15, dtype=LD), np.zeros((15, 15), dtype=LD)
    EPhi, EQ = np.zeros((15, 15), dtype=LD), np.zeros((15, 15), dtype=LD)
    eq = ev = ep = LD(0)            # 2-norm bounds of the mean's errors
    eqf = evf = epf = LD(0)         # ... of the first estimates the next interval reads
    u = U
    gm = LD(po["gravity_mag"])
    for i in range(max(nr - 1, 0)):
        if mutate == "drop_interval" and i == (nr - 1) // 2:
            continue
        m0, m1 = rd[i], rd[i + 1]
        dt = m1[0] - m0[0]
        w1, a1, w2, a2 = m0[1:4] - x["bg"], m0[4:7] - x["ba"], m1[1:4] - x["bg"], m1[4:7] - x["ba"]
        nq, nv, npos = predict_mean(x, po, dt, w1, a1, w2, a2)
        b = blocks_of(x, po, dt, w1, a1, nq, nv, npos)
        F, G, qc = assemble(b, dt, po)
        # ---- the mean's error recursion ----
        Wm, Am = max(norm(w1), norm(w2)), max(norm(a1), norm(a2))
        nv0, np0 = norm(x["v"]), norm(x["p"])
        if not po["use_rk4"]:
            w, a = ((w1 + w2) / 2, (a1 + a2) / 2) if po["imu_avg"] else (w1, a1)
            wn, na = norm(w), norm(a)
            e_w, e_a = 2 * u * Wm, 2 * u * Am
            if wn > 1e-20:
                th = wn * dt / 2
                e_wn = e_w + 4 * u * wn
                e_th = dt / 2 * e_wn + 3 * u * th
                c0, s = np.cos(th), np.sin(th)
                c1 = s / wn
                e_c0, e_s = e_th + S4 * abs(c0), e_th + S4 * abs(s)
                e_c1 = e_s / wn + abs(c1) * e_wn / wn + 2 * u * abs(c1)
            else:
                c0, c1, e_c0, e_c1 = LD(1), dt / 2, LD(0), u * dt
            mu = np.sqrt(c0 * c0 + c1 * c1 * wn * wn)
            e_raw = mu * eq + (e_c0 + e_c1 * wn + abs(c1) * e_w) * norm(x["q"]) + 16 * u * (abs(c0) + 2 * abs(c1) * wn)
            eq_n = e_raw / norm(c0 * x["q"] + c1 * omega_times(w, x["q"])) + 8 * u
            e_Rta = _R_err(eq) * na + e_a + 15 * u * na
            ev_n = ev + dt * e_Rta + 4 * u * (nv0 + na * dt + gm * dt)
            ep_n = ep + dt * ev + dt * dt / 2 * e_Rta + 6 * u * (np0 + nv0 * dt + (na + gm) * dt * dt / 2)
        else:
            kap = Wm * dt / 2
            assert kap < 0.1
            e_ws, e_as = 5 * u * (norm(w1) + norm(w2)), 5 * u * (norm(a1) + norm(a2))
            e_dq = dt * e_ws + 40 * u * kap + 16 * u
            eq_n = eq + e_dq + 24 * u
            e_Rs = _R_err(eq + e_dq + 34 * u)
            e_kv = dt * (e_Rs * Am + e_as + 15 * u * Am) + 3 * u * dt * (Am + gm)
            vmag = nv0 + (Am + gm) * dt
            ev_n = ev + e_kv + 6 * u * vmag
            ep_n = ep + dt * (ev + e_kv + 4 * u * vmag) + 6 * u * (np0 + dt * vmag)
        # ---- F's error, block by block ----
        phi = w1 * dt
        th = norm(phi)
        e_phi = 3 * u * th
        E_J = LD(0) if th < 1e-6 else e_phi + 12 * u + 6 * u / th
        if po["do_fej"]:
            E_RT = _R_err(eqf)
            E_Rth = 17 * (eq_n + eqf) + 130 * u
            e_av = ev_n + evf + 3 * u * (norm(nv) + norm(x["v_fej"]) + gm * dt)
            e_ap = ep_n + epf + dt * evf + 6 * u * (norm(npos) + norm(x["p_fej"]) + norm(x["v_fej"]) * dt + gm * dt * dt)
            E_V = _prod_err(e_av, np.abs(b["av"]).max(), E_RT, LD(1))
            E_P = _prod_err(e_ap, np.abs(b["ap"]).max(), E_RT, LD(1))
        else:
            E_RT = _R_err(eq)
            E_Rth = 2 * e_phi + 12 * u + 10 * u * th
            E_V = _prod_err(E_RT, LD(1), 3 * u * np.abs(b["av"]).max(), np.abs(b["av"]).max())
            E_P = (_prod_err(E_RT, LD(1), 4 * u * np.abs(b["ap"]).max(), np.abs(b["ap"]).max())) / 2
        E_RJ = _prod_err(E_Rth, np.abs(b["Rth"]).max(), E_J, np.abs(b["Jr"]).max())
        EF = np.zeros((15, 15), dtype=LD)
        EF[TH, TH] = E_Rth
        EF[TH, BG] = dt * E_RJ + 2 * u * dt * np.abs(b["RJ"]).max()
        EF[VV, TH], EF[PP, TH] = E_V, E_P
        EF[VV, BA] = dt * E_RT + 2 * u * dt
        EF[PP, BA] = dt * dt / 2 * E_RT + 3 * u * dt * dt / 2
        EF[PP, VV] = u * dt * np.eye(3, dtype=LD)
        EG = np.zeros((15, 12), dtype=LD)
        EG[TH, 0:3], EG[VV, 3:6], EG[PP, 3:6] = EF[TH, BG], EF[VV, BA], EF[PP, BA]
        aG = np.abs(G)
        cQd = (aG * qc) @ aG.T
        EQd = (EG * qc) @ aG.T + (aG * qc) @ EG.T + (EG * qc) @ EG.T + 13 * u * cQd
        Qd = (G * qc) @ G.T
        if mutate != "no_sym":
            Qd = (Qd + Qd.T) / 2
        # ---- Phi, Q and their bounds ----
        aF = np.abs(F)
        EPhi = aF @ EPhi + EF @ np.abs(Phi) + EF @ EPhi + 13 * u * (aF @ np.abs(Phi))
        cT = aF @ np.abs(Q)
        ET = aF @ EQ + EF @ np.abs(Q) + EF @ EQ + 13 * u * cT
        cT2 = cT @ aF.T + cQd
        ET2 = ET @ aF.T + cT @ EF.T + ET @ EF.T + 14 * u * cT2 + EQd
        EQ = (ET2 + ET2.T) / 2 + u * (cT2 + cT2.T) / 2
        Phi = F @ Phi
        if mutate == "no_sym":
            # a double-precision evaluation without either symmetrisation (the rounding is what breaks the symmetry)
            Qf, Ff = np.asarray(Q, dtype=np.float64), np.asarray(F, dtype=np.float64)
            Q = ld((Ff @ Qf) @ Ff.T + np.asarray(Qd, dtype=np.float64))
        else:
            Q = F @ Q @ F.T + Qd
            Q = (Q + Q.T) / 2
        x = dict(x, q=nq, p=npos, v=nv, q_fej=nq, p_fej=npos, v_fej=nv)
        eq, ev, ep = eq_n, ev_n, ep_n
        eqf, evf, epf = eq, ev, ep
    last_w = np.zeros(3, dtype=LD)
    if nr > 1:
        last_w = rd[nr - 2][1:4] - x["bg"]
    elif nr == 1:
        last_w = rd[0][1:4] - x["bg"]
    slack = 1 + LD(1e-6)  # gamma_K against K u and the second-order terms of the mean's recursion (both < 1e-9 relative)
    bnd = dict(q=eq * slack, p=ep * slack, v=ev * slack, Phi=EPhi * slack, Q=EQ * slack, last_w=u * np.abs(last_w))
    return dict(q=x["q"], p=x["p"], v=x["v"], Phi=Phi, Q=Q, last_w=last_w, n_intervals=max(nr - 1, 0), b=bnd)


def covariance(P, imu_id, t, clone=True, dt_id=-1, jitter=0.0):
    """EKFPropagation on the IMU's 15 columns with the truth's Phi, Q, the exact copy of the pose block and the time-offset term
    with dnc_dt = [last_w ; v], from the result t of integrate().  Returns (P_truth, bound): the bound is absolute, element by
    element; an element with a zero bound is a copy of the input."""
    u = U
    P = ld(P)
    n = P.shape[0]
    cols = imu_id + np.arange(15)
    Pt, C = ld_ref.ekf_propagation(P, imu_id, cols, t["Phi"], t["Q"])
    aP, aPhi = np.abs(P), np.abs(t["Phi"])
    EPhi, EQ = t["b"]["Phi"], t["b"]["Q"]
    E = np.zeros((n, n), dtype=LD)
    strip = aP[:, cols] @ EPhi.T
    E[:, cols] = strip
    E[cols, :] = strip.T
    S = aP[np.ix_(cols, cols)]
    E[np.ix_(cols, cols)] = EPhi @ S @ aPhi.T + aPhi @ S @ EPhi.T + EPhi @ S @ EPhi.T + EQ
    K = np.zeros((n, n))
    K[cols, :] = 15
    K[:, cols] = 15
    K[np.ix_(cols, cols)] = 32
    if clone:
        idx = np.concatenate([np.arange(n), imu_id + np.arange(6)])
        Pt, C, E, K = Pt[np.ix_(idx, idx)], C[np.ix_(idx, idx)], E[np.ix_(idx, idx)], K[np.ix_(idx, idx)]
        new = n + np.arange(6)
        if jitter:
            Pt[new, new] = Pt[new, new] * (1 + LD(jitter))
            C[new, new] = C[new, new] * (1 + LD(jitter))
            K[new, new] += 2
        if dt_id >= 0:
            d = np.concatenate([t["last_w"], t["v"]])
            ed = np.concatenate([t["b"]["last_w"], np.full(3, t["b"]["v"], dtype=LD)])
            ad = np.abs(d)
            aPt = np.abs(Pt)
            E1 = E.copy()
            E1[:, new] += np.outer(E[:, dt_id], ad + ed) + np.outer(aPt[:, dt_id], ed)
            P1, _ = ld_ref.augment_dt(Pt, n, dt_id, d)   # (only for |row dt after the column step|)
            a1 = aPt.copy()
            a1[:, new] += np.outer(aPt[:, dt_id], ad)
            E2 = E1.copy()
            E2[new, :] += np.outer(ad + ed, E1[dt_id, :]) + np.outer(ed, a1[dt_id, :])
            E = E2
            Pt, C = P1, ld_ref.augment_dt(C, n, dt_id, ad)[0]
            K[new, :] += 2
            K[:, new] += 2
    # rounding of the covariance arithmetic itself: K roundings per element on the chain's absolute companion, + 2 as everywhere
    B = E * (1 + LD(1e-6)) + (ld(K) + 2 * (K > 0)) * u * C
    return Pt, B
