// Propagator::propagate_and_clone on the device (state/Propagator.cpp:37-126, :343-454; StateHelper::augment_clone :588-625): the
// kernels of ovp_propagate_and_clone that the covariance kernels of k_ekf.hip do not already provide.
//   k_prop_integrate  one workgroup.  Per interval, in order: predict_and_compute (the mean, discrete or RK4, F in its FEJ or plain
//                     form, Qd = G Qc G^T symmetrised), then Phi <- F Phi and Q <- 1/2 ((F Q F^T + Qd) + (.)^T).  The mean is scalar
//                     work: every thread carries it in registers, wave-uniformly, and thread 0 stores the 3 x 3 blocks of F into LDS;
//                     Phi, Q, F and T = F Q live in LDS, one thread per element of the 15 x 15 products.  F is block-sparse (rows th:
//                     th bg; p: th p v ba; v: th v ba; bg: bg; ba: ba): the sums skip its zero blocks, which leaves every bit as the
//                     dense product has it.  Both triangles of Q come from one instruction sequence on the ordered pair (lo, hi):
//                     Q is symmetric to the bit.  No atomics, a fixed order: two calls give the same bits.
//   k_prop_clone_dt   StateHelper::clone of the pose block and the time-offset term in one pass: every new element is a function of
//                     old elements only (rows / columns below n), so nothing it reads is written by the launch.  The new block is
//                     computed on the ordered pair as well.
//   k_prop_finish     the verdict and the result block into mapped pinned memory, then the sequence word.
// Plain f64 VALU; sin / cos / sqrt are the device library's.
#include "ovp_kernels.h"

namespace ovp {

namespace {

struct M3 {
  double a[9];
};
__device__ __forceinline__ M3 m3_mul(const M3& A, const M3& B) {
  M3 C;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) C.a[3 * i + j] = A.a[3 * i] * B.a[j] + A.a[3 * i + 1] * B.a[3 + j] + A.a[3 * i + 2] * B.a[6 + j];
  return C;
}
__device__ __forceinline__ M3 m3_tr(const M3& A) { return M3{{A.a[0], A.a[3], A.a[6], A.a[1], A.a[4], A.a[7], A.a[2], A.a[5], A.a[8]}}; }
__device__ __forceinline__ M3 m3_skew(const double w[3]) { return M3{{0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0}}; }
__device__ __forceinline__ M3 m3_eye() { return M3{{1, 0, 0, 0, 1, 0, 0, 0, 1}}; }
__device__ __forceinline__ double norm3(const double w[3]) { return sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]); }

__device__ __forceinline__ M3 quat_2_rot(const double q[4]) {  // JPL, row-major
  const double x = q[0], y = q[1], z = q[2], w = q[3], a = 2.0 * w * w - 1.0;
  return M3{{a + 2 * x * x, 2 * w * z + 2 * x * y, -2 * w * y + 2 * x * z, -2 * w * z + 2 * y * x, a + 2 * y * y, 2 * w * x + 2 * y * z,
             2 * w * y + 2 * z * x, -2 * w * x + 2 * z * y, a + 2 * z * z}};
}
__device__ __forceinline__ void quatnorm(double q[4]) {
  if (q[3] < 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = -q[k];
  }
  const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] /= n;
}
__device__ __forceinline__ void quat_multiply(const double q[4], const double p[4], double o[4]) {
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  o[0] = w * p[0] + z * p[1] - y * p[2] + x * p[3];
  o[1] = -z * p[0] + w * p[1] + x * p[2] + y * p[3];
  o[2] = y * p[0] - x * p[1] + w * p[2] + z * p[3];
  o[3] = -x * p[0] - y * p[1] - z * p[2] + w * p[3];
  quatnorm(o);
}
__device__ __forceinline__ void omega_times(const double w[3], const double q[4], double o[4]) {  // Omega(w) q
  o[0] = w[2] * q[1] - w[1] * q[2] + w[0] * q[3];
  o[1] = -w[2] * q[0] + w[0] * q[2] + w[1] * q[3];
  o[2] = w[1] * q[0] - w[0] * q[1] + w[2] * q[3];
  o[3] = -w[0] * q[0] - w[1] * q[1] - w[2] * q[2];
}
__device__ __forceinline__ void m3_tmul(const M3& R, const double v[3], double o[3]) {  // R^T v
#pragma unroll
  for (int i = 0; i < 3; ++i) o[i] = R.a[i] * v[0] + R.a[3 + i] * v[1] + R.a[6 + i] * v[2];
}
__device__ __forceinline__ M3 exp_so3(const double w[3]) {
  const M3 S = m3_skew(w), S2 = m3_mul(S, S);
  const double th = norm3(w);
  const double A = th < 1e-7 ? 1.0 : sin(th) / th;
  const double B = th < 1e-7 ? 0.5 : (1.0 - cos(th)) / (th * th);
  M3 R = m3_eye();
#pragma unroll
  for (int i = 0; i < 9; ++i) R.a[i] += A * S.a[i] + B * S2.a[i];
  return R;
}
__device__ __forceinline__ M3 jl_so3(const double w[3]) {
  const double th = norm3(w);
  if (th < 1e-6) return m3_eye();
  const double a[3] = {w[0] / th, w[1] / th, w[2] / th};
  const M3 S = m3_skew(a);
  const double s = sin(th) / th, c = (1.0 - cos(th)) / th;
  M3 J;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) J.a[3 * i + j] = (i == j ? s : 0.0) + (1.0 - s) * a[i] * a[j] + c * S.a[3 * i + j];
  return J;
}

// Propagator::predict_mean_discrete (:456-503)
__device__ __forceinline__ void mean_discrete(bool avg, double dt, double g, const double q[4], const double p[3], const double v[3],
                                              const M3& R, const double w1[3], const double a1[3], const double w2[3],
                                              const double a2[3], double nq[4], double nv[3], double np[3]) {
  double w[3], a[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    w[k] = avg ? .5 * (w1[k] + w2[k]) : w1[k];
    a[k] = avg ? .5 * (a1[k] + a2[k]) : a1[k];
  }
  const double wn = norm3(w);
  double Oq[4];
  omega_times(w, q, Oq);
  const double c0 = wn > 1e-20 ? cos(0.5 * wn * dt) : 1.0;
  const double c1 = wn > 1e-20 ? 1 / wn * sin(0.5 * wn * dt) : 0.5 * dt;
#pragma unroll
  for (int k = 0; k < 4; ++k) nq[k] = c0 * q[k] + c1 * Oq[k];
  quatnorm(nq);
  double Rta[3];
  m3_tmul(R, a, Rta);
  const double gv[3] = {0.0, 0.0, g};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    nv[k] = v[k] + Rta[k] * dt - gv[k] * dt;
    np[k] = p[k] + v[k] * dt + 0.5 * Rta[k] * dt * dt - 0.5 * gv[k] * dt * dt;
  }
}

// Propagator::predict_mean_rk4 (:505-602): four stages on (dq, p, v), dq re-normalised at every stage
__device__ __forceinline__ void mean_rk4(double dt, double g, const double q0[4], const double p0[3], const double v0[3],
                                         const double w1[3], const double a1[3], const double w2[3], const double a2[3], double nq[4],
                                         double nv[3], double np[3]) {
  double w[3], a[3], wal[3], aj[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    w[k] = w1[k];
    a[k] = a1[k];
    wal[k] = (w2[k] - w1[k]) / dt;
    aj[k] = (a2[k] - a1[k]) / dt;
  }
  const double gv[3] = {0.0, 0.0, g};
  double kq[4][4], kp[4][3], kv[4][3];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const double frac = (s == 0) ? 0.0 : (s == 3 ? 1.0 : 0.5);
    if (s == 1 || s == 3) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        w[k] += 0.5 * wal[k] * dt;
        a[k] += 0.5 * aj[k] * dt;
      }
    }
    double dq[4] = {0.0, 0.0, 0.0, 1.0}, vs[3];
    if (s) {
#pragma unroll
      for (int k = 0; k < 4; ++k) dq[k] += frac * kq[s - 1][k];
      quatnorm(dq);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) vs[k] = v0[k] + (s ? frac * kv[s - 1][k] : 0.0);
    double qd[4], qs[4], Rta[3];
    omega_times(w, dq, qd);
    quat_multiply(dq, q0, qs);
    m3_tmul(quat_2_rot(qs), a, Rta);
#pragma unroll
    for (int k = 0; k < 4; ++k) kq[s][k] = 0.5 * qd[k] * dt;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      kp[s][k] = vs[k] * dt;
      kv[s][k] = (Rta[k] - gv[k]) * dt;
    }
  }
  double dq[4] = {0.0, 0.0, 0.0, 1.0};
#pragma unroll
  for (int k = 0; k < 4; ++k) dq[k] += (1.0 / 6.0) * kq[0][k] + (1.0 / 3.0) * kq[1][k] + (1.0 / 3.0) * kq[2][k] + (1.0 / 6.0) * kq[3][k];
  quatnorm(dq);
  quat_multiply(dq, q0, nq);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    np[k] = p0[k] + (1.0 / 6.0) * kp[0][k] + (1.0 / 3.0) * kp[1][k] + (1.0 / 3.0) * kp[2][k] + (1.0 / 6.0) * kp[3][k];
    nv[k] = v0[k] + (1.0 / 6.0) * kv[0][k] + (1.0 / 3.0) * kv[1][k] + (1.0 / 3.0) * kv[2][k] + (1.0 / 6.0) * kv[3][k];
  }
}

// error-state order th p v bg ba: row blocks 0..4; the column blocks a row block of F is not zero in
__device__ __forceinline__ unsigned f_blocks(int rb) {
  return rb == 0 ? 0x09u : rb == 1 ? 0x17u : rb == 2 ? 0x15u : rb == 3 ? 0x08u : 0x10u;
}
// sum_k A[i][k] B[k][j] over the non-zero blocks of row i of A = F (row-major 15 x 15 in LDS)
__device__ __forceinline__ double f_times(const double* F, const double* B, int i, int j) {
  const unsigned m = f_blocks(i / 3);
  double s = 0.0;
#pragma unroll
  for (int kb = 0; kb < 5; ++kb)
    if ((m >> kb) & 1u) {
#pragma unroll
      for (int kk = 0; kk < 3; ++kk) s = fma(F[15 * i + 3 * kb + kk], B[15 * (3 * kb + kk) + j], s);
    }
  return s;
}
// sum_k T[i][k] F[j][k] over the non-zero blocks of row j of F
__device__ __forceinline__ double times_ft(const double* T, const double* F, int i, int j) {
  const unsigned m = f_blocks(j / 3);
  double s = 0.0;
#pragma unroll
  for (int kb = 0; kb < 5; ++kb)
    if ((m >> kb) & 1u) {
#pragma unroll
      for (int kk = 0; kk < 3; ++kk) s = fma(T[15 * i + 3 * kb + kk], F[15 * j + 3 * kb + kk], s);
    }
  return s;
}
// G of (:425-435) read out of F: G[th][n_g] = F[th][bg], G[v][n_a] = F[v][ba], G[p][n_a] = F[p][ba], G[bg][n_wg] = G[ba][n_wa] = I
__device__ __forceinline__ double g_of(const double* F, int i, int k) {
  if (k < 3) return i < 3 ? F[15 * i + 9 + k] : 0.0;
  if (k < 6) return (i >= 3 && i < 9) ? F[15 * i + 12 + (k - 3)] : 0.0;
  if (k < 9) return i == 9 + (k - 6) ? 1.0 : 0.0;
  return i == 12 + (k - 9) ? 1.0 : 0.0;
}
__device__ __forceinline__ double gqg(const double* F, const double qc[4], int i, int j) {  // (G Qc G^T)[i][j]
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < 12; ++k) s = fma(g_of(F, i, k) * qc[k / 3], g_of(F, j, k), s);
  return s;
}

__device__ __forceinline__ void put3(double* F, int r0, int c0, const M3& B, double s) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) F[15 * (r0 + i) + c0 + j] = s * B.a[3 * i + j];
}

}  // namespace

__global__ __launch_bounds__(256) void k_prop_integrate(const PropParams* __restrict__ pp, const double* __restrict__ rd,
                                                        double* __restrict__ res) {
  __shared__ double Phi[225], Qs[225], Fs[225], Ts[225];  // row-major
  const int t = threadIdx.x;
  const PropParams& P = *pp;
  const int nr = P.n_readings, ni = nr > 1 ? nr - 1 : 0;
  const bool rk4 = P.use_rk4 != 0, avg = P.imu_avg != 0, fej = P.do_fej != 0;
  const double g = P.g;
  double q[4], p[3], v[3], qf[4], pf[3], vf[3], bg[3], ba[3];
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] = P.q[k], qf[k] = P.q_fej[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) p[k] = P.p[k], v[k] = P.v[k], pf[k] = P.p_fej[k], vf[k] = P.v_fej[k], bg[k] = P.bg[k], ba[k] = P.ba[k];
  const int ei = t / 15, ej = t - 15 * ei;  // this thread's element (t < 225)
  if (t < 225) {
    Phi[t] = ei == ej ? 1.0 : 0.0;
    Qs[t] = 0.0;
    Fs[t] = ei == ej ? 1.0 : 0.0;  // the identity blocks stay; thread 0 rewrites the others every interval
    Ts[t] = 0.0;
  }
  __syncthreads();
  for (int it = 0; it < ni; ++it) {
    // ---- predict_and_compute, wave-uniform ----
    const double* m0 = rd + 7 * (size_t)it;
    const double* m1 = m0 + 7;
    const double dt = m1[0] - m0[0];
    double w1[3], a1[3], w2[3], a2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      w1[k] = m0[1 + k] - bg[k];
      a1[k] = m0[4 + k] - ba[k];
      w2[k] = m1[1 + k] - bg[k];
      a2[k] = m1[4 + k] - ba[k];
    }
    const M3 R = quat_2_rot(q);
    double nq[4], nv[3], np[3];
    if (rk4) mean_rk4(dt, g, q, p, v, w1, a1, w2, a2, nq, nv, np);
    else mean_discrete(avg, dt, g, q, p, v, R, w1, a1, w2, a2, nq, nv, np);
    const double mwdt[3] = {-w1[0] * dt, -w1[1] * dt, -w1[2] * dt};
    const double pwdt[3] = {-mwdt[0], -mwdt[1], -mwdt[2]};
    const M3 Jr = jl_so3(pwdt);  // Jr(-w dt) = Jl(w dt)
    M3 Rth, RT, Vth, Pth;
    double ps;  // scale of the p-theta block
    if (fej) {
      RT = m3_tr(quat_2_rot(qf));
      Rth = m3_mul(quat_2_rot(nq), RT);
      double av[3], ap[3];
      const double gv[3] = {0.0, 0.0, g};
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        av[k] = nv[k] - vf[k] + gv[k] * dt;
        ap[k] = np[k] - pf[k] - vf[k] * dt + 0.5 * gv[k] * dt * dt;
      }
      Vth = m3_mul(m3_skew(av), RT);
      Pth = m3_mul(m3_skew(ap), RT);
      ps = -1.0;
    } else {
      RT = m3_tr(R);
      Rth = exp_so3(mwdt);
      double av[3], ap[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        av[k] = a1[k] * dt;
        ap[k] = a1[k] * dt * dt;
      }
      Vth = m3_mul(RT, m3_skew(av));
      Pth = m3_mul(RT, m3_skew(ap));
      ps = -0.5;
    }
    const M3 RJ = m3_mul(Rth, Jr);
    const double qc[4] = {P.sw2 / dt, P.sa2 / dt, P.swb2 * dt, P.sab2 * dt};
    if (t == 0) {
      put3(Fs, 0, 0, Rth, 1.0);
      put3(Fs, 0, 9, RJ, -dt);
      put3(Fs, 6, 0, Vth, -1.0);
      put3(Fs, 6, 12, RT, -dt);
      put3(Fs, 3, 0, Pth, ps);
      put3(Fs, 3, 12, RT, -0.5 * dt * dt);
      Fs[15 * 3 + 6] = dt;
      Fs[15 * 4 + 7] = dt;
      Fs[15 * 5 + 8] = dt;
    }
    // value and first estimate both become the propagated mean (:447-453)
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = qf[k] = nq[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = pf[k] = np[k], v[k] = vf[k] = nv[k];
    __syncthreads();
    // ---- Phi <- F Phi, T = F Q ----
    double phin = 0.0, tq = 0.0;
    if (t < 225) {
      phin = f_times(Fs, Phi, ei, ej);
      tq = f_times(Fs, Qs, ei, ej);
    }
    __syncthreads();
    if (t < 225) {
      Phi[t] = phin;
      Ts[t] = tq;
    }
    __syncthreads();
    // ---- Q <- 1/2 ((T F^T + Qd) + (.)^T), Qd = 1/2 (G Qc G^T + (.)^T): one sequence on the ordered pair ----
    if (t < 225) {
      const int lo = ei < ej ? ei : ej, hi = ei < ej ? ej : ei;
      const double qd = 0.5 * (gqg(Fs, qc, lo, hi) + gqg(Fs, qc, hi, lo));
      const double x = times_ft(Ts, Fs, lo, hi) + qd;
      const double y = times_ft(Ts, Fs, hi, lo) + qd;
      Qs[t] = 0.5 * (x + y);
    }
    __syncthreads();  // (F and T are rewritten by the next interval)
  }
  // ---- last angular velocity (:108-114), the mean, Phi and Q (column-major) ----
  if (t < 225) {
    res[OVP_PR_PHI + 15 * ej + ei] = Phi[t];
    res[OVP_PR_QS + 15 * ej + ei] = Qs[t];
  }
  if (t == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) res[OVP_PR_Q + k] = q[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      res[OVP_PR_P + k] = p[k];
      res[OVP_PR_V + k] = v[k];
      double lw = 0.0;
      if (nr > 1) lw = rd[7 * (size_t)(nr - 2) + 1 + k] - bg[k];
      else if (nr == 1) lw = rd[1 + k] - bg[k];
      res[OVP_PR_LW + k] = lw;
      res[OVP_PR_LW + 3 + k] = 0.0;
    }
    res[OVP_PR_VERDICT] = 0.0;
    res[OVP_PR_NI] = (double)ni;
  }
}

// StateHelper::EKFPropagation (:41-119) on the IMU's 15 contiguous columns, Phi and Q (column-major) read from the result block.
// Step 1: CPT[r][j] = sum_k P[r][imu + k] Phi[j][k], one thread per element.
__global__ __launch_bounds__(256) void k_prop15_cpt(const double* __restrict__ P, int ld, int n, int imu, const double* __restrict__ res,
                                                    double* __restrict__ CPT) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= n * 15) return;
  const int r = idx / 15, j = idx - 15 * r;
  const double* Phi = res + OVP_PR_PHI;
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < 15; ++k) s = fma(P[(size_t)r * ld + imu + k], Phi[15 * k + j], s);
  CPT[idx] = s;
}
// Step 2: the strips, their mirror images and the block Phi CPT[imu..] + Q.selfadjointView<Upper>; the block is computed on the
// ordered pair (lo, hi), so both of its triangles hold the same bits.  The negative-diagonal check covers every diagonal element.
__global__ __launch_bounds__(256) void k_prop15_write(double* __restrict__ P, int ld, int n, int imu, const double* __restrict__ res,
                                                      const double* __restrict__ CPT, int* __restrict__ negdiag) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= n * 15) return;
  const int r = idx / 15, j = idx - 15 * r;
  const int i = r - imu;
  if (i < 0 || i >= 15) {
    const double v = CPT[idx];
    P[(size_t)r * ld + imu + j] = v;
    P[(size_t)(imu + j) * ld + r] = v;
    if (j == 0 && P[(size_t)r * ld + r] < 0.0) *negdiag = 1;
    return;
  }
  const int lo = i < j ? i : j, hi = i < j ? j : i;
  const double* Phi = res + OVP_PR_PHI;
  double s = res[OVP_PR_QS + 15 * hi + lo];
#pragma unroll
  for (int k = 0; k < 15; ++k) s = fma(Phi[15 * k + lo], CPT[(size_t)(imu + k) * 15 + hi], s);
  P[(size_t)r * ld + imu + j] = s;
  if (i == j && s < 0.0) *negdiag = 1;
}

// thread (r, k): r over the n + 6 rows of the grown matrix, k over the six new columns
__global__ __launch_bounds__(256) void k_prop_clone_dt(double* __restrict__ P, int ld, int n, int src, int dt, double jitter,
                                                       const double* __restrict__ res) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= (n + 6) * 6) return;
  const int r = idx / 6, k = idx - 6 * r;
  double d[6] = {0, 0, 0, 0, 0, 0};
  if (dt >= 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) d[a] = res[OVP_PR_LW + a], d[3 + a] = res[OVP_PR_V + a];
  }
  double dk = 0.0;
#pragma unroll
  for (int a = 0; a < 6; ++a) dk = a == k ? d[a] : dk;
  if (r < n) {
    // the column step on the copied column; the row step gives the mirror image the same bits (P is symmetric, a product commutes)
    double v = P[(size_t)r * ld + src + k];
    if (dt >= 0) v = fma(P[(size_t)r * ld + dt], dk, v);
    P[(size_t)r * ld + n + k] = v;
    P[(size_t)(n + k) * ld + r] = v;
    return;
  }
  const int i = r - n;
  const int lo = i < k ? i : k, hi = i < k ? k : i;
  double dlo = 0.0, dhi = 0.0;
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    dlo = a == lo ? d[a] : dlo;
    dhi = a == hi ? d[a] : dhi;
  }
  double v = P[(size_t)(src + lo) * ld + src + hi];
  if (lo == hi) v *= (1.0 + jitter);  // ovp_cov_clone_jitter, as k_cov_clone
  if (dt >= 0) {
    // column step: + P[src+lo][dt] d_hi; row step: + d_lo x (row dt after the column step: P[dt][src+hi] + P[dt][dt] d_hi)
    v = fma(P[(size_t)(src + lo) * ld + dt], dhi, v);
    const double rowdt = fma(P[(size_t)dt * ld + dt], dhi, P[(size_t)dt * ld + src + hi]);
    v = fma(dlo, rowdt, v);
  }
  P[(size_t)r * ld + n + k] = v;
}

__global__ __launch_bounds__(256) void k_prop_finish(double* __restrict__ res, int* __restrict__ negdiag,
                                                     unsigned long long* __restrict__ host_block, volatile unsigned* word, unsigned seq) {
  const int t = threadIdx.x;
  __shared__ int neg;
  if (t == 0) {
    neg = *negdiag != 0;
    *negdiag = 0;
    res[OVP_PR_VERDICT] = neg ? 1.0 : 0.0;
  }
  __syncthreads();
  const unsigned long long* src = reinterpret_cast<const unsigned long long*>(res);
  for (int i = t; i < OVP_PR_DOUBLES; i += 256) host_block[i] = src[i];
  __threadfence_system();
  __syncthreads();
  if (t == 0) *word = seq;
}

}  // namespace ovp

extern "C" {

hipError_t ovp_launch_prop_integrate(const ovp::PropParams* pp, const double* readings, double* res, hipStream_t stream) {
  if (!pp || !res || (((size_t)res | (size_t)readings) & 7)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ovp::k_prop_integrate, dim3(1), dim3(256), 0, stream, pp, readings, res);
  return hipGetLastError();
}

hipError_t ovp_launch_prop_cov15(double* P, int ld, int n, int imu, const double* res, double* CPT, int* negdiag, hipStream_t stream) {
  if (n < 15 || ld < n || imu < 0 || imu + 15 > n || !CPT) return hipErrorInvalidValue;
  const int total = n * 15;
  hipLaunchKernelGGL(ovp::k_prop15_cpt, dim3((total + 255) / 256), dim3(256), 0, stream, (const double*)P, ld, n, imu, res, CPT);
  hipLaunchKernelGGL(ovp::k_prop15_write, dim3((total + 255) / 256), dim3(256), 0, stream, P, ld, n, imu, res, (const double*)CPT, negdiag);
  return hipGetLastError();
}

hipError_t ovp_launch_prop_clone_dt(double* P, int ld, int n, int src, int dt, double jitter, const double* res, hipStream_t stream) {
  if (n < 6 || ld < n + 6 || src < 0 || src + 6 > n || dt >= n || (dt >= src && dt < src + 6)) return hipErrorInvalidValue;
  const int total = (n + 6) * 6;
  hipLaunchKernelGGL(ovp::k_prop_clone_dt, dim3((total + 255) / 256), dim3(256), 0, stream, P, ld, n, src, dt, jitter, res);
  return hipGetLastError();
}

hipError_t ovp_launch_prop_finish(double* res, int* negdiag, void* host_block, unsigned* word, unsigned seq, hipStream_t stream) {
  if ((((size_t)res | (size_t)host_block) & 7)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ovp::k_prop_finish, dim3(1), dim3(256), 0, stream, res, negdiag, (unsigned long long*)host_block,
                     (volatile unsigned*)word, seq);
  return hipGetLastError();
}
}
