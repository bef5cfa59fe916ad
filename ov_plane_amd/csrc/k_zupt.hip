// UpdaterZeroVelocity::try_update on the resident covariance (update/UpdaterZeroVelocity.cpp:119-265): the kernels of
// ovp_zupt_update.  Every interval of the window contributes the same 6 x 9 block H0 over [theta, b_g, b_a] with its own diagonal
// weight dt_i D, so the 6 (n - 1)-row stacked system collapses, exactly, to a weighted mean residual, a within-window scatter, a
// 6 x 6 factorization and a rank-6 symmetric downdate (include/ovplane_hip.h has the algebra).
//   k_zupt_gate    one workgroup: T and rbar (pass 1), the scatter about rbar (pass 2: rho - rbar^T Rbar^-1 rbar cancels), the
//                  9 x 9 block of P' = P + Q_bias, Sbar = H0 P'_ss H0^T + Rbar, its factor, z, chi2 and the decision
//                  (:191-236).  Both reductions run over a fixed tree in a fixed order, no atomics: two calls give the same bits.
//   k_zupt_rows    Y = P'_{:,s} H0^T Lbar^-T (n x 6) and dx = Y z.  A kernel of its own: the columns s of P are an input of Y and
//                  an output of the downdate, so all of Y exists before any tile of P is written.
//   k_zupt_apply   P <- P + Q_bias - Y Y^T, one workgroup per lower 16 x 16 tile, the mirror image written with it (both triangles
//                  stay equal), the negative-diagonal check of the dense update; the last workgroup to finish publishes
//                  [flags | chi2 | rows | dx] into the context's mailbox, as k_dx_rows (k_tile.hip) does.
// The decision stays on the device: rows and apply return at the gate's word when the update was rejected, and nothing of P, the
// tables or a kept factor is touched.  Plain f64 VALU.
#include "ovp_kernels.h"

namespace ovp {

__device__ __forceinline__ int zupt_col(int imu_id, int k) { return imu_id + (k < 3 ? k : k + 6); }  // theta | b_g b_a

// sum of v over the 256 threads, the same tree whatever the data; every thread returns the total
__device__ __forceinline__ double zupt_tree_sum(double v, double* red) {
  const int t = threadIdx.x;
  __syncthreads();  // (red may still be read from the sum before)
  red[t] = v;
  __syncthreads();
#pragma unroll
  for (int off = 128; off > 0; off >>= 1) {
    if (t < off) red[t] += red[t + off];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(256) void k_zupt_gate(const double* __restrict__ P, int ld, const ZuptParams* __restrict__ zp,
                                                   const double* __restrict__ rd, double* __restrict__ work,
                                                   double* __restrict__ res) {
  __shared__ double red[256];
  __shared__ double Ps[81], H0[54], HP[54], S[36], L[36], Li[36], rbar[6], z[6];
  __shared__ double chi2_s;
  __shared__ int acc_s, spd_s;
  const int t = threadIdx.x;
  const ZuptParams& p = *zp;  // (uniform reads through the pointer: a by-value copy is indexed at run time and lands in scratch)
  const int ni = p.n_readings - 1;
  // the residual of interval i is that of its first reading (:141-166)
  auto residual = [&](int i, double r[6]) {
    const double* m = rd + 7 * (size_t)i;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      r[k] = -(m[1 + k] - p.bg[k]);
      r[3 + k] = -((m[4 + k] - p.ba[k]) - p.Rg[k]);
    }
  };
  // pass 1: T = sum dt_i, rbar = sum dt_i r_i / T
  double a[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int i = t; i < ni; i += 256) {
    const double dt = rd[7 * (size_t)(i + 1)] - rd[7 * (size_t)i];
    double r[6];
    residual(i, r);
    a[0] += dt;
#pragma unroll
    for (int k = 0; k < 6; ++k) a[1 + k] = fma(dt, r[k], a[1 + k]);
  }
  const double T = zupt_tree_sum(a[0], red);
  double rb[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) rb[k] = zupt_tree_sum(a[1 + k], red) / T;
  // pass 2: the scatter about rbar, sum dt_i (r_i - rbar)^T D (r_i - rbar)
  double sc = 0.0;
  for (int i = t; i < ni; i += 256) {
    const double dt = rd[7 * (size_t)(i + 1)] - rd[7 * (size_t)i];
    double r[6];
    residual(i, r);
    double ew = 0.0, ea = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double e0 = r[k] - rb[k], e1 = r[3 + k] - rb[3 + k];
      ew = fma(e0, e0, ew);
      ea = fma(e1, e1, ea);
    }
    sc = fma(dt, fma(p.d_w, ew, p.d_a * ea), sc);
  }
  const double scatter = zupt_tree_sum(sc, red);
  // the 9 x 9 block of P' and H0 = [[0, -I, 0], [-skew(R_jac g), 0, -I]]
  if (t < 81) {
    const int i = t / 9, j = t - 9 * i;
    double v = P[(size_t)zupt_col(p.imu_id, i) * ld + zupt_col(p.imu_id, j)];
    if (i == j && i >= 3) v += T * (i < 6 ? p.q_wb : p.q_ab);  // :184-186
    Ps[t] = v;
  }
  if (t >= 128 && t < 128 + 54) {
    const int u = t - 128, i = u / 9, j = u - 9 * i;
    double v = 0.0;
    if (i < 3) v = (j == 3 + i) ? -1.0 : 0.0;
    else if (j < 3) v = -p.S3[3 * (i - 3) + j];
    else v = (j == 3 + i) ? -1.0 : 0.0;
    H0[u] = v;
  }
  if (t < 6) rbar[t] = rb[t];
  __syncthreads();
  if (t < 54) {
    const int i = t / 9, j = t - 9 * i;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) s = fma(H0[9 * i + k], Ps[9 * k + j], s);
    HP[t] = s;
  }
  __syncthreads();
  if (t < 36) {
    const int i = t / 6, j = t - 6 * i;
    const int lo = i < j ? i : j, hi = i < j ? j : i;  // (one order for both triangles: S is symmetric to the bit)
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) s = fma(HP[9 * hi + k], H0[9 * lo + k], s);
    if (i == j) s += 1.0 / (T * (i < 3 ? p.d_w : p.d_a));  // Rbar = (T D)^-1
    S[t] = s;
  }
  __syncthreads();
  if (t == 0) {
    bool spd = true;
    for (int q = 0; q < 36; ++q) L[q] = 0.0;
    for (int q = 0; q < 6; ++q) {
      double d = S[6 * q + q];
      for (int k = 0; k < q; ++k) d -= L[6 * q + k] * L[6 * q + k];
      if (!(d > 0.0)) spd = false, d = 1.0;
      L[6 * q + q] = sqrt(d);
      for (int i = q + 1; i < 6; ++i) {
        double s = S[6 * i + q];
        for (int k = 0; k < q; ++k) s -= L[6 * i + k] * L[6 * q + k];
        L[6 * i + q] = s / L[6 * q + q];
      }
    }
    double c2 = 0.0;
    for (int i = 0; i < 6; ++i) {
      double s = rbar[i];
      for (int k = 0; k < i; ++k) s -= L[6 * i + k] * z[k];
      z[i] = s / L[6 * i + i];
      c2 += z[i] * z[i];
    }
    // Lbar^-1 (lower), column by column
    for (int c = 0; c < 6; ++c)
      for (int i = 0; i < 6; ++i) {
        double s = i == c ? 1.0 : 0.0;
        for (int k = c; k < i; ++k) s -= L[6 * i + k] * Li[6 * k + c];
        Li[6 * i + c] = i < c ? 0.0 : s / L[6 * i + i];
      }
    const double chi2 = spd ? scatter + c2 : 0.0;
    chi2_s = chi2;
    spd_s = spd ? 1 : 0;
    acc_s = (spd && (p.disparity_passed != 0 || (chi2 <= p.thr && p.vel_ok != 0))) ? 1 : 0;  // :231-236
  }
  __syncthreads();
  if (t < 36) work[OVP_ZW_L + t] = L[t];
  if (t < 6) {
    work[OVP_ZW_Z + t] = z[t];
    work[OVP_ZW_Q + t] = T * (t < 3 ? p.q_wb : p.q_ab);
  }
  if (t < 54) {
    work[OVP_ZW_H0 + t] = H0[t];
    // G = H0^T Lbar^-T: G[k][c] = sum_a H0[a][k] Li[c][a]
    const int k = t / 6, c = t - 6 * k;
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < 6; ++q) s = fma(H0[9 * q + k], Li[6 * c + q], s);
    work[OVP_ZW_G + t] = s;
  }
  if (t < OVP_ZUPT_RES_HEAD) {
    double v = 0.0;
    if (t == 0) v = acc_s ? 1.0 : 0.0;
    if (t == 1) v = chi2_s;
    if (t == 2) v = 6.0 * ni;
    if (t == 4) v = spd_s ? 0.0 : 1.0;
    res[t] = v;
  }
}

__global__ __launch_bounds__(64) void k_zupt_rows(const double* __restrict__ P, int ld, int n, int imu_id,
                                                  const double* __restrict__ work, double* __restrict__ Y, double* __restrict__ res) {
  if (res[0] == 0.0) return;
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  double pv[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const int c = zupt_col(imu_id, k);
    pv[k] = P[(size_t)c * ld + i];  // P[i][c] read along row c (both triangles are equal): the wave's loads run along a row
    if (k >= 3 && c == i) pv[k] += work[OVP_ZW_Q + k - 3];
  }
  double dx = 0.0;
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    double y = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) y = fma(pv[k], work[OVP_ZW_G + 6 * k + c], y);
    Y[6 * (size_t)i + c] = y;
    dx = fma(y, work[OVP_ZW_Z + c], dx);
  }
  res[OVP_ZUPT_RES_HEAD + i] = dx;
}

// `words` doubles of res into mapped pinned memory, then the sequence word behind them (one workgroup, every thread calls)
__device__ __forceinline__ void zupt_publish(const double* res, int words, unsigned long long* host_block, volatile unsigned* word,
                                             unsigned seq) {
  const unsigned long long* src = reinterpret_cast<const unsigned long long*>(res);
  for (int i = threadIdx.x; i < words; i += 256) host_block[i] = __builtin_nontemporal_load(src + i);
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) *word = seq;
}

// grid: the lower tiles, row by row (tile b = bi (bi + 1) / 2 + bj, bj <= bi)
__global__ __launch_bounds__(256) void k_zupt_apply(double* P, int ld, int n, int imu_id, const double* __restrict__ work,
                                                    const double* __restrict__ Y, double* res, unsigned* __restrict__ ticket,
                                                    unsigned long long* __restrict__ host_block, volatile unsigned* word,
                                                    unsigned seq) {
  const int t = threadIdx.x;
  if (res[0] == 0.0) {  // rejected: nothing of P is touched; the first workgroup reports
    if (blockIdx.x == 0) zupt_publish(res, OVP_ZUPT_RES_HEAD, host_block, word, seq);
    return;
  }
  int bi = (int)((sqrt(8.0 * (double)blockIdx.x + 1.0) - 1.0) * 0.5);
  while ((bi + 1) * (bi + 2) / 2 <= (int)blockIdx.x) ++bi;
  while (bi * (bi + 1) / 2 > (int)blockIdx.x) --bi;
  const int bj = (int)blockIdx.x - bi * (bi + 1) / 2;
  __shared__ double Yi[16][6], Yj[16][6];
  if (t < 96) {
    const int r = t / 6, c = t - 6 * r, g = bi * 16 + r;
    Yi[r][c] = g < n ? Y[6 * (size_t)g + c] : 0.0;
  } else if (t >= 128 && t < 224) {
    const int u = t - 128, r = u / 6, c = u - 6 * r, g = bj * 16 + r;
    Yj[r][c] = g < n ? Y[6 * (size_t)g + c] : 0.0;
  }
  __syncthreads();
  const int r = t >> 4, c = t & 15;
  const int gi = bi * 16 + r, gj = bj * 16 + c;
  if (gi < n && gj < n && (bi != bj || c <= r)) {
    double s = Yi[r][0] * Yj[c][0];
#pragma unroll
    for (int k = 1; k < 6; ++k) s = fma(Yi[r][k], Yj[c][k], s);
    double v = P[(size_t)gi * ld + gj];
    if (gi == gj) {
      const int k = gi - imu_id;
      if (k >= 9 && k < 15) v += work[OVP_ZW_Q + k - 9];
    }
    v -= s;
    P[(size_t)gi * ld + gj] = v;
    if (gi != gj) P[(size_t)gj * ld + gi] = v;
    else if (v < 0.0) res[3] = 1.0;
  }
  // the last workgroup to finish publishes (the ticket of k_dx_rows)
  __shared__ unsigned last;
  __threadfence();
  __syncthreads();
  if (t == 0) last = (atomicAdd(ticket, 1u) == gridDim.x - 1) ? 1u : 0u;
  __syncthreads();
  if (!last) return;
  __threadfence();
  zupt_publish(res, OVP_ZUPT_RES_HEAD + n, host_block, word, seq);
  if (t == 0) *ticket = 0u;
}

}  // namespace ovp

// imu_id: the value the staged block holds (the gate reads it there, rows and apply take it as an argument)
extern "C" hipError_t ovp_launch_zupt(double* P, int ld, int n, int imu_id, const ovp::ZuptParams* zp, const double* readings,
                                      double* work, double* Y, double* res, unsigned* ticket, void* host_block, unsigned* word,
                                      unsigned seq, hipEvent_t* ev, hipStream_t stream) {
  if (n < 1 || ld < n || imu_id < 0 || imu_id + 15 > n || (((size_t)res | (size_t)host_block) & 7)) return hipErrorInvalidValue;
  hipError_t e = hipSuccess;
  auto mark = [&](int k) {
    if (ev && e == hipSuccess) e = hipEventRecord(ev[k], stream);
  };
  const int nt = (n + 15) / 16;
  mark(0);
  hipLaunchKernelGGL(ovp::k_zupt_gate, dim3(1), dim3(256), 0, stream, (const double*)P, ld, zp, readings, work, res);
  mark(1);
  hipLaunchKernelGGL(ovp::k_zupt_rows, dim3((n + 63) / 64), dim3(64), 0, stream, (const double*)P, ld, n, imu_id, (const double*)work, Y,
                     res);
  mark(2);
  hipLaunchKernelGGL(ovp::k_zupt_apply, dim3(nt * (nt + 1) / 2), dim3(256), 0, stream, P, ld, n, imu_id, (const double*)work,
                     (const double*)Y, res, ticket, (unsigned long long*)host_block, (volatile unsigned*)word, seq);
  mark(3);
  return e != hipSuccess ? e : hipGetLastError();
}
