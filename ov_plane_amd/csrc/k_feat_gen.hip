// General point features on the device (ovp_msckf_general_features): observations of any camera, tracks of up to
// OVP_GEN_MAX_MEAS_DEV views - the features the wave-per-feature batch (k_feat.hip) cannot carry.  update/UpdaterHelper.cpp:195-440
// (rows), :515-546 (nullspace projection), update/UpdaterMSCKF.cpp:739-757 (gate against the prior).
//
// k_feat_gen: one workgroup of 256 threads per feature, everything of the gate in LDS.
//   rows      thread i < 2m builds row i with ovp_feat_model.h (the camera of the observation picks the calibration block);
//             a row is non-zero on 20 state columns only: its clone's 6 and its camera's 14.
//   projector U = orthonormal basis of range(H_f) (modified Gram-Schmidt, twice, in wave 0); Pi = I - U U^T.  The Givens rotations
//             of the reference leave N^T H_x with N an orthonormal basis of the complement - any such basis gives the same
//             chi2 and the same H^T Pi H, so the 2m rows are kept and Pi is applied instead of rotating them away.
//   gate      M = Pi B Pi + I with B = H_x P H_x^T (2 x 2 blocks per pair of observations, 20 x 20 blocks of P read from the resident
//             covariance), y = Pi r; chi2 = y^T M^-1 y = (N^T r)^T (N^T B N + I)^-1 (N^T r) - the reference's statistic (M is
//             N S N^T + U U^T).  Bordered Cholesky of [M | y] in packed LDS storage: (2m + 1)(2m + 2) / 2 <= 8385 doubles.
//   rows out  an accepted feature writes Hp = Pi H_x over its involved columns and y to global memory (the rows do not fit in LDS
//             beside M at 64 views: 128 x (6 * 64 + 14 * 4) doubles).
// k_gen_pair: one thread per entry of [A | b] over the union of the columns, the features added in index order: no atomics, the
// pair is the same bit for bit from run to run.
#include "ovplane_hip.h"
#include "ovp_dev.h"
#include "ovp_feat_model.h"
#include "ovp_kernels.h"

namespace ovp {

static constexpr int GEN_THREADS = 256;
static constexpr int GEN_ROWS = 2 * OVP_GEN_MAX_MEAS_DEV;              // 128
static constexpr int GEN_MPK = (GEN_ROWS + 1) * (GEN_ROWS + 2) / 2;    // packed [M | y] rows
static constexpr int GEN_NZ = 20;                                       // non-zero columns of a row: clone (6) + camera (14)

struct GenLds {
  double J[GEN_ROWS][GEN_NZ];  // row i: clone block (6) | extrinsics (6) | intrinsics (8), whitened
  double hf[GEN_ROWS][3];
  double r[GEN_ROWS];
  double U[GEN_ROWS][3];
  double BU[GEN_ROWS][3];
  double y[GEN_ROWS];
  double M[GEN_MPK];
  double small[16];            // [0..8] U^T B U, [9..11] U^T r, [12] pivot
  int col[OVP_GEN_MAX_MEAS_DEV][GEN_NZ];  // state column of every non-zero of observation a, -1 = not estimated
  int flag;
};

__device__ __forceinline__ double sym_at(const double* Mp, int i, int j) { return i >= j ? Mp[tri(i, j)] : Mp[tri(j, i)]; }

__global__ __launch_bounds__(GEN_THREADS) void k_feat_gen(const GenParams g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gen_lds_raw[];
  GenLds& s = *reinterpret_cast<GenLds*>(gen_lds_raw);
  const int f = blockIdx.x, tid = threadIdx.x;
  const int m = g.n_meas[f], nr = 2 * m;
  if (m < 2 || m > OVP_GEN_MAX_MEAS_DEV) {  // (the host refuses m > OVP_GEN_MAX_MEAS_DEV; fewer than two views: no rows)
    if (tid == 0) {
      g.chi2[f] = 0.0;
      g.accept[f] = 0;
    }
    return;
  }
  const size_t ob = (size_t)f * g.max_meas;
  // ---- rows (UpdaterHelper.cpp:335-440) ----
  if (tid < nr) {
    const int a = tid >> 1, rr = tid & 1;
    const int ci = g.clone_idx[ob + a], cam = g.cam_idx[ob + a];
    FeatParams p = g.fp;
    p.cal = g.cam_cal + 20 * cam;
    p.fisheye = g.cam_fisheye[cam];
    p.uv = g.uv;
    p.max_meas = g.max_meas;
    p.p_FinG = g.p_FinG;
    double jrow[6], crow[14], h[3], res;
    build_bearing_row<false>(p, f, a, rr, true, ci, jrow, crow, h, res);
#pragma unroll
    for (int k = 0; k < 6; ++k) s.J[tid][k] = jrow[k];
#pragma unroll
    for (int k = 0; k < 14; ++k) s.J[tid][6 + k] = crow[k];
    s.hf[tid][0] = h[0];
    s.hf[tid][1] = h[1];
    s.hf[tid][2] = h[2];
    s.r[tid] = res;
    if (rr == 0) {
      const int cid = g.fp.clone_id[ci], kid = g.cam_calib_id[cam], iid = g.cam_intr_id[cam];
#pragma unroll
      for (int k = 0; k < 6; ++k) s.col[a][k] = cid + k;
#pragma unroll
      for (int k = 0; k < 14; ++k) s.col[a][6 + k] = ((g.fp.calmask >> k) & 1) ? (k < 6 ? kid + k : iid + (k - 6)) : -1;
    }
  }
  if (tid == 0) s.flag = 0;
  __syncthreads();
  // ---- U: orthonormal basis of range(H_f), wave 0, lane l holds rows l and l + 64 ----
  if (tid < 64) {
    double u[2][3];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int c = 0; c < 3; ++c) u[h][c] = (tid + 64 * h < nr) ? s.hf[tid + 64 * h][c] : 0.0;
    bool degenerate = false;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
      for (int pass = 0; pass < 2; ++pass)
#pragma unroll
        for (int d = 0; d < c; ++d) {
          const double dot = wave_sum(u[0][d] * u[0][c] + u[1][d] * u[1][c]);
          u[0][c] -= dot * u[0][d];
          u[1][c] -= dot * u[1][d];
        }
      const double nrm = sqrt(wave_sum(u[0][c] * u[0][c] + u[1][c] * u[1][c]));
      degenerate = degenerate || !(nrm > 0.0);
      const double inv = nrm > 0.0 ? 1.0 / nrm : 0.0;
      u[0][c] *= inv;
      u[1][c] *= inv;
    }
#pragma unroll
    for (int h = 0; h < 2; ++h)
      if (tid + 64 * h < nr)
#pragma unroll
        for (int c = 0; c < 3; ++c) s.U[tid + 64 * h][c] = u[h][c];
    if (tid == 0 && degenerate) s.flag = 1;  // H_f without full column rank: the reference's projection is not defined
  }
  // ---- B = H_x P H_x^T, 2 x 2 block of every pair of observations (a >= b) into the packed lower triangle of M ----
  const int npairs = m * (m + 1) / 2;
  for (int pi = tid; pi < npairs; pi += GEN_THREADS) {
    int a = (int)((sqrt(8.0 * pi + 1.0) - 1.0) * 0.5);
    while (a * (a + 1) / 2 > pi) --a;
    while ((a + 1) * (a + 2) / 2 <= pi) ++a;
    const int b = pi - a * (a + 1) / 2;
    int cb[GEN_NZ];
#pragma unroll
    for (int l = 0; l < GEN_NZ; ++l) cb[l] = s.col[b][l];
    double t0[GEN_NZ], t1[GEN_NZ];
#pragma unroll
    for (int l = 0; l < GEN_NZ; ++l) t0[l] = t1[l] = 0.0;
    for (int k = 0; k < GEN_NZ; ++k) {
      const int ck = s.col[a][k];
      if (ck < 0) continue;
      const double j0 = s.J[2 * a][k], j1 = s.J[2 * a + 1][k];
      const double* Prow = g.P + (size_t)ck * g.ldp;
#pragma unroll
      for (int l = 0; l < GEN_NZ; ++l) {
        const double pv = cb[l] >= 0 ? Prow[cb[l] >= 0 ? cb[l] : 0] : 0.0;  // (the load stays inside P whatever the compiler hoists)
        t0[l] += j0 * pv;
        t1[l] += j1 * pv;
      }
    }
    double b00 = 0.0, b01 = 0.0, b10 = 0.0, b11 = 0.0;
#pragma unroll
    for (int l = 0; l < GEN_NZ; ++l) {
      const double jb0 = s.J[2 * b][l], jb1 = s.J[2 * b + 1][l];
      b00 += t0[l] * jb0;
      b01 += t0[l] * jb1;
      b10 += t1[l] * jb0;
      b11 += t1[l] * jb1;
    }
    s.M[tri(2 * a, 2 * b)] = b00;
    s.M[tri(2 * a + 1, 2 * b)] = b10;
    s.M[tri(2 * a + 1, 2 * b + 1)] = b11;
    if (a != b) s.M[tri(2 * a, 2 * b + 1)] = b01;
  }
  __syncthreads();
  // ---- projection: M = Pi B Pi + I, y = Pi r ----
  if (tid < nr) {
    double acc[3] = {0.0, 0.0, 0.0};
    for (int j = 0; j < nr; ++j) {
      const double bij = sym_at(s.M, tid, j);
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] += bij * s.U[j][c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) s.BU[tid][c] = acc[c];
  }
  __syncthreads();
  if (tid < 64) {
    double v[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) v[k] = 0.0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int i = tid + 64 * h;
      if (i < nr) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
          for (int d = 0; d < 3; ++d) v[3 * c + d] += s.U[i][c] * s.BU[i][d];
          v[9 + c] += s.U[i][c] * s.r[i];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) v[k] = wave_sum(v[k]);
    if (tid < 12) {
      double w = v[0];
#pragma unroll
      for (int k = 1; k < 12; ++k) w = tid == k ? v[k] : w;
      s.small[tid] = w;
    }
  }
  __syncthreads();
  {
    const int ntri = nr * (nr + 1) / 2;
    for (int e = tid; e < ntri + nr; e += GEN_THREADS) {
      if (e < ntri) {
        int i = (int)((sqrt(8.0 * e + 1.0) - 1.0) * 0.5);
        while (i * (i + 1) / 2 > e) --i;
        while ((i + 1) * (i + 2) / 2 <= e) ++i;
        const int j = e - i * (i + 1) / 2;
        double v = s.M[e] + (i == j ? 1.0 : 0.0);
        double q = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          v -= s.BU[i][c] * s.U[j][c] + s.U[i][c] * s.BU[j][c];
#pragma unroll
          for (int d = 0; d < 3; ++d) q += s.U[i][c] * s.small[3 * c + d] * s.U[j][d];
        }
        s.M[e] = v + q;
      } else {
        const int j = e - ntri;
        const double yj = s.r[j] - (s.U[j][0] * s.small[9] + s.U[j][1] * s.small[10] + s.U[j][2] * s.small[11]);
        s.y[j] = yj;
        s.M[tri(nr, j)] = yj;
      }
    }
  }
  __syncthreads();
  // ---- bordered Cholesky of [M | y]: row nr becomes L^-1 y ----
  for (int k = 0; k < nr; ++k) {
    if (tid == 0) {
      const double d = s.M[tri(k, k)];
      if (!(d > 0.0)) s.flag = 1;
      s.small[12] = sqrt(d);
      s.M[tri(k, k)] = s.small[12];
    }
    __syncthreads();
    if (s.flag) break;
    const double inv = 1.0 / s.small[12];
    for (int i = k + 1 + tid; i <= nr; i += GEN_THREADS) s.M[tri(i, k)] *= inv;
    __syncthreads();
    for (int i = k + 1 + tid; i <= nr; i += GEN_THREADS) {
      const double lik = s.M[tri(i, k)];
      const int jmax = i < nr ? i : nr - 1;
      for (int j = k + 1; j <= jmax; ++j) s.M[tri(i, j)] -= lik * s.M[tri(j, k)];
    }
    __syncthreads();
  }
  __shared__ int acc_sh;
  if (tid == 0) {
    double x2 = 0.0;
    for (int k = 0; k < nr; ++k) x2 += s.M[tri(nr, k)] * s.M[tri(nr, k)];
    if (s.flag) x2 = INFINITY;
    const bool ok = !s.flag && x2 <= g.chi2_mult * g.chi2_table[nr - 3];
    g.chi2[f] = x2;
    g.accept[f] = ok ? 1 : 0;
    acc_sh = ok ? 1 : 0;
  }
  __syncthreads();
  if (!acc_sh) return;
  // ---- the projected rows of an accepted feature: Hp = Pi H_x over its q columns (column-major), then y ----
  const int q = g.q[f];
  double* blk = g.hp + g.hp_off[f];
  for (int e = tid; e < nr * q; e += GEN_THREADS) blk[e] = 0.0;
  __syncthreads();
  if (tid < nr) {
    const int a = tid >> 1;
    const int* loc = g.loc + (size_t)f * g.nu;
    for (int k = 0; k < GEN_NZ; ++k) {
      const int ck = s.col[a][k];
      if (ck < 0) continue;
      blk[(size_t)loc[g.upos[ck]] * nr + tid] = s.J[tid][k];
    }
    blk[(size_t)q * nr + tid] = s.y[tid];
  }
  __syncthreads();
  for (int cc = tid; cc < q; cc += GEN_THREADS) {
    double* colp = blk + (size_t)cc * nr;
    double t[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < nr; ++i) {
      const double h = colp[i];
#pragma unroll
      for (int c = 0; c < 3; ++c) t[c] += s.U[i][c] * h;
    }
    for (int i = 0; i < nr; ++i) colp[i] -= s.U[i][0] * t[0] + s.U[i][1] * t[1] + s.U[i][2] * t[2];
  }
}

// [A | b] over the union of the columns: A[u][v] = sum_f Hp_f[:, u]^T Hp_f[:, v], b[v] = sum_f Hp_f[:, v]^T y_f over the accepted
// features in index order (row u = nu of the grid is b)
__global__ __launch_bounds__(256) void k_gen_pair(const GenParams g, double* __restrict__ A, double* __restrict__ b) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  const int nu = g.nu;
  if (e >= (long long)(nu + 1) * nu) return;
  const int u = (int)(e / nu), v = (int)(e % nu);
  if (u < nu && v > u) return;
  double acc = 0.0;
  for (int f = 0; f < g.n_feats; ++f) {
    if (!g.accept[f]) continue;
    const int* loc = g.loc + (size_t)f * nu;
    const int lv = loc[v];
    if (lv < 0) continue;
    const int lu = u < nu ? loc[u] : g.q[f];  // (column q of the block is y)
    if (lu < 0) continue;
    const int nr = 2 * g.n_meas[f];
    const double* cu = g.hp + g.hp_off[f] + (size_t)lu * nr;
    const double* cv = g.hp + g.hp_off[f] + (size_t)lv * nr;
    for (int i = 0; i < nr; ++i) acc += cu[i] * cv[i];
  }
  if (u < nu) {
    A[(size_t)u * nu + v] = acc;
    A[(size_t)v * nu + u] = acc;
  } else {
    b[v] = acc;
  }
}

}  // namespace ovp

extern "C" hipError_t ovp_launch_feat_gen(const ovp::GenParams* g, hipStream_t stream) {
  if (g->n_feats <= 0) return hipSuccess;
  const size_t lds = sizeof(ovp::GenLds);
  static unsigned long long attr_mask = 0;  // per device (ovp_kernels.h)
  if (ovp_lds_attr_needed(&attr_mask)) {
    const hipError_t e = hipFuncSetAttribute((const void*)ovp::k_feat_gen, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    ovp_lds_attr_done(&attr_mask);
  }
  hipLaunchKernelGGL(ovp::k_feat_gen, dim3(g->n_feats), dim3(ovp::GEN_THREADS), lds, stream, *g);
  return hipGetLastError();
}

extern "C" hipError_t ovp_launch_gen_pair(const ovp::GenParams* g, double* A, double* b, hipStream_t stream) {
  const long long n = (long long)(g->nu + 1) * g->nu;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(ovp::k_gen_pair, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, *g, A, b);
  return hipGetLastError();
}
