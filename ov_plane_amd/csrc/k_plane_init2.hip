// Plane initialisation behind the second-generation plane loop (ovp_plane_init_general; update/UpdaterPlane.cpp:296-481 ->
// StateHelper::initialize, state/StateHelper.cpp:398-586).
//
// Initialising a plane is the out-of-state plane update of the loop with a flat prior on the plane: the loop eliminates the three
// plane columns of the extended pair  E = [[E_xx E_xc][E_cx E_cc]], [b_x; b_c]  by their Schur complement, gates, and updates the
// variables that exist.  What is left is to append the plane.  The joint information matrix of (x, cp_1 .. cp_K) is block diagonal
// in the new planes (a plane's rows involve no other new plane), so with Z_k = E_xc,k E_cc,k^-1 and P+ the covariance behind the
// LAST accepted plane
//     Sigma(x, cp_k)    = -P+ Z_k
//     Sigma(cp_j, cp_k) = Z_j^T P+ Z_k + delta_jk E_cc,k^-1
//     d cp_k            = E_cc,k^-1 (b_c,k - E_cx,k dx_k)            (dx_k: the loop's correction for plane k)
//     cp_j             += -Z_j^T dx_k   for every later accepted plane k   (plane j is a state variable by then)
// which is what the sequence initialize, update, initialize, ... of the reference arrives at.  Three kernels, plain launches
// ordered by the stream:
//   k_plane_init_keep     per plane, behind k_plane_assemble2: the three plane rows of the extended pair, from the same partials
//   k_plane_init_solve    once: numbers the accepted planes, E_cc^-1, Z, d cp and the corrections between the new planes
//   k_plane_init_columns  twice: the cross blocks (one workgroup per 16 state columns), then the blocks between the new planes
#include "ovp_dev.h"
#include "ovp_kernels.h"
#include "k_plane_init2.h"

namespace ovp {

static constexpr int PI_THREADS = 320;  // one thread per column of a kept row (nk + 4 <= 292)

// ------------------------------------------------------------------------------------------------------------------------
// The plane rows of the extended pair of an out-of-state plane without SLAM landmarks, entry by entry as k_plane_assemble2 forms
// them (its `finish` for a row of kind 4): state column c: -sum of the G^T G partials; residual column: constraint moment 6 + a minus
// the partials; plane column j: constraint moment (a, j) minus the partials.  Sums in k_plane_assemble2's order.
// ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PI_THREADS) void k_plane_init_keep(const PlaneAsm a, double* __restrict__ keep) {
  const int t = threadIdx.x, n = a.n, w = n + 4;
  __shared__ double red[250], cst[10];
  if (t < 250) {
    const int ce = t % 10, cpart = t / 10;
    double sacc = 0.0;
    for (int f = cpart; f < a.nf; f += 25) sacc += a.cst[(size_t)f * 10 + ce];
    red[t] = sacc;
  }
  __syncthreads();
  if (t < 10) {
    double acc = 0.0;
    for (int l = 0; l < 25; ++l) acc += red[l * 10 + t];
    cst[t] = acc;
  }
  __syncthreads();
  for (int c = t; c < w; c += PI_THREADS)
    for (int r = 0; r < 3; ++r) {
      const int row = n + 1 + r;  // row > c or both among the last three
      const int I = max(row, c), J = min(row, c);
      const int ti = I >> 4, tj = J >> 4;
      const size_t off = (size_t)(ti * (ti + 1) / 2 + tj) * 256 + (I & 15) * 16 + (J & 15);
      double d = 0.0;
      for (int sp = 0; sp < a.n_split; ++sp) d += a.part[(size_t)sp * a.ntile * 256 + off];
      double s = 0.0;
      if (c == n) {
        s = cst[6 + r];
      } else if (c > n) {
        const int j = c - n - 1, lo = min(r, j), hi = max(r, j);
        s = cst[lo == 0 ? hi : (lo == 1 ? 2 + hi : 5)];
      }
      keep[(size_t)r * w + c] = s - d;
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// One workgroup.  Accepted planes are numbered by a prefix count over the loop's decisions (at most n_planes flags).
// ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_plane_init_solve(const PlaneInitTail p) {
  const int t = threadIdx.x, NP = p.n_planes, nk = p.nk, w = nk + 4;
  const int wave = t >> 6, lane = t & 63;
  __shared__ double Ai[9], part[4][3], tot[3];
  __shared__ int n_acc;
  const bool failed = p.flags && (p.flags[0] | p.flags[2]);
  if (t == 0) {
    int q = 0;
    for (int pl = 0; pl < NP; ++pl) {
      const bool ok = !failed && p.res[4 * pl + 1] > 0.5;
      p.slot[pl] = ok ? q : -1;
      if (ok) p.slot[NP + q++] = pl;
    }
    for (int i = q; i < NP; ++i) p.slot[NP + i] = -1;
    n_acc = q;
  }
  __syncthreads();
  const int K = n_acc;
  for (int q = 0; q < K; ++q) {
    const int pl = p.slot[NP + q];
    double* kp = p.keep + (size_t)pl * 3 * w;
    const double* dx = p.dx + (size_t)pl * p.dx_stride;
    if (t == 0) {
      const double a00 = kp[nk + 1], a01 = kp[nk + 2], a02 = kp[nk + 3], a11 = kp[w + nk + 2], a12 = kp[w + nk + 3],
                   a22 = kp[2 * w + nk + 3];
      const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
      const double id = 1.0 / (a00 * c00 + a01 * c01 + a02 * c02);
      Ai[0] = c00 * id;
      Ai[1] = c01 * id;
      Ai[2] = c02 * id;
      Ai[3] = Ai[1];
      Ai[4] = (a00 * a22 - a02 * a02) * id;
      Ai[5] = (a01 * a02 - a00 * a12) * id;
      Ai[6] = Ai[2];
      Ai[7] = Ai[5];
      Ai[8] = (a00 * a11 - a01 * a01) * id;
    }
    // E_cx dx
    double s[3] = {0.0, 0.0, 0.0};
    for (int c = t; c < nk; c += 256) {
      const double d = dx[c];
      for (int r = 0; r < 3; ++r) s[r] = fma(kp[(size_t)r * w + c], d, s[r]);
    }
    for (int r = 0; r < 3; ++r) {
      const double v = wave_sum(s[r]);
      if (lane == 0) part[wave][r] = v;
    }
    __syncthreads();
    if (t < 3) tot[t] = kp[(size_t)t * w + nk] - (((part[0][t] + part[1][t]) + part[2][t]) + part[3][t]);
    __syncthreads();
    if (t < 3) p.extra[3 * pl + t] = Ai[3 * t] * tot[0] + Ai[3 * t + 1] * tot[1] + Ai[3 * t + 2] * tot[2];
    // Z^T = E_cc^-1 E_cx in place, E_cc^-1 over E_cc
    for (int c = t; c < nk; c += 256) {
      const double x0 = kp[c], x1 = kp[w + c], x2 = kp[2 * w + c];
      for (int r = 0; r < 3; ++r) kp[(size_t)r * w + c] = Ai[3 * r] * x0 + Ai[3 * r + 1] * x1 + Ai[3 * r + 2] * x2;
    }
    if (t < 9) kp[(size_t)(t / 3) * w + nk + 1 + (t % 3)] = Ai[t];
    __syncthreads();
  }
  // plane j as a state variable under the later plane k: -Z_j^T dx_k  (one wave per pair)
  for (int pair = wave; pair < K * K; pair += 4) {
    const int qj = pair / K, qk = pair % K;
    if (qj >= qk) continue;
    const int pj = p.slot[NP + qj], pk = p.slot[NP + qk];
    const double* zj = p.keep + (size_t)pj * 3 * w;
    const double* dx = p.dx + (size_t)pk * p.dx_stride;
    double s[3] = {0.0, 0.0, 0.0};
    for (int c = lane; c < nk; c += 64) {
      const double d = dx[c];
      for (int r = 0; r < 3; ++r) s[r] = fma(zj[(size_t)r * w + c], d, s[r]);
    }
    for (int r = 0; r < 3; ++r) {
      const double v = wave_sum(s[r]);
      if (lane == 0) p.extra[3 * NP + ((size_t)pj * NP + pk) * 3 + r] = -v;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------------
// The new rows and columns of P.  One workgroup per 16 rows, 16 lanes per row, every accepted plane in turn.
//   corner == 0: rows = the n_state columns of the state:  P[r][n + 3 q + a] = P[n + 3 q + a][r] = -sum_c P[r][ids[c]] Z_q[a][c]
//   corner == 1: rows = the new columns themselves (the launch behind the first):  for row (qj, a), plane qk >= qj
//                P[n + 3 qj + a][n + 3 qk + b] = -sum_c Z_qj[a][c] P[ids[c]][n + 3 qk + b] + delta_jk E_cc^-1[a][b], and its mirror
// ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_plane_init_columns(const PlaneInitTail p, int corner) {
  if (p.flags && (p.flags[0] | p.flags[2])) return;
  const int NP = p.n_planes, nk = p.nk, w = nk + 4, n = p.n_state;
  const int row = 16 * blockIdx.x + (threadIdx.x >> 4), l = threadIdx.x & 15;
  int K = 0;
  while (K < NP && p.slot[NP + K] >= 0) ++K;
  const size_t ldp = (size_t)p.ldp;
  if (!corner) {
    const bool live = row < n;
    const double* pr = p.P + (size_t)(live ? row : 0) * ldp;
    for (int q = 0; q < K; ++q) {
      const double* z = p.keep + (size_t)p.slot[NP + q] * 3 * w;
      double s[3] = {0.0, 0.0, 0.0};
      if (live)
        for (int c = l; c < nk; c += 16) {
          const double pv = pr[p.ids ? p.ids[c] : c];
          for (int a = 0; a < 3; ++a) s[a] = fma(pv, z[(size_t)a * w + c], s[a]);
        }
      for (int a = 0; a < 3; ++a)
        for (int o = 8; o > 0; o >>= 1) s[a] += __shfl_down(s[a], o, 16);
      if (live && l == 0)
        for (int a = 0; a < 3; ++a) {
          p.P[(size_t)row * ldp + n + 3 * q + a] = -s[a];
          p.P[(size_t)(n + 3 * q + a) * ldp + row] = -s[a];
        }
    }
    return;
  }
  const bool live = row < 3 * K;
  const int qj = live ? row / 3 : 0, a = live ? row % 3 : 0;
  const double* zj = p.keep + (size_t)(K > 0 ? p.slot[NP + qj] : 0) * 3 * w;
  for (int qk = 0; qk < K; ++qk) {
    double s[3] = {0.0, 0.0, 0.0};
    if (live && qk >= qj)
      for (int c = l; c < nk; c += 16) {
        const double zv = zj[(size_t)a * w + c];
        const double* pc = p.P + (size_t)(p.ids ? p.ids[c] : c) * ldp + n + 3 * qk;
        for (int b = 0; b < 3; ++b) s[b] = fma(zv, pc[b], s[b]);
      }
    for (int b = 0; b < 3; ++b)
      for (int o = 8; o > 0; o >>= 1) s[b] += __shfl_down(s[b], o, 16);
    if (live && qk >= qj && l == 0)
      for (int b = 0; b < 3; ++b) {
        if (qk == qj && b < a) continue;  // (the lower half of a diagonal block is the mirror of its upper half)
        const double v = -s[b] + (qk == qj ? zj[(size_t)a * w + nk + 1 + b] : 0.0);
        p.P[(size_t)(n + 3 * qj + a) * ldp + n + 3 * qk + b] = v;
        p.P[(size_t)(n + 3 * qk + b) * ldp + n + 3 * qj + a] = v;
      }
  }
}

}  // namespace ovp

extern "C" {
hipError_t ovp_launch_plane_init_keep(const ovp::PlaneAsm* a, double* keep, hipStream_t stream) {
  hipLaunchKernelGGL(ovp::k_plane_init_keep, dim3(1), dim3(ovp::PI_THREADS), 0, stream, *a, keep);
  return hipGetLastError();
}
hipError_t ovp_launch_plane_init_solve(const ovp::PlaneInitTail* t, hipStream_t stream) {
  hipLaunchKernelGGL(ovp::k_plane_init_solve, dim3(1), dim3(256), 0, stream, *t);
  return hipGetLastError();
}
// both launches: the cross blocks over the state (tiles of 16 columns), then the blocks between the new columns
hipError_t ovp_launch_plane_init_columns(const ovp::PlaneInitTail* t, hipStream_t stream) {
  hipLaunchKernelGGL(ovp::k_plane_init_columns, dim3((t->n_state + 15) / 16), dim3(256), 0, stream, *t, 0);
  if (hipError_t e = hipGetLastError()) return e;
  hipLaunchKernelGGL(ovp::k_plane_init_columns, dim3((3 * t->n_planes + 15) / 16), dim3(256), 0, stream, *t, 1);
  return hipGetLastError();
}
}
