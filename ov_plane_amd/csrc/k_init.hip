// StateHelper::initialize downstream of its Givens split (state/StateHelper.cpp:448-487) as three kernels: the Mahalanobis gate
// on the prior (:464-475), StateHelper::initialize_invertible (:489-586) and the EKF update with the remaining rows in the
// reference's own S-form (StateHelper::EKFUpdate, :121-202).  The update rows of one landmark are few (2 m - 3): S = H P H^T + R
// is a small LDS matrix, and P+ = P - W W^T with W = P H^T L^-T is a rank-rup downdate every tile of P takes independently.
//
// Everything here is latency-bound (a few hundred kFLOP): the kernels are laid out so that no thread runs a loop of dependent
// global loads - gathers are staged into LDS by all threads at once, the K-loops then read LDS or unit-stride global memory.
//
//   H_all = [H_init ; H_up]   (m = k + rup rows), handed over transposed: Ht [cols][m]
//   k_init_m       M_all = P[:, ids] H_all^T                       n x m, many workgroups
//   k_init_core    S = H_up M_up[ids] + r I = L L^T, chi2 = |L^-1 res|^2, L^-1;  the new rows / columns of P   one workgroup
//   k_init_update  P+ = P - W W^T, dx = W y  with  W = M_up L^-T,  y = L^-1 res    (n + k)^2 / 256 workgroups
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ovp_dev.h"
#include "ovp_kernels.h"
#include "ovp_lds_sizes.h"

namespace ovp {

#define IM_ROWS 8
#define IC_MAX_COLS 704  // = OVP_LDG_CAP: columns of one dense block
#define IC_MAXE 13  // elements of [S | res | I] a thread of k_init_core owns: ceil(80 * 161 / 1024)
// grid = ceil(n / 8), 256 threads = 8 rows x 32 column lanes; dynamic LDS: 8 x cols doubles (+ cols x m for H^T, hs_in_lds)
__global__ __launch_bounds__(256) void k_init_m(const double* __restrict__ P, int ldp, int n, const int* __restrict__ ids, int cols,
                                                 const double* __restrict__ Ht, int m, double* __restrict__ Mall, int hs_in_lds) {
#define IB_PART 1
#include "k_init_body.h"
#undef IB_PART
}

// k_init_m behind a device-side predicate: skip[1] > 0.5 (attempt A of the same candidate was accepted) = nothing to do
__global__ __launch_bounds__(256) void k_init_m_sk(const double* __restrict__ skip, const double* __restrict__ P, int ldp, int n,
                                                    const int* __restrict__ ids, int cols, const double* __restrict__ Ht, int m,
                                                    double* __restrict__ Mall, int hs_in_lds) {
  if (skip[1] > 0.5) return;
#define IB_PART 1
#include "k_init_body.h"
#undef IB_PART
}

template <int NE>
__device__ __forceinline__ void ic_eliminate(double* Wm, int ldw, int rup, int W, int t, int* bad) {
  const int tot = rup * W;
  double v[NE];
  int ei[NE], ej[NE];
#pragma unroll
  for (int q = 0; q < NE; ++q) {
    const int e = t + 1024 * q;
    ei[q] = e < tot ? e / W : 0;      // (an element of row 0 is never touched: i > c fails for every c)
    ej[q] = e < tot ? e - ei[q] * W : 0;
    v[q] = Wm[ei[q] * ldw + ej[q]];
  }
  for (int c = 0; c < rup; ++c) {
    const double* rc = Wm + c * ldw;
    const double piv = rc[c];
    if (t == 0 && !(piv > 0.0)) *bad = 1;
    const double ip = 1.0 / piv;
#pragma unroll
    for (int q = 0; q < NE; ++q) {
      if (ei[q] > c && ej[q] > c) {
        v[q] = fma(-(rc[ei[q]] * ip), rc[ej[q]], v[q]);
        if (ei[q] == c + 1) Wm[(c + 1) * ldw + ej[q]] = v[q];
      }
    }
    __syncthreads();
  }
}

// One workgroup of 1024.  Dynamic LDS: Mg [cols][m] | Wm [rup][2 rup + 2] | Hs [cols][m] (only when it fits, hs_in_lds).
//   res[0] = chi2, res[1] = 1 accept / 0 reject (a non-positive pivot of S rejects), res[2] = 0 (the update's negative-diagonal
//   mark).  With rup == 0 there is no gate: res = {0, 1, 0}.
// Writes the k new rows / columns of P (harmless when the gate says no: the dimension then stays n), rows n .. n + k of M_up,
// Linv [rup][rup] row-major and y.
// The factorization is Gaussian elimination of [S | res | I] without pivoting, one barrier per column: row c of the reduced
// matrix is final after step c - 1, and divided by the square root of its pivot it is [L^T row c | y_c | L^-1 row c].
__global__ __launch_bounds__(1024) void k_init_core(double* __restrict__ P, int ldp, int n, const int* __restrict__ ids, int cols,
                                                     const double* __restrict__ Ht, int k, int rup, double* __restrict__ Mall,
                                                     const double* __restrict__ Hinv, const double* __restrict__ Rk,
                                                     const double* __restrict__ resid, double r_iso, double thr,
                                                     double* __restrict__ Linv, double* __restrict__ y, double* __restrict__ res,
                                                     int hs_in_lds) {
#define IB_PART 2
#include "k_init_body.h"
#undef IB_PART
}

// k_init_core behind the same predicate (the new rows / columns of P it would write are the accepted attempt's)
__global__ __launch_bounds__(1024) void k_init_core_sk(const double* __restrict__ skip, double* __restrict__ P, int ldp, int n,
                                                        const int* __restrict__ ids, int cols, const double* __restrict__ Ht, int k, int rup,
                                                        double* __restrict__ Mall, const double* __restrict__ Hinv,
                                                        const double* __restrict__ Rk, const double* __restrict__ resid, double r_iso,
                                                        double thr, double* __restrict__ Linv, double* __restrict__ y,
                                                        double* __restrict__ res, int hs_in_lds) {
  if (skip[1] > 0.5) return;
#define IB_PART 2
#include "k_init_body.h"
#undef IB_PART
}

#define IU_T 16
// Grid (T, T), T = ceil(n2 / 16); 256 threads.  Dynamic LDS: Li [rup][rup] | Mi, Mj [16][rup] | Wi, Wj [16][rup + 1].
// Pdst[tile] = Psrc[tile] - W_I W_J^T; the tiles of block column 0 also leave dx = W y.  Nothing is written when the gate said
// no (res[1] == 0): the caller then keeps Psrc.
__global__ __launch_bounds__(256) void k_init_update(const double* Psrc, double* Pdst /* may be Psrc: an element is read and written by its own thread only */, int ldp, int n2,
                                                      const double* __restrict__ Mall, int m, int k, int rup,
                                                      const double* __restrict__ Linv, const double* __restrict__ y,
                                                      double* __restrict__ res, double* __restrict__ dx) {
#define IB_PART 3
#include "k_init_body.h"
#undef IB_PART
}


// k_init_update behind the same predicate: when attempt A was accepted, workgroup (0, 0) forwards A's result block (res_len doubles)
// into this attempt's and nothing else happens - whoever reads `res` afterwards reads the block of the attempt that decided
__global__ __launch_bounds__(256) void k_init_update_sk(const double* __restrict__ skip, int res_len, const double* Psrc, double* Pdst,
                                                         int ldp, int n2, const double* __restrict__ Mall, int m, int k, int rup,
                                                         const double* __restrict__ Linv, const double* __restrict__ y,
                                                         double* __restrict__ res, double* __restrict__ dx) {
  if (skip[1] > 0.5) {
    if (blockIdx.x == 0 && blockIdx.y == 0)
      for (int e = threadIdx.x; e < res_len; e += 256) res[e] = skip[e];
    return;
  }
#define IB_PART 3
#include "k_init_body.h"
#undef IB_PART
}

}  // namespace ovp

extern "C" {
// skip == nullptr: the plain kernels; otherwise their _sk instances, which do nothing when skip[1] > 0.5 (k_init_update_sk then
// copies skip[0 .. res_len) to res)
hipError_t ovp_launch_init_m_sk(const double* skip, const double* P, int ldp, int n, const int* ids, int cols, const double* Ht, int m,
                                double* Mall, hipStream_t stream) {
  size_t lds = sizeof(double) * IM_ROWS * cols;
  const size_t hs = sizeof(double) * (size_t)cols * m;
  const int hs_in_lds = lds + hs <= 60 * 1024;  // keeps several workgroups per CU resident
  if (hs_in_lds) lds += hs;
  if (skip)
    hipLaunchKernelGGL(ovp::k_init_m_sk, dim3((n + IM_ROWS - 1) / IM_ROWS), dim3(256), lds, stream, skip, P, ldp, n, ids, cols, Ht, m,
                       Mall, hs_in_lds);
  else
    hipLaunchKernelGGL(ovp::k_init_m, dim3((n + IM_ROWS - 1) / IM_ROWS), dim3(256), lds, stream, P, ldp, n, ids, cols, Ht, m, Mall,
                       hs_in_lds);
  return hipGetLastError();
}

hipError_t ovp_launch_init_m(const double* P, int ldp, int n, const int* ids, int cols, const double* Ht, int m, double* Mall,
                             hipStream_t stream) {
  return ovp_launch_init_m_sk(nullptr, P, ldp, n, ids, cols, Ht, m, Mall, stream);
}

hipError_t ovp_launch_init_core_sk(const double* skip, double* P, int ldp, int n, const int* ids, int cols, const double* Ht, int k,
                                   int rup, double* Mall, const double* Hinv, const double* Rk, const double* resid, double r_iso,
                                   double thr, double* Linv, double* y, double* res, hipStream_t stream) {
  static unsigned long long attr_mask = 0;  // per device (ovp_kernels.h)
  if (ovp_lds_attr_needed(&attr_mask)) {
    (void)hipFuncSetAttribute((const void*)ovp::k_init_core, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ovp_init_max_lds());
    (void)hipFuncSetAttribute((const void*)ovp::k_init_update, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ovp_init_max_lds());
    (void)hipFuncSetAttribute((const void*)ovp::k_init_m, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ovp_init_max_lds());
    (void)hipFuncSetAttribute((const void*)ovp::k_init_core_sk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ovp_init_max_lds());
    (void)hipFuncSetAttribute((const void*)ovp::k_init_update_sk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ovp_init_max_lds());
    (void)hipFuncSetAttribute((const void*)ovp::k_init_m_sk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ovp_init_max_lds());
    (void)hipGetLastError();  // (a kernel with static LDS refuses the full 160 KB: harmless, a real shortage fails the launch itself)
    ovp_lds_attr_done(&attr_mask);
  }
  size_t lds = ovp_init_core_lds(k, rup, cols);
  const size_t hs = sizeof(double) * (size_t)cols * (k + rup);
  const int hs_in_lds = lds + hs <= ovp_init_max_lds();
  if (hs_in_lds) lds += hs;
  if (skip)
    hipLaunchKernelGGL(ovp::k_init_core_sk, dim3(1), dim3(1024), lds, stream, skip, P, ldp, n, ids, cols, Ht, k, rup, Mall, Hinv, Rk,
                       resid, r_iso, thr, Linv, y, res, hs_in_lds);
  else
    hipLaunchKernelGGL(ovp::k_init_core, dim3(1), dim3(1024), lds, stream, P, ldp, n, ids, cols, Ht, k, rup, Mall, Hinv, Rk, resid, r_iso,
                       thr, Linv, y, res, hs_in_lds);
  return hipGetLastError();
}

hipError_t ovp_launch_init_core(double* P, int ldp, int n, const int* ids, int cols, const double* Ht, int k, int rup, double* Mall,
                                const double* Hinv, const double* Rk, const double* resid, double r_iso, double thr, double* Linv,
                                double* y, double* res, hipStream_t stream) {
  return ovp_launch_init_core_sk(nullptr, P, ldp, n, ids, cols, Ht, k, rup, Mall, Hinv, Rk, resid, r_iso, thr, Linv, y, res, stream);
}

hipError_t ovp_launch_init_update_sk(const double* skip, int res_len, const double* Psrc, double* Pdst, int ldp, int n2,
                                     const double* Mall, int m, int k, int rup, const double* Linv, const double* y, double* res,
                                     double* dx, hipStream_t stream) {
  const int T = (n2 + IU_T - 1) / IU_T;
  const size_t lds = sizeof(double) * ((size_t)rup * rup + 2 * IU_T * rup + 2 * IU_T * (rup + 1));
  if (skip)
    hipLaunchKernelGGL(ovp::k_init_update_sk, dim3(T, T), dim3(256), lds, stream, skip, res_len, Psrc, Pdst, ldp, n2, Mall, m, k, rup,
                       Linv, y, res, dx);
  else
    hipLaunchKernelGGL(ovp::k_init_update, dim3(T, T), dim3(256), lds, stream, Psrc, Pdst, ldp, n2, Mall, m, k, rup, Linv, y, res, dx);
  return hipGetLastError();
}

hipError_t ovp_launch_init_update(const double* Psrc, double* Pdst, int ldp, int n2, const double* Mall, int m, int k, int rup,
                                  const double* Linv, const double* y, double* res, double* dx, hipStream_t stream) {
  return ovp_launch_init_update_sk(nullptr, 0, Psrc, Pdst, ldp, n2, Mall, m, k, rup, Linv, y, res, dx, stream);
}
}
