// UpdaterSLAM::delayed_init, candidate loop on the device (update/UpdaterSLAM.cpp:204-364, state/StateHelper.cpp:398-586).
//
// The candidates of a frame are sequential - every StateHelper::initialize ends in an EKF update that moves the poses the next
// candidate's Jacobians are evaluated at - so the loop cannot be batched, but nothing in it needs the HOST: per candidate
//
//   k_dinit_rows    one workgroup: Type::update of the device pose tables with the previous candidate's correction (its
//                   commit), the candidate's bearing rows at those tables (UpdaterHelper.cpp:345-444), the orthogonal split of
//                   H_f = Q [R3; 0] (Householder instead of the Givens sweep of StateHelper.cpp:434-446: init rows, update rows
//                   and everything derived from them are invariant under the choice of the orthogonal factor), H_L^-1 = R3^-1
//   k_init_m        (k_init.hip) M = P[:, ids] [H_init; H_up]^T on many workgroups (forming it inside k_dinit_rows - one workgroup,
//                   prefetched operand - was built in round 5, was no faster and read columns a rejected predecessor had just
//                   rewritten without a fence: removed in round 6)
//   k_init_core     (k_init.hip) chi2 of the update rows against the prior (:464-475), initialize_invertible (:520-573)
//   k_init_update   (k_init.hip) EKFUpdate with the update rows (:483-485), IN PLACE
//
// The covariance grows by three columns per candidate whatever the gate says: a rejected candidate leaves an inert block (unit
// diagonal, zero cross terms - written by the next commit) that no later product reads, so every launch geometry is known to
// the host up front and the whole loop is enqueued without a synchronisation; the host removes the inert blocks afterwards
// (ovp_cov_marginalize; rejections are rare) and applies the corrections to its own copy of the state.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_dinit.h"
#include "ovp_lds_sizes.h"
#include "ovp_feat_model.h"

namespace ovp {

typedef double double4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void dinit_rot_update(double* R, const double* dth) {
  // ext JPLQuat::update on a rotation matrix: R <- R(dq) R, dq = quatnorm([dth / 2, 1])
  double qx = 0.5 * dth[0], qy = 0.5 * dth[1], qz = 0.5 * dth[2], qw = 1.0;
  const double nn = 1.0 / sqrt(qx * qx + qy * qy + qz * qz + qw * qw);
  qx *= nn;
  qy *= nn;
  qz *= nn;
  qw *= nn;
  const double a = 2.0 * qw * qw - 1.0;
  double D[9];
  D[0] = a + 2.0 * qx * qx;
  D[1] = 2.0 * qw * qz + 2.0 * qx * qy;
  D[2] = -2.0 * qw * qy + 2.0 * qx * qz;
  D[3] = -2.0 * qw * qz + 2.0 * qy * qx;
  D[4] = a + 2.0 * qy * qy;
  D[5] = 2.0 * qw * qx + 2.0 * qy * qz;
  D[6] = 2.0 * qw * qy + 2.0 * qz * qx;
  D[7] = -2.0 * qw * qx + 2.0 * qz * qy;
  D[8] = a + 2.0 * qz * qz;
  double O[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) O[3 * i + j] = D[3 * i] * R[j] + D[3 * i + 1] * R[3 + j] + D[3 * i + 2] * R[6 + j];
  for (int i = 0; i < 9; ++i) R[i] = O[i];
}

// workgroup barrier that orders LDS traffic only: __syncthreads() carries a fence the compiler implements with s_waitcnt vmcnt(0),
// which would wait for every global load in flight - here the prefetched operand of the M product
__device__ __forceinline__ void di_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

#define DI_T 1024   // threads of the one workgroup

// (16 waves = 4 per SIMD: 128 VGPRs each; without the attribute the compiler aims at 8 waves per SIMD, stops at 64 registers and
// spills the prefetch to scratch - a dispatch that needs scratch behind ones that do not costs tens of microseconds on this stack)
__global__ __launch_bounds__(DI_T) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_dinit_rows(DinitParams dp) {
#define DI_GEN 0
#define DI_PL 0
#include "k_dinit_body.h"
#undef DI_PL
#undef DI_GEN
}

__global__ __launch_bounds__(DI_T) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_dinit_rows_gen(DinitGenParams gp) {
  const DinitParams& dp = gp.dp;
#define DI_GEN 1
#define DI_PL 0
#include "k_dinit_body.h"
#undef DI_PL
#undef DI_GEN
}

// the two above with the point-on-plane rows, the plane commit and the attempt-B predicate (ovp_slam_delayed_init_planes)
__global__ __launch_bounds__(DI_T) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_dinit_rows_pl(DinitParams dp, DinitPlaneParams pp) {
#define DI_GEN 0
#define DI_PL 1
#include "k_dinit_body.h"
#undef DI_PL
#undef DI_GEN
}

__global__ __launch_bounds__(DI_T) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_dinit_rows_gen_pl(DinitGenParams gp,
                                                                                                        DinitPlaneParams pp) {
  const DinitParams& dp = gp.dp;
#define DI_GEN 1
#define DI_PL 1
#include "k_dinit_body.h"
#undef DI_PL
#undef DI_GEN
}

}  // namespace ovp

extern "C" {
hipError_t ovp_launch_dinit_rows_pl(const ovp::DinitParams* dp, const ovp::DinitPlaneParams* pp, size_t lds, hipStream_t stream) {
  static unsigned long long attr_mask = 0;  // per device (ovp_kernels.h)
  if (ovp_lds_attr_needed(&attr_mask)) {
    (void)hipFuncSetAttribute((const void*)ovp::k_dinit_rows_pl, hipFuncAttributeMaxDynamicSharedMemorySize, OVP_DINIT_DYN_LDS);
    (void)hipGetLastError();
    ovp_lds_attr_done(&attr_mask);
  }
  hipLaunchKernelGGL(ovp::k_dinit_rows_pl, dim3(1), dim3(DI_T), lds, stream, *dp, *pp);
  return hipGetLastError();
}

hipError_t ovp_launch_dinit_rows_gen_pl(const ovp::DinitGenParams* gp, const ovp::DinitPlaneParams* pp, size_t lds, hipStream_t stream) {
  static unsigned long long attr_mask = 0;  // per device (ovp_kernels.h)
  if (ovp_lds_attr_needed(&attr_mask)) {
    (void)hipFuncSetAttribute((const void*)ovp::k_dinit_rows_gen_pl, hipFuncAttributeMaxDynamicSharedMemorySize, OVP_DINIT_DYN_LDS);
    (void)hipGetLastError();
    ovp_lds_attr_done(&attr_mask);
  }
  hipLaunchKernelGGL(ovp::k_dinit_rows_gen_pl, dim3(1), dim3(DI_T), lds, stream, *gp, *pp);
  return hipGetLastError();
}

hipError_t ovp_launch_dinit_rows_gen(const ovp::DinitGenParams* gp, size_t lds, hipStream_t stream) {
  static unsigned long long attr_mask = 0;  // per device (ovp_kernels.h)
  if (ovp_lds_attr_needed(&attr_mask)) {
    (void)hipFuncSetAttribute((const void*)ovp::k_dinit_rows_gen, hipFuncAttributeMaxDynamicSharedMemorySize, OVP_DINIT_DYN_LDS);
    (void)hipGetLastError();
    ovp_lds_attr_done(&attr_mask);
  }
  hipLaunchKernelGGL(ovp::k_dinit_rows_gen, dim3(1), dim3(DI_T), lds, stream, *gp);
  return hipGetLastError();
}

hipError_t ovp_launch_dinit_rows(const ovp::DinitParams* dp, size_t lds, hipStream_t stream) {
  static unsigned long long attr_mask = 0;  // per device (ovp_kernels.h)
  if (ovp_lds_attr_needed(&attr_mask)) {
    (void)hipFuncSetAttribute((const void*)ovp::k_dinit_rows, hipFuncAttributeMaxDynamicSharedMemorySize, OVP_DINIT_DYN_LDS);
    (void)hipGetLastError();  // (a kernel with static LDS refuses the full 160 KB: harmless, a real shortage fails the launch itself)
    ovp_lds_attr_done(&attr_mask);
  }
  hipLaunchKernelGGL(ovp::k_dinit_rows, dim3(1), dim3(DI_T), lds, stream, *dp);
  return hipGetLastError();
}
}
