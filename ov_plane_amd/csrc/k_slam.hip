// UpdaterSLAM::update on the device (update/UpdaterSLAM.cpp:424-673): one workgroup per landmark that has new measurements.
//
//   rows      get_feature_jacobian_full for a landmark that is a state variable (update/UpdaterHelper.cpp:195-513): the bearing rows
//             of its observations over [clone | calibration | landmark] and, when it lies on a plane of the state, the m identical
//             point-on-plane rows over [landmark | closest point] (:448-512) - built here from the device tables for GLOBAL_3D
//             landmarks; landmarks in an anchored / inverse-depth representation arrive with their dense block from the host
//             (the representation Jacobians of :35-193 are host scalar code), the gate below is the same
//   gate      chi2 = res^T (H P_marg H^T + I)^-1 res against the RESIDENT covariance (:526-547): P_marg is gathered column chunk by
//             column chunk into LDS, S eliminated in LDS (Gaussian elimination without pivoting = the LLT of :532, one barrier per
//             column).  The bearing rows come first, so the statistic of the no-plane fallback (:547-609: the same rows without
//             the constraint) is the partial sum over the leading 2 m pivots of the SAME elimination - no second pass
//   scatter   accepted rows go into the stacked system H^T [global columns][rows] that StateHelper::EKFUpdate (k_init.hip S-form,
//             or the information form above 80 rows) reads; rejected landmarks / dropped constraint rows stay zero rows, which
//             change neither the correction nor the covariance (S gets a unit pivot, W a zero column)
// general   k_slam_gate_gen (ovp_slam_update_general): the same body (k_slam_body.h), every observation with its own camera's tables
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_slam.h"
#include "ovp_lds_sizes.h"
#include "ovp_feat_model.h"

namespace ovp {

__global__ __launch_bounds__(256) void k_slam_gate(SlamParams sp) {
#define SLAM_GEN 0
#include "k_slam_body.h"
#undef SLAM_GEN
}

__global__ __launch_bounds__(256) void k_slam_gate_gen(SlamGenParams gp) {
  const SlamParams& sp = gp.sp;
#define SLAM_GEN 1
#include "k_slam_body.h"
#undef SLAM_GEN
}

}  // namespace ovp

extern "C" {
hipError_t ovp_launch_slam_gate(const ovp::SlamParams* sp, int n_landmarks, size_t lds, hipStream_t stream) {
  static unsigned long long attr_mask = 0;  // per device (ovp_kernels.h)
  if (ovp_lds_attr_needed(&attr_mask)) {
    (void)hipFuncSetAttribute((const void*)ovp::k_slam_gate, hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024);
    (void)hipGetLastError();  // (a kernel with static LDS refuses the full 160 KB: harmless, a real shortage fails the launch itself)
    ovp_lds_attr_done(&attr_mask);
  }
  hipLaunchKernelGGL(ovp::k_slam_gate, dim3(n_landmarks), dim3(256), lds, stream, *sp);
  return hipGetLastError();
}

hipError_t ovp_launch_slam_gate_gen(const ovp::SlamGenParams* gp, int n_landmarks, size_t lds, hipStream_t stream) {
  static unsigned long long attr_mask = 0;  // per device (ovp_kernels.h)
  if (ovp_lds_attr_needed(&attr_mask)) {
    (void)hipFuncSetAttribute((const void*)ovp::k_slam_gate_gen, hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024);
    (void)hipGetLastError();
    ovp_lds_attr_done(&attr_mask);
  }
  hipLaunchKernelGGL(ovp::k_slam_gate_gen, dim3(n_landmarks), dim3(256), lds, stream, *gp);
  return hipGetLastError();
}
}
