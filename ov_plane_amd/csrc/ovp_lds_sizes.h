// LDS sizes of the SLAM kernels (k_slam.hip, k_init.hip, k_dinit.hip) and the limits the host compares them against.  Plain C++,
// no HIP header: the launchers, the entry points (through ovp_ctx.h) and the host-only planner (ovp_slam_plan.h) share it.
#pragma once
#include <stddef.h>

// ---- k_slam_gate / k_slam_gate_gen (k_slam_body.h) ----
#define SL_CW 16                                      // columns of P_marg staged per chunk
static const size_t OVP_SLAM_GATE_MAX_LDS = 150 * 1024;  // a landmark's block beyond it is refused; with its copy of H only below it
inline size_t ovp_slam_gate_lds(int rows_max, int cols_max, int with_h) {
  size_t d = (size_t)rows_max * (rows_max + 2) + rows_max + (size_t)rows_max * SL_CW + (size_t)cols_max * SL_CW +
             (size_t)((cols_max + 1) / 2 + 1);
  if (with_h) d += (size_t)rows_max * cols_max;
  return d * sizeof(double);
}

// ---- k_init_core and its _sk instance: StateHelper::initialize / the S-form EKF update in one workgroup ----
// LDS bytes of k_init_core without its copy of H^T; the caller refuses problems above ovp_init_max_lds()
inline size_t ovp_init_core_lds(int k, int rup, int cols) {
  return sizeof(double) * ((size_t)cols * (k + rup) + (size_t)rup * (2 * rup + 2));
}
inline size_t ovp_init_max_lds() { return 152 * 1024; }
inline int ovp_init_max_rows() { return 80; }
// k new columns and rup update rows over cols columns fit the one workgroup (k = 0: the S-form of StateHelper::EKFUpdate)
inline bool ovp_init_fits(int k, int rup, int cols) {
  return rup <= ovp_init_max_rows() && ovp_init_core_lds(k, rup, cols) <= ovp_init_max_lds();
}

// ---- k_dinit_rows and its _gen / _pl instances ----
#define OVP_DINIT_DYN_LDS (138 * 1024)  // dynamic LDS of k_dinit_rows (160 KB minus its static tables)
#define DINIT_MAX_ROWS_THREADS 1024     // (one thread per row in the rows kernel's workgroup)
// rows = 2m or (the _pl instances) 3m, cols = columns of H_x with the plane's three
inline size_t ovp_dinit_pl_rows_lds(int rows, int cols) {
  const int W = (cols + 4) | 1;
  return sizeof(double) * ((size_t)rows * W + rows + 8 + (size_t)(cols + 2) / 2 + 2);
}
inline size_t ovp_dinit_gen_rows_lds(int m_obs, int cols) { return ovp_dinit_pl_rows_lds(2 * m_obs, cols); }
inline size_t ovp_dinit_rows_lds(int m_obs, int ncal) { return ovp_dinit_pl_rows_lds(2 * m_obs, 6 * m_obs + ncal); }
