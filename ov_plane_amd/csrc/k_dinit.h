// Parameter block of the delayed-initialisation loop kernel (k_dinit.hip; update/UpdaterSLAM.cpp:204-364).
#pragma once
#include "ovp_kernels.h"

namespace ovp {

struct DinitParams {
  FeatParams fp;          // the candidates as a feature batch (uv, clone_idx, n_meas, p_FinG), pose tables, 1 / sigma_pix, do_fej, calmask
  int cand;               // candidate index in the batch, -1 = commit only (behind the last candidate)
  int m_obs;              // its observations (n_meas[cand]; known to the host, spares the kernel a dependent load)
  int n, n_max;           // covariance dimension in front of this candidate; capacity (layout of the result blocks)
  double* P;              // resident covariance (fp.ldp)
  double* clone_R;        // writable pose tables (the commit of the previous candidate)
  double* clone_p;
  double* cal;
  const double* prev_res; // result block of the previous candidate [chi2 | accepted | negdiag | - | dx (n) ...], nullptr = none
  const int* ids;         // [cols] state columns of the candidate's H_x: clone blocks in observation order, estimated calibration
  int idv[208];           // the same list by value (scalar reads in the kernel; 6 * OVP_MAX_MEAS + 14 = 206 entries at most)
  // outputs for k_init_m / k_init_core / k_init_update
  double* Ht;             // [cols][rows]
  double* Hinv;           // [9] H_L^-1 row-major
  double* Rk;             // [9] R_init = I
  double* resid;          // [rows - 3] residual of the update rows
  double* res;            // this candidate's result block: res[4 + n_max .. +3) = H_L^-1 res_init
};

// the general instance (ovp_slam_delayed_init_general): candidates with observations of any camera, at most OVP_MAX_MEAS_DEV of them
struct DinitGenParams {
  DinitParams dp;         // dp.idv unused; dp.cal = camera 0's table of ovp_state_upload (committed as well)
  double* cam_cal;        // [OVP_GEN_MAX_CAMS][20] tables of ovp_cameras_upload: the rows read them, every commit updates them
  int n_cams;
  int cam_fisheye[OVP_GEN_MAX_CAMS], cam_calib_id[OVP_GEN_MAX_CAMS], cam_intr_id[OVP_GEN_MAX_CAMS];
  const int* cam_idx;     // [n_feats][max_meas] camera of every observation
  int cols;               // columns of the candidate's H_x
  int ocol[OVP_MAX_MEAS_DEV];         // local column of observation a's clone block (a clone seen by two cameras has one block)
  int ccol[OVP_GEN_MAX_CAMS];         // local column of camera c's first estimated calibration column (-1 = not a camera of it)
  int idg[6 * OVP_MAX_MEAS_DEV + 14 * OVP_GEN_MAX_CAMS];  // the state columns of the list, by value
};

// the _pl instances (ovp_slam_delayed_init_planes): the device plane table and this attempt's part in it
#define OVP_DINIT_PLTAB 8  // doubles per plane: cp (3) | cp_fej (3) | Type::id() | -
struct DinitPlaneParams {
  double* tab;         // [n_planes][OVP_DINIT_PLTAB]; every accepted candidate's commit adds its correction to every cp
  int n_planes;
  int slot;            // plane of this attempt, 1-based (its m point-on-plane rows and three columns), 0 = none
  double white_c;      // 1 / sigma_constraint
  const double* skip;  // attempt B of a plane candidate: attempt A's result block (skip[1] > 0.5 = A accepted, nothing to do)
};

}  // namespace ovp

extern "C" {
hipError_t ovp_launch_dinit_rows(const ovp::DinitParams* dp, size_t lds, hipStream_t stream);
hipError_t ovp_launch_dinit_rows_gen(const ovp::DinitGenParams* gp, size_t lds, hipStream_t stream);
hipError_t ovp_launch_dinit_rows_pl(const ovp::DinitParams* dp, const ovp::DinitPlaneParams* pp, size_t lds, hipStream_t stream);
hipError_t ovp_launch_dinit_rows_gen_pl(const ovp::DinitGenParams* gp, const ovp::DinitPlaneParams* pp, size_t lds, hipStream_t stream);
}
