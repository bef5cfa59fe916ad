// Launchers of the plane initialisation behind the second-generation plane loop (k_plane_init2.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "k_plane2.h"

namespace ovp {

// What the tail of ovp_plane_init_general works on.  Plane pl of the call owns keep[pl * 3 * (nk + 4) ...]: three rows over
// [nk loop columns | residual | 3 plane columns] = [E_cx | b_c | E_cc] of its extended pair (k_plane_init_keep), turned in place into
// [Z^T | b_c | E_cc^-1] by k_plane_init_solve.
struct PlaneInitTail {
  const double* res;    // [n_planes][4] results of the loop ([1] > 0.5: accepted)
  int n_planes;
  double* keep;
  int nk;               // columns of the loop's leading block (the same for every plane: no plane of the call is in the state)
  const double* dx;     // [n_planes][dx_stride] corrections of the loop, in the loop's column order
  int dx_stride;
  const int* flags;     // [0] | [2] != 0: a factorization of the loop failed - nothing is written (nullptr: not looked at)
  int* slot;            // [n_planes] position among the accepted planes (-1: not accepted) | [n_planes] plane of a position
  double* extra;        // [3 n_planes] d cp of every plane | [n_planes][n_planes][3] correction of plane j by the later plane k
  // the resident covariance the columns are appended to
  double* P;
  int ldp, n_state;
  const int* ids;       // [nk] loop column -> state column (nullptr: identity)
};

}  // namespace ovp

extern "C" {
hipError_t ovp_launch_plane_init_keep(const ovp::PlaneAsm* a, double* keep, hipStream_t stream);
hipError_t ovp_launch_plane_init_solve(const ovp::PlaneInitTail* t, hipStream_t stream);
hipError_t ovp_launch_plane_init_columns(const ovp::PlaneInitTail* t, hipStream_t stream);
}
