// Parameter block and launchers of the general on-plane feature kernels of the plane loop (k_plane_feat_gen.hip).
#pragma once
#include <hip/hip_runtime.h>
#include "ovp_kernels.h"

namespace ovp {

static constexpr int PG_ROWS = 2 * OVP_GEN_MAX_MEAS_DEV + 1;  // 2m bearing rows + the merged point-on-plane row

// state column (in the loop's column order) of calibration column k of camera c, -1 = not estimated
struct PlaneGenCols {
  int col[OVP_GEN_MAX_CAMS][14];
};

struct PlaneGenParams {
  FeatParams fp;          // clone tables (clone_id in the loop's column order), do_fej, white_px, calmask; cal / fisheye / uv / p_FinG per observation
  const double* cam_cal;  // [OVP_GEN_MAX_CAMS][20] tables of ovp_cameras_upload, as the previous plane's commit left them
  int cam_fisheye[OVP_GEN_MAX_CAMS];
  PlaneGenCols cc;
  // the general batch (device)
  const float* uv;
  const int* clone_idx;
  const int* cam_idx;
  const int* n_meas;
  const double* p_FinG;
  int max_meas;
  const int* list;  // [n_local] the general features lying on this plane, batch order
  int n_local;
  // the plane (PlaneParams)
  int plane, in_state, plane_sid;
  double white_c;
  const double* cp;
  const double* cp_fej;
  int n;  // state columns of the plane's pair: column n = residual, n + 1 .. n + 3 = an out-of-state plane
  // staging (global): feature fl owns hp + fl * hp_stride = its projected rows over all n + 4 columns, column-major with 2m + 1 rows
  // per column, and mark + fl * mark_stride = 1 where the column is one of its own
  double* hp;
  size_t hp_stride;
  int* mark;
  int mark_stride;
  // the contribution: one more split of the G^T G partials of k_plane_assemble2 (which SUBTRACTS them: the negative of the sum is
  // stored), tile-packed over n + 4 columns, and one more constraint-moment record carrying the projected residual energy
  double* part_split;
  double* cst_rec;
};

}  // namespace ovp

extern "C" {
// rows, projection and contribution of the general features of one plane: k_plane_feat_gen (one workgroup per feature), then
// k_plane_gen_pair (one workgroup per 16 x 16 tile of the pair, features summed in list order)
hipError_t ovp_launch_plane_feat_gen(const ovp::PlaneGenParams* g, hipStream_t stream);
// behind k_chol2: an accepted plane's correction applied to every camera table of ovp_cameras_upload
hipError_t ovp_launch_plane_gen_commit(const double* res, const double* dx, double* cam_cal, int n_cams, const ovp::PlaneGenCols* cc,
                                       unsigned calmask, hipStream_t stream);
}
