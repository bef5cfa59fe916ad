// Options and per-call results of the test harness over the host mirror (host_capi.cpp; hostlib.RunOpts mirrors the layout).
// Internal: the harness is not part of the shipped boundary (include/ovplane_hip.h).
//
// The harness keeps no state between calls.  Every ovph_run_* entry that takes options takes them as its last argument (NULL =
// ovph_run_opts_defaults); a struct whose `size` is not sizeof(ovph_run_opts) is refused with OVPH_E_OPTS before anything is
// touched.  Pointers in the struct are borrowed for the duration of the call only.  An all-zero struct with `size` set behaves as
// the defaults do: the fields whose default is not zero are only read behind a switch that is off by default.
#pragma once
#include <stdint.h>

#define OVPH_E_OPTS (-40)

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ovph_run_opts {
  uint32_t size;     // sizeof(ovph_run_opts)
  int32_t fisheye;   // lens model of camera 0 (0 = radtan, 1 = equidistant)
  // features arrive with normalised measurements [F][M][2] and NO position: the updater triangulates them itself
  // (update/UpdaterMSCKF.cpp:120-166) before the update
  const float *uv_norm;
  // no plane estimates are handed over, the updater runs plane_fitting / optimize_plane itself
  int32_t fit_planes, fit_min_feat;
  double fit_max_cond;
  int32_t fit_variant;
  // ovph_run_updater mode 0: hold every landmark in this ext LandmarkRepresentation (1..4), anchored in this clone slot
  int32_t slam_rep, slam_anchor;
  int32_t feat_rep_slam;      // mode 1: StateOptions::feat_rep_slam of the landmarks delayed_init creates
  const int32_t *slam_plane;  // mode 3: plane of every SLAM landmark (0 = none)
  // a second camera (num_cameras = 2) with these calibration values, its variables behind camera 0's; cam_of_meas [F][M] says
  // which camera took each measurement of the feature batch
  const double *cam1_q, *cam1_p, *cam1_intr;
  const int32_t *cam_of_meas;
  // StateOptions::gpu_<name>
  int32_t general_features, general_planes, general_plane_init, fused_plane_fit, general_slam, dinit_planes, batched_retire, featdb;
  const double *p_noplane;  // mode 1: positions before plane refinement of the candidates (Feature::p_FinG_original, [F][3])
  // ovph_run_msckf_update: the State lives on `device` and the updater takes the sharded point loop on this communicator
  void *comm;
  int32_t comm_rank, comm_world, device;
  // ovph_run_sequence: per-frame IMU value [K][16] and IMU pose covariance [K][36] (column-major) after each frame; with
  // seq_uv_norm [F][M][2] the features arrive untriangulated
  double *seq_traj, *seq_posecov;
  const float *seq_uv_norm;
  // ... planar regularities in the loop: plane id (0 = none) of every feature of the concatenated list -> feat2plane.
  // seq_plane_mode 1: point-on-plane constraints with planes estimated per update (UpdaterMSCKF, planes stay out of the state);
  // 2: additionally UpdaterPlane::init_vio_plane before the update (core/VioManager.cpp:583-588), planes join the state (the final
  // covariance is then larger than N and not returned)
  const int32_t *seq_plane;
  int32_t seq_plane_mode, seq_plane_min_feat;
  double seq_sigma_c;
  // ---- results of the call ----
  int32_t seq_planes_in_state;  // ovph_run_sequence: planes the state holds at the end
  int32_t last_shard[2];        // ovph_run_msckf_update: this rank's index range of the point batch
  double last_cam1[15];         // [q (4) | p (3) | intrinsics (8)] of camera 1 after a run that had one (untouched otherwise)
} ovph_run_opts;

// size set, fit_min_feat = 20, fit_max_cond = 100, comm_world = 1, seq_plane_min_feat = 20, seq_sigma_c = 0.01, the rest zero
void ovph_run_opts_defaults(ovph_run_opts *o);
// what a mirror of the struct has to agree with: sizeof, and offsetof of every member in declaration order (returns the member
// count; writes at most `cap` offsets)
int ovph_run_opts_size(void);
int ovph_run_opts_layout(int *offsets, int cap);

// ov_plane::TrackPlane's image half (ov_plane_trackplane.h) on a sequence of n_frames images [n_frames][height][width] with one
// mask [height][width] (NULL: none), on a context of its own on `device`: frame 0 is fed, the n_pts points (ids, uv [n_pts][2]) are
// added, every later frame is fed.  Per frame f: n_kept[f] kept ids / points in kept_ids[f][n_pts] / kept_uv[f][n_pts][2], and what
// perform_matching_klt returned for the points that went in: n_match[f], match_uv[f][n_pts][2], match_mask[f][n_pts].
// pyr_levels is the reference's (images - 1).  Returns 0 or the first failing call's code.
int ovph_run_klt_sequence(int device, int width, int height, int n_frames, const uint8_t *frames, const uint8_t *mask, int pyr_levels,
                          int win_size, int hist_method, int n_pts, const int64_t *ids, const float *uv, int32_t *n_kept,
                          int64_t *kept_ids, float *kept_uv, int32_t *n_match, float *match_uv, uint8_t *match_mask);
// the same with the mirror's own detection (feed_new_camera(.., detect = true) from an empty tracker): detector5 = [num_features,
// grid_x, grid_y, threshold, min_px_dist]; per frame f the ids / points held behind it in kept_ids[f][max_points] /
// kept_uv[f][max_points][2].  OVP_E_CAPACITY when a frame holds more than max_points.
int ovph_run_klt_detect_sequence(int device, int width, int height, int n_frames, const uint8_t *frames, const uint8_t *mask,
                                 int pyr_levels, int win_size, int hist_method, int max_points, const int32_t *detector5, int32_t *n_kept,
                                 int64_t *kept_ids, float *kept_uv);
// ovph_run_klt_sequence with the epipolar check on (feed_new_camera(.., false, true) under set_camera(mode, intrinsics8) and
// set_epipolar_options(0.999, max_iters, seed)): per frame f additionally kept_uvn[f][n_pts][2], the kept points' undistorted
// coordinates, and reset[f] (:520-530).
int ovph_run_klt_epipolar_sequence(int device, int width, int height, int n_frames, const uint8_t *frames, const uint8_t *mask,
                                   int pyr_levels, int win_size, int hist_method, int n_pts, const int64_t *ids, const float *uv,
                                   int mode, const double *intrinsics8, int max_iters, uint32_t seed, int32_t *n_kept, int64_t *kept_ids,
                                   float *kept_uv, float *kept_uvn, int32_t *reset);
// TrackPlane::feed_monocular (ov_plane_trackplane.h) over the fused entry ovp_klt_match_frame, a FeatureDatabase(max_slots,
// max_meas) attached through set_database: frame f at times[f], the points added behind the first frame together with their first
// observation (uv_norm = uv), check = the epipolar check.  Per frame what ovph_run_klt_epipolar_sequence returns; at the end the
// database's read-back of every input id: db_slot / db_count [n_pts] (count -1: not held), db_ts [n_pts][max_meas], db_uv / db_uvn
// [n_pts][max_meas][2].
int ovph_run_klt_frame_sequence(int device, int width, int height, int n_frames, const uint8_t *frames, const uint8_t *mask,
                                const double *times, int pyr_levels, int win_size, int hist_method, int n_pts, const int64_t *ids,
                                const float *uv, int mode, const double *intrinsics8, int check, int max_iters, uint32_t seed,
                                int max_slots, int max_meas, int32_t *n_kept, int64_t *kept_ids, float *kept_uv, float *kept_uvn,
                                int32_t *reset, int32_t *db_slot, int32_t *db_count, double *db_ts, float *db_uv, float *db_uvn);
// ovph_run_klt_detect_sequence under set_intake(hist_method, downsample, clahe_clip, tiles_x, tiles_y): the frames go through
// ovp_klt_feed_image_opts - CLAHE included - and with downsample frames [n_frames][height][width] and the mask are the full-size
// ones, halved on the device; the points are pixels of the (width / 2) x (height / 2) image.
int ovph_run_klt_intake_sequence(int device, int width, int height, int n_frames, const uint8_t *frames, const uint8_t *mask,
                                 int pyr_levels, int win_size, int hist_method, int downsample, double clahe_clip, int tiles_x,
                                 int tiles_y, int max_points, const int32_t *detector5, int32_t *n_kept, int64_t *kept_ids,
                                 float *kept_uv);

// ov_plane::FeatureDatabase (ov_plane_featdb.h) on a context of its own on `device`: n_frames frames, frame f with n_obs[f]
// observations (ids / uv / uv_norm concatenated) at times[f].  Per frame, as VioManager::do_feature_propagate_update goes
// (core/VioManager.cpp:373-506, :855-869): update_feature, select over the last max_clone_size + 1 times, to_delete on everything
// selected, cleanup(), and cleanup_measurements(oldest) once the window is full; new SLAM features join the landmark list, lost
// landmarks leave it.  out receives per frame, every list as (length, items): the table's ids, cls, count, cleaned, flags, the four
// totals, lost, marg, maxtracks, slam_delayed, slam_update, landmarks_marg, features_not_containing_newer(t),
// features_containing(oldest), and (count, to_delete) of get_feature(first id) or (-1, 0).  *used = values written.
int ovph_run_featdb_sequence(int device, int max_slots, int max_meas, int n_frames, const double *times, const int32_t *n_obs,
                             const int64_t *ids, const float *uv, const float *uv_norm, int max_clone_size, int max_slam_features,
                             int64_t *out, long cap, long *used);

#ifdef __cplusplus
}
#endif
