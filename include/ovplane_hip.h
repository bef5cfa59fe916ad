/*
 * libovplane_hip.so - C-ABI of the MI355X-native MSCKF(+plane) EKF update path for rpng/ov_plane.
 *
 * The reference has no FFI layer: the boundary is the C++ surface that VioManager calls
 * (SURVEY.md §8b).  Each entry point below names the reference method(s) it replaces; citations are
 * relative to /root/reference/ov_plane/src/.  Plain pointers and sizes only, no C++/torch types.
 *
 * Conventions
 *   - all matrices are f64; the covariance is handed over ROW-major == column-major (it is symmetric)
 *     with an explicit leading dimension;
 *   - `id` always means Type::id() = column offset of a variable in State::_Cov;
 *   - every function returns 0 on success, a positive hipError_t, or a negative OVP_E_* code;
 *   - one context per filter, not thread-safe (matches the reference: at most one update in flight - the staged entry points keep
 *     per-update words in host-mapped memory that the kernels read, e.g. the output slots of the features of a point update, so
 *     ovp_msckf_fetch_results must have returned before the next update of the same context is enqueued);
 *   - work is enqueued on the context's stream; functions that return results to host memory
 *     synchronise that stream unless their name ends in _async (then call ovp_sync()).
 */
#ifndef OVPLANE_HIP_H
#define OVPLANE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OVP_MAX_MEAS 32 /* max observations per feature handled by the wave-per-feature kernels */

enum {
  OVP_E_ARG = -1,       /* bad argument */
  OVP_E_CAPACITY = -2,  /* exceeds the capacity given to ovp_ctx_create */
  OVP_E_NOTSPD = -3,    /* a Cholesky factorisation hit a non-positive pivot */
  OVP_E_NEGDIAG = -4,   /* negative covariance diagonal (reference: std::exit, StateHelper.cpp:177-187) */
  OVP_E_NODEVICE = -5,  /* no HIP device / wrong architecture */
  OVP_E_STATE = -6,     /* call order violated (e.g. update before upload) */
  OVP_E_TIMEOUT = -7,   /* a device-side hand-over between the two workgroups of the plane solve did not arrive (bounded spin) */
  OVP_E_RCCL = -8,      /* librccl could not be loaded, or an RCCL call failed (message on stderr) */
  OVP_E_PEER = -9       /* sharded update: another rank's build failed; every rank of the call reports an error (errors are collective) */
};

typedef struct ovp_ctx ovp_ctx;

/* Options read on the path: update/UpdaterOptions.h:37-53, state/StateOptions.h:41-153. */
typedef struct {
  double sigma_px;                /* UpdaterOptions::sigma_pix                 */
  double chi2_multiplier;         /* UpdaterOptions::chi2_multipler            */
  double sigma_constraint;        /* StateOptions::sigma_constraint            */
  int do_fej;                     /* StateOptions::do_fej                      */
  int do_calib_camera_pose;       /* StateOptions::do_calib_camera_pose        */
  int do_calib_camera_intrinsics; /* StateOptions::do_calib_camera_intrinsics  */
  int skip_plane_used;            /* point update only: 1 = leave out the features the accepted planes of the preceding
                                     ovp_msckf_plane_update on this batch consumed (the reference erases them from feature_vec
                                     before the point loop, update/UpdaterMSCKF.cpp:657-666); the mask stays on the device */
} ovp_update_opts;

/* Values of the ov_type variables the Jacobians read (state/State.h:86-121): clone poses (value and
 * first-estimate), camera extrinsics/intrinsics.  MONOCULAR ONLY: one camera (cam 0, radtan or equidistant) - every shipped
 * configuration of the reference sets max_cameras: 1; the per-camera measurement loop of update/UpdaterHelper.cpp:335-344 is
 * taken for a single camera id, a stereo pair would need a second calibration block and camera index per measurement.
 * Host pointers. */
typedef struct {
  int n_state;               /* N = State::_Cov.rows()                       */
  int n_clones;
  const double *clone_q;     /* [n_clones*4] JPL q_GtoI: PoseJPL::Rot()      */
  const double *clone_p;     /* [n_clones*3] p_IinG:     PoseJPL::pos()      */
  const double *clone_q_fej; /* PoseJPL::Rot_fej()                           */
  const double *clone_p_fej; /* PoseJPL::pos_fej()                           */
  const int *clone_id;       /* [n_clones] Type::id()                        */
  double calib_q[4];         /* R_ItoC (State::_calib_IMUtoCAM.at(0))        */
  double calib_p[3];         /* p_IinC                                       */
  int calib_id;              /* ignored unless do_calib_camera_pose          */
  double intrinsics[8];      /* fx fy cx cy k1 k2 p1 p2 (State::_cam_intrinsics.at(0)); k1..k4 for the fisheye model */
  int intr_id;               /* ignored unless do_calib_camera_intrinsics    */
  int cam_fisheye;           /* 0 = ext CamRadtan, 1 = ext CamEqui (State::_cam_intrinsics_cameras.at(0), call sites
                                update/UpdaterHelper.cpp:365,389) */
} ovp_state_tables;

/* SoA form of a vector of UpdaterHelper::UpdaterHelperFeature (update/UpdaterHelper.h:62-105),
 * GLOBAL_3D representation (the only one the shipped configs use; UpdaterHelper.cpp:39-43,455-456). */
typedef struct {
  int n_feats;
  int max_meas;          /* row pitch of uv / clone_idx, <= OVP_MAX_MEAS                       */
  const float *uv;       /* [n_feats*max_meas*2] raw pixel measurements (f32, UpdaterHelper.h:68) */
  const int *clone_idx;  /* [n_feats*max_meas] index into the clone tables, -1 = padding       */
  const int *n_meas;     /* [n_feats]                                                          */
  const double *p_FinG;  /* [n_feats*3] linearisation point (fej == value for MSCKF features)  */
} ovp_feature_batch;

/* Result summary of one update step. */
typedef struct {
  int n_accepted;      /* features that passed the chi2 gate (UpdaterMSCKF.cpp:755)            */
  int n_rows;          /* stacked rows before compression = sum (2m-3) over accepted features   */
  int n_cols;          /* involved state columns                                                */
  int neg_diag;        /* 1 if the updated covariance has a negative diagonal entry             */
  int not_spd;         /* 1 if a factorisation failed                                           */
  int reserved[3];
} ovp_update_info;

#define OVP_PLANE_MAX_SLAM 80 /* SLAM landmarks on ONE out-of-state plane handled by ovp_msckf_plane_update: above every
                                 max_slam_features of the shipped configurations (25 .. 75), so that no plane of a real frame meets it;
                                 each landmark also adds three involved columns to the loop's 287-column budget */

/* ---- context --------------------------------------------------------------------------------- */
/* stream: a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream) or NULL to let the library create its own.
 * Sizes: n_state_max <= 700 (the feature kernels stage projector rows in LDS); states up to 288 columns take the register-
 * resident factorizations, larger ones the sub-state update (a batch may then touch at most 288 columns to stay fast);
 * ovp_msckf_plane_update above 287 columns runs its loop on the columns the planes of the call involve (clones, calibration, the
 * planes that are state variables, the SLAM landmarks on the others: at most 287 of them, OVP_E_CAPACITY beyond) and carries the
 * rest of the state along; ovp_plane_init and ovp_plane_init_general are that loop on planes outside the state (any state size, at
 * most 287 clone and calibration columns). */
int ovp_ctx_create(int device, int n_state_max, int n_clones_max, int n_feats_max, void *stream, ovp_ctx **out);
int ovp_ctx_destroy(ovp_ctx *ctx);
int ovp_sync(ovp_ctx *ctx);
/* the hipStream_t all work of the context is ordered on (to enqueue a collective between the staged calls) */
int ovp_ctx_stream(ovp_ctx *ctx, void **stream);
const char *ovp_version(void);
const char *ovp_error_string(int code);

/* ---- covariance residency (State::_Cov lives on the device) --------------------------------- */
/* replaces direct access to State::_Cov (friend StateHelper, state/State.h:123-133) */
int ovp_cov_upload(ovp_ctx *ctx, const double *P_host, int n, int ld);
int ovp_cov_download(ovp_ctx *ctx, double *P_host, int n, int ld);
/* device-to-device variant: P_dev is a device pointer (n x n, ld) */
int ovp_cov_set_device(ovp_ctx *ctx, const double *P_dev, int n, int ld);
/* StateHelper::get_marginal_covariance (state/StateHelper.cpp:231-259): out is host [sum(size)^2] col-major */
int ovp_cov_marginal(ovp_ctx *ctx, const int *ids, const int *sizes, int n_vars, double *out_host);

/* ---- state tables / feature batch ----------------------------------------------------------- */
int ovp_state_upload(ovp_ctx *ctx, const ovp_state_tables *st);
/* host -> device copy of a feature batch */
int ovp_batch_upload(ovp_ctx *ctx, const ovp_feature_batch *host_batch);
/* zero-copy: the pointers inside dev_batch are DEVICE pointers that stay valid until the next bind/upload */
int ovp_batch_bind_device(ovp_ctx *ctx, const ovp_feature_batch *dev_batch);
/* Restricts the POINT updates that follow (ovp_msckf_update / ovp_msckf_build_gate_gram_async) to the features [lo, hi) of the
 * uploaded batch - the shard of one rank when the whole frame is resident on every GPU (the plane loop runs on the
 * whole frame everywhere, the leftovers are split by index range, no second upload).  lo = hi = -1 lifts the restriction, lo >= hi
 * >= 0 is an empty shard; every upload / bind lifts it. */
int ovp_batch_set_range(ovp_ctx *ctx, int lo, int hi);

/* ---- the update step ------------------------------------------------------------------------ */
/* UpdaterMSCKF::update point-feature path (update/UpdaterMSCKF.cpp:671-814):
 *   get_feature_jacobian_full (UpdaterHelper.cpp:195-513) -> nullspace projection (:515-546) -> chi2 gate
 *   (UpdaterMSCKF.cpp:739-764) -> stacking (:767-785) -> measurement compression (UpdaterHelper.cpp:548-579)
 *   -> StateHelper::EKFUpdate (StateHelper.cpp:121-202) with R = I.
 * On return P (device) holds the updated covariance; dx_host[n_state] is the correction the caller applies with
 * Type::update; accepted_host[n_feats] / chi2_host[n_feats] mirror the per-feature gate (0 = rejected: the
 * reference sets to_delete and erases it from feature_vec). Any of the host outputs may be NULL. */
int ovp_msckf_update(ovp_ctx *ctx, const ovp_update_opts *opts, double *dx_host, uint8_t *accepted_host,
                     double *chi2_host, ovp_update_info *info);

/* Features the batch format cannot carry - a track of more than OVP_MAX_MEAS observations, observations of a camera other than
 * camera 0 (the reference loops over every camera's measurements of a feature, update/UpdaterHelper.cpp:335-344, and stacks any
 * number of them, update/UpdaterMSCKF.cpp:686-691) - join the SAME update as dense blocks: block k is the feature's system after
 * the nullspace projection, H_k (rows[k] x cols[k], column-major, concatenated in H), its state columns (col_ids, Type::id() +
 * offset, concatenated) and residual (res, concatenated), noise already whitened (R = I).  The call gates every block against the
 * RESIDENT covariance - chi2 = r^T (H P H^T + I)^-1 r <= chi2_multiplier * quantile_0.95(rows), update/UpdaterMSCKF.cpp:739-757 -
 * and keeps the information pair of the accepted ones; the next ovp_msckf_update / ovp_msckf_build_gate_gram_async of the context
 * adds it to the pair of the batch, so batch features and dense blocks are ONE EKF update as in the reference.  Any call that
 * writes the covariance in between drops the pending pair.  Slow path (marginal of the involved columns to the host, gates on
 * the host): meant for the few features per frame that need it.  accepted / chi2: per block, may be NULL. */
int ovp_msckf_dense_blocks(ovp_ctx *ctx, double chi2_multiplier, int n_blocks, const int *rows, const int *cols, const double *H,
                           const int *col_ids, const double *res, uint8_t *accepted, double *chi2);

/* ---- general point features: any camera, long tracks (device form of the dense blocks above) ---------------------------------
 * The batch format carries camera 0 and at most OVP_MAX_MEAS views.  A feature outside that - observations of another camera (the
 * reference loops over every camera of a feature, update/UpdaterHelper.cpp:335-344), a track longer than OVP_MAX_MEAS (stacked
 * without a limit, update/UpdaterMSCKF.cpp:686-691) - takes these entries instead of ovp_msckf_dense_blocks: rows, nullspace
 * projection, gate and information pair are formed on the device (csrc/k_feat_gen.hip).
 * Limits: OVP_MAX_CAMERAS cameras, OVP_GEN_MAX_MEAS observations per feature (2m <= 128 rows: the rows and the packed
 * (2m+1)-row gate matrix of one feature live in the LDS of its workgroup; the projected rows are staged in global memory, 2m x the
 * feature's involved columns <= 4 * 14 + 6 * 64). */
#define OVP_MAX_CAMERAS 4
#define OVP_GEN_MAX_MEAS 64

/* State::_calib_IMUtoCAM.at(k) / _cam_intrinsics.at(k) / _cam_intrinsics_cameras.at(k) of one camera (state/State.cpp:52-72) */
typedef struct {
  double calib_q[4];     /* R_ItoC as JPL quaternion              */
  double calib_p[3];     /* p_IinC                                */
  int calib_id;          /* Type::id(); read when do_calib_camera_pose */
  double intrinsics[8];  /* fx fy cx cy k1 k2 p1 p2 (k1..k4 fisheye) */
  int intr_id;           /* Type::id(); read when do_calib_camera_intrinsics */
  int fisheye;           /* 0 = ext CamRadtan, 1 = ext CamEqui    */
} ovp_camera_tables;

/* camera k of the context = cams[k], k < n_cams <= OVP_MAX_CAMERAS; replaces the previous tables (host pointers, copied).  The
 * clone tables stay those of ovp_state_upload. */
int ovp_cameras_upload(ovp_ctx *ctx, int n_cams, const ovp_camera_tables *cams);

/* A vector of UpdaterHelper::UpdaterHelperFeature with per-observation camera (update/UpdaterHelper.h:62-105; GLOBAL_3D), host
 * pointers, observation k of feature f at [f * max_meas + k]. */
typedef struct {
  int n_feats;
  int max_meas;          /* row pitch of uv / clone_idx / cam_idx */
  const float *uv;       /* [n_feats*max_meas*2] raw pixels (f32, UpdaterHelper.h:68) */
  const int *clone_idx;  /* [n_feats*max_meas] clone slot */
  const int *cam_idx;    /* [n_feats*max_meas] camera of the observation (< n_cams of ovp_cameras_upload) */
  const int *n_meas;     /* [n_feats] <= OVP_GEN_MAX_MEAS */
  const double *p_FinG;  /* [n_feats*3] linearisation point (fej == value for MSCKF features) */
} ovp_general_batch;

/* UpdaterMSCKF::update for features of a general batch (update/UpdaterMSCKF.cpp:695-764): get_feature_jacobian_full over every
 * camera's observations (update/UpdaterHelper.cpp:195-440: clone columns, per-camera extrinsics / intrinsics as the options say,
 * whitened by 1/sigma_px), nullspace projection (:515-546, orthogonal projector onto the complement of H_f's range), gate against
 * the RESIDENT covariance chi2 = r^T (H P H^T + I)^-1 r <= chi2_multiplier * quantile_0.95(2m - 3) (UpdaterMSCKF.cpp:739-757), all
 * on the device.  Same contract as ovp_msckf_dense_blocks: the information pair of the accepted features (summed in feature order,
 * no atomics: bit-reproducible) joins the next ovp_msckf_update / ovp_msckf_build_gate_gram_async / ovp_msckf_update_sharded of the
 * context as ONE EKF update; a call that writes the covariance in between drops it; a second call replaces it.  Features with fewer
 * than 2 observations are rejected with chi2 = 0.  accepted / chi2 [n_feats], may be NULL.  Needs ovp_state_upload,
 * ovp_cameras_upload and a covariance.  OVP_E_CAPACITY: n_meas > OVP_GEN_MAX_MEAS; OVP_E_ARG: a camera without tables, a clone slot
 * outside the tables, n_meas > max_meas (all checked on the host before anything is enqueued). */
int ovp_msckf_general_features(ovp_ctx *ctx, const ovp_update_opts *opts, const ovp_general_batch *batch, uint8_t *accepted,
                               double *chi2);

/* Staged form of the same step, for feature-sharded multi-GPU runs:
 *   stage 1 (per rank, local shard): build + project + gate + local information pair
 *            Ab_dev = [A | b], A = sum_f Hp_f^T Hp_f (n_state x n_state), b = sum_f Hp_f^T r_f,
 *            written to the device buffer returned by ovp_gram_buffer() (f64, (n_state+1) * ld_gram);
 *   (caller all-reduces that buffer over RCCL)
 *   stage 2 (every rank or rank 0): EKF update from the summed pair. */
/* NOTE for callers that touch the pair between the two stages: the update reads Ab only on the columns a point batch involves
 * (the clone poses and the estimated calibration; everything in front of the first of those columns is taken to be zero - the
 * factor of P is then formed in reversed index order and the update runs on the trailing block).  Summing pairs of the same
 * kind over ranks keeps that property; writing other columns does not, and such contributions would be dropped silently -
 * set OVP_POINT_NO_FLIP=1 in the environment (full-width update) for a caller that needs them. */
int ovp_msckf_build_gate_gram_async(ovp_ctx *ctx, const ovp_update_opts *opts);
int ovp_gram_buffer(ovp_ctx *ctx, double **Ab_dev, int *n_rows, int *ld);
int ovp_ekf_update_from_gram_async(ovp_ctx *ctx);
int ovp_msckf_fetch_results(ovp_ctx *ctx, double *dx_host, uint8_t *accepted_host, double *chi2_host,
                            ovp_update_info *info);

/* ---- feature-sharded update over RCCL (no counterpart in the reference, which runs on one core) -----------------
 * One process per GPU, every rank with the same covariance, pose tables and frame resident.  ovp_msckf_update_sharded =
 * ovp_batch_set_range(this rank's balanced share of the features the update is about) -> ovp_msckf_build_gate_gram_async ->
 * ncclAllReduce(sum, f64) of [A | b] on the context's stream -> ovp_ekf_update_from_gram_async -> ovp_msckf_fetch_results: every
 * rank ends with the same covariance and correction (the all-reduced pair is bit-identical on all ranks, the update is
 * deterministic).  nccl_comm is an ncclComm_t of the caller (a C++ host links RCCL itself and owns the communicator); the three
 * helpers below create one for callers that do not (bench.py, the tests): the id of rank 0 travels by whatever means the launcher
 * has.  RCCL is bound with dlopen at first use (OVP_RCCL_LIB overrides the name).  world = 1 / comm = NULL: no collective.
 * accepted / chi2 are filled for this rank's share [*shard_lo, *shard_hi) only (zero elsewhere); with opts->skip_plane_used the
 * share is taken from the features the preceding ovp_msckf_plane_update left. */
typedef struct { char internal[128]; } ovp_rccl_id; /* = ncclUniqueId */
int ovp_rccl_unique_id(ovp_rccl_id *id);
int ovp_rccl_comm_create(const ovp_rccl_id *id, int rank, int world, int device, void **nccl_comm);
int ovp_rccl_comm_destroy(void *nccl_comm);
/* ncclAllReduce(sum, f64) of the pair of ovp_gram_buffer() on the context's stream: the collective between
 * ovp_msckf_build_gate_gram_async and ovp_ekf_update_from_gram_async for callers that drive the stages themselves */
int ovp_rccl_allreduce_gram(ovp_ctx *ctx, void *nccl_comm);
/* the index range [*lo, *hi) of the resident batch that ovp_msckf_update_sharded gives to `rank` of `world` (for callers that drive the
 * staged entries and ovp_batch_set_range themselves): balanced over the features of the update, consecutive ranks tile the batch,
 * lo == hi = an empty share */
int ovp_shard_range(ovp_ctx *ctx, const ovp_update_opts *opts, int rank, int world, int *lo, int *hi);
/* the same arithmetic without a context (pure host code, no device): used[n_feats] = the mask ovp_msckf_plane_update returned
 * (non-zero = consumed by an accepted plane), NULL = no plane loop ran */
int ovp_shard_range_of_mask(const uint8_t *used, int n_feats, int rank, int world, int *lo, int *hi);
/* ERRORS ARE COLLECTIVE: argument / call-order errors are detected before the collective from inputs that are the same on every
 * rank; a rank whose build fails afterwards still enters the all-reduce (zero pair, one more summed f64 word raised), so its peers
 * complete the call and return OVP_E_PEER - no rank is left waiting inside RCCL.  After OVP_E_PEER the covariance of the
 * context is invalid (OVP_E_STATE until the next ovp_cov_upload): the reference treats every failure on this path as fatal
 * (state/StateHelper.cpp:185-187). */
int ovp_msckf_update_sharded(ovp_ctx *ctx, const ovp_update_opts *opts, void *nccl_comm, int rank, int world, double *dx_host,
                             uint8_t *accepted_host, double *chi2_host, ovp_update_info *info, int *shard_lo, int *shard_hi);
/* Completes accepted_host[n_feats] (and chi2_host, may be NULL) of a sharded update on EVERY rank: the shares are disjoint and zero
 * elsewhere, so an ncclAllReduce(sum) is a gather.  For callers that act on every feature's decision on every replica - the
 * Updater surface erases rejected features from feature_vec (update/UpdaterMSCKF.cpp:755-757).  Collective; nccl_comm = NULL: no-op. */
int ovp_rccl_gather_decisions(ovp_ctx *ctx, void *nccl_comm, uint8_t *accepted_host, double *chi2_host);

/* ext ov_core::FeatureInitializerOptions (open_vins ov_core/src/feat/FeatureInitializerOptions.h; not in the reference tree) */
typedef struct {
  int refine_features; /* run single_gaussnewton after the linear triangulation (UpdaterMSCKF.cpp:153-155) */
  int max_runs;
  double init_lamda, max_lamda, min_dx, min_dcost, lam_mult;
  double min_dist, max_dist, max_baseline, max_cond_number;
  int triangulate_1d; /* single_triangulation_1d instead of single_triangulation: depth along the anchor bearing (UpdaterMSCKF.cpp:148-152) */
  int reserved;
} ovp_triang_opts;
void ovp_triang_defaults(ovp_triang_opts *o);

/* ext FeatureInitializer::single_triangulation (+ single_gaussnewton) for every feature of the uploaded batch, against the
 * camera poses of the clones (update/UpdaterMSCKF.cpp:120-166; same block in UpdaterSLAM.cpp:129-144, UpdaterPlane.cpp:139-164).
 * uv_norm [n_feats*max_meas*2] f32 (host) = Feature::uvs_norm in the layout of ovp_feature_batch::uv.  The positions become
 * the linearisation points of the batch on the device (the next update uses them) and are returned in p_FinG_out
 * [n_feats*3] (host, may be NULL); ok[f] = 0 where the reference erases the feature.  Needs ovp_state_upload and a batch. */
int ovp_triangulate(ovp_ctx *ctx, const ovp_triang_opts *opts, const float *uv_norm, double *p_FinG_out, uint8_t *ok);
/* ext FeatureInitializer::single_triangulation (+ single_gaussnewton / single_triangulation_1d) over a general batch: every
 * observation with the pose of its own camera, R_GtoC = R_ItoC(cam) R_GtoI, p_CinG = p_IinG - R_GtoC^T p_IinC(cam)
 * (update/UpdaterMSCKF.cpp:120-166 over all cameras of the feature).  Anchor: the last observation of the lowest camera index that
 * saw the feature (ext Feature::anchor_cam_id / anchor_clone_timestamp).  uv_norm in the layout of batch->uv; batch->p_FinG is
 * not read.  p_FinG_out [n_feats*3] (may be NULL), ok [n_feats]: 0 where the reference erases the feature.  Same limits and
 * argument checks as ovp_msckf_general_features. */
int ovp_triangulate_general(ovp_ctx *ctx, const ovp_triang_opts *opts, const ovp_general_batch *batch, const float *uv_norm,
                            double *p_FinG_out, uint8_t *ok);

/* Planes touched by an update (host pointers): plane k (0-based) has reference id k+1.
 * plane_of_feat[f] = 0 for a free point, else the id of the plane feature f lies on (VioManager's feat2plane map,
 * core/VioManager.cpp:516-533). cp / cp_fej: closest-point estimates (State::_features_PLANE value()/fej() for in-state
 * planes, the PlaneFitting estimate otherwise, update/UpdaterMSCKF.cpp:467-475). plane_state_id[k] = Type::id() or -1. */
typedef struct {
  int n_planes;
  const int *plane_of_feat;   /* [n_feats of the uploaded batch] */
  const double *cp;           /* [n_planes*3] */
  const double *cp_fej;       /* [n_planes*3] */
  const int *plane_state_id;  /* [n_planes] */
  /* SLAM landmarks that lie on planes which are NOT in the state (update/UpdaterMSCKF.cpp:232-252), ovp_msckf_plane_update
   * only: each contributes one point-on-plane row whose feature Jacobian stays in the landmark's three state columns
   * (:545-552).  n_slam = 0 / NULL pointers when there are none. */
  int n_slam;                 /* at most OVP_PLANE_MAX_SLAM of them on one plane (OVP_E_CAPACITY beyond) */
  const int *slam_plane;      /* [n_slam] 1-based plane slot */
  const int *slam_state_id;   /* [n_slam] Type::id() of the landmark */
  const double *slam_p;       /* [n_slam*3] Landmark::get_xyz(false) */
  const double *slam_p_fej;   /* [n_slam*3] Landmark::get_xyz(true) */
  /* Diagnostics (ovp_msckf_plane_update only; NULL in production): force_decision[k] = 1 accepts / 0 rejects plane k whatever
   * its chi2 says (the statistic is still computed and returned), any other value lets the gate decide.  The reference has the
   * same switch in spirit (chi2_multipler = 99999 in the simulation configs); with it the parity tests compare states and
   * covariances under the oracle's own accept / reject sequence, separately from the decision statistics. */
  const uint8_t *force_decision; /* [n_planes] */
} ovp_plane_batch;

/* UpdaterMSCKF::update, per-plane loop with MSCKF features (update/UpdaterMSCKF.cpp:411-649): for every plane in
 * ascending id: point-on-plane Jacobians (update/UpdaterHelper.cpp:448-512), UpdaterPlane::nullspace_project_inplace /
 * measurement_compress_inplace (update/UpdaterPlane.cpp:483-552), plane appended (in state) or projected out, plane-level
 * chi2, StateHelper::EKFUpdate.  Planes are sequential: pose tables, calibration, in-state planes and P on the device are
 * updated after every accepted plane.  Needs a batch given with ovp_batch_upload (features with 2..31 observations).
 * Outputs (host, any may be NULL): dx_planes[n_planes*n_state] the correction of every plane (zeros if rejected / skipped)
 * for the caller to apply in order with Type::update; plane_ok; plane_chi2; plane_dof (rows of the reference's test);
 * feat_used[n_feats] = 1 for features consumed by an accepted plane (reference: to_delete + feature_vec_used). */
int ovp_msckf_plane_update(ovp_ctx *ctx, const ovp_update_opts *opts, const ovp_plane_batch *planes, double *dx_planes,
                           uint8_t *plane_ok, double *plane_chi2, int *plane_dof, uint8_t *feat_used);

/* The same loop with the on-plane features the batch format cannot carry - observations of another camera, tracks of more than
 * OVP_MAX_MEAS views - stacked behind the batch's: the reference builds the 2m bearing rows of an on-plane MSCKF feature over every
 * camera that saw it (update/UpdaterHelper.cpp:335-344) and its m point-on-plane rows (:448-512) whatever the length of the track,
 * and the plane loop (update/UpdaterMSCKF.cpp:411-649) uses them all.  general = such features (ovp_general_batch; p_FinG = their
 * linearisation points), plane_of_gen[general->n_feats] = 1-based plane slot as plane_of_feat, 0 = not on a plane: ignored by this
 * call.  For every plane the general features lying on it are linearised at the state the previous plane left (clone tables, every
 * camera of ovp_cameras_upload, the in-state planes), their rows are projected onto the complement of H_f's range and their
 * contribution enters the plane's extended pair in front of the Schur complement and the normalisation (csrc/k_plane_feat_gen.hip):
 * an out-of-state plane, an in-state plane and the gate statistic see batch features and general features as ONE system.  The row
 * counts of the gate, the column order of the loop and the sub-state form above 287 columns count the general features' clones and
 * the calibration columns of their cameras.  An accepted plane's commit also corrects the tables of ovp_cameras_upload.
 * gen_used[general->n_feats] = 1 for the general features an accepted plane consumed (may be NULL); the other outputs as above.
 * Needs ovp_cameras_upload when a general feature lies on a plane.  Limits of the general entries, checked on the host before
 * anything is enqueued (covariance and tables untouched): OVP_E_CAPACITY for n_meas > OVP_GEN_MAX_MEAS; OVP_E_ARG for a camera
 * without tables, a clone slot outside the tables, n_meas > max_meas, plane_of_gen outside [0, n_planes].  With no general feature
 * on a plane the call enqueues exactly what ovp_msckf_plane_update enqueues and returns the same bits. */
int ovp_msckf_plane_update_general(ovp_ctx *ctx, const ovp_update_opts *opts, const ovp_plane_batch *planes,
                                   const ovp_general_batch *general, const int *plane_of_gen, double *dx_planes, uint8_t *plane_ok,
                                   double *plane_chi2, int *plane_dof, uint8_t *feat_used, uint8_t *gen_used);

/* UpdaterPlane::init_vio_plane, core (update/UpdaterPlane.cpp:296-481): for every plane of the batch (none of them in the
 * state; plane_state_id is ignored), in ascending id: stack the on-plane MSCKF features with sigma_c * const_init_multi,
 * project out the feature, compress, StateHelper::initialize(plane, ..., const_init_chi2) = chi2 test of the part that
 * does not involve the plane, covariance augmentation by 3 and EKF update with the remaining rows.
 * Every accepted plane appends 3 columns to the state (new_ids[k] = its Type::id(), else -1); cp_new[3k..] is its
 * initialised value; dx_planes[k*dx_stride ..] the correction of the pre-existing variables to apply with Type::update
 * (dx_stride >= final state size).  Upstream triangulation / plane fitting is the caller's job.
 * This is ovp_plane_init_general (below) with general == NULL: the same code, the same bits, the same refusals.  In particular
 * plane_chi2 of a rejected plane is a finite statistic, and the capacity check is made up front and is all-or-nothing:
 * n + 3 * (planes with at least 3 usable features) > n_state_max returns OVP_E_CAPACITY before anything is written. */
int ovp_plane_init(ovp_ctx *ctx, const ovp_update_opts *opts, const ovp_plane_batch *planes, double const_init_multi,
                   double const_init_chi2, double *dx_planes, int dx_stride, uint8_t *plane_ok, double *plane_chi2,
                   int *plane_dof, int *new_ids, double *cp_new, uint8_t *feat_used);

/* The same initialisation in one device pass, over features of any camera and any track length up to OVP_GEN_MAX_MEAS views: the
 * reference stacks every measurement of every camera of an on-plane feature (update/UpdaterHelper.cpp:335-344, 448-512) and
 * init_vio_plane (update/UpdaterPlane.cpp:296-481) uses them all.  general / plane_of_gen / gen_used as in
 * ovp_msckf_plane_update_general (general == NULL or an empty batch: the uploaded camera-0 batch only); the other arguments as in
 * ovp_plane_init.
 * For every plane in ascending id the on-plane features of the batch and of the general batch form ONE system, linearised at the
 * state the previous accepted plane left (clone tables, calibration, the tables of ovp_cameras_upload); the gate is
 * ovp_plane_init's (threshold const_init_chi2 * q95(rows_c), plane_dof = rows_c, counted over both kinds of features and the
 * calibration columns of the cameras that saw them; fewer than 3 features or rows_c - 3 < 1: skipped).  Initialising a plane is
 * the plane loop's out-of-state update with a flat prior on the plane, so everything in front of the gate is that loop
 * (its column order, diagonal boost, retry on a semi-definite prior, marginal + push-through above 288 columns); behind the last
 * plane the accepted planes are appended from the device-resident decisions (csrc/k_plane_init2.hip): with Z_k = E_xc,k E_cc,k^-1
 * and P+ the loop's final covariance, cross block -P+ Z_k, plane blocks Z_j^T P+ Z_k + delta_jk E_cc,k^-1,
 * d cp_k = E_cc,k^-1 (b_c,k - E_cx,k dx_k), and an earlier plane j receives -Z_j^T dx_k from every later accepted plane k.
 * One enqueue, and the host waits once (a state above 288 columns: twice, as the plane loop there); it does not read a plane's
 * decision to enqueue the next.  dx_planes[k*dx_stride ..] covers the variables that existed before plane k, the planes
 * initialised earlier in the same call included.
 * Refused on the host before anything is enqueued, covariance, size and tables untouched: OVP_E_CAPACITY for a general feature
 * above OVP_GEN_MAX_MEAS views, for more than 287 involved columns (clones + calibration of every uploaded camera), for
 * n + 3 * (planes with at least 3 features) > n_state_max; OVP_E_ARG as ovp_msckf_plane_update_general.  A failed factorization
 * or a timed-out hand-over rejects its plane and every later one as in the plane loop: no column is written then and
 * ovp_cov_size is unchanged. */
int ovp_plane_init_general(ovp_ctx *ctx, const ovp_update_opts *opts, const ovp_plane_batch *planes, double const_init_multi,
                           double const_init_chi2, double *dx_planes, int dx_stride, uint8_t *plane_ok, double *plane_chi2,
                           int *plane_dof, int *new_ids, double *cp_new, uint8_t *feat_used, const ovp_general_batch *general,
                           const int *plane_of_gen, uint8_t *gen_used);

/* StateHelper::EKFUpdate (state/StateHelper.cpp:121-202) for a dense H handed over by the host
 * (UpdaterSLAM::update, StateHelper::initialize, merge_planes...): H is [rows x cols] column-major with leading
 * dimension ld, col_ids[cols] gives the state column of every H column, R = I. */
int ovp_ekf_update(ovp_ctx *ctx, const double *H_host, int rows, int cols, int ld, const int *col_ids,
                   const double *res_host, double *dx_host, ovp_update_info *info);

/* Landmarks of the state that were re-observed (UpdaterSLAM::update, update/UpdaterSLAM.cpp:424-673), host pointers.
 * The measurement arrays are laid out as in ovp_feature_batch (one "feature" per landmark).  A landmark held in GLOBAL_3D
 * (feat_rep_slam of every shipped configuration) has its rows built on the device from the tables of ovp_state_upload; one held in
 * an anchored / inverse-depth representation arrives with the dense block [H_x | H_f] the host built (the representation Jacobians
 * of update/UpdaterHelper.cpp:35-193 are host scalar code; for the single inverse depth AFTER the bearing projection of
 * UpdaterSLAM.cpp:499-515) - pre_rows[l] > 0 marks it, the gate and the update are the same. */
typedef struct {
  int n_landmarks;
  int max_meas;               /* row pitch of uv / clone_idx, <= OVP_MAX_MEAS */
  const float *uv;            /* [n_landmarks*max_meas*2] raw pixels of the new observations (Feature::uvs) */
  const int *clone_idx;       /* [n_landmarks*max_meas] clone slot of every observation */
  const int *n_meas;          /* [n_landmarks] */
  const double *p_FinG;       /* [n_landmarks*3] Landmark::get_xyz(false) */
  const double *p_FinG_fej;   /* [n_landmarks*3] Landmark::get_xyz(true) */
  const int *landmark_id;     /* [n_landmarks] Type::id() */
  /* point-on-plane rows (:465-475): Type::id() of the plane of the STATE the landmark lies on, -1 = none; NULL = no planes */
  const int *plane_state_id;  /* [n_landmarks] */
  const double *cp;           /* [n_landmarks*3] State::_features_PLANE.at(..)->value() of that plane */
  const double *cp_fej;       /* [n_landmarks*3] ->fej() */
  /* host-built blocks, NULL when every landmark is GLOBAL_3D */
  const int *pre_rows;        /* [n_landmarks] 0 = rows built on the device */
  const int *pre_cols;        /* [n_landmarks] */
  const double *pre_H;        /* blocks of the marked landmarks in order: [rows x cols] column-major, then res [rows] */
  const int *pre_ids;         /* their state columns, cols per block, in order */
} ovp_slam_batch;

/* UpdaterSLAM::update (update/UpdaterSLAM.cpp:424-673) on the resident covariance: get_feature_jacobian_full for a landmark of the
 * state (UpdaterHelper.cpp:195-513, bearing rows + the point-on-plane rows of :448-512), chi2 test against the marginal covariance
 * (:526-547), the no-plane fallback for a landmark whose plane rows fail (:547-609), stacking (:627-651) and ONE
 * StateHelper::EKFUpdate (:673).  All gates see the covariance in front of the call, as in the reference.
 * status[l]: 0 = rejected (reference: should_marg + to_delete), 1 = accepted, 2 = accepted without its plane
 * (_features_SLAM_to_PLANE[featid] = 0); chi2[l] = statistic of the stage that decided.  dx_host[n_state] for Type::update. */
int ovp_slam_update(ovp_ctx *ctx, const ovp_update_opts *opts, const ovp_slam_batch *batch, double *dx_host, uint8_t *status,
                    double *chi2, ovp_update_info *info);

/* UpdaterSLAM::delayed_init downstream of triangulation (update/UpdaterSLAM.cpp:204-364) for GLOBAL_3D landmarks without plane rows
 * (candidates on a plane of the state: ovp_slam_delayed_init_planes below, the same loop with their point-on-plane rows):
 * the candidates of the batch one after the other - get_feature_jacobian_full at the pose tables as the previous candidate left
 * them, StateHelper::initialize (Givens split :434-446, chi2 of the update rows with dof = all rows :464-475,
 * initialize_invertible :489-586, EKFUpdate with the update rows :483-485) - as ONE enqueue with one synchronisation: the loop
 * runs on the device (csrc/k_dinit.hip), three launches per candidate, the device pose tables are updated on the way.
 * Every accepted candidate appends a 3-dof landmark: new_id[l] = its Type::id() after the call (ids are handed out in order over
 * the accepted ones, as the reference does), else -1.  delta_init[3l..] = H_L^-1 res_init, which the caller adds to the new
 * landmark's value (:577); dx[l*dx_stride ..] = the correction of candidate l's EKF update for every variable that was in the
 * state at that point (the landmarks initialised earlier in the call and its own included, at their final ids), to be applied
 * in order with Type::update; zeros for a rejected candidate.  dx_stride >= state size + 3 * n_feats.
 * OVP_E_CAPACITY (nothing touched): the state would outgrow the context, or a track is too long for the one-workgroup S-form -
 * the caller then takes ovp_cov_initialize candidate by candidate. */
int ovp_slam_delayed_init(ovp_ctx *ctx, const ovp_update_opts *opts, const ovp_feature_batch *candidates, uint8_t *ok,
                          double *chi2, int *new_id, double *delta_init, double *dx, int dx_stride);

/* ---- SLAM landmarks seen by any camera (csrc/k_slam.hip k_slam_gate_gen, csrc/k_dinit.hip k_dinit_rows_gen) ----------------------
 * The two SLAM entries above read camera 0's tables of ovp_state_upload for every observation.  These read EVERY camera, camera 0
 * included, from the tables of ovp_cameras_upload: observation k of landmark / candidate l was taken by camera
 * cam_idx[l * max_meas + k] (update/UpdaterHelper.cpp:335-344 loops over the cameras of a feature).  OVP_E_ARG without those tables
 * or with a cam_idx outside [0, n_cams).
 *
 * ovp_slam_update_general: ovp_slam_update's semantics, outputs and status codes (bearing rows, point-on-plane rows of in-state
 * planes, the no-plane fallback = status 2, host-built pre_* blocks in the same call, one EKF update); a landmark's block spans its
 * clones, the estimated calibration columns of every camera that observed it, the landmark and its plane.  n_meas <= OVP_MAX_MEAS
 * per landmark (the new observations of this update).  OVP_E_CAPACITY: a block beyond the gate kernel's LDS - nothing was
 * enqueued, the covariance is unchanged, the caller may take its dense form. */
int ovp_slam_update_general(ovp_ctx *ctx, const ovp_update_opts *opts, const ovp_slam_batch *batch, const int *cam_idx,
                            double *dx_host, uint8_t *status, double *chi2, ovp_update_info *info);

/* ovp_slam_delayed_init_general: ovp_slam_delayed_init's contract (GLOBAL_3D candidates without plane rows, one enqueue, inert
 * blocks of rejected candidates removed behind the loop, ids handed out in order) for candidates of a general batch (p_FinG = their
 * triangulated positions).  A candidate's H_x spans the clone blocks of its distinct clones (a clone seen by two cameras is one
 * block) and the estimated calibration columns of each of its cameras.  Every candidate's commit applies the previous correction
 * to the pose tables, to camera 0's calibration of ovp_state_upload and to every camera of ovp_cameras_upload: after the call the
 * device tables are what the caller gets by applying the returned dx in order (ovp_msckf_general_features reads them without a
 * re-upload).  At most OVP_MAX_MEAS observations per candidate; a candidate beyond that or beyond the one-workgroup S-form
 * (k_init.hip) gives OVP_E_CAPACITY with nothing touched. */
int ovp_slam_delayed_init_general(ovp_ctx *ctx, const ovp_update_opts *opts, const ovp_general_batch *candidates, uint8_t *ok,
                                  double *chi2, int *new_id, double *delta_init, double *dx, int dx_stride);

/* ---- delayed initialisation of candidates that lie on planes of the state (csrc/k_dinit.hip k_dinit_rows_pl / k_dinit_rows_gen_pl,
 * csrc/k_init.hip k_init_*_sk) ---------------------------------------------------------------------------------------------------
 * update/UpdaterSLAM.cpp:204-364 with use_plane_constraint_slamd: a candidate with m observations whose plane is a state variable
 * gets, behind its 2m bearing rows, m equal point-on-plane rows (update/UpdaterHelper.cpp:447-512: residual -(n^T p - d)/sigma_c at
 * the current values, H_f = n^T/sigma_c and H_c_plane in the plane's three columns at the first estimates when do_fej - the new
 * landmark's first estimate is its value, the plane has cp_fej), and StateHelper::initialize runs on those 3m rows (chi2 of the
 * 3m - 3 update rows against chi2_multiplier * quantile_0.95(3m)).  If that fails the candidate is tried once more without its plane,
 * linearised at p_FinG_noplane (the position before plane refinement, UpdaterSLAM.cpp:320-321); if that fails too it is rejected.
 * Every accepted candidate moves the state, the closest points of the planes included (Vec::update is additive): the planes live in
 * a device table during the call, and the next candidate on the same plane is linearised at the corrected plane. */
typedef struct {
  int n_planes;                 /* planes of the STATE the candidates refer to */
  const int *plane_state_id;    /* [n_planes] Type::id()                       */
  const double *cp, *cp_fej;    /* [n_planes*3] value() / fej() (cp_fej NULL = cp) */
  const int *plane_of_cand;     /* [n_feats] 0 = none, else 1-based slot (the convention of ovp_plane_batch::plane_of_feat) */
  const double *p_FinG_noplane; /* [n_feats*3] linearisation point of the fallback attempt (features_p_FinG_original);
                                   NULL = the same point as the first attempt */
} ovp_dinit_planes;

/* The loop of ovp_slam_delayed_init / ovp_slam_delayed_init_general - ONE enqueue, one synchronisation - for candidates with or
 * without a plane.  candidates->cam_idx == NULL: every observation is camera 0's, tables of ovp_state_upload (the rows of
 * ovp_slam_delayed_init); otherwise the general rows over ovp_cameras_upload.  At most OVP_MAX_MEAS observations per candidate.
 * A plane candidate is enqueued as two attempts on the same three-column slot; the second reads the first one's verdict on the
 * device and does nothing when it was accepted (no host round trip in between).
 * status[l]: 0 rejected, 1 accepted (with its plane rows if it had a plane), 2 accepted by the fallback without them (the caller
 * sets _features_SLAM_to_PLANE[featid] = 0) - the codes of ovp_slam_update; chi2[l] = statistic of the attempt that decided.
 * new_id, delta_init, dx, dx_stride, the removal of rejected candidates' blocks and OVP_E_NEGDIAG as ovp_slam_delayed_init; the dx
 * of an accepted candidate carries the correction of every plane's closest point at its state id, which the device table has
 * already taken.  With planes == NULL, n_planes == 0 or plane_of_cand all zero the outputs equal those of ovp_slam_delayed_init /
 * ovp_slam_delayed_init_general on the same input.
 * OVP_E_ARG (checked before anything is enqueued): plane_of_cand outside [0, n_planes], a plane_state_id outside the covariance, a
 * closest point of zero norm.  OVP_E_CAPACITY (nothing touched): as the entries above; a plane candidate has 3m - 3 update rows and
 * three more columns, and the LDS of k_init_core (ovp_init_core_lds(3, 3m - 3, 6m + 17) against 152 KB) binds first: with all 14
 * calibration columns estimated a camera-0 plane candidate fits up to m = 22 observations (m = 30 without a plane). */
int ovp_slam_delayed_init_planes(ovp_ctx *ctx, const ovp_update_opts *opts, const ovp_general_batch *candidates,
                                 const ovp_dinit_planes *planes, uint8_t *status, double *chi2, int *new_id, double *delta_init,
                                 double *dx, int dx_stride);

/* StateHelper::EKFPropagation (state/StateHelper.cpp:41-119): new variables occupy [new_start, new_start+phi_size),
 * Phi is [phi_size x sum(old_sizes)] column-major, Q is [phi_size x phi_size] (upper triangle read). */
int ovp_cov_propagate(ovp_ctx *ctx, int new_start, int phi_size, const int *old_ids, const int *old_sizes, int n_old,
                      const double *Phi_host, const double *Q_host, int *neg_diag);

/* StateHelper::clone (state/StateHelper.cpp:346-396): appends an exact copy of [src_id, src_id+size) at the end, bit for bit
 * as the reference.  The covariance is then positive SEMI-definite until the next propagation; the update entry points fall back
 * to their pivot-dropping / S-form paths when chol(P) meets the zero pivot.
 * ovp_cov_clone_jitter(ctx, rel) > 0 restores the round-2 behaviour (diagonal of the new block stored rel above the copied
 * value, default 0 = off): it keeps such a prior on the fast path at the price of a 1e-11-level departure from the reference. */
int ovp_cov_clone(ovp_ctx *ctx, int src_id, int size);
int ovp_cov_clone_jitter(ovp_ctx *ctx, double relative_inflation);
/* StateHelper::marginalize (state/StateHelper.cpp:276-344): removes rows/cols [id, id+size). */
int ovp_cov_marginalize(ovp_ctx *ctx, int id, int size);
/* StateHelper::marginalize (state/StateHelper.cpp:276-344) for several variables at once: removes the rows/cols of every range
 * [ids[r], ids[r]+sizes[r]) in ONE pass over the covariance (k_retire.hip), where a loop of ovp_cov_marginalize copies it once
 * per variable.  ids / sizes use the numbering the state has BEFORE the call and may come in any order.  The covariance and
 * ovp_cov_size afterwards are bit-equal to ovp_cov_marginalize called once per range in descending order of id.
 * Checked on the host before anything is touched: a range outside [0, n), a size below 1 or two ranges that overlap ->
 * OVP_E_ARG; no covariance -> OVP_E_STATE; n_ranges == 0 -> 0, and nothing is launched or written.  Does not wait for the device. */
int ovp_cov_marginalize_many(ovp_ctx *ctx, int n_ranges, const int *ids, const int *sizes);

/* StateHelper::merge_planes_and_marginalize (state/StateHelper.cpp:654-757) from the first fused pair to the last retired plane,
 * one enqueue and one wait.  The caller has run the reference's two loops as a plan (none of its renames, erasures or retirements
 * depends on a pair's acceptance) and names the pairs in the order the reference meets them; all columns are those the state has
 * BEFORE the call.
 * Per pair (:693-734): res = (0 - (cp_new - cp_old)) / sigma, H = [I, -I] / sigma over the two planes' columns,
 * S = H P H^T + I, chi2 = res^T S^-1 res, the angle of the two unit normals in degrees; accepted when
 * chi2 < plane_merge_chi2 * chi2_0.95(3) AND angle < plane_merge_deg_max, and then a three-row StateHelper::EKFUpdate (:121-202).
 * Pair k+1 sees the covariance and the closest points pair k left (cp += dx, closest points are Vec(3)); a plane may take part
 * in several pairs, but none after it was fused away.  Removing rows / columns changes no other entry of the covariance, so the
 * removals are deferred: behind the last pair every range of retire_* leaves in one pass, as ovp_cov_marginalize_many does it.  The
 * old plane of every pair must be among them (it leaves whether or not its pair was accepted).
 * Outputs per pair: accepted, chi2, angle_deg, and dx [n] at dx + k * dx_stride (dx_stride >= n = ovp_cov_size before the call),
 * zero for a rejected pair.  The caller applies the accepted corrections IN ORDER through its variables' update: a quaternion
 * update does not add, so they cannot be summed.
 * Checked on the host before anything is touched: a column outside the state, new == old (or overlapping), an old column missing
 * from retire_*, overlapping retire ranges, a pair naming a plane not in plane_col or one an earlier pair fused away ->
 * OVP_E_ARG; more than 64 pairs -> OVP_E_CAPACITY.  A negative diagonal after a merge is OVP_E_NEGDIAG behind the wait, with the
 * call carried out, as ovp_ekf_update reports it. */
typedef struct {
  int n_pairs;            /* merges, in the order the reference meets them          */
  const int *new_col;     /* [n_pairs] first column of the surviving plane           */
  const int *old_col;     /* [n_pairs] first column of the plane that is fused away  */
  int n_planes;           /* distinct planes named above                             */
  const int *plane_col;   /* [n_planes] their first columns                          */
  const double *cp;       /* [3 * n_planes] their closest points (values) at entry   */
  double sigma_plane_merge, plane_merge_chi2, plane_merge_deg_max;
  int n_retire;           /* ranges that leave behind the merges (olds included)     */
  const int *retire_ids, *retire_sizes;
} ovp_plane_merge_in;
int ovp_planes_merge_retire(ovp_ctx *ctx, const ovp_plane_merge_in *in, uint8_t *accepted /* [n_pairs] */,
                            double *chi2 /* [n_pairs] */, double *angle_deg /* [n_pairs] */,
                            double *dx /* [n_pairs * dx_stride] */, int dx_stride);

/* UpdaterZeroVelocity::try_update from the stacked system to the corrected covariance (update/UpdaterZeroVelocity.cpp:119-265),
 * gate and update in one device pass: one upload, one enqueue, one wait.  The caller keeps the preamble (:71-111), selects the
 * readings (Propagator::select_imu_readings, :99-101), runs the disparity test (:207-227) and compares |v| with
 * zupt_max_velocity BEFORE the call - both are inputs of the decision - and does the bookkeeping behind it (:245-247, :267-271).
 * Every interval i of the n_readings - 1 contributes the same 6 x 9 block H0 = [[0, -I, 0], [-skew(R_jac g), 0, -I]] over
 * [theta, b_g, b_a] (columns imu_id + {0..2, 9..14}), the residual r_i = -[w_i - b_g ; a_i - b_a - R g] of its FIRST reading
 * (:141-166) and the noise zupt_noise_multiplier * sigma^2 / dt_i (:168-180).  With T = sum dt_i, rbar = sum dt_i r_i / T,
 * D = diag(1 / (mult sigma_w^2) I3, 1 / (mult sigma_a^2) I3), Rbar = (T D)^-1 and P' = P + Q_bias on the bias block,
 * Q_bias = T diag(sigma_wb I3, sigma_ab I3) (sigmas, not squares, as :184-186 has it), the stacked form equals, exactly,
 *   chi2 = sum dt_i (r_i - rbar)^T D (r_i - rbar) + rbar^T Sbar^-1 rbar,   Sbar = H0 P'_ss H0^T + Rbar  (6 x 6, = Lbar Lbar^T)
 *   P+ = P' - Y Y^T,  dx = Y z,   Y = P'_{:,s} H0^T Lbar^-T (n x 6),  z = Lbar^-1 rbar
 * with 6 (n_readings - 1) degrees of freedom (:191-204, :256-265).  The sums run over a fixed tree in a fixed order, no atomics:
 * two calls on the same input return the same bits.
 *   accepted = disparity_passed || (chi2 <= chi2_threshold && vel_ok)                                       (:231-236)
 * chi2_threshold = chi2_multipler * ovp_chi2_quantile_095(6 (n_readings - 1)), computed by the caller.
 * Rejected: the covariance, the device tables and a factor the plane loop left are bit for bit as before, dx_host is zero.
 * Accepted: P is the reference's EKFPropagation (Phi = I) followed by its EKFUpdate, dx_host [ovp_cov_size] the correction the
 * caller applies through its variables' update; a negative diagonal is OVP_E_NEGDIAG behind the wait with the call carried out, as
 * ovp_ekf_update reports it.  A non-positive pivot of Sbar ends the call as rejected with OVP_E_NOTSPD (out and info are filled).
 * Checked on the host before anything is enqueued: fewer than two readings, a dt_i <= 0, imu_id < 0 or imu_id + 15 > n ->
 * OVP_E_ARG; more than OVP_ZUPT_MAX_READINGS readings -> OVP_E_CAPACITY; no covariance -> OVP_E_STATE.
 * info (may be NULL): n_rows = 6 (n_readings - 1), n_cols = 9, n_accepted, not_spd, neg_diag. */
#define OVP_ZUPT_MAX_READINGS 4096 /* readings of one call (the staging block; a 400 Hz IMU / 10 Hz camera window holds 42) */
typedef struct {
  int n_readings;          /* readings Propagator::select_imu_readings returned                    */
  const double *readings;  /* [n_readings][7] rows (t, w_m xyz, a_m xyz)                            */
  int imu_id;              /* Type::id() of the IMU (error order th p v bg ba)                      */
  double R_GtoI[9];        /* row-major rotation of the residual (value)                            */
  double R_GtoI_jac[9];    /* ... of the Jacobian: the first estimate with do_fej, else the value   */
  double b_g[3], b_a[3];
  double gravity_mag;
  double sigma_w, sigma_a, sigma_wb, sigma_ab; /* continuous-time noise densities (NoiseManager)    */
  double zupt_noise_multiplier;
  double chi2_threshold;
  int vel_ok;              /* |v| <= zupt_max_velocity                                              */
  int disparity_passed;    /* :207-227                                                              */
  int time_kernels;        /* diagnostics: events around the three kernels (adds a synchronisation) */
} ovp_zupt_in;
typedef struct {
  int accepted;
  int rows;                /* 6 (n_readings - 1)                                                    */
  double chi2;
  float kernel_ms[3];      /* with time_kernels: gate, rows, apply; else 0                          */
} ovp_zupt_out;
int ovp_zupt_update(ovp_ctx *ctx, const ovp_zupt_in *in, double *dx_host, ovp_zupt_out *out, ovp_update_info *info);

/* Propagator::propagate_and_clone behind its preamble (state/Propagator.cpp:37-126), from the selected IMU readings to the
 * augmented clone, in one device pass: one upload (readings, IMU state and scalars in one staged block), one enqueue, one wait.
 * It replaces the host integration of the window (:84-102, predict_and_compute :343-454 with predict_mean_discrete / _rk4),
 * StateHelper::EKFPropagation (state/StateHelper.cpp:41-119) on the IMU's 15 columns and StateHelper::augment_clone (:588-625).
 * The caller keeps the two fatal checks, the time offsets and Propagator::select_imu_readings (:39-82) and, behind the call, sets
 * the IMU's value and first estimate from `out`, the timestamp, and registers the clone at out->clone_id.
 * The reference's sequence, nothing reordered.  Per interval of the n_readings - 1: the mean (discrete, honouring imu_avg and the
 * small-angle branch of the quaternion integrator, or RK4), F in its FEJ form (the first estimates are the inputs' for the first
 * interval and the propagated mean afterwards, :447-453) or its plain form, Qd = G Qc G^T symmetrised; Phi <- F Phi,
 * Q <- 1/2 ((F Q F^T + Qd) + (.)^T).  last_w is the second-to-last reading minus b_g, the only reading minus b_g, or zero (:108-114).
 * Then EKFPropagation with Phi, Q; with `clone` an exact copy of the pose block [imu_id, imu_id + 6) appended at the end
 * (ovp_cov_clone_jitter honoured as ovp_cov_clone does); with dt_id >= 0 the time-offset term of ovp_cov_augment_dt on the new
 * block with dnc_dt = [last_w ; v propagated].  Phi, Q and dnc_dt stay on the device between the kernels; the wait brings back
 * [mean | last_w | Phi | Q | verdict] through a mailbox.  Fixed order, no atomics: two calls on the same input return the same bits;
 * Q and the covariance are symmetric to the bit.  n_readings of 0 or 1 is legal: Phi = I, Q = 0, the mean unchanged.
 * Drops a kept factor, as everything that writes the covariance; does not touch the device pose tables (the caller uploads its
 * tables before the next update).
 * Refused on the host before anything is enqueued, the covariance, its size and a kept factor bit for bit as before: a NULL
 * argument, imu_id < 0 or imu_id + 15 > n, dt_id inside the IMU block or >= n (or < -1), a non-increasing time stamp -> OVP_E_ARG;
 * n_readings > OVP_PROP_MAX_READINGS, or clone and n + 6 > n_state_max -> OVP_E_CAPACITY; no covariance -> OVP_E_STATE.  A negative
 * diagonal is OVP_E_NEGDIAG behind the wait with the call carried out (clone included, size grown) and `out` filled, as
 * ovp_cov_propagate reports it. */
#define OVP_PROP_MAX_READINGS 4096
typedef struct {
  int n_readings;          /* what Propagator::select_imu_readings returned; 0 and 1 are legal (Phi = I, Q = 0) */
  const double *readings;  /* [n_readings][7] (t, w_m xyz, a_m xyz), the layout of ovp_zupt_in::readings */
  int imu_id;              /* Type::id() of the IMU, error order th p v bg ba */
  double q[4], p[3], v[3], bg[3], ba[3];   /* State::_imu value (JPL q_GtoI) */
  double q_fej[4], p_fej[3], v_fej[3];     /* first estimates (read with do_fej) */
  double gravity_mag;
  double sigma_w, sigma_a, sigma_wb, sigma_ab;  /* continuous-time densities (NoiseManager) */
  int use_rk4, imu_avg, do_fej;
  int clone;               /* 1: StateHelper::augment_clone behind the propagation; 0: propagation only */
  int dt_id;               /* Type::id() of calib_dt_CAMtoIMU, -1 = not estimated (no rank-one term) */
  int time_kernels;        /* diagnostics as in ovp_zupt_in */
} ovp_propagate_in;
typedef struct {
  double q[4], p[3], v[3]; /* propagated mean (value and first estimate both become it, Propagator.cpp:447-453) */
  double last_w[3];        /* :108-114 */
  int n_intervals, clone_id /* id of the appended pose, -1 without clone */, neg_diag;
  double Phi[225], Q[225]; /* Phi_summed / Qd_summed, column-major 15 x 15, for the tests and the trace */
  float kernel_ms[4];      /* with time_kernels: integration, EKFPropagation, clone + time offset, publish; else 0 */
} ovp_propagate_out;
int ovp_propagate_and_clone(ovp_ctx *ctx, const ovp_propagate_in *in, ovp_propagate_out *out);

/* StateHelper::augment_clone, time-offset part (state/StateHelper.cpp:613-624):
 *   Cov[:, pose..pose+5] += Cov[:, dt] * dnc_dt^T ;  Cov[pose..pose+5, :] += dnc_dt * Cov[dt, :]   (in that order)
 * OVP_E_ARG when the pose block or dt_id leaves the state, or dt_id lies inside the pose block. */
int ovp_cov_augment_dt(ovp_ctx *ctx, int pose_id, int dt_id, const double dnc_dt[6]);
/* StateHelper::initialize_invertible, covariance part (state/StateHelper.cpp:520-573): appends a k-dimensional variable
 * (k <= 6) at the end of the state.  H_R [k x cols] column-major (ld) with per-column state ids, H_Linv [k x k] and
 * R [k x k] column-major (upper triangle of R read).  New cross-covariance = -P H_R^T H_Linv^T,
 * new block = H_Linv (H_R P H_R^T + R) H_Linv^T.  The caller applies H_Linv * res to the new variable's value. */
int ovp_cov_initialize_invertible(ovp_ctx *ctx, const double *H_R_host, int k, int cols, int ld, const int *col_ids,
                                  const double *H_Linv_host, const double *R_host);
/* StateHelper::initialize downstream of its Givens split (state/StateHelper.cpp:448-487) as ONE device sequence with one
 * synchronisation: Mahalanobis test of the update rows against the prior (:464-475), StateHelper::initialize_invertible with the
 * init rows (:489-586) and StateHelper::EKFUpdate with the update rows (:483-485).  The three separate calls (ovp_cov_marginal,
 * ovp_cov_initialize_invertible, ovp_ekf_update) cost a host round trip each - 0.4 ms per landmark of UpdaterSLAM::delayed_init.
 *   Hx_init [k x cols], H_up [rup x cols] column-major (leading dimensions k and rup), col_ids[cols]; H_Linv, R_init [k x k];
 *   res_up [rup]; noise of the update rows = r_iso * I (every caller whitens to an isotropic R); chi2_threshold =
 *   multiplier * quantile(rows of the FULL residual), as the reference compares.
 * accepted = 0: the test failed, nothing changed.  accepted = 1: the state has k more columns, dx_host[n + k] is the correction of
 * the EKF update (zeros when rup == 0 or do_update == 0); the caller applies H_Linv * res_init to the new variable's value. */
int ovp_cov_initialize(ovp_ctx *ctx, const double *Hx_init, const double *H_up, int k, int rup, int cols, const int *col_ids,
                       const double *H_Linv, const double *R_init, const double *res_up, double r_iso, double chi2_threshold,
                       int do_update, int *accepted, double *chi2, double *dx_host);
/* current covariance dimension */
int ovp_cov_size(ovp_ctx *ctx);

/* 0.95 chi-square quantile used by the gate (boost::math::quantile, update/UpdaterMSCKF.cpp:59-62) */
double ovp_chi2_quantile_095(int dof);

/* ---- plane fitting -------------------------------------------------------------------------------
 * PlaneFitting::plane_fitting (track_plane/PlaneFitting.cpp:84-199) for a batch of planes: RANSAC with the reference's fixed
 * parameters (5-point sets, 200 iterations, 80 % inliers, 5 cm, std::mt19937(8888) + std::shuffle) followed by the refit on the
 * inlier set.  Plane k owns the points [feat_start[k], feat_start[k+1]).  shuffle_variant selects which libstdc++ the
 * hypothesis sets mimic: 0 = GCC <= 10 (the reference's Ubuntu 18.04 / 20.04), 1 = GCC >= 11.
 * Outputs: abcd [n_planes*4] (unit normal, offset), inlier [n_points] (-> feats = best_inliers, :190), ok [n_planes]. */
typedef struct {
  int n_planes;
  const int *feat_start;  /* [n_planes + 1] */
  const double *p_FinG;   /* [n_points*3] Feature::p_FinG */
  int min_inlier_num;     /* StateOptions::plane_msckf_min_feat / plane_init_min_feat */
  double max_cond;        /* StateOptions::plane_msckf_max_cond / plane_init_max_cond */
  int shuffle_variant;
} ovp_planefit_batch;
int ovp_plane_fitting(ovp_ctx *ctx, const ovp_planefit_batch *batch, double *abcd, uint8_t *inlier, uint8_t *ok);

/* PlaneFitting::optimize_plane (track_plane/PlaneFitting.cpp:201-514) for a batch of planes: joint refinement of the plane's
 * closest point and its features over reprojection + point-on-plane factors (ceres/Factor_PointOnPlane.cpp) under
 * CauchyLoss(1), Ceres' dogleg trust-region loop with its default options and at most 12 iterations, then the inlier tests of
 * :456-498.  Observations of feature f are [obs_start[f], obs_start[f] + n_obs[f]); n_obs = 0 marks a SLAM feature (kept
 * constant, :274-279).  R_GtoC / p_CinG are the clonesCAM poses of every observation, uv_norm the normalised measurements.
 * Outputs per plane: cp_out (input value when the call fails), ok, iterations; per feature: p_out (refined position if kept,
 * else the input), kept (-> feats = inliers, :511).  At most 256 features per plane. */
typedef struct {
  int n_planes;
  const int *feat_start;    /* [n_planes + 1] */
  const double *p_FinG;     /* [n_feats*3] */
  const int *obs_start;     /* [n_feats] */
  const int *n_obs;         /* [n_feats] */
  int n_obs_total;
  const double *uv_norm;    /* [n_obs_total*2] */
  const double *R_GtoC;     /* [n_obs_total*9] row-major */
  const double *p_CinG;     /* [n_obs_total*3] */
  const double *cp;         /* [n_planes*3] initial closest points */
  const uint8_t *fix_plane; /* [n_planes] plane is in the state: keep cp constant */
  double sigma_px_norm;     /* sigma_pix / focal length (update/UpdaterMSCKF.cpp:271-272) */
  double sigma_c;           /* StateOptions::sigma_constraint */
  double R_GtoI[9], p_IinG[3]; /* current IMU pose (stateI) */
  double R_ItoC[9], p_IinC[3]; /* camera extrinsics (calib0) */
} ovp_planeopt_batch;
int ovp_plane_optimize(ovp_ctx *ctx, const ovp_planeopt_batch *batch, double *cp_out, double *p_out, uint8_t *kept,
                       uint8_t *ok, int *iterations);

/* The front end of the plane path for ALL planes of a frame in one device pass: PlaneFitting::plane_fitting
 * (track_plane/PlaneFitting.cpp:84-199) followed by PlaneFitting::optimize_plane (:201-514), driven as the loop of
 * update/UpdaterMSCKF.cpp:262-401 drives them, over features of any camera and any track length.  One upload, the launches, one
 * download, one synchronisation (the per-plane pair ovp_plane_fitting + ovp_plane_optimize costs 2 round trips per plane).
 *   batch    the planes' features (clone_idx, cam_idx, n_meas, p_FinG; uv is not read); n_meas = 0 marks a SLAM landmark that is
 *            held constant (:274-279).  No limit on n_meas other than max_meas.
 *   uv_norm  [n_feats*max_meas*2] f32, in the layout of batch->uv (as for ovp_triangulate_general)
 *   in       plane k owns the features [feat_start[k], feat_start[k+1]); cp[k] its closest point (read for in-state planes);
 *            fix_plane[k] != 0: the plane is in the state - RANSAC is skipped and every feature goes to the refinement with cp
 *            constant (UpdaterMSCKF.cpp:265-316).  A free plane with fewer than 4 features fails (:320-321).  refine = 0: fit
 *            only (StateOptions::use_refine_plane_feat off).
 * The camera pose of every observation comes from the resident tables: R_GtoC = R_ItoC(cam) R_GtoI(clone),
 * p_CinG = p_IinG - R_GtoC^T p_IinC(cam) (clones of ovp_state_upload, cameras of ovp_cameras_upload); the "current camera" of the
 * inlier tests (:444-453) is camera 0 of those tables at the pose R_GtoI / p_IinG given here.
 * Device sequence: k_planefit_poses (pose table) -> k_plane_ransac over the free planes -> k_planefit_link (per plane: the inliers
 * in their order, cp0 = -n d (:352), the observation lists of the refinement with pose and measurement of every item; a plane
 * whose fit failed gets an empty list) -> k_plane_refine on those device-resident lists.
 * Outputs (host, any may be NULL).  Per plane: fit_ok (1 for an in-state plane), abcd [4] (RANSAC + refit; zeros when it did not
 * run or failed), ok (fit and refinement), cp_out [3] (the input cp when not ok), iterations.  Per feature, at its input index:
 * inlier (RANSAC; 1 on an in-state plane), kept (final), p_out [3] (the refined position if kept, else the input).
 * poses [n_clones * n_cams * 12]: the pose table, entry (clone slot, camera) = R_GtoC row-major, then p_CinG.
 * Checked on the host before anything is enqueued - OVP_E_CAPACITY: more than 256 features on one plane; OVP_E_ARG: a camera
 * without tables, a clone slot outside the tables, n_meas > max_meas, feat_start not ascending or not ending at n_feats;
 * OVP_E_STATE: no ovp_state_upload / ovp_cameras_upload - both must precede the call (camera 0's extrinsics are read from the
 * host copy ovp_cameras_upload keeps). */
typedef struct {
  int n_planes;
  const int *feat_start;    /* [n_planes + 1] */
  const double *cp;         /* [n_planes*3] */
  const uint8_t *fix_plane; /* [n_planes] */
  int min_inlier_num;       /* StateOptions::plane_msckf_min_feat / plane_init_min_feat */
  double max_cond;          /* StateOptions::plane_msckf_max_cond / plane_init_max_cond */
  int shuffle_variant;      /* as ovp_planefit_batch */
  int refine;               /* 0 = fit only */
  double sigma_px_norm;     /* sigma_pix / focal length */
  double sigma_c;           /* StateOptions::sigma_constraint */
  double R_GtoI[9], p_IinG[3]; /* current IMU pose (stateI) */
} ovp_planefront_in;
typedef struct {
  uint8_t *fit_ok;   /* [n_planes] */
  double *abcd;      /* [n_planes*4] */
  uint8_t *ok;       /* [n_planes] */
  double *cp_out;    /* [n_planes*3] */
  int *iterations;   /* [n_planes] */
  uint8_t *inlier;   /* [n_feats] */
  uint8_t *kept;     /* [n_feats] */
  double *p_out;     /* [n_feats*3] */
  double *poses;     /* [n_clones*n_cams*12] */
} ovp_planefront_out;
int ovp_plane_fit_refine(ovp_ctx *ctx, const ovp_general_batch *batch, const float *uv_norm, const ovp_planefront_in *in,
                         const ovp_planefront_out *out);

/* ---- plane detection from tracked features ----------------------------------------------------- */
/* TrackPlaneOptions (track_plane/TrackPlaneOptions.h:44-80), same names and defaults (ovp_trackplane_defaults). */
typedef struct {
  int max_tri_side_px;       /* 200  */
  int max_norm_count;        /* 5, at most OVP_DET_MAX_NORMS */
  double max_norm_avg_max;   /* 25.0 */
  double max_norm_avg_var;   /* 25.0 */
  double max_norm_deg;       /* 25.0 */
  double max_dist_between_z; /* 0.10 */
  int max_pairwise_px;       /* 100  */
  int min_norms;             /* 3    */
  int check_old_feats;       /* 1    */
  int filter_num_feat;       /* 4, in 2 .. OVP_DET_MAX_FILTER_K */
  double filter_z_thresh;    /* 1.2  */
  int feat_init_min_obs;     /* 4    */
  double min_dist;           /* 0.10 */
  double max_dist;           /* 60   */
  double max_cond_number;    /* 8000 */
} ovp_trackplane_opts;
#define OVP_DET_MAX_POINTS 1024  /* tracked points of one frame (and so active features of one plane) */
#define OVP_DET_MAX_NORMS 16     /* normals kept per feature */
#define OVP_DET_MAX_FILTER_K 16  /* neighbours averaged by the spatial filter */
void ovp_trackplane_defaults(ovp_trackplane_opts *opts);
/* The per-feature history of TrackPlane (hist_feat_linsys_A / _b / _count, hist_feat_inG, hist_feat_norms_inG: track_plane/
 * TrackPlane.h) as a device table of feature slots, with the feature id -> slot map, hist_feat_to_plane, hist_plane_to_oldplanes
 * and the plane id counter on the host.  One detector per context; it goes with ovp_ctx_destroy.  _reset forgets every feature and plane. */
int ovp_plane_detector_create(ovp_ctx *ctx, const ovp_trackplane_opts *opts);
int ovp_plane_detector_destroy(ovp_ctx *ctx);
int ovp_plane_detector_reset(ovp_ctx *ctx);
/* First call of a frame: TrackPlane::perform_plane_detection_monocular, track_plane/TrackPlane.cpp:608-708 (remove_feats, the
 * linear triangulation systems and their gates).  ids [n] distinct feature ids, uv [2n] pixel positions (f32), uv_norm [2n] the
 * undistorted normalised coordinates of the same points (f64 here; the reference's undistort_cv returns a cv::Point2f, so a caller
 * who wants the reference's numbers rounds them to f32 first), R_GtoC [9] row-major and p_CinG [3] the newest clone's camera pose.
 * Outputs (either may be NULL): has_est [n]: bit 0 = the feature has a 3-D estimate, bit 1 = this frame's solution passed the gates (the vertices of the frame's triangulation are these
 * points, in this order), p_FinG [3n].  n > OVP_DET_MAX_POINTS: OVP_E_CAPACITY and nothing is touched; n = 0 returns at once, as
 * the reference does. */
int ovp_plane_detect_triangulate(ovp_ctx *ctx, int n, const int64_t *ids, const float *uv, const double *uv_norm, const double *R_GtoC,
                                 const double *p_CinG, uint8_t *has_est, double *p_FinG);
/* Second call of a frame: TrackPlane.cpp:728-1095 (triangle normals, per-feature normal history and avg_norm, pairwise matching,
 * greedy merge, spatial filter, pruning).  tris [3*n_tris] index the vertices of the preceding ovp_plane_detect_triangulate;
 * tris = NULL: the library triangulates them itself (ovp_delaunay; with ovp_plane_detector_set_device_delaunay on, the triangles
 * the first call's device triangulation left). */
int ovp_plane_detect_planes(ovp_ctx *ctx, int n_tris, const int32_t *tris);
/* on != 0: ovp_plane_detect_triangulate also triangulates the frame's vertices on the device (k_det_delaunay behind
 * k_det_triangulate: the vertices compacted on the device, pixel positions from `uv`, the triangles in the same result block and
 * the same wait), and ovp_plane_detect_planes(ctx, 0, NULL) uses those triangles where it otherwise calls the host triangulation
 * - the same triangles, so the same planes.  A frame whose device triangulation reported an overflow of its table takes the
 * host triangulation as before; explicit tris are used as before.  Default off; OVP_E_STATE without a detector. */
int ovp_plane_detector_set_device_delaunay(ovp_ctx *ctx, int on);
/* TrackPlane::get_feature2plane (track_plane/TrackPlane.h:140-143): ascending feature id; *n = entries (also when cap is smaller) */
int ovp_plane_detector_map(ovp_ctx *ctx, int64_t *ids, int64_t *planes, int cap, int *n);
/* TrackPlane::get_plane2oldplane (track_plane/TrackPlane.h:145-149): the merge history of the planes in the map as (surviving id,
 * old id) pairs, pairs [2*cap]; *n = pairs (also when cap is smaller).  With the values of ovp_plane_detector_map (the active planes)
 * this is what StateHelper::merge_planes_and_marginalize takes every frame (core/VioManager.cpp:513-534). */
int ovp_plane_detector_merges(ovp_ctx *ctx, int64_t *pairs, int cap, int *n);
/* DIAGNOSTICS / TESTS, not part of a frame (a frame is the two calls above): the spatial filter alone (TrackPlane.cpp:1003-1058)
 * on planes given as point lists: plane k = p_FinG rows feat_start[k] ..
 * feat_start[k+1]; mean_dist [n] = mean of the filter_num_feat smallest squared f32 distances to the plane's other points, flagged
 * [n] = fails the z-test.  A plane of at most filter_num_feat points is left alone (zeros); more than OVP_DET_MAX_POINTS in one
 * plane: OVP_E_CAPACITY.  Uses the staging of the context's detector (OVP_E_STATE without one), none of its history. */
int ovp_plane_spatial_filter(ovp_ctx *ctx, int n_planes, const int *feat_start, const double *p_FinG, int filter_num_feat,
                             double filter_z_thresh, double *mean_dist, uint8_t *flagged);
/* Delaunay triangulation of n pixel positions (incremental Bowyer-Watson, host arithmetic only - no context): tris [3*cap], each
 * triangle positively oriented in (x, y), its smallest index first, the list sorted (a point at the position of an earlier one
 * is left out, a zero-area triangle of a point exactly on a hull edge is dropped); *n_tris = count (OVP_E_CAPACITY above cap;
 * 2n always suffices).  Stands where the reference calls CDT (TrackPlane.cpp:717-723). */
int ovp_delaunay(int n, const float *xy, int32_t *tris, int cap, int *n_tris);
/* The same triangulation on the device (k_det_delaunay: one workgroup, the same algorithm, insertion order and predicates - the
 * triangles of ovp_delaunay, bit for bit): one upload, one launch, one publication.  Needs a context, no detector.
 * n > OVP_DET_MAX_POINTS: OVP_E_CAPACITY, nothing enqueued; n < 3: no triangles, no launch.  No fallback to the host: an overflow
 * of the kernel's triangle table (possible only after inconsistent predicate signs) is OVP_E_CAPACITY. */
int ovp_delaunay_device(ovp_ctx *ctx, int n, const float *xy, int32_t *tris, int cap, int *n_tris);
/* tests: what = "feat": out = [count, valid, p_FinG(3), n_norms, avg_norm(3), normals(3*n_norms)] of feature id; "filter": out =
 * [id, plane, mean of the neighbour distances, z-score flag] per point of every plane the last frame's filter looked at; "timer": id != 0
 * puts events around the kernels (and a stream synchronisation behind each publication) from the next frame on, "time": GPU
 * milliseconds of the last timed frame's kernels [triangulate, normals, match, filter] ([3] also behind a timed
 * ovp_plane_spatial_filter); "time_delaunay": GPU milliseconds of k_det_delaunay [in the last timed frame, in the last timed
 * ovp_delaunay_device of this context]; "tris": [source of the last ovp_plane_detect_planes' triangles: 0 the caller's, 1 the host
 * triangulation, 2 the device's; device triangulation on; of the last frame's device triangulation: overflow, vertices, most
 * table slots in use, largest cavity].  Returns the number of doubles (or < 0). */
long ovp_plane_detector_debug(ovp_ctx *ctx, const char *what, int64_t id, double *out, long cap);

/* ---- re-triangulation of a frame's active tracks ------------------------------------------------ */
/* VioManager::retriangulate_active_tracks (core/VioManagerHelper.cpp:220-418): every point tracked into the frame becomes a
 * position in G (active_tracks_posinG) and, when camera 0 sees it in this frame, a (u, v, depth) triple (active_tracks_uvd).
 * Not built: the display images (:229-234) and the distort_d branch at :387-391, which the `continue` at :376 makes unreachable. */
#define OVP_AT_MAX_POINTS 1024     /* distinct tracked features of one camera in one frame */
#define OVP_AT_MAX_LANDMARKS 1024  /* SLAM landmarks of the state */
/* The history active_feat_linsys_A / _b / _count (core/VioManager.h) as a device table of feature slots - A's upper triangle, b,
 * count - with the feature id -> slot map on the host.  One object per context; it goes with ovp_ctx_destroy.  _reset forgets
 * every feature (a VioManager that starts again). */
int ovp_active_tracks_create(ovp_ctx *ctx);
int ovp_active_tracks_destroy(ovp_ctx *ctx);
int ovp_active_tracks_reset(ovp_ctx *ctx);
typedef struct {
  /* :240-241, :251, :268 the frame's observations (get_last_obs / get_last_ids), camera by camera in the caller's sensor_ids
   * order - a feature's observations are walked in this order, and the order decides what it keeps (see ovp_active_tracks_update) */
  int n_obs;
  const int32_t *cam_idx;  /* [n_obs] camera id, 0 .. n_cams - 1; camera 0's pixels are feat_uvs_in_cam0 (:273-275) */
  const int64_t *feat_id;  /* [n_obs] at most one observation per feature and camera */
  const float *uv;         /* [2 n_obs] raw pixel (cv::Point2f pt_d, :272) */
  const double *uv_norm;   /* [2 n_obs] undistorted normalised coordinates (:283; f64 here - the reference's undistort_cv returns a
                              cv::Point2f, so a caller who wants the reference's numbers rounds them to f32 first) */
  /* :254-263 per camera id: R_GtoCi = R_ItoC R_GtoI and p_CiinG of the newest clone.  Arguments, not the context's resident tables:
   * the stage runs after the updaters have corrected the host state */
  int n_cams;              /* 1 .. OVP_MAX_CAMERAS */
  const double *R_GtoC;    /* [n_cams * 9] row-major */
  const double *p_CinG;    /* [n_cams * 3] */
  /* :360-368 camera 0's extrinsics and the newest clone, :399-400 camera 0's image size */
  double R_ItoC0[9], p_IinC0[3], R_GtoI[9], p_IinG[3];
  int width, height;
  /* :321-322 featinit_options */
  double min_dist, max_dist, max_cond_number;
  /* :342-357 the SLAM landmarks of the state */
  int n_slam;
  const int64_t *slam_id;        /* [n_slam] distinct */
  const double *slam_xyz;        /* [3 n_slam] get_xyz(false): in G, or in the anchor camera for a relative representation */
  const uint8_t *slam_relative;  /* [n_slam] LandmarkRepresentation::is_relative_representation */
  /* of the relative ones (entries of the others are not read; all four may be NULL when none is relative): the anchor clone
   * (_anchor_clone_timestamp) and the anchor camera's extrinsics (_anchor_cam_id), :348-352 */
  const double *slam_anchor_R_GtoI, *slam_anchor_p_IinG, *slam_anchor_R_ItoC, *slam_anchor_p_IinC; /* [9 n_slam], [3 n_slam], ... */
} ovp_active_tracks_in;
typedef struct {
  int cap;          /* in: entries the arrays hold */
  int n_feats, n;   /* out: distinct tracked features; entries = n_feats + n_slam (set also when cap is too small) */
  int64_t *ids;     /* [cap] the distinct tracked features in order of first appearance, then the landmarks in input order */
  uint8_t *flags;   /* [cap] bit 0: the id has a position (active_tracks_posinG), bit 1: it has a uvd (active_tracks_uvd) */
  double *p_FinG;   /* [3 cap] zeros without bit 0 */
  double *uvd;      /* [3 cap] (u_raw, v_raw, depth in camera 0 of the newest clone); zeros without bit 1 */
} ovp_active_tracks_out;
/* One frame, as the reference - its quirks included:
 *  - :277-280 a tracked feature whose id is a SLAM landmark gives camera 0 its pixel but no row to any system; it leaves the table,
 *    its tracked entry has no flag, and its position and uvd are reported in the landmark's entry;
 *  - :293-301 per observation the frame's system is OLD + A_i with count OLD + 1, "old" being what the previous frame left: a feature
 *    seen by several cameras in one frame keeps only its LAST observation's term.  A feature the previous frame did not leave is
 *    inserted with std::map::insert, which does not replace: it keeps its FIRST observation's term, count 1;
 *  - :304 the system is solved after each observation once the count is above 3 (a literal, not feat_init_min_obs), gated in the
 *    observing camera (:321-322: condition number, min_dist <= z <= max_dist, finite norm); the last solve that passes stays;
 *  - :331-334 a feature not observed in this frame leaves the table and starts again from nothing;
 *  - :342-357 the landmarks' positions (global, or anchored -> global) overwrite or extend the position set;
 *  - :372-410 a position whose id camera 0 sees is dropped from the uvd set for depth < 0.1, u < 0, (int) u >= width, v < 0,
 *    (int) v >= height.
 * n_obs = 0 with landmarks still reports the landmarks (:338).  Checked on the host before anything is touched or enqueued -
 * OVP_E_CAPACITY: more than OVP_AT_MAX_POINTS observations of one camera, more than OVP_AT_MAX_LANDMARKS landmarks, out->cap too
 * small; OVP_E_ARG: a camera id outside the call's, two observations of one feature in one camera, a repeated landmark id, a relative
 * landmark without the anchor arrays.  OVP_E_STATE without ovp_active_tracks_create.  One upload, one compute launch
 * (k_active_tracks), one publication through the object's own mailbox; two runs give the same bits. */
int ovp_active_tracks_update(ovp_ctx *ctx, const ovp_active_tracks_in *in, ovp_active_tracks_out *out);
/* tests: what = "feat": out = [count, A upper triangle (00 01 02 11 12 22), b(3)] of feature id's slot (returns 0 when the id has
 * none); "size": [features in the table]; "timer": id != 0 puts events around the kernel (and a stream synchronisation behind the
 * publication) from the next frame on, "time": GPU milliseconds of the last timed frame's kernel.  Returns the number of doubles
 * (or < 0). */
long ovp_active_tracks_debug(ovp_ctx *ctx, const char *what, int64_t id, double *out, long cap);

/* ---- feature database: a frame's tracks to the update's batch ------------------------------------ */
/* ext ov_core::FeatureDatabase between the tracker and the updaters, as VioManager::do_feature_propagate_update uses it
 * (core/VioManager.cpp:373-506, :855-869), and the cleaning of update/UpdaterMSCKF.cpp:74-100.  ov_core is not in the reference
 * tree: the database's methods are RECALLED from their published form and UNPINNED; tests/featdb_ref.py is the restatement they
 * are held to and names every recalled convention.  The call sites above are pinned.  One camera (camera 0), as ovp_state_tables:
 * the camera filter of :386-403 is a no-op.  The table lives on the device - max_slots <= OVP_FEATDB_MAX_SLOTS feature slots (the
 * tracker's point limit) of max_meas <= OVP_MAX_MEAS observations (time stamp f64, uv f32, uv_norm f32), a count, a to_delete flag
 * and the id per slot; the id -> slot map and a shadow of the counts and time stamps are the host's, so that every refusal below
 * is decided on the host with nothing touched.  The hash map's iteration order is replaced by this library's own rule: every list
 * is in ascending feature id.  Integer decisions and copies only: two runs give the same bytes. */
#define OVP_FEATDB_MAX_SLOTS 4096
#define OVP_FEATDB_NONE 0     /* still tracked, not at the marginalisation time */
#define OVP_FEATDB_LOST 1     /* :376 features_not_containing_newer(state->_timestamp, false, true) */
#define OVP_FEATDB_MARG 2     /* :380 features_containing(state->margtimestep(), false, true); lost and marg is marg (:405-415) */
#define OVP_FEATDB_MAXTRACK 3 /* :418-436 marg with more than max_clone_size measurements */
#define OVP_FEATDB_FLAG_TOO_FEW 1  /* fewer than 2 measurements are left after the cleaning (update/UpdaterMSCKF.cpp:94) */
#define OVP_FEATDB_FLAG_DELETED 2  /* Feature::to_delete */
/* One database per context (a second create: OVP_E_STATE, the first stays; it goes with ovp_ctx_destroy).  OVP_E_ARG outside the
 * limits.  _reset forgets every feature and the gathered batch. */
int ovp_featdb_create(ovp_ctx *ctx, int max_slots, int max_meas);
int ovp_featdb_destroy(ovp_ctx *ctx);
int ovp_featdb_reset(ovp_ctx *ctx);
/* ext FeatureDatabase::update_feature for the n observations of one frame (TrackBase feeds them one by one): ids [n] distinct
 * (OVP_E_ARG otherwise), uv / uv_norm [2n] f32.  A new id takes a free slot; a feature whose to_delete is set keeps collecting
 * measurements, as in the reference.  One upload, one launch (k_featdb_append, a thread per observation), no wait.
 * OVP_E_CAPACITY with nothing touched: more live features than slots, or an id whose slot already holds max_meas observations. */
int ovp_featdb_append(ovp_ctx *ctx, double timestamp, int n, const int64_t *ids, const float *uv, const float *uv_norm);
typedef struct ovp_featdb_classify_in {
  const double *clone_times; /* [n_clones] State::_clones_IMU's keys after cloning, ascending (update/UpdaterMSCKF.cpp:74-78) */
  int n_clones;              /* <= OVP_MAX_MEAS */
  int max_clone_size;        /* StateOptions::max_clone_size (:424) */
  double t_now;              /* state->_timestamp (:376) */
  double marg_time;          /* state->margtimestep() (state/State.h:70) */
  int want_marg;             /* :379 clones > max_clone_size || clones > 5 */
  int reserved;
} ovp_featdb_classify_in;
typedef struct ovp_featdb_classify_out {
  int cap;          /* in: entries the arrays hold */
  int n;            /* out: live features (set also when cap is too small: OVP_E_CAPACITY) */
  int64_t *ids;     /* [cap] ascending */
  int32_t *cls;     /* [cap] OVP_FEATDB_NONE / _LOST / _MARG / _MAXTRACK */
  int32_t *count;   /* [cap] observations held */
  int32_t *cleaned; /* [cap] observations left after ext Feature::clean_old_measurements(clone_times): those whose time stamp
                       equals a clone time exactly */
  uint8_t *flags;   /* [cap] OVP_FEATDB_FLAG_* */
  int32_t totals[4]; /* lost, marg, maxtrack, to_delete */
} ovp_featdb_classify_out;
/* zeros, max_clone_size 11, want_marg 1 */
void ovp_featdb_classify_defaults(ovp_featdb_classify_in *o);
/* :373-436 and update/UpdaterMSCKF.cpp:74-100 for every live feature, nothing modified: "newer" is a last time stamp >= t_now,
 * "containing" and the cleaning compare doubles exactly, both queries skip to_delete.  One upload, one launch (k_featdb_classify),
 * one publication through the database's mailbox, one wait.  OVP_E_ARG: clone times not strictly ascending, a NaN. */
int ovp_featdb_classify(ovp_ctx *ctx, const ovp_featdb_classify_in *in, ovp_featdb_classify_out *out);
/* Feature::to_delete = true of the named features - what the updaters do to a feature they used or refused (e.g.
 * update/UpdaterMSCKF.cpp:95).  An unknown id: OVP_E_ARG, nothing touched. */
int ovp_featdb_mark_deleted(ovp_ctx *ctx, int n, const int64_t *ids);
/* The ovp_feature_batch of the n named features, in the caller's order, built in the database's own device buffers and bound as
 * ovp_batch_bind_device binds a caller's (replaces the host packing in front of ovp_batch_upload): per feature the observations
 * that survive clean_old_measurements(clone_times), in stored order, as uv and uv_norm [n][max_meas][2], clone_idx (the index of
 * the time stamp among clone_times, -1 = padding) and n_meas; the row pitch is the database's max_meas.  old_index == NULL: p_FinG
 * is zero.  Otherwise p_FinG[f] is that of feature old_index[f] of the batch gathered before, bit for bit - the batch rebuilt from
 * the survivors of a triangulation (update/UpdaterMSCKF.cpp:120-166 erases features).  One upload, one launch (k_featdb_gather, a
 * wave per feature), no wait.  Refused with nothing touched: OVP_E_ARG for an unknown id, a feature with no observation left, one
 * with more than the pitch, an old index outside the former batch; OVP_E_STATE for old_index without a former batch;
 * OVP_E_CAPACITY for n above the slots or the context's n_feats_max.  n = 0 binds an empty batch. */
int ovp_featdb_gather(ovp_ctx *ctx, int n, const int64_t *ids, const int *old_index, const double *clone_times, int n_clones);
/* ovp_triangulate on the gathered batch, uv_norm read from the database's device buffer: the same kernel and launcher, no upload
 * of measurements.  OVP_E_STATE unless the context's batch is the one ovp_featdb_gather bound last. */
int ovp_featdb_triangulate(ovp_ctx *ctx, const ovp_triang_opts *opts, double *p_FinG_out, uint8_t *ok);
/* :855 ext FeatureDatabase::cleanup() (do_cleanup != 0: every feature whose to_delete is set goes) and then :865
 * cleanup_measurements(t) (t not NaN: every observation with a time stamp < t goes, the rest closes up in stored order, a
 * feature left without observations goes).  One launch (k_featdb_cleanup), one publication - the new counts and the freed slots,
 * which the host's map and shadow follow - one wait. */
int ovp_featdb_cleanup(ovp_ctx *ctx, int do_cleanup, double measurements_before_or_nan);
/* ext FeatureDatabase::get_feature (:472) and a test's read-back: *count = -1 for an id the database does not hold, otherwise its
 * observations (as many as cap holds) in stored order; slot, to_delete, timestamps, uv [2 cap], uv_norm [2 cap] may be NULL.
 * Synchronous. */
int ovp_featdb_get(ovp_ctx *ctx, int64_t id, int *slot, int *count, int *to_delete, double *timestamps, float *uv, float *uv_norm,
                   int cap);
/* tests: what = "uv" / "uv_norm" / "clone_idx" / "n_meas" / "p_FinG": the gathered batch (OVP_E_STATE before one); "dims": int32
 * [max_slots, max_meas, live features, gathered features or -1]; "cleanup": int64 [id, new count, freed] per feature that was live
 * at the last ovp_featdb_cleanup; "timer": level != 0 puts events around the kernel of every call from the next one on (and a
 * stream synchronisation behind it), "time": float GPU milliseconds of the last timed kernel.  Returns the number of bytes (or < 0). */
long ovp_featdb_debug(ovp_ctx *ctx, const char *what, int level, void *out, long cap);

/* ---- image front end: equalisation, image pyramid, pyramidal KLT ---------------------------------- */
/* TrackPlane::feed_new_camera (track_plane/TrackPlane.cpp:40-92: cv::equalizeHist :65, cv::buildOpticalFlowPyramid) and the
 * cv::calcOpticalFlowPyrLK call of perform_matching (:1299-1357).  OpenCV is not in the reference tree: the stage is restated from
 * its published form (Bouguet's pyramidal Lucas-Kanade with OpenCV's externally visible conventions: Scharr gradients, reflect-101
 * image borders, zero gradient borders, 30 iterations / 0.01 px, minEigThreshold 1e-4) and is UNPINNED; tests/klt_ref.py is the
 * restatement it is held to.  Detection (:1173-1297) is ovp_klt_detect below, the epipolar check (:1331-1350) ovp_klt_epipolar, the
 * intake options (histogram_method CLAHE :66-70, downsample_cameras core/VioManager.cpp:279-289) ovp_klt_feed_image_opts and
 * ovp_klt_halve.  Not built: stereo, the display images. */
#define OVP_KLT_MAX_POINTS 4096
#define OVP_KLT_MAX_LEVELS 8
#define OVP_KLT_HIST_NONE 0       /* TrackBase::HistogramMethod, in its order */
#define OVP_KLT_HIST_HISTOGRAM 1
#define OVP_KLT_HIST_CLAHE 2      /* parameters needed: use ovp_klt_feed_image_opts (ovp_klt_feed_image: OVP_E_ARG) */
/* One tracker per context (a second create that succeeds replaces the first, one that fails leaves the first in place and usable;
 * the tracker goes with ovp_ctx_destroy): two pyramids of n_levels images
 * (n_levels = maxLevel + 1: the reference's pyr_levels = 5 is 6; 1..OVP_KLT_MAX_LEVELS, every level at least 2 x 2), previous and
 * current, swapped by index and never copied.  win: the window's side (:1326 win_size), odd, 3..21 - a lane of the point's wave
 * holds ceil(win^2 / 64) <= 7 window pixels in registers.  max_points <= OVP_KLT_MAX_POINTS.  OVP_E_ARG outside these.
 * _reset forgets both images. */
int ovp_klt_create(ovp_ctx *ctx, int width, int height, int n_levels, int win, int max_points);
int ovp_klt_destroy(ovp_ctx *ctx);
int ovp_klt_reset(ovp_ctx *ctx);
/* :40-92 one 8-bit image (height rows of `stride` bytes): uploaded, equalised (:65; OVP_KLT_HIST_NONE skips it), the pyramid built
 * into the "current" half; the former current half is "previous" from here on.  One upload and one enqueue (histogram, LUT + apply,
 * one launch per level), no wait.  The image is copied before the call returns.  OVP_E_STATE without ovp_klt_create; OVP_E_ARG for
 * CLAHE (parameters needed: use ovp_klt_feed_image_opts), a null image, stride < width. */
int ovp_klt_feed_image(ovp_ctx *ctx, const uint8_t *img, int stride, int hist_method);
/* The intake options of one image: histogram_method (track_plane/TrackPlane.cpp:62-72; CLAHE :66-70 is
 * cv::createCLAHE(10.0, Size(8, 8))->apply) and downsample_cameras (core/VioManager.cpp:279-289: cv::pyrDown of image and mask to
 * Size(cols / 2.0, rows / 2.0) in front of the tracker; the reference's options loader halves the intrinsics to match,
 * core/VioManagerOptions.h:252-264).  CLAHE is RECALLED from OpenCV's published clahe.cpp and UNPINNED; tests/clahe_ref.py is the
 * restatement it is held to and names every convention (extension on both axes when either is not divisible, the clip limit's
 * truncation and floor of 1, the strided residual, the LUT's and the blend's rounding half to even, weights from the unclamped tile
 * index). */
typedef struct ovp_klt_intake {
  int hist_method;            /* OVP_KLT_HIST_NONE / _HISTOGRAM / _CLAHE */
  double clahe_clip;          /* 10.0; 0: no clipping, as in OpenCV */
  int clahe_tiles_x, clahe_tiles_y;   /* 8, 8; each 1..16 */
  int downsample;             /* 0 / 1 */
  int src_width, src_height;  /* size of the image handed over; with downsample the tracker's size is (src_width/2, src_height/2), integer division */
} ovp_klt_intake;
/* hist_method HISTOGRAM (TrackBase's default), clip 10.0 and 8 x 8 tiles (:67-68), no downsampling, a source size of 0 x 0: the
 * caller names the size */
void ovp_klt_intake_defaults(ovp_klt_intake *o);
/* ovp_klt_feed_image under these options (:40-92 behind core/VioManager.cpp:279-289): one upload - with downsample of the full-size
 * image (src_height rows of `stride` bytes), which k_klt_pyrdown halves to the tracker's size, the image the equalisation reads -
 * then the equalisation (CLAHE: k_clahe_lut, one workgroup per tile, and k_clahe_apply; the tile LUTs stay readable through
 * ovp_klt_debug "clahe_lut"), the pyramid, no wait.  Without downsample and with NONE or HISTOGRAM it leaves the current half
 * bit-equal to ovp_klt_feed_image.  Integer outputs: two runs give the same bytes.  The first call that halves allocates the
 * full-size buffers (and waits for the stream once).  Decided on the host with nothing touched: OVP_E_STATE without a tracker;
 * OVP_E_ARG for a null argument, an unknown method, downsample outside 0..1, tiles outside 1..16, a clip that is negative or not
 * finite, a source size other than the tracker's (with downsample: src_width / 2 or src_height / 2 other than the tracker's, or
 * below 1), stride < src_width.  The tile geometry and the clip limit are checked for every method. */
int ovp_klt_feed_image_opts(ovp_ctx *ctx, const uint8_t *img, int stride, const ovp_klt_intake *intake);
/* core/VioManager.cpp:284-288 the second cv::pyrDown, the one on the mask (and the debug view of the image's halving): src
 * (src_height rows of `stride` bytes) to dst [src_height / 2][src_width / 2], rows packed - the same 5-tap kernel, rounding and
 * reflect-101 as a pyramid level, to floor(w / 2) x floor(h / 2) where a pyramid level has (w + 1) / 2.  The mask is consumed on
 * the host (keep rule, detector), so this entry waits.  Any size up to 32768 x 32768, whatever the tracker's; it uses the tracker's
 * buffers and stream: OVP_E_STATE without one.  OVP_E_ARG for a null argument, stride < src_width, src_width / 2 < 1 or
 * src_height / 2 < 1. */
int ovp_klt_halve(ovp_ctx *ctx, const uint8_t *src, int stride, int src_width, int src_height, uint8_t *dst);
/* :1326-1330 n points of the previous image (pts_prev [2n] f32 pixels) into the current one, starting at guess [2n] (NULL: pts_prev,
 * as the reference passes pts1 = pts0 with OPTFLOW_USE_INITIAL_FLOW): pts_out [2n], status [n] (1 found; 0: the window left the
 * image at level 0 or the texture gate refused level 0 - pts_out then holds where the coarser levels left the point).  The error
 * output the reference ignores (:1327) is not computed.  One upload, one launch (k_klt_track, one wave per point), one publication
 * through the tracker's mailbox; f32, every sum in a fixed order: two runs give the same bits.  Decided on the host with nothing
 * enqueued and the outputs untouched: OVP_E_STATE before two images were fed, OVP_E_CAPACITY for n > max_points, OVP_E_ARG for a
 * non-finite coordinate; n = 0 returns at once.  No point or guess, however far outside, makes the kernel read outside a level. */
int ovp_klt_track(ovp_ctx *ctx, int n, const float *pts_prev, const float *guess, float *pts_out, uint8_t *status);
/* Grider_FAST::perform_griding as perform_detection_monocular calls it (track_plane/TrackPlane.cpp:1262; the stage replaces the
 * device part of :1173-1297): cv::FAST (9 of 16, non-maximum suppression) on every grid cell of level 0 of a half (0: current,
 * 1: previous), the K strongest corners of a cell, cv::cornerSubPix ((5,5), 20 iterations, 0.001) on each.  Grider_FAST and OpenCV
 * are not in the reference tree: the stage is RECALLED from its published form and UNPINNED; tests/fast_ref.py is the restatement
 * it is held to.  Ties of equal score go in raster order (row, then column) - this library's own rule, the reference leaves them to
 * std::sort.  num_features < grid_x grid_y shrinks the grid as Grider_FAST does; K = (int)(num_features / cells) + 1; cells of
 * (width / grid_x) x (height / grid_y) pixels, as many as fit (more than grid_x per row when the division leaves a remainder).
 * Returns EVERY selected candidate - at most K per cell, whatever the mask (the mask test, the occupancy grid and the ids are the
 * caller's: ov_plane::TrackPlane::perform_detection_monocular, capi.KltTracker.detect) - in output order (cell ascending, then
 * score descending): n_out, xy_int [2n] the corner's pixel, response [n] its score (the largest threshold it is still a corner
 * at), xy_refined [2n] f32, cell [n]; the arrays hold `cap` points.  Three launches (k_fast_score_nms, k_fast_select,
 * k_fast_subpix: one wave per point) and one publication through the tracker's mailbox: one enqueue, one wait.  The integer outputs
 * are the same bytes on every run, and so are the refined positions (every sum in a fixed order).  Decided on the host with nothing
 * enqueued and the outputs untouched: OVP_E_STATE without a tracker or without an image in that half; OVP_E_ARG for a threshold
 * outside 0..255, num_features or a grid dimension below 1, a grid dimension above the image's, half outside 0..1, a null output;
 * OVP_E_CAPACITY for more than OVP_FAST_MAX_CELLS cells, K above OVP_FAST_MAX_K, K cells above cap or above the tracker's
 * max_points.  n_out = 0 is a success.  Every image read is clamped into the level. */
#define OVP_FAST_MAX_CELLS 4096
#define OVP_FAST_MAX_K 256
int ovp_klt_detect(ovp_ctx *ctx, int half, int num_features, int grid_x, int grid_y, int threshold, int *n_out, int32_t *xy_int,
                   int32_t *response, float *xy_refined, int32_t *cell, int cap);
/* The epipolar check of perform_matching (:1331-1350): undistort_cv of both point sets, cv::findFundamentalMat(FM_RANSAC, threshold,
 * confidence) on the normalised points, mask_out = status & mask_rsc.  OpenCV and ov_core are not in the reference tree: the stage
 * is RECALLED from its published form (cv::undistortPoints' 5 iterations, cv::fisheye::undistortPoints' Newton steps, run7Point,
 * computeError, checkSubset, RANSACPointSetRegistrator::run without a refit) and UNPINNED; tests/epi_ref.py is the restatement it
 * is held to.  This library's own: the draws (a stateless counter-based generator - cv::RNG's cannot be reproduced), at most
 * OVP_EPI_MAX_SUBSET_TRIES sets per hypothesis, the null space by elimination with complete pivoting, and that every one of
 * max_iters hypotheses is evaluated on the device (the sequential loop's early stop is replayed over their counts). */
#define OVP_EPI_MAX_ITERS 1024
#define OVP_EPI_MAX_SUBSET_TRIES 8
#define OVP_EPI_MIN_POINTS 10     /* :1319 */
#define OVP_EPI_MODE_NORMALISED 0 /* the points are normalised coordinates already: passed through */
#define OVP_EPI_MODE_RADTAN 1     /* intrinsics fx fy cx cy k1 k2 p1 p2 */
#define OVP_EPI_MODE_EQUIDISTANT 2 /* intrinsics fx fy cx cy k1 k2 k3 k4 */
typedef struct ovp_epipolar_opts {
  int32_t mode;          /* OVP_EPI_MODE_* */
  int32_t max_iters;     /* 1..OVP_EPI_MAX_ITERS; 1000 */
  double intrinsics[8];
  double threshold;      /* in normalised units, > 0: the caller's 2.0 / max(fx, fy) (:1341-1344) */
  double confidence;     /* in (0, 1); 0.999 */
  uint32_t seed;
  uint32_t reserved;
} ovp_epipolar_opts;
typedef struct ovp_epipolar_info {
  double F[9];           /* the winner, row-major, F33 = 1 unless it was tiny; zeros without a model */
  int32_t best_count;    /* its inliers among all n points, status or not */
  int32_t winner_h, winner_model; /* -1 without a model */
  int32_t niters;        /* of the replayed loop, at its end */
  int32_t n_with_model;  /* hypotheses that gave at least one model */
  int32_t too_few;       /* n < OVP_EPI_MIN_POINTS (:1319-1323): the mask is all zeros */
  int32_t no_model;      /* no hypothesis beat 6 inliers: the mask is all zeros */
  int32_t stop;          /* the first hypothesis the replayed loop did not look at */
} ovp_epipolar_info;
void ovp_epipolar_defaults(ovp_epipolar_opts *o);
/* n points: pts0 / pts1 [2n] f32 pixels of the previous and the current image (normalised values in mode 0), status [n] (NULL: all
 * ones; the RANSAC sees every point whatever its status, :1333-1344).  Writes mask_out [n], uvn0 / uvn1 [2n] f32 (the undistorted
 * coordinates) and info; any output may be NULL.  One upload, four launches (k_epi_undistort, k_epi_models, k_epi_count,
 * k_epi_select), one publication through the tracker's mailbox: one enqueue, one wait.  f64 with contraction off; two runs give
 * the same bytes.  Decided on the host with nothing enqueued and the outputs untouched: OVP_E_STATE without a tracker,
 * OVP_E_CAPACITY for n > max_points, OVP_E_ARG for n < 0, a null input, a non-finite coordinate or intrinsic, an unknown mode, a
 * threshold that is not positive and finite, a confidence outside (0, 1), max_iters outside 1..OVP_EPI_MAX_ITERS.  n = 0 returns
 * at once; n < OVP_EPI_MIN_POINTS returns success with a zero mask and too_few (the coordinates are still undistorted). */
int ovp_klt_epipolar(ovp_ctx *ctx, const ovp_epipolar_opts *opts, int n, const float *pts0, const float *pts1, const uint8_t *status,
                     uint8_t *mask_out, float *uvn0, float *uvn1, ovp_epipolar_info *info);
/* The back half of TrackPlane::feed_monocular in one device pass (track_plane/TrackPlane.cpp:510-567): the temporal KLT
 * (:515, :1326-1330), the epipolar check (:1331-1350), the keep rule (:536-551) and database->update_feature (:553-557), which
 * ovp_klt_track, ovp_klt_epipolar, the caller's own keep rule and ovp_featdb_append carry out as four entries with host code between
 * them.  The kernels in front are those entries' own, unchanged, reading the device-resident points and status; k_klt_keep_append
 * (one workgroup) then applies the keep rule - mask_epi != 0, !(x < 0), !(y < 0), trunc(x) < cols, trunc(y) < rows, evaluated in
 * float (no conversion overflows, a NaN is dropped), and mask[(int) y][(int) x] <= 127, read only behind the bounds test - compacts
 * the survivors in order and, with to_database, appends each to the context's feature database: a known id to its slot, the k-th
 * fresh survivor to the k-th slot ovp_featdb_append would hand out, so that slots, table and every later call equal the unfused
 * sequence's byte for byte.  Integer decisions and copies behind the unchanged kernels: two runs give the same bytes.
 * One upload (points, ids, per-candidate slot / fresh flag, the free-slot list, the RANSAC's table, the mask when given), N
 * launches (k_klt_track; with check k_epi_undistort, k_epi_models, k_epi_count, k_epi_select, without it and with epi
 * k_epi_undistort alone - of both point sets, the kernel as it is; k_klt_keep_append), one publication through the tracker's
 * mailbox, one wait.  The first call (and the first with a mask) grows the tracker's staging - the mask's device buffer is its
 * tail - and result block and waits for the stream once.
 * The rules of feed_monocular, applied on the host before anything is enqueued: n = 0 returns at once with n_kept = 0; with check
 * and n < OVP_EPI_MIN_POINTS the call succeeds with info.too_few, keep and mask_epi all zeros, no KLT and nothing appended
 * (:1319-1323; pts_out, status and uvn are not written).
 * Refused on the host with nothing enqueued, the outputs untouched and the database untouched - OVP_E_STATE: no tracker, fewer than
 * two images fed, to_database without ovp_featdb_create; OVP_E_CAPACITY: n > max_points, with to_database a candidate whose slot
 * already holds max_meas observations, or live features + fresh candidates above the slot count; OVP_E_ARG: a null input, n < 0,
 * duplicate ids, a non-finite coordinate, mask_stride < width, epi == NULL with check or to_database, with to_database a NaN time
 * stamp, anything ovp_klt_epipolar refuses in epi.  Both database conditions are STRICTER than the unfused sequence, which learns the
 * survivors first and counts only those: a frame this entry refuses for capacity may pass there.
 * A failure behind the checks (a HIP error of a launch or of the publication, a mailbox wait that fails) returns its code with the
 * outputs unwritten; the staged upload is left for the next call's begin to wait out, which is safe.  NOT recovered: with
 * to_database, if the wait fails after k_klt_keep_append has run, the device table may hold the frame's observations while the
 * host's id -> slot map and shadow do not - the database is then out of step with the device and has to be reset (ovp_featdb_reset)
 * or destroyed; nothing in the library repairs it.
 * With the timer on ("timer" of ovp_klt_debug) the call fills its own slots of "time": k_klt_track, the epipolar slots (the four
 * kernels with check; k_epi_undistort alone and three zeros without it; four zeros without epi) and k_klt_keep_append. */
typedef struct ovp_klt_frame_in {
  int n;                       /* points of the previous image, <= the tracker's max_points */
  const float *pts_prev;       /* [2n] */
  const int64_t *ids;          /* [n] distinct */
  double timestamp;            /* message.timestamp (:556) */
  const uint8_t *mask;         /* the current image's mask, the tracker's size, or NULL (no mask) */
  int mask_stride;
  const ovp_epipolar_opts *epi;/* camera mode + intrinsics (+ RANSAC options); NULL only if check == 0 && to_database == 0 */
  int check;                   /* 1: perform_matching's epipolar check decides (mask_out = status & mask_rsc); 0: the status alone */
  int to_database;             /* 1: the survivors are appended to the context's feature database */
} ovp_klt_frame_in;
typedef struct ovp_klt_frame_out {   /* every array may be NULL */
  int n_kept;
  uint8_t *keep;      /* [n] */
  float   *pts_out;   /* [2n] where KLT left every point */
  uint8_t *status;    /* [n] KLT status */
  uint8_t *mask_epi;  /* [n] status & mask_rsc (== status when check == 0) */
  float   *uvn;       /* [2n] undistort_cv of pts_out (only when epi != NULL) */
  int32_t *kept_index;/* [n] the first n_kept entries: the indices of the survivors, ascending */
  ovp_epipolar_info info; /* of the check; without it zeros and winner -1 */
} ovp_klt_frame_out;
int ovp_klt_match_frame(ovp_ctx *ctx, const ovp_klt_frame_in *in, ovp_klt_frame_out *out);
/* tests: what = "cur" / "prev": the bytes of pyramid level `level` of that half (rows packed); "equalized": level 0 of the current
 * half; "dims": int32 [width, height] of the level; "iters": uint8 [n][8] iterations per level of the last ovp_klt_track (none
 * behind an ovp_klt_detect, which takes the mailbox); "score" / "nms": uint8 [height][width], the level-0 score map of the last
 * ovp_klt_detect and the same after suppression (OVP_E_STATE before one); "refine" (TESTS ONLY: synchronous, and it overwrites the mailbox's device block): k_fast_subpix on level = n points of the
 * caller's on level 0 of the current half - out holds float [2n] starting positions on entry and the refined ones on return;
 * "timer": level != 0 puts events around the kernels (and a stream synchronisation behind each entry) from the next call on,
 * "time": float GPU milliseconds of the last timed calls [equalise, pyramid launches together, k_klt_track, k_fast_score_nms,
 * k_fast_select, k_fast_subpix, k_epi_undistort, k_epi_models, k_epi_count, k_epi_select, the intake's halving, k_clahe_lut,
 * k_clahe_apply (the last three 0 where the last feed did not run them), k_klt_keep_append of the last ovp_klt_match_frame] - as
 * many as cap holds, at least the first 3.  "frame_uv" / "frame_uvn": float [n_kept][2], the compacted survivors (pixels; undistorted,
 * with epi) the last ovp_klt_match_frame published - OVP_E_STATE once another entry has taken the mailbox.
 * "clahe_lut": uint8 [tiles_y tiles_x][256], the tile LUTs of the last CLAHE feed (OVP_E_STATE before one).  Of the last ovp_klt_epipolar that ran its RANSAC (n >= OVP_EPI_MIN_POINTS; OVP_E_STATE before one; H its max_iters, level is
 * ignored): "epi_samples"
 * int32 [H][7] (-1 without a set), "epi_models" int32 [H] n_models then double [H][3][9] (the doubles start at the next multiple
 * of 8 bytes), "epi_counts" int32 [H][3], "epi_table" int32 [n + 1].  Returns the number of bytes (or < 0). */
long ovp_klt_debug(ovp_ctx *ctx, const char *what, int level, void *out, long cap);

/* ---- diagnostics ---------------------------------------------------------------------------- */
/* copies an internal device buffer to host for tests: name in {"A","b","L","T","Lt","Y","G","rec","chi2",
 * "gramS","syrk"}; returns the byte count copied (or <0).
 * Of the last ovp_slam_update / ovp_slam_update_general (OVP_E_STATE before one), valid until the next call that uses the same
 * scratch: "slam_cols" int32 [gcols], the call's column list; "slam_Ht" double [gcols][m_total], the stacked H^T (row g = state
 * column slam_cols[g]); "slam_res" double [m_total]; "slam_M" double [n][m_total], M = P[:, columns] H^T, where the S-form ran
 * (OVP_E_STATE behind the information form); "slam_dims" int32 [m_total, gcols, 1 where the S-form ran, 1 where the gate kept a
 * landmark's block in LDS].  A call that fails before its gate leaves nothing to read (OVP_E_STATE).
 * "point_route": the route the last ovp_msckf_update / ovp_msckf_build_gate_gram_async planned (OVP_E_STATE before one), int32
 * [feature launch: 0 fused with chol(P) in workgroup 0, 1 fused shape with workgroup 0 idle, 2 one wave per feature | chol(P): 0 none
 * (the plane loop's factor), 1 workgroup 0, 2 side stream, 3 main stream behind the feature launch | second half: 0 tile kernels,
 * 1 sub-state, 2 global-memory fallback | reversed-order factor | leading block of T | diagonal entries boosted | features that own
 * rows | sub-state columns]; touches no stream. */
long ovp_debug_read(ovp_ctx *ctx, const char *name, void *host, long max_bytes);
/* like ovp_kernel_timer, for the dominant kernel of the plane loop (k_chol2: both factorizations, gate, solve and commit of one
 * plane): enable = 1: HIP events around every k_chol2 launch of ovp_msckf_plane_update AND around the whole loop; enable = 2: around
 * the whole loop only (first launch .. covariance product; read through ovp_host_timing [7]) - events between dependent launches
 * cost microseconds each, so the loop's own time is taken without the per-launch ones */
int ovp_plane_kernel_timer(ovp_ctx *ctx, int enable, int reset, float *avg_ms, int *n_launches);
/* host clock of the two update entry points, accumulated since the last reset (ms): ovp_msckf_plane_update [0] entry -> first
 * launch (grouping of the features by plane, staging tables), [1] entry -> last launch enqueued, [2] wait for the device, [3] calls;
 * ovp_msckf_update [4] enqueue, [5] wait for the published results, [6] calls; [7] the plane loop on the DEVICE clock (HIP events around the whole loop,
 * accumulated only while ovp_plane_kernel_timer is enabled).  bench.py reports them per step. */
int ovp_host_timing(ovp_ctx *ctx, int reset, double *out8);
/* tile Cholesky (the factorization every EKF update and every plane of the plane loop runs) on a host matrix: dense factor of the
 * matrix bordered with brow ((n+1) x (n+1), row-major; brow may be NULL), z = L^-1 brow, y = L^-T z, pivots; avg_ms = average
 * duration over `reps` launches.  n <= ovp_chol2_max_n() (287). */
int ovp_debug_chol2(ovp_ctx *ctx, const double *A_host, int n, int lda, const double *brow_host, int add_identity, double *L_host,
                    double *z_host, double *y_host, double *piv_host, int reps, float *avg_ms);
/* pivot floor of the following ovp_debug_chol2 calls (0 = none): a pivot below it drops its column, as the range part of the
 * plane loop's solve does for the directions a plane's rows do not determine */
void ovp_debug_chol2_floor(double piv_floor);
/* per-stage GPU time of the last update in milliseconds: [0]=build/gate, [1]=gram, [2]=ekf, [3]=total */
int ovp_last_timings(ovp_ctx *ctx, float *ms4);
/* enables hipEvent timing of the dominant kernel; returns avg ms per launch since last reset */
int ovp_kernel_timer(ovp_ctx *ctx, int enable, int reset, float *avg_ms_feat, int *n_launches);

#ifdef __cplusplus
}
#endif
#endif /* OVPLANE_HIP_H */
