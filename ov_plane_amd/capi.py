"""ctypes binding of libovplane_hip.so (include/ovplane_hip.h).

The library is the product: there is no CPU fallback.  Importing this module without the built extension, or
creating a context without a gfx950 device, raises."""
from __future__ import annotations

import ctypes as C
import os
import time

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OVP_LIB_AB") or os.path.join(_HERE, "libovplane_hip.so")  # OVP_LIB_AB: another build of the same library (A/B timing runs)
OVP_MAX_MEAS = 32
OVP_EPI_MIN_POINTS = 10  # ovplane_hip.h (:1319)
OVP_E_ARG, OVP_E_CAPACITY, OVP_E_NOTSPD, OVP_E_NEGDIAG, OVP_E_NODEVICE, OVP_E_STATE, OVP_E_TIMEOUT = -1, -2, -3, -4, -5, -6, -7


class OvpError(RuntimeError):
    def __init__(self, code, where):
        self.code = code
        try:
            msg = lib().ovp_error_string(code).decode()
        except Exception:  # pragma: no cover
            msg = "?"
        super().__init__("%s failed with code %d (%s)" % (where, code, msg))


class UpdateOpts(C.Structure):
    _fields_ = [
        ("sigma_px", C.c_double),
        ("chi2_multiplier", C.c_double),
        ("sigma_constraint", C.c_double),
        ("do_fej", C.c_int),
        ("do_calib_camera_pose", C.c_int),
        ("do_calib_camera_intrinsics", C.c_int),
        ("skip_plane_used", C.c_int),
    ]


class StateTables(C.Structure):
    _fields_ = [
        ("n_state", C.c_int),
        ("n_clones", C.c_int),
        ("clone_q", C.POINTER(C.c_double)),
        ("clone_p", C.POINTER(C.c_double)),
        ("clone_q_fej", C.POINTER(C.c_double)),
        ("clone_p_fej", C.POINTER(C.c_double)),
        ("clone_id", C.POINTER(C.c_int)),
        ("calib_q", C.c_double * 4),
        ("calib_p", C.c_double * 3),
        ("calib_id", C.c_int),
        ("intrinsics", C.c_double * 8),
        ("intr_id", C.c_int),
        ("cam_fisheye", C.c_int),
    ]


class FeatureBatch(C.Structure):
    _fields_ = [
        ("n_feats", C.c_int),
        ("max_meas", C.c_int),
        ("uv", C.c_void_p),
        ("clone_idx", C.c_void_p),
        ("n_meas", C.c_void_p),
        ("p_FinG", C.c_void_p),
    ]


class PlaneBatch(C.Structure):
    _fields_ = [
        ("n_planes", C.c_int),
        ("plane_of_feat", C.c_void_p),
        ("cp", C.c_void_p),
        ("cp_fej", C.c_void_p),
        ("plane_state_id", C.c_void_p),
        ("n_slam", C.c_int),
        ("slam_plane", C.c_void_p),
        ("slam_state_id", C.c_void_p),
        ("slam_p", C.c_void_p),
        ("slam_p_fej", C.c_void_p),
        ("force_decision", C.c_void_p),
    ]


class SlamBatch(C.Structure):
    _fields_ = [
        ("n_landmarks", C.c_int),
        ("max_meas", C.c_int),
        ("uv", C.c_void_p),
        ("clone_idx", C.c_void_p),
        ("n_meas", C.c_void_p),
        ("p_FinG", C.c_void_p),
        ("p_FinG_fej", C.c_void_p),
        ("landmark_id", C.c_void_p),
        ("plane_state_id", C.c_void_p),
        ("cp", C.c_void_p),
        ("cp_fej", C.c_void_p),
        ("pre_rows", C.c_void_p),
        ("pre_cols", C.c_void_p),
        ("pre_H", C.c_void_p),
        ("pre_ids", C.c_void_p),
    ]


class UpdateInfo(C.Structure):
    _fields_ = [
        ("n_accepted", C.c_int),
        ("n_rows", C.c_int),
        ("n_cols", C.c_int),
        ("neg_diag", C.c_int),
        ("not_spd", C.c_int),
        ("reserved", C.c_int * 3),
    ]


class CameraTables(C.Structure):
    _fields_ = [
        ("calib_q", C.c_double * 4),
        ("calib_p", C.c_double * 3),
        ("calib_id", C.c_int),
        ("intrinsics", C.c_double * 8),
        ("intr_id", C.c_int),
        ("fisheye", C.c_int),
    ]


class GeneralBatch(C.Structure):
    _fields_ = [
        ("n_feats", C.c_int),
        ("max_meas", C.c_int),
        ("uv", C.c_void_p),
        ("clone_idx", C.c_void_p),
        ("cam_idx", C.c_void_p),
        ("n_meas", C.c_void_p),
        ("p_FinG", C.c_void_p),
    ]


class DinitPlanes(C.Structure):
    """ovp_dinit_planes: the planes of the state the candidates of ovp_slam_delayed_init_planes refer to."""
    _fields_ = [
        ("n_planes", C.c_int),
        ("plane_state_id", C.c_void_p),
        ("cp", C.c_void_p),
        ("cp_fej", C.c_void_p),
        ("plane_of_cand", C.c_void_p),
        ("p_FinG_noplane", C.c_void_p),
    ]


OVP_MAX_CAMERAS = 4
OVP_GEN_MAX_MEAS = 64

_LIB = None

# every symbol include/ovplane_hip.h declares (checked by the CPU test-suite)
class PlaneFitBatch(C.Structure):
    _fields_ = [("n_planes", C.c_int), ("feat_start", C.POINTER(C.c_int)), ("p_FinG", C.POINTER(C.c_double)),
                ("min_inlier_num", C.c_int), ("max_cond", C.c_double), ("shuffle_variant", C.c_int)]


class PlaneOptBatch(C.Structure):
    _fields_ = [("n_planes", C.c_int), ("feat_start", C.POINTER(C.c_int)), ("p_FinG", C.POINTER(C.c_double)),
                ("obs_start", C.POINTER(C.c_int)), ("n_obs", C.POINTER(C.c_int)), ("n_obs_total", C.c_int),
                ("uv_norm", C.POINTER(C.c_double)), ("R_GtoC", C.POINTER(C.c_double)), ("p_CinG", C.POINTER(C.c_double)),
                ("cp", C.POINTER(C.c_double)), ("fix_plane", C.POINTER(C.c_ubyte)), ("sigma_px_norm", C.c_double),
                ("sigma_c", C.c_double), ("R_GtoI", C.c_double * 9), ("p_IinG", C.c_double * 3),
                ("R_ItoC", C.c_double * 9), ("p_IinC", C.c_double * 3)]


class PlaneFrontIn(C.Structure):
    _fields_ = [("n_planes", C.c_int), ("feat_start", C.c_void_p), ("cp", C.c_void_p), ("fix_plane", C.c_void_p),
                ("min_inlier_num", C.c_int), ("max_cond", C.c_double), ("shuffle_variant", C.c_int), ("refine", C.c_int),
                ("sigma_px_norm", C.c_double), ("sigma_c", C.c_double), ("R_GtoI", C.c_double * 9), ("p_IinG", C.c_double * 3)]


class PlaneFrontOut(C.Structure):
    _fields_ = [("fit_ok", C.c_void_p), ("abcd", C.c_void_p), ("ok", C.c_void_p), ("cp_out", C.c_void_p),
                ("iterations", C.c_void_p), ("inlier", C.c_void_p), ("kept", C.c_void_p), ("p_out", C.c_void_p),
                ("poses", C.c_void_p)]


class TrackPlaneOpts(C.Structure):
    """ovp_trackplane_opts: TrackPlaneOptions of the reference, same names (defaults: trackplane_defaults())."""
    _fields_ = [("max_tri_side_px", C.c_int), ("max_norm_count", C.c_int), ("max_norm_avg_max", C.c_double),
                ("max_norm_avg_var", C.c_double), ("max_norm_deg", C.c_double), ("max_dist_between_z", C.c_double),
                ("max_pairwise_px", C.c_int), ("min_norms", C.c_int), ("check_old_feats", C.c_int), ("filter_num_feat", C.c_int),
                ("filter_z_thresh", C.c_double), ("feat_init_min_obs", C.c_int), ("min_dist", C.c_double), ("max_dist", C.c_double),
                ("max_cond_number", C.c_double)]


OVP_DET_MAX_POINTS, OVP_DET_MAX_NORMS, OVP_DET_MAX_FILTER_K = 1024, 16, 16
OVP_AT_MAX_POINTS, OVP_AT_MAX_LANDMARKS, OVP_MAX_CAMERAS = 1024, 1024, 4


class ActiveTracksIn(C.Structure):
    """ovp_active_tracks_in"""
    _fields_ = [("n_obs", C.c_int), ("cam_idx", C.c_void_p), ("feat_id", C.c_void_p), ("uv", C.c_void_p), ("uv_norm", C.c_void_p),
                ("n_cams", C.c_int), ("R_GtoC", C.c_void_p), ("p_CinG", C.c_void_p),
                ("R_ItoC0", C.c_double * 9), ("p_IinC0", C.c_double * 3), ("R_GtoI", C.c_double * 9), ("p_IinG", C.c_double * 3),
                ("width", C.c_int), ("height", C.c_int),
                ("min_dist", C.c_double), ("max_dist", C.c_double), ("max_cond_number", C.c_double),
                ("n_slam", C.c_int), ("slam_id", C.c_void_p), ("slam_xyz", C.c_void_p), ("slam_relative", C.c_void_p),
                ("slam_anchor_R_GtoI", C.c_void_p), ("slam_anchor_p_IinG", C.c_void_p), ("slam_anchor_R_ItoC", C.c_void_p),
                ("slam_anchor_p_IinC", C.c_void_p)]


class ActiveTracksOut(C.Structure):
    """ovp_active_tracks_out"""
    _fields_ = [("cap", C.c_int), ("n_feats", C.c_int), ("n", C.c_int), ("ids", C.c_void_p), ("flags", C.c_void_p),
                ("p_FinG", C.c_void_p), ("uvd", C.c_void_p)]

class PlaneMergeIn(C.Structure):
    """ovp_plane_merge_in"""
    _fields_ = [("n_pairs", C.c_int), ("new_col", C.c_void_p), ("old_col", C.c_void_p), ("n_planes", C.c_int),
                ("plane_col", C.c_void_p), ("cp", C.c_void_p), ("sigma_plane_merge", C.c_double), ("plane_merge_chi2", C.c_double),
                ("plane_merge_deg_max", C.c_double), ("n_retire", C.c_int), ("retire_ids", C.c_void_p), ("retire_sizes", C.c_void_p)]


OVP_ZUPT_MAX_READINGS = 4096


class ZuptIn(C.Structure):
    """ovp_zupt_in"""
    _fields_ = [("n_readings", C.c_int), ("readings", C.c_void_p), ("imu_id", C.c_int), ("R_GtoI", C.c_double * 9),
                ("R_GtoI_jac", C.c_double * 9), ("b_g", C.c_double * 3), ("b_a", C.c_double * 3), ("gravity_mag", C.c_double),
                ("sigma_w", C.c_double), ("sigma_a", C.c_double), ("sigma_wb", C.c_double), ("sigma_ab", C.c_double),
                ("zupt_noise_multiplier", C.c_double), ("chi2_threshold", C.c_double), ("vel_ok", C.c_int),
                ("disparity_passed", C.c_int), ("time_kernels", C.c_int)]


class ZuptOut(C.Structure):
    """ovp_zupt_out"""
    _fields_ = [("accepted", C.c_int), ("rows", C.c_int), ("chi2", C.c_double), ("kernel_ms", C.c_float * 3)]


OVP_PROP_MAX_READINGS = 4096


class PropagateIn(C.Structure):
    """ovp_propagate_in"""
    _fields_ = [("n_readings", C.c_int), ("readings", C.c_void_p), ("imu_id", C.c_int), ("q", C.c_double * 4), ("p", C.c_double * 3),
                ("v", C.c_double * 3), ("bg", C.c_double * 3), ("ba", C.c_double * 3), ("q_fej", C.c_double * 4),
                ("p_fej", C.c_double * 3), ("v_fej", C.c_double * 3), ("gravity_mag", C.c_double), ("sigma_w", C.c_double),
                ("sigma_a", C.c_double), ("sigma_wb", C.c_double), ("sigma_ab", C.c_double), ("use_rk4", C.c_int),
                ("imu_avg", C.c_int), ("do_fej", C.c_int), ("clone", C.c_int), ("dt_id", C.c_int), ("time_kernels", C.c_int)]


class PropagateOut(C.Structure):
    """ovp_propagate_out"""
    _fields_ = [("q", C.c_double * 4), ("p", C.c_double * 3), ("v", C.c_double * 3), ("last_w", C.c_double * 3),
                ("n_intervals", C.c_int), ("clone_id", C.c_int), ("neg_diag", C.c_int), ("Phi", C.c_double * 225),
                ("Q", C.c_double * 225), ("kernel_ms", C.c_float * 4)]


EXPORTS = [
    "ovp_ctx_create", "ovp_ctx_destroy", "ovp_sync", "ovp_version", "ovp_error_string", "ovp_cov_upload",
    "ovp_cov_download", "ovp_cov_set_device", "ovp_cov_marginal", "ovp_state_upload", "ovp_batch_upload",
    "ovp_batch_bind_device", "ovp_batch_set_range", "ovp_msckf_update", "ovp_msckf_build_gate_gram_async", "ovp_gram_buffer",
    "ovp_ekf_update_from_gram_async", "ovp_msckf_fetch_results", "ovp_ekf_update", "ovp_cov_propagate",
    "ovp_cov_clone", "ovp_cov_marginalize", "ovp_cov_size", "ovp_chi2_quantile_095", "ovp_debug_read",
    "ovp_last_timings", "ovp_kernel_timer", "ovp_msckf_plane_update", "ovp_cov_augment_dt", "ovp_cov_initialize_invertible", "ovp_plane_init",
    "ovp_ctx_stream", "ovp_cov_initialize", "ovp_debug_chol2", "ovp_debug_chol2_floor", "ovp_plane_kernel_timer", "ovp_host_timing", "ovp_triang_defaults", "ovp_triangulate", "ovp_plane_fitting", "ovp_plane_optimize",
    "ovp_slam_update", "ovp_cov_clone_jitter", "ovp_rccl_unique_id", "ovp_rccl_comm_create", "ovp_rccl_comm_destroy",
    "ovp_rccl_allreduce_gram", "ovp_msckf_update_sharded", "ovp_slam_delayed_init", "ovp_shard_range", "ovp_shard_range_of_mask",
    "ovp_rccl_gather_decisions", "ovp_msckf_dense_blocks", "ovp_cameras_upload", "ovp_msckf_general_features",
    "ovp_triangulate_general", "ovp_slam_update_general", "ovp_slam_delayed_init_general",
    "ovp_slam_delayed_init_planes", "ovp_msckf_plane_update_general", "ovp_plane_fit_refine",
    "ovp_trackplane_defaults", "ovp_plane_detector_create", "ovp_plane_detector_destroy", "ovp_plane_detector_reset",
    "ovp_plane_detect_triangulate", "ovp_plane_detect_planes", "ovp_plane_detector_map", "ovp_delaunay", "ovp_plane_detector_debug", "ovp_plane_spatial_filter", "ovp_plane_detector_merges",
    "ovp_plane_init_general", "ovp_delaunay_device", "ovp_plane_detector_set_device_delaunay",
    "ovp_active_tracks_create", "ovp_active_tracks_destroy", "ovp_active_tracks_reset", "ovp_active_tracks_update",
    "ovp_active_tracks_debug",
    "ovp_cov_marginalize_many", "ovp_planes_merge_retire", "ovp_zupt_update",
    "ovp_propagate_and_clone",
    "ovp_klt_create", "ovp_klt_destroy", "ovp_klt_reset", "ovp_klt_feed_image", "ovp_klt_track", "ovp_klt_debug", "ovp_klt_detect",
    "ovp_epipolar_defaults", "ovp_klt_epipolar",
    "ovp_klt_intake_defaults", "ovp_klt_feed_image_opts", "ovp_klt_halve", "ovp_klt_match_frame",
    "ovp_featdb_create", "ovp_featdb_destroy", "ovp_featdb_reset", "ovp_featdb_append", "ovp_featdb_classify_defaults",
    "ovp_featdb_classify", "ovp_featdb_mark_deleted", "ovp_featdb_gather", "ovp_featdb_triangulate", "ovp_featdb_cleanup",
    "ovp_featdb_get", "ovp_featdb_debug",
]


class FeatDbClassifyIn(C.Structure):
    """ovp_featdb_classify_in"""
    _fields_ = [("clone_times", C.c_void_p), ("n_clones", C.c_int), ("max_clone_size", C.c_int), ("t_now", C.c_double),
                ("marg_time", C.c_double), ("want_marg", C.c_int), ("reserved", C.c_int)]


class FeatDbClassifyOut(C.Structure):
    """ovp_featdb_classify_out"""
    _fields_ = [("cap", C.c_int), ("n", C.c_int), ("ids", C.c_void_p), ("cls", C.c_void_p), ("count", C.c_void_p),
                ("cleaned", C.c_void_p), ("flags", C.c_void_p), ("totals", C.c_int32 * 4)]


class EpipolarOpts(C.Structure):
    """ovp_epipolar_opts"""
    _fields_ = [("mode", C.c_int32), ("max_iters", C.c_int32), ("intrinsics", C.c_double * 8), ("threshold", C.c_double),
                ("confidence", C.c_double), ("seed", C.c_uint32), ("reserved", C.c_uint32)]


class EpipolarInfo(C.Structure):
    """ovp_epipolar_info"""
    _fields_ = [("F", C.c_double * 9), ("best_count", C.c_int32), ("winner_h", C.c_int32), ("winner_model", C.c_int32),
                ("niters", C.c_int32), ("n_with_model", C.c_int32), ("too_few", C.c_int32), ("no_model", C.c_int32), ("stop", C.c_int32)]


class KltFrameIn(C.Structure):
    """ovp_klt_frame_in"""
    _fields_ = [("n", C.c_int), ("pts_prev", C.c_void_p), ("ids", C.c_void_p), ("timestamp", C.c_double), ("mask", C.c_void_p),
                ("mask_stride", C.c_int), ("epi", C.c_void_p), ("check", C.c_int), ("to_database", C.c_int)]


class KltFrameOut(C.Structure):
    """ovp_klt_frame_out"""
    _fields_ = [("n_kept", C.c_int), ("keep", C.c_void_p), ("pts_out", C.c_void_p), ("status", C.c_void_p), ("mask_epi", C.c_void_p),
                ("uvn", C.c_void_p), ("kept_index", C.c_void_p), ("info", EpipolarInfo)]


class Intake(C.Structure):
    """ovp_klt_intake"""
    _fields_ = [("hist_method", C.c_int), ("clahe_clip", C.c_double), ("clahe_tiles_x", C.c_int), ("clahe_tiles_y", C.c_int),
                ("downsample", C.c_int), ("src_width", C.c_int), ("src_height", C.c_int)]


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "libovplane_hip.so is not built (run `python -c 'import __graft_entry__ as g; g.build()'`); "
                "the HIP extension is mandatory, there is no CPU path")
        L = C.CDLL(LIB_PATH)
        L.ovp_version.restype = C.c_char_p
        L.ovp_error_string.restype = C.c_char_p
        L.ovp_error_string.argtypes = [C.c_int]
        L.ovp_chi2_quantile_095.restype = C.c_double
        L.ovp_chi2_quantile_095.argtypes = [C.c_int]
        L.ovp_debug_read.restype = C.c_long
        L.ovp_debug_read.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_long]
        L.ovp_ctx_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
        L.ovp_ctx_destroy.argtypes = [C.c_void_p]
        L.ovp_sync.argtypes = [C.c_void_p]
        L.ovp_cov_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.ovp_cov_download.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.ovp_cov_set_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.ovp_cov_marginal.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.ovp_state_upload.argtypes = [C.c_void_p, C.POINTER(StateTables)]
        L.ovp_batch_upload.argtypes = [C.c_void_p, C.POINTER(FeatureBatch)]
        L.ovp_batch_bind_device.argtypes = [C.c_void_p, C.POINTER(FeatureBatch)]
        L.ovp_msckf_update.argtypes = [C.c_void_p, C.POINTER(UpdateOpts), C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.POINTER(UpdateInfo)]
        L.ovp_msckf_build_gate_gram_async.argtypes = [C.c_void_p, C.POINTER(UpdateOpts)]
        L.ovp_gram_buffer.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.ovp_ekf_update_from_gram_async.argtypes = [C.c_void_p]
        L.ovp_msckf_fetch_results.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(UpdateInfo)]
        L.ovp_ekf_update.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.POINTER(UpdateInfo)]
        L.ovp_cov_clone_jitter.argtypes = [C.c_void_p, C.c_double]
        L.ovp_slam_delayed_init.argtypes = [C.c_void_p, C.POINTER(UpdateOpts), C.POINTER(FeatureBatch), C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_int]
        L.ovp_rccl_unique_id.argtypes = [C.c_void_p]
        L.ovp_rccl_comm_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.ovp_rccl_comm_destroy.argtypes = [C.c_void_p]
        L.ovp_rccl_allreduce_gram.argtypes = [C.c_void_p, C.c_void_p]
        L.ovp_shard_range.argtypes = [C.c_void_p, C.POINTER(UpdateOpts), C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.ovp_msckf_dense_blocks.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p]
        L.ovp_cameras_upload.argtypes = [C.c_void_p, C.c_int, C.POINTER(CameraTables)]
        L.ovp_msckf_general_features.argtypes = [C.c_void_p, C.POINTER(UpdateOpts), C.POINTER(GeneralBatch), C.c_void_p, C.c_void_p]
        L.ovp_triangulate_general.argtypes = [C.c_void_p, C.POINTER(TriangOpts), C.POINTER(GeneralBatch), C.c_void_p, C.c_void_p,
                                              C.c_void_p]
        L.ovp_shard_range_of_mask.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.ovp_rccl_gather_decisions.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ovp_msckf_update_sharded.argtypes = [C.c_void_p, C.POINTER(UpdateOpts), C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.POINTER(UpdateInfo), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.ovp_slam_update.argtypes = [C.c_void_p, C.POINTER(UpdateOpts), C.POINTER(SlamBatch), C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.POINTER(UpdateInfo)]
        L.ovp_slam_update_general.argtypes = [C.c_void_p, C.POINTER(UpdateOpts), C.POINTER(SlamBatch), C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.POINTER(UpdateInfo)]
        L.ovp_slam_delayed_init_general.argtypes = [C.c_void_p, C.POINTER(UpdateOpts), C.POINTER(GeneralBatch), C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.ovp_slam_delayed_init_planes.argtypes = [C.c_void_p, C.POINTER(UpdateOpts), C.POINTER(GeneralBatch), C.POINTER(DinitPlanes),
                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.ovp_msckf_plane_update.argtypes = [C.c_void_p, C.POINTER(UpdateOpts), C.POINTER(PlaneBatch), C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ovp_msckf_plane_update_general.argtypes = [C.c_void_p, C.POINTER(UpdateOpts), C.POINTER(PlaneBatch), C.POINTER(GeneralBatch),
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ovp_plane_init.argtypes = [C.c_void_p, C.POINTER(UpdateOpts), C.POINTER(PlaneBatch), C.c_double, C.c_double,
                                     C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p]
        L.ovp_plane_init_general.argtypes = [C.c_void_p, C.POINTER(UpdateOpts), C.POINTER(PlaneBatch), C.c_double, C.c_double,
                                             C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.POINTER(GeneralBatch), C.c_void_p, C.c_void_p]
        L.ovp_cov_propagate.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                        C.c_void_p, C.POINTER(C.c_int)]
        L.ovp_cov_clone.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.ovp_cov_marginalize.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.ovp_cov_marginalize_many.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.ovp_planes_merge_retire.argtypes = [C.c_void_p, C.POINTER(PlaneMergeIn), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_int]
        L.ovp_zupt_update.argtypes = [C.c_void_p, C.POINTER(ZuptIn), C.c_void_p, C.POINTER(ZuptOut), C.POINTER(UpdateInfo)]
        L.ovp_propagate_and_clone.argtypes = [C.c_void_p, C.POINTER(PropagateIn), C.POINTER(PropagateOut)]
        L.ovp_cov_size.argtypes = [C.c_void_p]
        L.ovp_cov_augment_dt.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.ovp_cov_initialize_invertible.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                    C.c_void_p]
        L.ovp_cov_initialize.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_int, C.POINTER(C.c_int),
                                         C.POINTER(C.c_double), C.c_void_p]
        L.ovp_last_timings.argtypes = [C.c_void_p, C.c_void_p]
        L.ovp_kernel_timer.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int)]
        L.ovp_ctx_stream.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.ovp_plane_kernel_timer.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int)]
        L.ovp_host_timing.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.ovp_triang_defaults.argtypes = [C.POINTER(TriangOpts)]
        L.ovp_triang_defaults.restype = None
        L.ovp_triangulate.argtypes = [C.c_void_p, C.POINTER(TriangOpts), C.c_void_p, C.c_void_p, C.c_void_p]
        L.ovp_plane_fitting.argtypes = [C.c_void_p, C.POINTER(PlaneFitBatch), C.c_void_p, C.c_void_p, C.c_void_p]
        L.ovp_plane_optimize.argtypes = [C.c_void_p, C.POINTER(PlaneOptBatch), C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p]
        L.ovp_plane_fit_refine.argtypes = [C.c_void_p, C.POINTER(GeneralBatch), C.c_void_p, C.POINTER(PlaneFrontIn),
                                           C.POINTER(PlaneFrontOut)]
        L.ovp_trackplane_defaults.argtypes = [C.POINTER(TrackPlaneOpts)]
        L.ovp_trackplane_defaults.restype = None
        L.ovp_plane_detector_create.argtypes = [C.c_void_p, C.POINTER(TrackPlaneOpts)]
        L.ovp_plane_detector_destroy.argtypes = [C.c_void_p]
        L.ovp_plane_detector_reset.argtypes = [C.c_void_p]
        L.ovp_plane_detect_triangulate.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 7
        L.ovp_plane_detect_planes.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.ovp_plane_detector_map.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.ovp_delaunay.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.ovp_plane_spatial_filter.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p]
        L.ovp_plane_detector_merges.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.ovp_delaunay_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.ovp_plane_detector_set_device_delaunay.argtypes = [C.c_void_p, C.c_int]
        L.ovp_plane_detector_debug.restype = C.c_long
        L.ovp_plane_detector_debug.argtypes = [C.c_void_p, C.c_char_p, C.c_int64, C.c_void_p, C.c_long]
        L.ovp_active_tracks_create.argtypes = [C.c_void_p]
        L.ovp_active_tracks_destroy.argtypes = [C.c_void_p]
        L.ovp_active_tracks_reset.argtypes = [C.c_void_p]
        L.ovp_active_tracks_update.argtypes = [C.c_void_p, C.POINTER(ActiveTracksIn), C.POINTER(ActiveTracksOut)]
        L.ovp_active_tracks_debug.restype = C.c_long
        L.ovp_active_tracks_debug.argtypes = [C.c_void_p, C.c_char_p, C.c_int64, C.c_void_p, C.c_long]
        L.ovp_klt_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        L.ovp_klt_destroy.argtypes = [C.c_void_p]
        L.ovp_klt_reset.argtypes = [C.c_void_p]
        L.ovp_klt_feed_image.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.ovp_klt_track.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ovp_klt_detect.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_int]
        L.ovp_epipolar_defaults.restype = None
        L.ovp_epipolar_defaults.argtypes = [C.c_void_p]
        L.ovp_klt_epipolar.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p]
        L.ovp_klt_intake_defaults.restype = None
        L.ovp_klt_intake_defaults.argtypes = [C.c_void_p]
        L.ovp_klt_feed_image_opts.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.ovp_klt_halve.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.ovp_klt_match_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.ovp_klt_debug.restype = C.c_long
        L.ovp_klt_debug.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_long]
        L.ovp_featdb_create.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.ovp_featdb_destroy.argtypes = [C.c_void_p]
        L.ovp_featdb_reset.argtypes = [C.c_void_p]
        L.ovp_featdb_append.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ovp_featdb_classify_defaults.restype = None
        L.ovp_featdb_classify_defaults.argtypes = [C.c_void_p]
        L.ovp_featdb_classify.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.ovp_featdb_mark_deleted.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.ovp_featdb_gather.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.ovp_featdb_triangulate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ovp_featdb_cleanup.argtypes = [C.c_void_p, C.c_int, C.c_double]
        L.ovp_featdb_get.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.ovp_featdb_debug.restype = C.c_long
        L.ovp_featdb_debug.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_long]
        _LIB = L
    return _LIB


def _chk(code, where):
    if code != 0:
        raise OvpError(code, where)


def trackplane_defaults(**over) -> TrackPlaneOpts:
    """TrackPlaneOptions' defaults (ovp_trackplane_defaults), with the named fields replaced."""
    o = TrackPlaneOpts()
    lib().ovp_trackplane_defaults(C.byref(o))
    for k, v in over.items():
        if k not in dict(TrackPlaneOpts._fields_):
            raise KeyError(k)
        setattr(o, k, v)
    return o


def intake_defaults(**over) -> Intake:
    """the intake options' defaults (ovp_klt_intake_defaults: HISTOGRAM, clip 10, 8 x 8 tiles, no downsampling), with the named
    fields replaced; hist_method also by name ("NONE", "HISTOGRAM", "CLAHE").  src_width / src_height left at 0 are filled in
    from the image by KltTracker.feed_image_opts."""
    o = Intake()
    lib().ovp_klt_intake_defaults(C.byref(o))
    for k, v in over.items():
        if k not in dict(Intake._fields_):
            raise KeyError(k)
        setattr(o, k, KltTracker.HIST[v] if k == "hist_method" and isinstance(v, str) else v)
    return o


def delaunay(xy):
    """ovp_delaunay: Delaunay triangles of the pixel positions xy [n, 2] (f32), canonical order; host arithmetic, no GPU."""
    xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
    cap = max(2 * len(xy), 1)
    tris = np.zeros((cap, 3), dtype=np.int32)
    nt = C.c_int(0)
    _chk(lib().ovp_delaunay(len(xy), xy.ctypes.data, tris.ctypes.data, cap, C.byref(nt)), "ovp_delaunay")
    return tris[:nt.value].copy()


def delaunay_device(ctx, xy):
    """ovp_delaunay_device: the triangles of delaunay(xy), computed by the device kernel of the context (no fallback to the host)."""
    xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
    cap = max(2 * len(xy), 1)
    tris = np.zeros((cap, 3), dtype=np.int32)
    nt = C.c_int(0)
    _chk(lib().ovp_delaunay_device(ctx.handle, len(xy), xy.ctypes.data, tris.ctypes.data, cap, C.byref(nt)), "ovp_delaunay_device")
    return tris[:nt.value].copy()


class PlaneDetector:
    """The plane detector of a context (ovp_plane_detector_*): TrackPlane::perform_plane_detection_monocular on the device.
    feed() is one frame; feature2plane() the reference's get_feature2plane()."""

    def __init__(self, ctx, opts=None):
        self.ctx = ctx
        self.opts = opts if opts is not None else trackplane_defaults()
        _chk(lib().ovp_plane_detector_create(ctx.handle, C.byref(self.opts)), "ovp_plane_detector_create")

    def close(self):
        _chk(lib().ovp_plane_detector_destroy(self.ctx.handle), "ovp_plane_detector_destroy")

    def reset(self):
        _chk(lib().ovp_plane_detector_reset(self.ctx.handle), "ovp_plane_detector_reset")

    def set_device_delaunay(self, on=True):
        """the frame's triangles come from the device triangulation behind the first call (default off: the host's)"""
        _chk(lib().ovp_plane_detector_set_device_delaunay(self.ctx.handle, 1 if on else 0), "ovp_plane_detector_set_device_delaunay")

    def triangulate(self, ids, uv, uv_norm, R_GtoC, p_CinG):
        """first call of a frame -> (has_est [n] bool, p_FinG [n, 3])"""
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        n = len(ids)
        uv = np.ascontiguousarray(uv, dtype=np.float32).reshape(n, 2)
        uvn = np.ascontiguousarray(uv_norm, dtype=np.float64).reshape(n, 2)
        R = np.ascontiguousarray(R_GtoC, dtype=np.float64).reshape(3, 3)
        p = np.ascontiguousarray(p_CinG, dtype=np.float64).reshape(3)
        has = np.zeros(n, dtype=np.uint8)
        pf = np.zeros((n, 3))
        _chk(lib().ovp_plane_detect_triangulate(self.ctx.handle, n, ids.ctypes.data, uv.ctypes.data, uvn.ctypes.data, R.ctypes.data,
                                                p.ctypes.data, has.ctypes.data, pf.ctypes.data), "ovp_plane_detect_triangulate")
        self.accepted = (has & 2) != 0  # this frame's solution passed the gates
        return (has & 1) != 0, pf

    def planes(self, tris=None):
        """second call of a frame; tris [nt, 3] over the frame's vertices (None: the library's own Delaunay triangulation)"""
        if tris is None:
            _chk(lib().ovp_plane_detect_planes(self.ctx.handle, 0, None), "ovp_plane_detect_planes")
        else:
            tris = np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
            _chk(lib().ovp_plane_detect_planes(self.ctx.handle, len(tris), tris.ctypes.data), "ovp_plane_detect_planes")

    def feed(self, ids, uv, uv_norm, R_GtoC, p_CinG):
        if len(ids) == 0:
            return self.feature2plane()
        self.triangulate(ids, uv, uv_norm, R_GtoC, p_CinG)
        self.planes()
        return self.feature2plane()

    def feature2plane(self):
        n = C.c_int(0)
        _chk(lib().ovp_plane_detector_map(self.ctx.handle, None, None, 0, C.byref(n)), "ovp_plane_detector_map")
        ids, pl = np.zeros(max(n.value, 1), dtype=np.int64), np.zeros(max(n.value, 1), dtype=np.int64)
        _chk(lib().ovp_plane_detector_map(self.ctx.handle, ids.ctypes.data, pl.ctypes.data, n.value, C.byref(n)), "ovp_plane_detector_map")
        return {int(a): int(b) for a, b in zip(ids[:n.value], pl[:n.value])}

    def plane2oldplane(self):
        """TrackPlane::get_plane2oldplane: {surviving plane id: set of the ids merged into it}"""
        n = C.c_int(0)
        _chk(lib().ovp_plane_detector_merges(self.ctx.handle, None, 0, C.byref(n)), "ovp_plane_detector_merges")
        pairs = np.zeros((max(n.value, 1), 2), dtype=np.int64)
        _chk(lib().ovp_plane_detector_merges(self.ctx.handle, pairs.ctypes.data, n.value, C.byref(n)), "ovp_plane_detector_merges")
        out = {}
        for a, b in pairs[:n.value]:
            out.setdefault(int(a), set()).add(int(b))
        return out

    def _debug(self, what, fid, cap):
        out = np.zeros(cap)
        k = lib().ovp_plane_detector_debug(self.ctx.handle, what, int(fid), out.ctypes.data, cap)
        if k < 0:
            raise OvpError(int(k), "ovp_plane_detector_debug")
        return out[:k]

    def feature(self, fid):
        """tests: the history of one feature -> dict(count, valid, p_FinG, avg_norm, normals [k, 3] oldest first)"""
        o = self._debug(b"feat", fid, 9 + 3 * OVP_DET_MAX_NORMS)
        return dict(count=int(o[0]), valid=bool(o[1]), p_FinG=o[2:5].copy(), avg_norm=o[6:9].copy(), normals=o[9:].reshape(-1, 3).copy())

    def filter_rows(self):
        """tests: [feature id, plane id, mean neighbour distance, flagged] per point the last frame's spatial filter looked at"""
        return self._debug(b"filter", 0, 4 * OVP_DET_MAX_POINTS).reshape(-1, 4)

    def timer(self, on=True):
        """events around the kernels from the next frame on (diagnostics: adds a stream synchronisation per publication)"""
        self._debug(b"timer", 1 if on else 0, 1)

    def kernel_ms(self):
        """GPU milliseconds of the last timed frame's kernels [triangulate, normals, match, filter]"""
        return self._debug(b"time", 0, 4)

    def delaunay_ms(self):
        """GPU milliseconds of the Delaunay kernel [in the last timed frame, in the last timed delaunay_device of the context]"""
        return self._debug(b"time_delaunay", 0, 2)

    def tris_info(self):
        """the last planes() call's triangles: dict(source = "caller" / "host" / "device", device_on, and of the frame's device
        triangulation overflow, vertices, peak_slots, max_cavity)"""
        o = self._debug(b"tris", 0, 6)
        return dict(source=("caller", "host", "device")[int(o[0])], device_on=bool(o[1]), overflow=int(o[2]), vertices=int(o[3]),
                    peak_slots=int(o[4]), max_cavity=int(o[5]))

    def spatial_filter(self, planes, filter_num_feat=None, filter_z_thresh=None):
        """ovp_plane_spatial_filter on a list of [n_k, 3] point arrays -> list of (mean_dist [n_k], flagged [n_k] bool)"""
        start = np.concatenate([[0], np.cumsum([len(p) for p in planes])]).astype(np.int32)
        P = np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.float64).reshape(-1, 3) for p in planes]))
        dist, flag = np.zeros(len(P)), np.zeros(len(P), dtype=np.uint8)
        k = self.opts.filter_num_feat if filter_num_feat is None else filter_num_feat
        z = self.opts.filter_z_thresh if filter_z_thresh is None else filter_z_thresh
        _chk(lib().ovp_plane_spatial_filter(self.ctx.handle, len(planes), start.ctypes.data, P.ctypes.data, int(k), float(z),
                                            dist.ctypes.data, flag.ctypes.data), "ovp_plane_spatial_filter")
        return [(dist[a:b].copy(), flag[a:b].astype(bool)) for a, b in zip(start[:-1], start[1:])]


class ActiveTracks:
    """The active tracks of a context (ovp_active_tracks_*): VioManager::retriangulate_active_tracks on the device.  update() is
    one frame; the per-feature history stays on the device between frames."""

    def __init__(self, ctx):
        self.ctx = ctx
        _chk(lib().ovp_active_tracks_create(ctx.handle), "ovp_active_tracks_create")

    def close(self):
        _chk(lib().ovp_active_tracks_destroy(self.ctx.handle), "ovp_active_tracks_destroy")

    def reset(self):
        _chk(lib().ovp_active_tracks_reset(self.ctx.handle), "ovp_active_tracks_reset")

    def update(self, cam_idx, ids, uv, uv_norm, R_GtoC, p_CinG, R_ItoC0, p_IinC0, R_GtoI, p_IinG, width, height, min_dist=0.1,
               max_dist=60.0, max_cond_number=10000.0, slam_ids=(), slam_xyz=(), slam_relative=None, slam_anchor=None):
        """One frame.  Observations in the caller's order: cam_idx [n], ids [n], uv [n, 2] raw pixels, uv_norm [n, 2]; R_GtoC
        [n_cams, 3, 3] / p_CinG [n_cams, 3] by camera id; camera 0's extrinsics, the newest clone, the image size, the gates
        (featinit_options); the landmarks: slam_ids, slam_xyz [m, 3], slam_relative [m] and, for the relative ones, slam_anchor =
        (R_GtoI [m, 3, 3], p_IinG [m, 3], R_ItoC [m, 3, 3], p_IinC [m, 3]).
        Returns dict(posinG {id: (3,)}, uvd {id: (3,)}, and the raw arrays ids, flags, p_FinG, uvd_all, n_feats)."""
        f64 = lambda a, *sh: np.ascontiguousarray(a, dtype=np.float64).reshape(*sh)  # noqa: E731
        cam = np.ascontiguousarray(cam_idx, dtype=np.int32).reshape(-1)
        n = len(cam)
        fid = np.ascontiguousarray(ids, dtype=np.int64).reshape(n)
        uv = np.ascontiguousarray(uv, dtype=np.float32).reshape(n, 2)
        uvn = f64(uv_norm, n, 2)
        R, p = f64(R_GtoC, -1, 3, 3), f64(p_CinG, -1, 3)
        sid = np.ascontiguousarray(slam_ids, dtype=np.int64).reshape(-1)
        m = len(sid)
        sx = f64(slam_xyz, m, 3)
        rel = np.ascontiguousarray(slam_relative if slam_relative is not None else np.zeros(m), dtype=np.uint8).reshape(m)
        a = ActiveTracksIn()
        a.n_obs, a.cam_idx, a.feat_id, a.uv, a.uv_norm = n, cam.ctypes.data, fid.ctypes.data, uv.ctypes.data, uvn.ctypes.data
        a.n_cams, a.R_GtoC, a.p_CinG = len(R), R.ctypes.data, p.ctypes.data
        a.R_ItoC0[:], a.p_IinC0[:] = list(f64(R_ItoC0, 9)), list(f64(p_IinC0, 3))
        a.R_GtoI[:], a.p_IinG[:] = list(f64(R_GtoI, 9)), list(f64(p_IinG, 3))
        a.width, a.height = int(width), int(height)
        a.min_dist, a.max_dist, a.max_cond_number = float(min_dist), float(max_dist), float(max_cond_number)
        a.n_slam, a.slam_id, a.slam_xyz, a.slam_relative = m, sid.ctypes.data, sx.ctypes.data, rel.ctypes.data
        keep = None
        if slam_anchor is not None:
            keep = (f64(slam_anchor[0], m, 3, 3), f64(slam_anchor[1], m, 3), f64(slam_anchor[2], m, 3, 3), f64(slam_anchor[3], m, 3))
            a.slam_anchor_R_GtoI, a.slam_anchor_p_IinG, a.slam_anchor_R_ItoC, a.slam_anchor_p_IinC = (k.ctypes.data for k in keep)
        cap = max(len(set(fid.tolist())) + m, 1)
        o = ActiveTracksOut()
        out_ids, flags = np.zeros(cap, dtype=np.int64), np.zeros(cap, dtype=np.uint8)
        pf, uvd = np.zeros((cap, 3)), np.zeros((cap, 3))
        o.cap, o.ids, o.flags, o.p_FinG, o.uvd = cap, out_ids.ctypes.data, flags.ctypes.data, pf.ctypes.data, uvd.ctypes.data
        t0 = time.perf_counter()
        rc = lib().ovp_active_tracks_update(self.ctx.handle, C.byref(a), C.byref(o))
        self.last_call_ms = 1e3 * (time.perf_counter() - t0)  # the entry alone, without this method's array and dict work
        _chk(rc, "ovp_active_tracks_update")
        k = o.n
        out_ids, flags, pf, uvd = out_ids[:k], flags[:k], pf[:k], uvd[:k]
        return dict(posinG={int(i): pf[j].copy() for j, i in enumerate(out_ids) if flags[j] & 1},
                    uvd={int(i): uvd[j].copy() for j, i in enumerate(out_ids) if flags[j] & 2},
                    ids=out_ids, flags=flags, p_FinG=pf, uvd_all=uvd, n_feats=int(o.n_feats))

    def _debug(self, what, fid, cap):
        out = np.zeros(cap)
        k = lib().ovp_active_tracks_debug(self.ctx.handle, what, int(fid), out.ctypes.data, cap)
        if k < 0:
            raise OvpError(int(k), "ovp_active_tracks_debug")
        return out[:k]

    def debug(self, fid):
        """tests: the slot of one feature -> dict(count, A [3, 3], b [3]), or None when the table does not hold the id"""
        o = self._debug(b"feat", fid, 10)
        if len(o) == 0:
            return None
        a = o[1:7]
        return dict(count=int(o[0]), A=np.array([[a[0], a[1], a[2]], [a[1], a[3], a[4]], [a[2], a[4], a[5]]]), b=o[7:10].copy())

    def size(self):
        """features in the table"""
        return int(self._debug(b"size", 0, 1)[0])

    def timer(self, on=True):
        """events around the kernel from the next frame on (diagnostics: adds a stream synchronisation per frame)"""
        self._debug(b"timer", 1 if on else 0, 1)

    def kernel_ms(self):
        """GPU milliseconds of the last timed frame's kernel"""
        return float(self._debug(b"time", 0, 1)[0])


FEATDB_NONE, FEATDB_LOST, FEATDB_MARG, FEATDB_MAXTRACK = 0, 1, 2, 3


def featdb_select(ids, cls, landmark_ids, max_slam_features, slam_delay_ok):
    """core/VioManager.cpp:373-506 on a published class table (ids ascending): feats_lost, feats_marg, the maxtracks left over, the
    new SLAM features (the LAST valid_amount of the maxtracks, :447-460, on the ascending-id order) and the SLAM features to update;
    landmarks_marg: the state's landmarks the database no longer holds (:466-480 should_marg).  One camera, no ArUco."""
    pick = lambda c: [int(i) for i, k in zip(ids, cls) if k == c]  # noqa: E731
    lost, marg, maxtracks = pick(FEATDB_LOST), pick(FEATDB_MARG), pick(FEATDB_MAXTRACK)
    landmark_ids = [int(i) for i in landmark_ids]
    slam = []
    if max_slam_features > 0 and slam_delay_ok and len(landmark_ids) < max_slam_features:
        valid = min(max_slam_features - len(landmark_ids), len(maxtracks))
        if valid > 0:
            slam, maxtracks = maxtracks[len(maxtracks) - valid:], maxtracks[:len(maxtracks) - valid]
    live = set(int(i) for i in ids)
    gone = [lm for lm in landmark_ids if lm not in live]
    slam += [lm for lm in landmark_ids if lm in live]
    left = set(landmark_ids) - set(gone)
    return dict(lost=lost, marg=marg, maxtracks=maxtracks, slam_delayed=[i for i in slam if i not in left],
                slam_update=[i for i in slam if i in left], landmarks_marg=gone)


class FeatureDatabase:
    """The feature database of a context (ovp_featdb_*): ext ov_core::FeatureDatabase on the device, under the reference's method
    names.  update_feature takes one frame's observations at once; every list is in ascending feature id."""

    def __init__(self, ctx, max_slots=4096, max_meas=32):
        self.ctx, self.S, self.M = ctx, int(max_slots), int(max_meas)
        _chk(lib().ovp_featdb_create(ctx.handle, self.S, self.M), "ovp_featdb_create")
        self.table = None

    def close(self):
        _chk(lib().ovp_featdb_destroy(self.ctx.handle), "ovp_featdb_destroy")

    def reset(self):
        _chk(lib().ovp_featdb_reset(self.ctx.handle), "ovp_featdb_reset")

    def update_feature(self, timestamp, ids, uv, uv_norm):
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        uv = np.ascontiguousarray(uv, dtype=np.float32)
        uvn = np.ascontiguousarray(uv_norm, dtype=np.float32)
        if uv.size != 2 * len(ids) or uvn.size != 2 * len(ids):
            raise ValueError("uv and uv_norm hold one pair per id")
        _chk(lib().ovp_featdb_append(self.ctx.handle, float(timestamp), len(ids), ids.ctypes.data, uv.ctypes.data, uvn.ctypes.data),
             "ovp_featdb_append")

    def classify(self, clone_times, t_now, marg_time, max_clone_size, want_marg):
        ct = np.ascontiguousarray(clone_times, dtype=np.float64)
        a = FeatDbClassifyIn()
        lib().ovp_featdb_classify_defaults(C.byref(a))
        a.clone_times, a.n_clones, a.max_clone_size = ct.ctypes.data, len(ct), int(max_clone_size)
        a.t_now, a.marg_time, a.want_marg = float(t_now), float(marg_time), 1 if want_marg else 0
        cap = self.S
        ids, cls, cnt, cln = (np.zeros(cap, dtype=t) for t in (np.int64, np.int32, np.int32, np.int32))
        fl = np.zeros(cap, dtype=np.uint8)
        o = FeatDbClassifyOut(cap, 0, ids.ctypes.data, cls.ctypes.data, cnt.ctypes.data, cln.ctypes.data, fl.ctypes.data)
        _chk(lib().ovp_featdb_classify(self.ctx.handle, C.byref(a), C.byref(o)), "ovp_featdb_classify")
        n = o.n
        self.table = dict(ids=ids[:n].copy(), cls=cls[:n].copy(), count=cnt[:n].copy(), cleaned=cln[:n].copy(), flags=fl[:n].copy(),
                          totals=np.array(list(o.totals), dtype=np.int32))
        return self.table

    def features_not_containing_newer(self, timestamp):
        """(timestamp, remove = false, skip_deleted = true)"""
        r = self.classify([], timestamp, np.inf, 1 << 30, False)
        return [int(i) for i in r["ids"][r["cls"] == FEATDB_LOST]]

    def features_containing(self, timestamp):
        """(timestamp, remove = false, skip_deleted = true)"""
        r = self.classify([], -np.inf, timestamp, 1 << 30, True)
        return [int(i) for i in r["ids"][r["cls"] == FEATDB_MARG]]

    def select(self, state_times, t_now, max_clone_size, landmark_ids=(), max_slam_features=0, slam_delay_ok=True):
        """core/VioManager.cpp:373-506: state_times are the clone times after cloning, ascending; the marginalisation time is the
        oldest (state/State.h:70).  Returns featdb_select's lists, with the published table under "table"."""
        st = np.asarray(state_times, dtype=np.float64)
        want = len(st) > max_clone_size or len(st) > 5   # :379
        t = self.classify(st, t_now, st[0] if len(st) else np.inf, max_clone_size, want)
        return dict(featdb_select(t["ids"], t["cls"], landmark_ids, max_slam_features, slam_delay_ok), table=t)

    def mark_deleted(self, ids):
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        _chk(lib().ovp_featdb_mark_deleted(self.ctx.handle, len(ids), ids.ctypes.data), "ovp_featdb_mark_deleted")

    def gather(self, ids, clone_times, old_index=None):
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        ct = np.ascontiguousarray(clone_times, dtype=np.float64)
        oi = None if old_index is None else np.ascontiguousarray(old_index, dtype=np.int32)
        _chk(lib().ovp_featdb_gather(self.ctx.handle, len(ids), ids.ctypes.data, None if oi is None else oi.ctypes.data, ct.ctypes.data,
                                     len(ct)), "ovp_featdb_gather")
        self.ctx.n_feats = len(ids)

    def _debug(self, what, dtype, count):
        out = np.zeros(max(count, 1), dtype=dtype)
        k = lib().ovp_featdb_debug(self.ctx.handle, what, 0, out.ctypes.data, out.nbytes)
        if k < 0:
            raise OvpError(int(k), "ovp_featdb_debug")
        return out[: k // out.itemsize]

    def dims(self):
        return [int(v) for v in self._debug(b"dims", np.int32, 4)]

    def gathered(self):
        """the bound batch, read back: uv, uv_norm [F, M, 2], clone_idx [F, M], n_meas [F], p_FinG [F, 3]"""
        F, M = self.dims()[3], self.M
        if F < 0:
            return None
        return dict(uv=self._debug(b"uv", np.float32, 2 * F * M).reshape(F, M, 2), uv_norm=self._debug(b"uv_norm", np.float32, 2 * F * M).reshape(F, M, 2),
                    clone_idx=self._debug(b"clone_idx", np.int32, F * M).reshape(F, M), n_meas=self._debug(b"n_meas", np.int32, F),
                    p_FinG=self._debug(b"p_FinG", np.float64, 3 * F).reshape(F, 3))

    def triangulate(self, opts=None):
        """ovp_featdb_triangulate on the gathered batch; returns dict(p_FinG [F,3], ok [F])."""
        o = opts if opts is not None else triang_defaults()
        F = max(self.dims()[3], 0)   # the gathered batch's size, whatever the context's batch has become since
        p = np.zeros((max(F, 1), 3))
        ok = np.zeros(max(F, 1), dtype=np.uint8)
        _chk(lib().ovp_featdb_triangulate(self.ctx.handle, C.byref(o), p.ctypes.data, ok.ctypes.data), "ovp_featdb_triangulate")
        return dict(p_FinG=p[:F], ok=ok[:F].astype(bool))

    def cleanup(self, do_cleanup=True, before=float("nan")):
        """cleanup() and, with `before`, cleanup_measurements(before) behind it; returns int64 [n, 3]: id, new count, freed"""
        _chk(lib().ovp_featdb_cleanup(self.ctx.handle, 1 if do_cleanup else 0, float(before)), "ovp_featdb_cleanup")
        return self._debug(b"cleanup", np.int64, 3 * self.S).reshape(-1, 3)

    def cleanup_measurements(self, timestamp):
        return self.cleanup(False, timestamp)

    def get_feature(self, fid):
        M = self.M
        slot, cnt, dele = C.c_int(-1), C.c_int(-1), C.c_int(0)
        ts, uv, uvn = np.zeros(M), np.zeros((M, 2), dtype=np.float32), np.zeros((M, 2), dtype=np.float32)
        _chk(lib().ovp_featdb_get(self.ctx.handle, int(fid), C.byref(slot), C.byref(cnt), C.byref(dele), ts.ctypes.data, uv.ctypes.data,
                                  uvn.ctypes.data, M), "ovp_featdb_get")
        if cnt.value < 0:
            return None
        n = cnt.value
        return dict(count=n, to_delete=dele.value, ts=ts[:n], uv=uv[:n], uv_norm=uvn[:n], slot=slot.value)


class KltTracker:
    """The image front end of a context (ovp_klt_*): TrackPlane::feed_new_camera's equalisation and pyramid, the
    cv::calcOpticalFlowPyrLK call of perform_matching and the keep rule of feed_monocular, on the device.  The algorithm is restated
    from its published form and unpinned (include/ovplane_hip.h).  add_points seeds or tops up with a caller's points; detect()
    is perform_detection_monocular (:1173-1297) on the device's candidates (ovp_klt_detect: recalled and unpinned as well), and
    step(detect=True) feed_monocular's use of it.  detector: dict(num_features, grid_x, grid_y, threshold, min_px_dist)."""

    HIST = {"NONE": 0, "HISTOGRAM": 1, "CLAHE": 2}
    DETECTOR_KEYS = ("num_features", "grid_x", "grid_y", "threshold", "min_px_dist")

    def __init__(self, ctx, width, height, n_levels=6, win=15, max_points=4096, detector=None):
        self.ctx, self.width, self.height, self.n_levels, self.win = ctx, int(width), int(height), int(n_levels), int(win)
        self.max_points = int(max_points)
        self.detector = None if detector is None else {k: int(detector[k]) for k in self.DETECTOR_KEYS}
        self.currid = 0          # :1292 ++currid: the first id is 1
        self._mask_last = None   # img_mask_last: the mask of the previous image, for the top-up
        _chk(lib().ovp_klt_create(ctx.handle, self.width, self.height, self.n_levels, self.win, int(max_points)), "ovp_klt_create")
        self.ids_last = np.zeros(0, dtype=np.int64)
        self.pts_last = np.zeros((0, 2), dtype=np.float32)
        self._fed = 0
        self.camera = None       # (mode, intrinsics [8]): undistort_cv's camera for step(database=) without the epipolar check

    def close(self):
        _chk(lib().ovp_klt_destroy(self.ctx.handle), "ovp_klt_destroy")

    def reset(self):
        _chk(lib().ovp_klt_reset(self.ctx.handle), "ovp_klt_reset")
        self.ids_last, self.pts_last, self._fed = np.zeros(0, dtype=np.int64), np.zeros((0, 2), dtype=np.float32), 0
        self.currid, self._mask_last = 0, None

    def feed_image(self, img, hist="HISTOGRAM"):
        """one 8-bit image [height, width]: equalised, its pyramid built into the current half; does not wait for the device"""
        img = np.asarray(img)
        if img.dtype != np.uint8 or img.shape != (self.height, self.width):
            raise ValueError("an 8-bit image of %d x %d is expected" % (self.width, self.height))
        if img.strides[1] != 1 or img.strides[0] < self.width:
            img = np.ascontiguousarray(img)
        t0 = time.perf_counter()
        rc = lib().ovp_klt_feed_image(self.ctx.handle, img.ctypes.data, int(img.strides[0]), self.HIST[hist])
        self.last_feed_ms = 1e3 * (time.perf_counter() - t0)
        _chk(rc, "ovp_klt_feed_image")
        self._fed += 1

    def feed_image_opts(self, img, intake):
        """ovp_klt_feed_image_opts: one 8-bit image under the intake options (intake_defaults) - [height, width], or with
        intake.downsample the full-size image [2 height (+ 1), 2 width (+ 1)], halved on the device; does not wait for the device.
        A source size of 0 in the intake is the image's."""
        img = np.asarray(img)
        if img.dtype != np.uint8 or img.ndim != 2:
            raise ValueError("an 8-bit image is expected")
        if img.strides[1] != 1 or img.strides[0] < img.shape[1]:
            img = np.ascontiguousarray(img)
        o = Intake.from_buffer_copy(intake)
        if o.src_width == 0 and o.src_height == 0:
            o.src_height, o.src_width = img.shape
        elif (o.src_height, o.src_width) != img.shape:
            raise ValueError("the intake names a source of %d x %d" % (o.src_width, o.src_height))
        t0 = time.perf_counter()
        rc = lib().ovp_klt_feed_image_opts(self.ctx.handle, img.ctypes.data, int(img.strides[0]), C.byref(o))
        self.last_feed_ms = 1e3 * (time.perf_counter() - t0)
        _chk(rc, "ovp_klt_feed_image_opts")
        self._fed += 1

    def halve(self, img):
        """ovp_klt_halve: cv::pyrDown of an 8-bit image or mask [h, w] to [h // 2, w // 2] on the device (downsample_cameras'
        halving, core/VioManager.cpp:279-289); waits for the result"""
        img = np.asarray(img)
        if img.dtype != np.uint8 or img.ndim != 2:
            raise ValueError("an 8-bit image is expected")
        if img.strides[1] != 1 or img.strides[0] < img.shape[1]:
            img = np.ascontiguousarray(img)
        h, w = img.shape
        out = np.zeros((max(h // 2, 0), max(w // 2, 0)), dtype=np.uint8)
        _chk(lib().ovp_klt_halve(self.ctx.handle, img.ctypes.data, int(img.strides[0]), w, h, out.ctypes.data), "ovp_klt_halve")
        return out

    def clahe_lut(self, tiles_x, tiles_y):
        """tests: the tile LUTs of the last CLAHE feed -> [tiles_y, tiles_x, 256] uint8"""
        return self._debug(b"clahe_lut", 0, 256 * tiles_x * tiles_y).reshape(tiles_y, tiles_x, 256).copy()

    def track(self, pts_prev, guess=None):
        """pts_prev [n, 2] of the previous image into the current one, from guess (None: pts_prev) -> (pts [n, 2] f32, status [n])"""
        p = np.ascontiguousarray(pts_prev, dtype=np.float32).reshape(-1, 2)
        n = len(p)
        g = None if guess is None else np.ascontiguousarray(guess, dtype=np.float32).reshape(n, 2)
        out, st = np.zeros((n, 2), dtype=np.float32), np.zeros(n, dtype=np.uint8)
        t0 = time.perf_counter()
        rc = lib().ovp_klt_track(self.ctx.handle, n, p.ctypes.data, None if g is None else g.ctypes.data, out.ctypes.data, st.ctypes.data)
        self.last_track_ms = 1e3 * (time.perf_counter() - t0)
        _chk(rc, "ovp_klt_track")
        return out, st

    def add_points(self, ids, uv):
        """seeds or tops up the tracked set with points of the last image fed (detection is the caller's)"""
        self.ids_last = np.concatenate([self.ids_last, np.asarray(ids, dtype=np.int64).reshape(-1)])
        self.pts_last = np.concatenate([self.pts_last, np.asarray(uv, dtype=np.float32).reshape(-1, 2)])

    def detect_candidates(self, half=0, num_features=None, grid_x=None, grid_y=None, threshold=None, cap=None):
        """ovp_klt_detect on a half (0 current, 1 previous): every selected candidate, mask-independent, in output order ->
        dict(xy [n, 2] int32, response [n] int32, refined [n, 2] f32, cell [n] int32).  Options default to the detector's."""
        o = self.detector or {}
        nf, gx, gy, th = (int(o[k] if v is None else v) for k, v in zip(self.DETECTOR_KEYS, (num_features, grid_x, grid_y, threshold)))
        cap = self.max_points if cap is None else int(cap)
        m = max(cap, 1)
        n = C.c_int(-1)
        xy, resp = np.full((m, 2), -1, dtype=np.int32), np.full(m, -1, dtype=np.int32)
        ref, cell = np.full((m, 2), -1.0, dtype=np.float32), np.full(m, -1, dtype=np.int32)
        t0 = time.perf_counter()
        rc = lib().ovp_klt_detect(self.ctx.handle, int(half), nf, gx, gy, th, C.byref(n), xy.ctypes.data, resp.ctypes.data, ref.ctypes.data,
                                  cell.ctypes.data, cap)
        self.last_detect_ms = 1e3 * (time.perf_counter() - t0)
        self.last_detect_raw = (n.value, xy, resp, ref, cell)  # (tests: untouched by a refusal)
        _chk(rc, "ovp_klt_detect")
        k = n.value
        return dict(xy=xy[:k].copy(), response=resp[:k].copy(), refined=ref[:k].copy(), cell=cell[:k].copy())

    def detect(self, half=0, mask=None, pts=None, ids=None):
        """TrackPlane::perform_detection_monocular (:1173-1297) on level 0 of a half: walks pts / ids (None: none) through the
        occupancy grid, returns them when fewer than 5 % of num_features are missing, else accepts the device's candidates in order
        and numbers them ++currid.  Returns (pts [m, 2] f32, ids [m] int64).  Every candidate is refined on the device and the
        masked ones are dropped afterwards; the reference drops them before the refinement, which is the same: cornerSubPix treats
        each point on its own."""
        o = self.detector
        if o is None:
            raise ValueError("the tracker was made without detector options")
        cols, rows, mpd = self.width, self.height, o["min_px_dist"]
        pts = np.zeros((0, 2), dtype=np.float32) if pts is None else np.asarray(pts, dtype=np.float32).reshape(-1, 2)
        ids = np.zeros(0, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64).reshape(-1)
        mask = np.zeros((rows, cols), dtype=np.uint8) if mask is None else np.asarray(mask, dtype=np.uint8)
        f32 = np.float32
        wc, hc = int(f32(cols) / f32(mpd)), int(f32(rows) / f32(mpd))                      # :1180-1181 size_close
        sx, sy = f32(cols) / f32(o["grid_x"]), f32(rows) / f32(o["grid_y"])                  # :1183-1184
        occ = np.zeros((hc, wc), dtype=bool)
        upd = mask.copy()
        kp, ki = [], []
        for p, i in zip(pts, ids):
            x, y = int(p[0]), int(p[1])
            if x < 10 or x >= cols - 10 or y < 10 or y >= rows - 10:                        # :1195-1199
                continue
            xc, yc = int(p[0] / f32(mpd)), int(p[1] / f32(mpd))
            if xc < 0 or xc >= wc or yc < 0 or yc >= hc:                                    # :1203-1207
                continue
            xg, yg = int(np.floor(p[0] / sx)), int(np.floor(p[1] / sy))
            if xg < 0 or xg >= o["grid_x"] or yg < 0 or yg >= o["grid_y"]:                  # :1211-1215
                continue
            if occ[yc, xc] or mask[y, x] > 127:                                             # :1217-1228
                continue
            occ[yc, xc] = True
            if x - mpd >= 0 and x + mpd < cols and y - mpd >= 0 and y + mpd < rows:        # :1235-1239 the rectangle, when it fits
                upd[y - mpd:y + mpd + 1, x - mpd:x + mpd + 1] = 255
            kp.append(p), ki.append(int(i))
        self.last_detected = False
        if (o["num_features"] - len(ki)) >= o["num_features"] * (1.0 - 0.95):              # :1246-1249
            c = self.detect_candidates(half)
            self.last_detected = True
            for (x, y), p in zip(c["xy"], c["refined"]):
                if upd[y, x] > 127:                                                 # Grider_FAST's mask test, on the corner's pixel
                    continue
                xc, yc = int(p[0] / f32(mpd)), int(p[1] / f32(mpd))                         # :1265-1281
                if xc < 0 or xc >= wc or yc < 0 or yc >= hc or occ[yc, xc]:
                    continue
                occ[yc, xc] = True
                self.currid += 1                                                            # :1292
                kp.append(p), ki.append(self.currid)
        return np.array(kp, dtype=np.float32).reshape(-1, 2), np.array(ki, dtype=np.int64)

    CAMERA_MODES = {"normalised": 0, "radtan": 1, "equidistant": 2}

    def epipolar(self, pts0, pts1, status=None, camera=None, **opts):
        """ovp_klt_epipolar: the epipolar check of perform_matching (:1331-1350) on pts0 / pts1 [n, 2] f32 (pixels; normalised values
        without a camera), status [n] (None: all ones).  camera: None, or (mode, intrinsics [8]) with mode "normalised", "radtan" or
        "equidistant".  opts: threshold (default 2 / max(fx, fy), :1341-1344), confidence, max_iters, seed.  -> dict(mask [n] uint8,
        uvn0 / uvn1 [n, 2] f32, F [3, 3], count, winner (h, model), niters, stop, n_with_model, too_few, no_model)"""
        o = EpipolarOpts()
        lib().ovp_epipolar_defaults(C.byref(o))
        if camera is not None:
            mode, intr = camera
            o.mode = self.CAMERA_MODES[mode] if isinstance(mode, str) else int(mode)
            o.intrinsics[:] = [float(v) for v in intr]
            if o.mode:
                o.threshold = 2.0 / max(float(intr[0]), float(intr[1]))
        for k, v in opts.items():
            if k not in ("threshold", "confidence", "max_iters", "seed"):
                raise TypeError("unknown option %s" % k)
            setattr(o, k, v)
        p0 = np.ascontiguousarray(pts0, dtype=np.float32).reshape(-1, 2)
        n = len(p0)
        p1 = np.ascontiguousarray(pts1, dtype=np.float32).reshape(n, 2)
        st = None if status is None else np.ascontiguousarray(status, dtype=np.uint8).reshape(n)
        mask, u0, u1 = np.full(n, 255, dtype=np.uint8), np.full((n, 2), -1.0, dtype=np.float32), np.full((n, 2), -1.0, dtype=np.float32)
        info = EpipolarInfo()
        info.winner_h = -7
        t0 = time.perf_counter()
        rc = lib().ovp_klt_epipolar(self.ctx.handle, C.byref(o), n, p0.ctypes.data, p1.ctypes.data, None if st is None else st.ctypes.data,
                                    mask.ctypes.data, u0.ctypes.data, u1.ctypes.data, C.byref(info))
        self.last_epipolar_ms = 1e3 * (time.perf_counter() - t0)
        self.last_epipolar_raw = (mask, u0, u1, info)  # (tests: untouched by a refusal)
        _chk(rc, "ovp_klt_epipolar")
        self._epi_shape = (int(o.max_iters), n)
        if n == 0:
            return dict(mask=mask, uvn0=u0, uvn1=u1, F=np.zeros((3, 3)), count=0, winner=(-1, -1), niters=0, stop=0, n_with_model=0,
                        too_few=False, no_model=False)
        return dict(mask=mask, uvn0=u0, uvn1=u1, F=np.array(info.F[:]).reshape(3, 3), count=int(info.best_count),
                    winner=(int(info.winner_h), int(info.winner_model)), niters=int(info.niters), stop=int(info.stop),
                    n_with_model=int(info.n_with_model), too_few=bool(info.too_few), no_model=bool(info.no_model))

    def _epipolar_opts(self, camera=None, **opts):
        o = EpipolarOpts()
        lib().ovp_epipolar_defaults(C.byref(o))
        if camera is not None:
            mode, intr = camera
            o.mode = self.CAMERA_MODES[mode] if isinstance(mode, str) else int(mode)
            o.intrinsics[:] = [float(v) for v in intr]
            if o.mode:
                o.threshold = 2.0 / max(float(intr[0]), float(intr[1]))
        for k, v in opts.items():
            if k not in ("threshold", "confidence", "max_iters", "seed"):
                raise TypeError("unknown option %s" % k)
            setattr(o, k, v)
        return o

    def match_frame(self, pts_prev, ids, timestamp=0.0, mask=None, epipolar=None, check=False, database=None, compacted=False):
        """ovp_klt_match_frame: the back half of feed_monocular (:510-567) in one device pass - KLT from pts_prev [n, 2] with
        guess = pts_prev, the epipolar check (check=True) or the undistortion alone, the keep rule under mask [height, width] (None:
        none), and with database (a FeatureDatabase of this context) the survivors' update_feature.  epipolar: None, or
        dict(camera=, threshold=, confidence=, max_iters=, seed=) as step takes it.  -> dict(n_kept, keep [n] bool, pts [n, 2],
        status [n], mask [n], uvn [n, 2] (None without epipolar), kept_index [n_kept], info (EpipolarInfo), and with the check the
        fields epipolar() returns).  compacted=True (tests) adds kept_uv / kept_uvn [n_kept, 2] as the device compacted them, read
        back through two further debug calls; nothing above this entry needs them (pts[keep] and uvn[keep] are the same bytes)."""
        p = np.ascontiguousarray(pts_prev, dtype=np.float32).reshape(-1, 2)
        n = len(p)
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(n)
        o = None if epipolar is None else self._epipolar_opts(**epipolar)
        a = KltFrameIn()
        a.n, a.pts_prev, a.ids, a.timestamp = n, p.ctypes.data, ids.ctypes.data, float(timestamp)
        if mask is not None:
            mask = np.asarray(mask)
            if mask.dtype != np.uint8 or mask.shape != (self.height, self.width):
                raise ValueError("an 8-bit mask of %d x %d is expected" % (self.width, self.height))
            if mask.strides[1] != 1 or mask.strides[0] < self.width:
                mask = np.ascontiguousarray(mask)
            a.mask, a.mask_stride = mask.ctypes.data, int(mask.strides[0])
        a.epi = None if o is None else C.addressof(o)
        a.check, a.to_database = (1 if check else 0), (0 if database is None else 1)
        m = max(n, 1)
        keep, st, me = (np.full(m, 255, dtype=np.uint8) for _ in range(3))
        out, uvn = np.full((m, 2), -1.0, dtype=np.float32), np.full((m, 2), -1.0, dtype=np.float32)
        idx = np.full(m, -1, dtype=np.int32)
        r = KltFrameOut()
        r.n_kept, r.info.winner_h = -7, -7
        r.keep, r.pts_out, r.status, r.mask_epi, r.uvn, r.kept_index = (v.ctypes.data for v in (keep, out, st, me, uvn, idx))
        t0 = time.perf_counter()
        rc = lib().ovp_klt_match_frame(self.ctx.handle, C.byref(a), C.byref(r))
        self.last_frame_ms = 1e3 * (time.perf_counter() - t0)
        self.last_frame_raw = (r, keep, out, st, me, uvn, idx)  # (tests: untouched by a refusal)
        _chk(rc, "ovp_klt_match_frame")
        k, info = r.n_kept, r.info
        res = dict(n_kept=k, keep=keep[:n] != 0, pts=out[:n], status=st[:n], mask=me[:n], uvn=None if o is None else uvn[:n],
                   kept_index=idx[:k].copy(), info=info)
        if compacted:
            ran = n > 0 and not (check and n < OVP_EPI_MIN_POINTS)   # (otherwise nothing was published)
            none = np.zeros((0, 2), np.float32)
            res.update(kept_uv=self._debug(b"frame_uv", 0, 8 * k, np.float32).reshape(-1, 2).copy() if ran else none,
                       kept_uvn=self._debug(b"frame_uvn", 0, 8 * k, np.float32).reshape(-1, 2).copy() if ran and o is not None else none)
        if check:
            self._epi_shape = (int(o.max_iters), n)
            res.update(F=np.array(info.F[:]).reshape(3, 3), count=int(info.best_count), winner=(int(info.winner_h), int(info.winner_model)),
                       niters=int(info.niters), stop=int(info.stop), n_with_model=int(info.n_with_model), too_few=bool(info.too_few),
                       no_model=bool(info.no_model), uvn1=res["uvn"])
        return res

    def epipolar_stages(self):
        """tests: what the kernels of the last epipolar() left -> dict(samples [H, 7], n_models [H], models [H, 3, 9], counts [H, 3],
        table [n + 1])"""
        H, n = self._epi_shape
        off = (4 * H + 7) & ~7
        m = self._debug(b"epi_models", 0, off + 8 * 27 * H)
        return dict(samples=self._debug(b"epi_samples", 0, 28 * H, np.int32).reshape(H, 7).copy(),
                    n_models=m[:4 * H].view(np.int32).copy(), models=m[off:].view(np.float64).reshape(H, 3, 9).copy(),
                    counts=self._debug(b"epi_counts", 0, 12 * H, np.int32).reshape(H, 3).copy(),
                    table=self._debug(b"epi_table", 0, 4 * (n + 1), np.int32).copy())

    def step(self, img, mask=None, hist="HISTOGRAM", detect=False, epipolar=None, intake=None, database=None, timestamp=None,
             fused=False):
        """feed_monocular :505-567 minus detection and the epipolar check: feeds img, tracks pts_last into it with guess = pts_last,
        keeps a point unless x < 0, y < 0, (int) x >= cols, (int) y >= rows, mask > 127 at the truncated pixel, or status 0.
        Returns (ids, pts) of the kept points, which are pts_last / ids_last from here on.
        detect=True is feed_monocular :477-567 minus the epipolar check: without points it detects on the current image and returns
        (:477-491); otherwise it tops pts_last up on the previous half under the previous image's mask (:505-507), then tracks.
        epipolar: None, or dict(camera=(mode, intrinsics), threshold=, confidence=, max_iters=, seed=): perform_matching in full
        (:1299-1357) - fewer than 10 points go in: no KLT, nothing is kept (:1319-1323); none goes in: the reset of :520-530
        (last_reset); otherwise mask_out = status & mask_rsc decides with the rules above, and last_uv_norm holds the kept points'
        undistorted coordinates (:555).
        intake: None, or the intake options (intake_defaults): the image is fed through feed_image_opts (hist is not looked at),
        and with intake.downsample img and mask are the full-size ones - the mask is halved on the device (halve) before the keep
        rule and the detector use it (core/VioManager.cpp:279-289).
        database: None, or the context's FeatureDatabase: the kept points go to database.update_feature(timestamp, ids, uv,
        uv_norm) (:553-557); uv_norm needs a camera - epipolar=, or without the check the tracker's `camera` attribute
        ((mode, intrinsics): the undistortion alone decides nothing).  fused=False: the existing entries, one after the other -
        track, epipolar, the keep rule here, append.  fused=True: the same frame through ovp_klt_match_frame (match_frame), one
        entry; last_match, last_uv_norm, last_epipolar (without the stage read-backs), last_reset and last_keep are filled alike."""
        cam = None
        if database is not None or fused:
            if timestamp is None and database is not None:
                raise ValueError("a database needs the frame's timestamp")
            cam = epipolar if epipolar is not None else (None if self.camera is None else dict(camera=self.camera, max_iters=1))
            if database is not None and cam is None:
                raise ValueError("a database needs uv_norm: give epipolar= or set the tracker's camera")
        self.last_keep = np.zeros(0, dtype=bool)
        if intake is None:
            self.feed_image(img, hist)
        else:
            self.feed_image_opts(img, intake)
            if intake.downsample and mask is not None:
                mask = self.halve(np.asarray(mask, dtype=np.uint8))
        self.last_uv_norm, self.last_reset = np.zeros((0, 2), dtype=np.float32), False
        self.last_match = (np.zeros((0, 2), dtype=np.float32), np.zeros(0, dtype=np.uint8))
        if detect:
            mask_prev, self._mask_last = self._mask_last, (None if mask is None else np.array(mask, dtype=np.uint8))
            if len(self.ids_last) == 0:
                self.pts_last, self.ids_last = self.detect(0, mask)
                return self.ids_last.copy(), self.pts_last.copy()
            self.pts_last, self.ids_last = self.detect(1, mask_prev, self.pts_last, self.ids_last)
            self.last_topped = (self.ids_last.copy(), self.pts_last.copy())
        if epipolar is not None and self._fed >= 2:
            if len(self.ids_last) == 0:          # :1307 an empty mask -> :520-530
                self.last_reset = True
                return self.ids_last.copy(), self.pts_last.copy()
            if len(self.ids_last) < 10:          # :1319-1323 all zeros, no KLT
                self.ids_last, self.pts_last = np.zeros(0, dtype=np.int64), np.zeros((0, 2), dtype=np.float32)
                return self.ids_last.copy(), self.pts_last.copy()
        if self._fed < 2 or len(self.ids_last) == 0:
            return self.ids_last.copy(), self.pts_last.copy()
        if fused:
            r = self.match_frame(self.pts_last, self.ids_last, 0.0 if timestamp is None else timestamp, mask, cam,
                                 check=epipolar is not None, database=database)
            self.last_match, keep = (r["pts"], r["status"]), r["keep"]
            if epipolar is not None:
                self.last_epipolar = {k: v for k, v in r.items() if k in ("mask", "uvn1", "F", "count", "winner", "niters", "stop",
                                                                          "n_with_model", "too_few", "no_model")}
            self.last_keep = keep
            self.ids_last, self.pts_last = self.ids_last[keep], r["pts"][keep]
            if cam is not None:
                self.last_uv_norm = r["uvn"][keep]
            return self.ids_last.copy(), self.pts_last.copy()
        p, st = self.track(self.pts_last, self.pts_last)
        self.last_match = (p, st)  # of the points that went into this step, in their order
        if epipolar is not None:
            self.last_epipolar = self.epipolar(self.pts_last, p, st, **epipolar)
            st, uvn = self.last_epipolar["mask"], self.last_epipolar["uvn1"]
        elif cam is not None:   # the undistortion alone: one hypothesis, its mask not looked at
            uvn = self.epipolar(self.pts_last, p, st, **cam)["uvn1"]
        x, y = p[:, 0], p[:, 1]
        xi, yi = np.clip(x, 0, self.width - 1).astype(np.int64), np.clip(y, 0, self.height - 1).astype(np.int64)
        keep = (st != 0) & ~(x < 0) & ~(y < 0) & (np.trunc(x) < self.width) & (np.trunc(y) < self.height)
        if mask is not None:
            keep &= ~(np.asarray(mask)[yi, xi] > 127)
        self.last_keep = keep
        self.ids_last, self.pts_last = self.ids_last[keep], p[keep]
        if epipolar is not None or cam is not None:
            self.last_uv_norm = uvn[keep]
        if database is not None:
            database.update_feature(timestamp, self.ids_last, self.pts_last, self.last_uv_norm)   # :553-557
        return self.ids_last.copy(), self.pts_last.copy()

    def _debug(self, what, level, nbytes, dtype=np.uint8):
        out = np.zeros(max(nbytes, 1), dtype=np.uint8)
        k = lib().ovp_klt_debug(self.ctx.handle, what, int(level), out.ctypes.data, nbytes)
        if k < 0:
            raise OvpError(int(k), "ovp_klt_debug")
        return out[:k].view(dtype)

    def level(self, level, half="cur"):
        """tests: pyramid level `level` of the current ("cur") or previous ("prev") half -> [h, w] uint8"""
        w, h = self._debug(b"dims", level, 8, np.int32)
        return self._debug(half.encode(), level, int(w) * int(h)).reshape(int(h), int(w)).copy()

    def equalized(self):
        return self._debug(b"equalized", 0, self.width * self.height).reshape(self.height, self.width).copy()

    def iters(self, n):
        """iterations per level [n, n_levels] of the last track of n points"""
        return self._debug(b"iters", 0, 8 * n).reshape(n, 8)[:, :self.n_levels].astype(np.int32)

    def timer(self, on=True):
        """events around the kernels from the next call on (diagnostics: adds a stream synchronisation per entry)"""
        self._debug(b"timer", 1 if on else 0, 0)

    def kernel_ms(self):
        """GPU milliseconds of the last timed calls: dict(equalize, pyramid, track, score_nms, select, subpix, epi_undistort,
        epi_models, epi_count, epi_select, halve, clahe_lut, clahe_apply, keep_append)"""
        t = self._debug(b"time", 0, 56, np.float32)
        return dict(zip(("equalize", "pyramid", "track", "score_nms", "select", "subpix", "epi_undistort", "epi_models", "epi_count",
                         "epi_select", "halve", "clahe_lut", "clahe_apply", "keep_append"), (float(v) for v in t)))

    def refine(self, xy):
        """tests: k_fast_subpix from the starting positions xy [n, 2] on level 0 of the current half -> [n, 2] f32"""
        buf = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2).copy()
        k = lib().ovp_klt_debug(self.ctx.handle, b"refine", len(buf), buf.ctypes.data, buf.nbytes)
        if k < 0:
            raise OvpError(int(k), "ovp_klt_debug")
        return buf

    def score_map(self, what="score"):
        """tests: the level-0 score map ("score") of the last detect, or the same after suppression ("nms") -> [h, w] uint8"""
        return self._debug(what.encode(), 0, self.width * self.height).reshape(self.height, self.width).copy()


def rccl_unique_id() -> bytes:
    """ncclGetUniqueId through the library's own binding of RCCL (128 bytes, to be handed to every rank)."""
    buf = C.create_string_buffer(128)
    _chk(lib().ovp_rccl_unique_id(buf), "ovp_rccl_unique_id")
    return buf.raw


def rccl_comm_create(uid: bytes, rank: int, world: int, device: int = 0) -> int:
    """ncclCommInitRank (collective over all ranks); returns the ncclComm_t as an integer handle."""
    assert len(uid) == 128
    comm = C.c_void_p()
    _chk(lib().ovp_rccl_comm_create(C.create_string_buffer(uid, 128), int(rank), int(world), int(device), C.byref(comm)),
         "ovp_rccl_comm_create")
    return comm.value


def rccl_comm_destroy(comm: int):
    _chk(lib().ovp_rccl_comm_destroy(C.c_void_p(comm)), "ovp_rccl_comm_destroy")


def shard_range_of_mask(used, n_feats: int, rank: int, world: int):
    """ovp_shard_range_of_mask: the index range of the resident batch ovp_msckf_update_sharded gives to `rank` (pure host
    arithmetic of the library - callable without a GPU)."""
    import numpy as np

    lo, hi = C.c_int(0), C.c_int(0)
    u = None if used is None else np.ascontiguousarray(np.asarray(used).astype(np.uint8))
    _chk(lib().ovp_shard_range_of_mask(u.ctypes.data if u is not None else None, int(n_feats), int(rank), int(world), C.byref(lo),
                                       C.byref(hi)), "ovp_shard_range_of_mask")
    return lo.value, hi.value


def opts_from_scene(sc) -> UpdateOpts:
    o = sc.opts
    return UpdateOpts(o["sigma_px"], o["chi2_mult"], o["sigma_c"], int(o["do_fej"]), int(o["do_calib_pose"]),
                      int(o["do_calib_intr"]), 0)


class TriangOpts(C.Structure):
    _fields_ = [("refine_features", C.c_int), ("max_runs", C.c_int), ("init_lamda", C.c_double), ("max_lamda", C.c_double),
                ("min_dx", C.c_double), ("min_dcost", C.c_double), ("lam_mult", C.c_double), ("min_dist", C.c_double),
                ("max_dist", C.c_double), ("max_baseline", C.c_double), ("max_cond_number", C.c_double), ("triangulate_1d", C.c_int),
                ("reserved", C.c_int)]


def triang_defaults(**over):
    o = TriangOpts()
    lib().ovp_triang_defaults(C.byref(o))
    for k, v in over.items():
        setattr(o, k, v)
    return o


class Context:
    """One filter's device context: resident covariance, pose tables, feature batch, work buffers."""

    def __init__(self, n_state_max, n_clones_max, n_feats_max, device=0, stream=None):
        self._h = C.c_void_p()
        self._keep = []
        _chk(lib().ovp_ctx_create(device, int(n_state_max), int(n_clones_max), int(n_feats_max),
                                  C.c_void_p(stream) if stream else None, C.byref(self._h)), "ovp_ctx_create")
        self.n_state_max = int(n_state_max)
        self.n_feats = 0

    def close(self):
        if self._h:
            lib().ovp_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    # -- covariance -----------------------------------------------------------------------------
    def cov_upload(self, P, ld=None):
        """ld: leading dimension of the host copy the entry reads (>= n, default n); the rows are laid out with it first"""
        P = np.ascontiguousarray(P, dtype=np.float64)
        n = P.shape[0]
        if ld is not None and int(ld) != n:
            ld = int(ld)
            host = np.full((n, max(ld, n)), np.nan)
            host[:, :n] = P
            _chk(lib().ovp_cov_upload(self._h, host.ctypes.data, n, ld), "ovp_cov_upload")
            return
        _chk(lib().ovp_cov_upload(self._h, P.ctypes.data, n, n), "ovp_cov_upload")

    def cov_set_device(self, dev_ptr, n, ld):
        _chk(lib().ovp_cov_set_device(self._h, C.c_void_p(dev_ptr), n, ld), "ovp_cov_set_device")

    def cov_download(self, ld=None):
        """ld: leading dimension of the host copy the entry writes (>= n, default n); the n x n block is returned either way"""
        n = lib().ovp_cov_size(self._h)
        if ld is not None and int(ld) != n:
            ld = int(ld)
            host = np.full((n, max(ld, n)), np.nan)
            _chk(lib().ovp_cov_download(self._h, host.ctypes.data, n, ld), "ovp_cov_download")
            assert np.isnan(host[:, n:]).all()  # the entry writes the n columns of a row only
            return np.ascontiguousarray(host[:, :n])
        P = np.zeros((n, n))
        _chk(lib().ovp_cov_download(self._h, P.ctypes.data, n, n), "ovp_cov_download")
        return P

    def cov_augment_dt(self, pose_id, dt_id, dnc_dt):
        """StateHelper::augment_clone's time-offset Jacobian on the pose block at pose_id (ovp_cov_augment_dt)"""
        d = np.ascontiguousarray(dnc_dt, dtype=np.float64).reshape(6)
        _chk(lib().ovp_cov_augment_dt(self._h, int(pose_id), int(dt_id), d.ctypes.data), "ovp_cov_augment_dt")

    def cov_initialize_invertible(self, H_R, col_ids, H_Linv, R, ld=None):
        """StateHelper::initialize_invertible's covariance part (ovp_cov_initialize_invertible): H_R [k, cols] with the state
        column of each of its columns, H_Linv and R [k, k]; the covariance grows by k.  ld: leading dimension of the column-major
        H_R the entry reads (>= k, default k)."""
        H_R = np.asarray(H_R, dtype=np.float64)
        k, cols = H_R.shape
        ld = k if ld is None else int(ld)
        hr = np.full((cols, max(ld, k)), np.nan)  # row a = column a of H_R, ld apart
        hr[:, :k] = H_R.T
        col_ids = np.ascontiguousarray(col_ids, dtype=np.int32).reshape(-1)
        assert len(col_ids) == cols
        Hi = np.asfortranarray(np.asarray(H_Linv, dtype=np.float64).reshape(k, k))
        Rk = np.asfortranarray(np.asarray(R, dtype=np.float64).reshape(k, k))
        _chk(lib().ovp_cov_initialize_invertible(self._h, hr.ctypes.data, k, cols, ld, col_ids.ctypes.data, Hi.ctypes.data,
                                                 Rk.ctypes.data), "ovp_cov_initialize_invertible")

    def cov_size(self):
        return lib().ovp_cov_size(self._h)

    def cov_marginal(self, ids, sizes):
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        sizes = np.ascontiguousarray(sizes, dtype=np.int32)
        m = int(sizes.sum())
        out = np.zeros((m, m))
        _chk(lib().ovp_cov_marginal(self._h, ids.ctypes.data, sizes.ctypes.data, len(ids), out.ctypes.data),
             "ovp_cov_marginal")
        return out

    def cov_propagate(self, new_start, old_ids, old_sizes, Phi, Q):
        Phi = np.asfortranarray(Phi, dtype=np.float64)
        Q = np.asfortranarray(Q, dtype=np.float64)
        old_ids = np.ascontiguousarray(old_ids, dtype=np.int32)
        old_sizes = np.ascontiguousarray(old_sizes, dtype=np.int32)
        neg = C.c_int(0)
        _chk(lib().ovp_cov_propagate(self._h, int(new_start), int(Phi.shape[0]), old_ids.ctypes.data,
                                     old_sizes.ctypes.data, len(old_ids), Phi.ctypes.data, Q.ctypes.data,
                                     C.byref(neg)), "ovp_cov_propagate")
        return neg.value

    def cov_clone(self, src_id, size):
        _chk(lib().ovp_cov_clone(self._h, int(src_id), int(size)), "ovp_cov_clone")

    def cov_clone_jitter(self, rel):
        """relative inflation of a cloned block's diagonal (0 = exact copy as the reference, the default)"""
        _chk(lib().ovp_cov_clone_jitter(self._h, float(rel)), "ovp_cov_clone_jitter")

    def cov_marginalize(self, vid, size):
        _chk(lib().ovp_cov_marginalize(self._h, int(vid), int(size)), "ovp_cov_marginalize")

    def cov_marginalize_many(self, ids, sizes):
        """StateHelper::marginalize for several variables in one pass (ids / sizes in the numbering before the call, any order)"""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        sizes = np.ascontiguousarray(sizes, dtype=np.int32)
        assert ids.shape == sizes.shape and ids.ndim == 1
        _chk(lib().ovp_cov_marginalize_many(self._h, len(ids), ids.ctypes.data, sizes.ctypes.data), "ovp_cov_marginalize_many")

    def planes_merge_retire(self, new_col, old_col, plane_col, cp, sigma, chi2_mult, deg_max, retire_ids, retire_sizes):
        """StateHelper::merge_planes_and_marginalize from the first fused pair to the last retired plane (ovp_planes_merge_retire).
        Returns dict(accepted [n_pairs] bool, chi2, angle_deg, dx [n_pairs, n], neg_diag); every column is the one the state has
        before the call."""
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
        new_col, old_col, plane_col, retire_ids, retire_sizes = map(i32, (new_col, old_col, plane_col, retire_ids, retire_sizes))
        cp = np.ascontiguousarray(cp, dtype=np.float64).reshape(-1)
        assert len(new_col) == len(old_col) and len(cp) == 3 * len(plane_col) and len(retire_ids) == len(retire_sizes)
        m = PlaneMergeIn()
        m.n_pairs, m.new_col, m.old_col = len(new_col), new_col.ctypes.data, old_col.ctypes.data
        m.n_planes, m.plane_col, m.cp = len(plane_col), plane_col.ctypes.data, cp.ctypes.data
        m.sigma_plane_merge, m.plane_merge_chi2, m.plane_merge_deg_max = float(sigma), float(chi2_mult), float(deg_max)
        m.n_retire, m.retire_ids, m.retire_sizes = len(retire_ids), retire_ids.ctypes.data, retire_sizes.ctypes.data
        n, k = self.cov_size(), max(len(new_col), 1)
        acc, chi2, ang, dx = np.zeros(k, np.uint8), np.zeros(k), np.zeros(k), np.zeros((k, n))
        rc = lib().ovp_planes_merge_retire(self._h, C.byref(m), acc.ctypes.data, chi2.ctypes.data, ang.ctypes.data, dx.ctypes.data, n)
        if rc not in (0, OVP_E_NEGDIAG):
            raise OvpError(rc, "ovp_planes_merge_retire")
        k = len(new_col)
        return dict(accepted=acc[:k].astype(bool), chi2=chi2[:k], angle_deg=ang[:k], dx=dx[:k], neg_diag=rc == OVP_E_NEGDIAG)

    def zupt_update(self, readings, imu_id, R_GtoI, R_GtoI_jac, b_g, b_a, po, chi2_threshold, noise_mult=10.0, vel_ok=True,
                    disparity_passed=False, time_kernels=False):
        """UpdaterZeroVelocity::try_update's gate and update in one device pass (ovp_zupt_update).  readings [n, 7] = what
        Propagator::select_imu_readings returned; R_GtoI [3, 3] the value and R_GtoI_jac the rotation of the Jacobian (the first
        estimate with do_fej); po: dict with sigma_w, sigma_a, sigma_wb, sigma_ab, gravity_mag; chi2_threshold =
        chi2_multipler * chi2_quantile_095(6 (n - 1)).  Returns dict(accepted, chi2, rows, dx [n], neg_diag, kernel_ms [3])."""
        f64 = lambda a, *sh: np.ascontiguousarray(a, dtype=np.float64).reshape(*sh)  # noqa: E731
        rd = f64(readings, -1, 7)
        z = ZuptIn()
        z.n_readings, z.readings, z.imu_id = len(rd), rd.ctypes.data, int(imu_id)
        z.R_GtoI[:], z.R_GtoI_jac[:] = list(f64(R_GtoI, 9)), list(f64(R_GtoI_jac, 9))
        z.b_g[:], z.b_a[:] = list(f64(b_g, 3)), list(f64(b_a, 3))
        z.gravity_mag = float(po["gravity_mag"])
        z.sigma_w, z.sigma_a, z.sigma_wb, z.sigma_ab = (float(po[k]) for k in ("sigma_w", "sigma_a", "sigma_wb", "sigma_ab"))
        z.zupt_noise_multiplier, z.chi2_threshold = float(noise_mult), float(chi2_threshold)
        z.vel_ok, z.disparity_passed, z.time_kernels = int(bool(vel_ok)), int(bool(disparity_passed)), int(bool(time_kernels))
        o, info = ZuptOut(), UpdateInfo()
        dx = np.zeros(max(self.cov_size(), 1))
        rc = lib().ovp_zupt_update(self._h, C.byref(z), dx.ctypes.data, C.byref(o), C.byref(info))
        if rc not in (0, OVP_E_NEGDIAG):
            raise OvpError(rc, "ovp_zupt_update")
        return dict(accepted=bool(o.accepted), chi2=o.chi2, rows=o.rows, dx=dx[:self.cov_size()], neg_diag=rc == OVP_E_NEGDIAG,
                    kernel_ms=np.array(o.kernel_ms[:]), info=info)

    def propagate_and_clone(self, readings, imu_id, x, po, clone=True, dt_id=-1, time_kernels=False):
        """Propagator::propagate_and_clone behind its preamble in one device pass (ovp_propagate_and_clone).  readings [n, 7] =
        what Propagator::select_imu_readings returned (n = 0 and 1 are legal); x: dict with q, p, v, bg, ba, q_fej, p_fej, v_fej
        (JPL q_GtoI); po: dict with sigma_w, sigma_a, sigma_wb, sigma_ab, gravity_mag, use_rk4, imu_avg, do_fej.  Returns
        dict(q, p, v, last_w, Phi [15, 15], Q [15, 15], n_intervals, clone_id, neg_diag, kernel_ms [4])."""
        f64 = lambda a, *sh: np.ascontiguousarray(a, dtype=np.float64).reshape(*sh)  # noqa: E731
        rd = f64(readings, -1, 7)
        z = PropagateIn()
        z.n_readings, z.readings, z.imu_id = len(rd), (rd.ctypes.data if len(rd) else None), int(imu_id)
        for k, m in (("q", 4), ("p", 3), ("v", 3), ("bg", 3), ("ba", 3), ("q_fej", 4), ("p_fej", 3), ("v_fej", 3)):
            getattr(z, k)[:] = list(f64(x[k], m))
        z.gravity_mag = float(po["gravity_mag"])
        z.sigma_w, z.sigma_a, z.sigma_wb, z.sigma_ab = (float(po[k]) for k in ("sigma_w", "sigma_a", "sigma_wb", "sigma_ab"))
        z.use_rk4, z.imu_avg, z.do_fej = (int(bool(po[k])) for k in ("use_rk4", "imu_avg", "do_fej"))
        z.clone, z.dt_id, z.time_kernels = int(bool(clone)), int(dt_id), int(bool(time_kernels))
        o = PropagateOut()
        rc = lib().ovp_propagate_and_clone(self._h, C.byref(z), C.byref(o))
        if rc not in (0, OVP_E_NEGDIAG):
            raise OvpError(rc, "ovp_propagate_and_clone")
        return dict(q=np.array(o.q[:]), p=np.array(o.p[:]), v=np.array(o.v[:]), last_w=np.array(o.last_w[:]),
                    Phi=np.array(o.Phi[:]).reshape(15, 15).T.copy(), Q=np.array(o.Q[:]).reshape(15, 15).T.copy(),
                    n_intervals=o.n_intervals, clone_id=o.clone_id, neg_diag=rc == OVP_E_NEGDIAG,
                    kernel_ms=np.array(o.kernel_ms[:]))

    # -- state / batch ---------------------------------------------------------------------------
    def state_upload(self, sc, state=None):
        s = sc if state is None else state
        bufs = dict(
            clone_q=np.ascontiguousarray(s["clone_q"], dtype=np.float64),
            clone_p=np.ascontiguousarray(s["clone_p"], dtype=np.float64),
            clone_q_fej=np.ascontiguousarray(s["clone_q_fej"], dtype=np.float64),
            clone_p_fej=np.ascontiguousarray(s["clone_p_fej"], dtype=np.float64),
            clone_id=np.ascontiguousarray(sc.ids["clones"], dtype=np.int32),
        )
        st = StateTables()
        st.n_state = int(sc.N)
        st.n_clones = int(bufs["clone_q"].shape[0])
        dp = C.POINTER(C.c_double)
        st.clone_q = bufs["clone_q"].ctypes.data_as(dp)
        st.clone_p = bufs["clone_p"].ctypes.data_as(dp)
        st.clone_q_fej = bufs["clone_q_fej"].ctypes.data_as(dp)
        st.clone_p_fej = bufs["clone_p_fej"].ctypes.data_as(dp)
        st.clone_id = bufs["clone_id"].ctypes.data_as(C.POINTER(C.c_int))
        st.calib_q[:] = list(s["calib_q"])
        st.calib_p[:] = list(s["calib_p"])
        st.calib_id = int(sc.ids["calib"])
        st.intrinsics[:] = list(s["intr"])
        st.intr_id = int(sc.ids["intr"])
        st.cam_fisheye = 1 if sc.get("fisheye", False) else 0
        _chk(lib().ovp_state_upload(self._h, C.byref(st)), "ovp_state_upload")

    def state_tables(self, sc, state=None):
        """The ovp_state_tables struct of a scene, built once (with the arrays it points into): callers that upload the same
        tables every frame (bench.py) pass it to state_upload_prepared and skip the per-call marshalling."""
        s = sc if state is None else state
        bufs = dict(
            clone_q=np.ascontiguousarray(s["clone_q"], dtype=np.float64), clone_p=np.ascontiguousarray(s["clone_p"], dtype=np.float64),
            clone_q_fej=np.ascontiguousarray(s["clone_q_fej"], dtype=np.float64),
            clone_p_fej=np.ascontiguousarray(s["clone_p_fej"], dtype=np.float64), clone_id=np.ascontiguousarray(sc.ids["clones"], dtype=np.int32))
        st = StateTables()
        st.n_state = int(sc.N)
        st.n_clones = int(bufs["clone_q"].shape[0])
        dp = C.POINTER(C.c_double)
        st.clone_q = bufs["clone_q"].ctypes.data_as(dp)
        st.clone_p = bufs["clone_p"].ctypes.data_as(dp)
        st.clone_q_fej = bufs["clone_q_fej"].ctypes.data_as(dp)
        st.clone_p_fej = bufs["clone_p_fej"].ctypes.data_as(dp)
        st.clone_id = bufs["clone_id"].ctypes.data_as(C.POINTER(C.c_int))
        st.calib_q[:] = list(s["calib_q"])
        st.calib_p[:] = list(s["calib_p"])
        st.calib_id = int(sc.ids["calib"])
        st.intrinsics[:] = list(s["intr"])
        st.intr_id = int(sc.ids["intr"])
        st.cam_fisheye = 1 if sc.get("fisheye", False) else 0
        st._keep = bufs
        return st

    def state_upload_prepared(self, st):
        _chk(lib().ovp_state_upload(self._h, C.byref(st)), "ovp_state_upload")

    def prepared_frame(self, sc, opts_plane=None, opts_point=None):
        """Everything a frame's calls need on the Python side, marshalled once: state tables, feature batch, plane batch, output
        arrays.  bench.py times the C-ABI, not ctypes struct building and numpy allocations (~70 us of a config-3 step)."""
        return PreparedFrame(self, sc, opts_plane, opts_point)

    def batch_upload(self, uv, clone_idx, n_meas, p_FinG):
        uv = np.ascontiguousarray(uv, dtype=np.float32)
        clone_idx = np.ascontiguousarray(clone_idx, dtype=np.int32)
        n_meas = np.ascontiguousarray(n_meas, dtype=np.int32)
        p_FinG = np.ascontiguousarray(p_FinG, dtype=np.float64)
        fb = FeatureBatch(int(uv.shape[0]), int(uv.shape[1]) if uv.ndim > 1 else 1, uv.ctypes.data,
                          clone_idx.ctypes.data, n_meas.ctypes.data, p_FinG.ctypes.data)
        _chk(lib().ovp_batch_upload(self._h, C.byref(fb)), "ovp_batch_upload")
        self.n_feats = int(uv.shape[0])

    def batch_bind_device(self, n_feats, max_meas, uv_ptr, clone_idx_ptr, n_meas_ptr, p_ptr):
        fb = FeatureBatch(int(n_feats), int(max_meas), uv_ptr, clone_idx_ptr, n_meas_ptr, p_ptr)
        _chk(lib().ovp_batch_bind_device(self._h, C.byref(fb)), "ovp_batch_bind_device")
        self.n_feats = int(n_feats)

    def batch_upload_scene(self, sc, feats=None):
        sel = slice(None) if feats is None else np.asarray(feats)
        self.batch_upload(sc.uv[sel], sc.clone_idx[sel], sc.n_meas[sel], sc.p_FinG[sel])

    # -- update ----------------------------------------------------------------------------------
    def msckf_update(self, opts: UpdateOpts, raise_on_error=True):
        n = self.cov_size()
        dx = np.zeros(n)
        acc = np.zeros(max(self.n_feats, 1), dtype=np.uint8)
        chi2 = np.zeros(max(self.n_feats, 1))
        info = UpdateInfo()
        rc = lib().ovp_msckf_update(self._h, C.byref(opts), dx.ctypes.data, acc.ctypes.data, chi2.ctypes.data,
                                    C.byref(info))
        if rc != 0 and raise_on_error:
            raise OvpError(rc, "ovp_msckf_update")
        return dict(dx=dx, accepted=acc[: self.n_feats].astype(bool), chi2=chi2[: self.n_feats], info=info, rc=rc)

    def msckf_dense_blocks(self, chi2_mult, blocks):
        """ovp_msckf_dense_blocks: blocks = list of (H [rows, cols], col_ids [cols], res [rows]) - features the batch format cannot
        carry, after the nullspace projection.  Returns (accepted [bool], chi2); the accepted ones join the next msckf_update."""
        nb = len(blocks)
        rows = np.array([b[0].shape[0] for b in blocks], dtype=np.int32)
        cols = np.array([b[0].shape[1] for b in blocks], dtype=np.int32)
        H = np.concatenate([np.asfortranarray(b[0], dtype=np.float64).ravel(order="F") for b in blocks]) if nb else np.zeros(1)
        ids = np.concatenate([np.asarray(b[1], dtype=np.int32) for b in blocks]) if nb else np.zeros(1, dtype=np.int32)
        res = np.concatenate([np.asarray(b[2], dtype=np.float64) for b in blocks]) if nb else np.zeros(1)
        acc = np.zeros(max(nb, 1), dtype=np.uint8)
        chi2 = np.zeros(max(nb, 1))
        _chk(lib().ovp_msckf_dense_blocks(self._h, C.c_double(float(chi2_mult)), nb, rows.ctypes.data, cols.ctypes.data, H.ctypes.data,
                                          np.ascontiguousarray(ids).ctypes.data, res.ctypes.data, acc.ctypes.data, chi2.ctypes.data),
             "ovp_msckf_dense_blocks")
        return acc[:nb].astype(bool), chi2[:nb]

    # -- general point features (any camera, long tracks) ---------------------------------------------------------------------
    def cameras_upload(self, sc, state=None):
        """ovp_cameras_upload from a scene: camera 0 = the scene's calibration, camera 1 = sc.cam1 (synth.make_stereo_scene) when
        present.  A scene with `cams` (a list of dicts calib_q, calib_p, intr, calib_id, intr_id, fisheye: any number of cameras,
        a lens model each) uploads that list instead, camera k = cams[k].  `state` overrides the values as in state_upload; for a
        scene with `cams` it must carry the list as well."""
        s = sc if state is None else state
        if "cams" in sc:
            if "cams" not in s:
                raise ValueError("the scene has `cams`: a `state` override must carry its own `cams` list")
            self.cameras_upload_tables([(t["calib_q"], t["calib_p"], t["intr"], t["calib_id"], t["intr_id"], 1 if t["fisheye"] else 0)
                                        for t in s["cams"]])
            return
        fish = 1 if sc.get("fisheye", False) else 0
        cams = [(s["calib_q"], s["calib_p"], s["intr"], sc.ids["calib"], sc.ids["intr"], fish)]
        c1 = s.get("cam1", None) if state is not None else None
        c1 = c1 if c1 is not None else sc.get("cam1", None)
        if c1 is not None:
            cams.append((c1["calib_q"], c1["calib_p"], c1["intr"], sc.ids["calib1"], sc.ids["intr1"], 0))
        self.cameras_upload_tables(cams)

    def cameras_upload_tables(self, cams):
        """cams: list of (calib_q, calib_p, intrinsics, calib_id, intr_id, fisheye), camera k = cams[k]."""
        arr = (CameraTables * len(cams))()
        for k, (q, p, intr, cid, iid, fish) in enumerate(cams):
            arr[k].calib_q[:] = [float(v) for v in q]
            arr[k].calib_p[:] = [float(v) for v in p]
            arr[k].calib_id = int(cid)
            arr[k].intrinsics[:] = [float(v) for v in intr]
            arr[k].intr_id = int(iid)
            arr[k].fisheye = int(fish)
        _chk(lib().ovp_cameras_upload(self._h, len(cams), arr), "ovp_cameras_upload")

    @staticmethod
    def _general_batch(uv, clone_idx, cam_idx, n_meas, p_FinG=None):
        uv = np.ascontiguousarray(uv, dtype=np.float32)
        F = int(uv.shape[0])
        M = int(uv.shape[1]) if uv.ndim > 1 else 1
        keep = dict(uv=uv, clone_idx=np.ascontiguousarray(clone_idx, dtype=np.int32),
                    cam_idx=np.ascontiguousarray(np.zeros((F, M)) if cam_idx is None else cam_idx, dtype=np.int32),
                    n_meas=np.ascontiguousarray(n_meas, dtype=np.int32),
                    p_FinG=np.ascontiguousarray(np.zeros((F, 3)) if p_FinG is None else p_FinG, dtype=np.float64))
        gb = GeneralBatch(F, M, keep["uv"].ctypes.data, keep["clone_idx"].ctypes.data, keep["cam_idx"].ctypes.data,
                          keep["n_meas"].ctypes.data, keep["p_FinG"].ctypes.data)
        gb._keep = keep
        return gb

    def msckf_general_features(self, opts: UpdateOpts, sc=None, feats=None, uv=None, clone_idx=None, cam_idx=None, n_meas=None,
                               p_FinG=None, raise_on_error=True):
        """ovp_msckf_general_features on the features `feats` of a scene (fields uv, clone_idx, cam_idx, n_meas, p_FinG; a scene
        without cam_idx is camera 0 only) or on explicit arrays.  Returns (accepted [bool], chi2, rc); the accepted ones join the
        next msckf_update."""
        if sc is not None:
            sel = slice(None) if feats is None else np.asarray(feats)
            uv, clone_idx, n_meas, p_FinG = sc.uv[sel], sc.clone_idx[sel], sc.n_meas[sel], sc.p_FinG[sel]
            cam_idx = sc.cam_idx[sel] if "cam_idx" in sc else None
        gb = self._general_batch(uv, clone_idx, cam_idx, n_meas, p_FinG)
        F = gb.n_feats
        acc = np.zeros(max(F, 1), dtype=np.uint8)
        chi2 = np.zeros(max(F, 1))
        rc = lib().ovp_msckf_general_features(self._h, C.byref(opts), C.byref(gb), acc.ctypes.data, chi2.ctypes.data)
        if rc != 0 and raise_on_error:
            raise OvpError(rc, "ovp_msckf_general_features")
        return acc[:F].astype(bool), chi2[:F], rc

    def triangulate_general(self, sc=None, feats=None, uv_norm=None, clone_idx=None, cam_idx=None, n_meas=None, opts=None,
                            raise_on_error=True):
        """ovp_triangulate_general on the features `feats` of a scene (uv_norm, clone_idx, cam_idx, n_meas) or on explicit
        arrays; returns dict(p_FinG [F,3], ok [F], rc)."""
        if sc is not None:
            sel = slice(None) if feats is None else np.asarray(feats)
            uv_norm, clone_idx, n_meas = sc.uv_norm[sel], sc.clone_idx[sel], sc.n_meas[sel]
            cam_idx = sc.cam_idx[sel] if "cam_idx" in sc else None
        o = opts if opts is not None else triang_defaults()
        uvn = np.ascontiguousarray(uv_norm, dtype=np.float32)
        gb = self._general_batch(uvn, clone_idx, cam_idx, n_meas)
        F = gb.n_feats
        p = np.zeros((max(F, 1), 3))
        ok = np.zeros(max(F, 1), dtype=np.uint8)
        rc = lib().ovp_triangulate_general(self._h, C.byref(o), C.byref(gb), uvn.ctypes.data, p.ctypes.data, ok.ctypes.data)
        if rc != 0 and raise_on_error:
            raise OvpError(rc, "ovp_triangulate_general")
        return dict(p_FinG=p[:F], ok=ok[:F].astype(bool), rc=rc)

    def msckf_update_sharded(self, opts: UpdateOpts, comm, rank=0, world=1, raise_on_error=True):
        """ovp_msckf_update_sharded: this rank's share of the point features -> pair -> ncclAllReduce -> update (comm: handle from
        rccl_comm_create or None for a single rank).  Results as msckf_update plus the shard's index range."""
        n, F = self.cov_size(), self.n_feats
        dx = np.zeros(n)
        acc = np.zeros(max(F, 1), dtype=np.uint8)
        chi2 = np.zeros(max(F, 1))
        info = UpdateInfo()
        lo, hi = C.c_int(0), C.c_int(0)
        rc = lib().ovp_msckf_update_sharded(self._h, C.byref(opts), C.c_void_p(comm) if comm else None, int(rank), int(world),
                                            dx.ctypes.data, acc.ctypes.data, chi2.ctypes.data, C.byref(info), C.byref(lo), C.byref(hi))
        if raise_on_error:
            _chk(rc, "ovp_msckf_update_sharded")
        return dict(dx=dx, accepted=acc[:F].astype(bool), chi2=chi2[:F], info=info, rc=rc, shard=(lo.value, hi.value))

    def shard_range(self, opts: UpdateOpts, rank, world):
        lo, hi = C.c_int(0), C.c_int(0)
        _chk(lib().ovp_shard_range(self._h, C.byref(opts), int(rank), int(world), C.byref(lo), C.byref(hi)), "ovp_shard_range")
        return lo.value, hi.value

    def rccl_gather_decisions(self, comm, accepted, chi2=None):
        """ovp_rccl_gather_decisions: completes a sharded update's per-feature decisions on every rank (in place; collective)."""
        acc = np.ascontiguousarray(np.asarray(accepted).astype(np.uint8))
        ch = None if chi2 is None else np.ascontiguousarray(np.asarray(chi2, dtype=np.float64))
        _chk(lib().ovp_rccl_gather_decisions(self._h, C.c_void_p(comm) if comm else None, acc.ctypes.data,
                                             ch.ctypes.data if ch is not None else None), "ovp_rccl_gather_decisions")
        return acc.astype(bool), ch

    def rccl_allreduce_gram(self, comm):
        _chk(lib().ovp_rccl_allreduce_gram(self._h, C.c_void_p(comm)), "ovp_rccl_allreduce_gram")

    def batch_set_range(self, lo=-1, hi=-1):
        """Point updates that follow take the features [lo, hi) of the uploaded batch only (-1, -1 = all of it)."""
        _chk(lib().ovp_batch_set_range(self._h, int(lo), int(hi)), "ovp_batch_set_range")

    def build_gate_gram_async(self, opts: UpdateOpts):
        _chk(lib().ovp_msckf_build_gate_gram_async(self._h, C.byref(opts)), "ovp_msckf_build_gate_gram_async")

    def gram_buffer(self):
        p = C.c_void_p()
        rows, ld = C.c_int(), C.c_int()
        _chk(lib().ovp_gram_buffer(self._h, C.byref(p), C.byref(rows), C.byref(ld)), "ovp_gram_buffer")
        return p.value, rows.value, ld.value

    def ekf_update_from_gram_async(self):
        _chk(lib().ovp_ekf_update_from_gram_async(self._h), "ovp_ekf_update_from_gram_async")

    def fetch_results(self, raise_on_error=True):
        n = self.cov_size()
        dx = np.zeros(n)
        acc = np.zeros(max(self.n_feats, 1), dtype=np.uint8)
        chi2 = np.zeros(max(self.n_feats, 1))
        info = UpdateInfo()
        rc = lib().ovp_msckf_fetch_results(self._h, dx.ctypes.data, acc.ctypes.data, chi2.ctypes.data, C.byref(info))
        if rc != 0 and raise_on_error:
            raise OvpError(rc, "ovp_msckf_fetch_results")
        return dict(dx=dx, accepted=acc[: self.n_feats].astype(bool), chi2=chi2[: self.n_feats], info=info, rc=rc)

    def plane_update(self, opts: UpdateOpts, plane_of_feat, cp, cp_fej, plane_state_id, raise_on_error=True, slam=None,
                     force_decision=None):
        """UpdaterMSCKF::update per-plane loop. Returns dict(dx [n_planes, n], ok, chi2, dof, used).
        slam = dict(plane [k] 1-based, id [k], p [k,3], p_fej [k,3]): SLAM landmarks lying on out-of-state planes."""
        plane_of_feat = np.ascontiguousarray(plane_of_feat, dtype=np.int32)
        cp = np.ascontiguousarray(cp, dtype=np.float64)
        cp_fej = np.ascontiguousarray(cp_fej, dtype=np.float64)
        sid = np.ascontiguousarray(plane_state_id, dtype=np.int32)
        npl = int(sid.shape[0])
        n = self.cov_size()
        dx = np.zeros((max(npl, 1), n))
        ok = np.zeros(max(npl, 1), dtype=np.uint8)
        chi2 = np.zeros(max(npl, 1))
        dof = np.zeros(max(npl, 1), dtype=np.int32)
        used = np.zeros(max(self.n_feats, 1), dtype=np.uint8)
        pb = PlaneBatch(npl, plane_of_feat.ctypes.data, cp.ctypes.data, cp_fej.ctypes.data, sid.ctypes.data)
        if slam is not None and len(slam["id"]):
            s_pl = np.ascontiguousarray(slam["plane"], dtype=np.int32)
            s_id = np.ascontiguousarray(slam["id"], dtype=np.int32)
            s_p = np.ascontiguousarray(slam["p"], dtype=np.float64)
            s_pf = np.ascontiguousarray(slam["p_fej"], dtype=np.float64)
            pb.n_slam = len(s_id)
            pb.slam_plane, pb.slam_state_id = s_pl.ctypes.data, s_id.ctypes.data
            pb.slam_p, pb.slam_p_fej = s_p.ctypes.data, s_pf.ctypes.data
        if force_decision is not None:
            fd = np.ascontiguousarray(force_decision, dtype=np.uint8)
            assert fd.shape[0] == npl
            pb.force_decision = fd.ctypes.data
        rc = lib().ovp_msckf_plane_update(self._h, C.byref(opts), C.byref(pb), dx.ctypes.data, ok.ctypes.data,
                                          chi2.ctypes.data, dof.ctypes.data, used.ctypes.data)
        if rc != 0 and raise_on_error:
            raise OvpError(rc, "ovp_msckf_plane_update")
        return dict(dx=dx[:npl], ok=ok[:npl].astype(bool), chi2=chi2[:npl], dof=dof[:npl],
                    used=used[: self.n_feats].astype(bool), rc=rc)

    def plane_update_general(self, opts: UpdateOpts, plane_of_feat, cp, cp_fej, plane_state_id, sc=None, feats=None, uv=None,
                             clone_idx=None, cam_idx=None, n_meas=None, p_FinG=None, plane_of_gen=None, raise_on_error=True,
                             slam=None, force_decision=None):
        """ovp_msckf_plane_update_general: the plane loop with the on-plane features of a general batch behind the uploaded batch's.
        The general batch = the features `feats` of a scene (uv, clone_idx, cam_idx, n_meas, p_FinG; plane_of_gen defaults to their
        sc.plane_id; a scene without cam_idx is camera 0 only) or explicit arrays; None / empty = no general features.
        Returns plane_update's dict plus gen_used [bool]."""
        if sc is not None:
            sel = np.asarray(feats, dtype=np.int64)
            uv, clone_idx, n_meas, p_FinG = sc.uv[sel], sc.clone_idx[sel], sc.n_meas[sel], sc.p_FinG[sel]
            cam_idx = sc.cam_idx[sel] if "cam_idx" in sc else None
            if plane_of_gen is None:
                plane_of_gen = sc.plane_id[sel]
        if uv is None or len(uv) == 0:
            gb = GeneralBatch(0, 0, None, None, None, None, None)
            pog = np.zeros(1, dtype=np.int32)
        else:
            gb = self._general_batch(uv, clone_idx, cam_idx, n_meas, p_FinG)
            pog = np.ascontiguousarray(plane_of_gen, dtype=np.int32)
            assert pog.shape[0] == gb.n_feats
        GF = gb.n_feats
        plane_of_feat = np.ascontiguousarray(plane_of_feat, dtype=np.int32)
        cp = np.ascontiguousarray(cp, dtype=np.float64)
        cp_fej = np.ascontiguousarray(cp_fej, dtype=np.float64)
        sid = np.ascontiguousarray(plane_state_id, dtype=np.int32)
        npl = int(sid.shape[0])
        n = self.cov_size()
        dx = np.zeros((max(npl, 1), n))
        ok = np.zeros(max(npl, 1), dtype=np.uint8)
        chi2 = np.zeros(max(npl, 1))
        dof = np.zeros(max(npl, 1), dtype=np.int32)
        used = np.zeros(max(self.n_feats, 1), dtype=np.uint8)
        gused = np.zeros(max(GF, 1), dtype=np.uint8)
        pb = PlaneBatch(npl, plane_of_feat.ctypes.data, cp.ctypes.data, cp_fej.ctypes.data, sid.ctypes.data)
        if slam is not None and len(slam["id"]):
            s_pl = np.ascontiguousarray(slam["plane"], dtype=np.int32)
            s_id = np.ascontiguousarray(slam["id"], dtype=np.int32)
            s_p = np.ascontiguousarray(slam["p"], dtype=np.float64)
            s_pf = np.ascontiguousarray(slam["p_fej"], dtype=np.float64)
            pb.n_slam = len(s_id)
            pb.slam_plane, pb.slam_state_id = s_pl.ctypes.data, s_id.ctypes.data
            pb.slam_p, pb.slam_p_fej = s_p.ctypes.data, s_pf.ctypes.data
        if force_decision is not None:
            fd = np.ascontiguousarray(force_decision, dtype=np.uint8)
            assert fd.shape[0] == npl
            pb.force_decision = fd.ctypes.data
        rc = lib().ovp_msckf_plane_update_general(self._h, C.byref(opts), C.byref(pb), C.byref(gb), pog.ctypes.data, dx.ctypes.data,
                                                  ok.ctypes.data, chi2.ctypes.data, dof.ctypes.data, used.ctypes.data, gused.ctypes.data)
        if rc != 0 and raise_on_error:
            raise OvpError(rc, "ovp_msckf_plane_update_general")
        return dict(dx=dx[:npl], ok=ok[:npl].astype(bool), chi2=chi2[:npl], dof=dof[:npl], used=used[: self.n_feats].astype(bool),
                    gen_used=gused[:GF].astype(bool), rc=rc)

    def plane_init(self, opts: UpdateOpts, plane_of_feat, cp, const_init_multi, const_init_chi2, raise_on_error=True):
        """UpdaterPlane::init_vio_plane core (ovp_plane_init: ovp_plane_init_general without a general batch).
        Returns dict(dx [n_planes, stride], ok, chi2, dof, new_ids, cp, used, rc)."""
        plane_of_feat = np.ascontiguousarray(plane_of_feat, dtype=np.int32)
        cp = np.ascontiguousarray(cp, dtype=np.float64)
        npl = int(cp.shape[0])
        sid = -np.ones(max(npl, 1), dtype=np.int32)
        stride = self.n_state_max
        dx = np.zeros((max(npl, 1), stride))
        ok = np.zeros(max(npl, 1), dtype=np.uint8)
        chi2 = np.zeros(max(npl, 1))
        dof = np.zeros(max(npl, 1), dtype=np.int32)
        nid = np.zeros(max(npl, 1), dtype=np.int32)
        cpn = np.zeros((max(npl, 1), 3))
        used = np.zeros(max(self.n_feats, 1), dtype=np.uint8)
        pb = PlaneBatch(npl, plane_of_feat.ctypes.data, cp.ctypes.data, cp.ctypes.data, sid.ctypes.data)
        rc = lib().ovp_plane_init(self._h, C.byref(opts), C.byref(pb), C.c_double(const_init_multi),
                                  C.c_double(const_init_chi2), dx.ctypes.data, C.c_int(stride), ok.ctypes.data, chi2.ctypes.data,
                                  dof.ctypes.data, nid.ctypes.data, cpn.ctypes.data, used.ctypes.data)
        if rc != 0 and raise_on_error:
            raise OvpError(rc, "ovp_plane_init")
        return dict(dx=dx[:npl], ok=ok[:npl].astype(bool), chi2=chi2[:npl], dof=dof[:npl], new_ids=nid[:npl], cp=cpn[:npl],
                    used=used[: self.n_feats].astype(bool), rc=rc)

    def plane_init_general(self, opts: UpdateOpts, plane_of_feat, cp, const_init_multi, const_init_chi2, sc=None, feats=None,
                           uv=None, clone_idx=None, cam_idx=None, n_meas=None, p_FinG=None, plane_of_gen=None, raise_on_error=True):
        """ovp_plane_init_general: init_vio_plane's core in one device pass over the uploaded batch's on-plane features and those of
        a general batch (any camera, long tracks), given as in plane_update_general; None / empty = no general features.
        Returns plane_init's dict plus gen_used [bool] and rc."""
        if sc is not None:
            sel = np.asarray(feats, dtype=np.int64)
            uv, clone_idx, n_meas, p_FinG = sc.uv[sel], sc.clone_idx[sel], sc.n_meas[sel], sc.p_FinG[sel]
            cam_idx = sc.cam_idx[sel] if "cam_idx" in sc else None
            if plane_of_gen is None:
                plane_of_gen = sc.plane_id[sel]
        if uv is None or len(uv) == 0:
            gb = GeneralBatch(0, 0, None, None, None, None, None)
            pog = np.zeros(1, dtype=np.int32)
        else:
            gb = self._general_batch(uv, clone_idx, cam_idx, n_meas, p_FinG)
            pog = np.ascontiguousarray(plane_of_gen, dtype=np.int32)
            assert pog.shape[0] == gb.n_feats
        GF = gb.n_feats
        plane_of_feat = np.ascontiguousarray(plane_of_feat, dtype=np.int32)
        cp = np.ascontiguousarray(cp, dtype=np.float64)
        npl = int(cp.shape[0])
        sid = -np.ones(max(npl, 1), dtype=np.int32)
        stride = self.n_state_max
        dx = np.zeros((max(npl, 1), stride))
        ok = np.zeros(max(npl, 1), dtype=np.uint8)
        chi2 = np.zeros(max(npl, 1))
        dof = np.zeros(max(npl, 1), dtype=np.int32)
        nid = np.zeros(max(npl, 1), dtype=np.int32)
        cpn = np.zeros((max(npl, 1), 3))
        used = np.zeros(max(self.n_feats, 1), dtype=np.uint8)
        gused = np.zeros(max(GF, 1), dtype=np.uint8)
        pb = PlaneBatch(npl, plane_of_feat.ctypes.data, cp.ctypes.data, cp.ctypes.data, sid.ctypes.data)
        rc = lib().ovp_plane_init_general(self._h, C.byref(opts), C.byref(pb), C.c_double(const_init_multi),
                                          C.c_double(const_init_chi2), dx.ctypes.data, C.c_int(stride), ok.ctypes.data,
                                          chi2.ctypes.data, dof.ctypes.data, nid.ctypes.data, cpn.ctypes.data, used.ctypes.data,
                                          C.byref(gb), pog.ctypes.data, gused.ctypes.data)
        if rc != 0 and raise_on_error:
            raise OvpError(rc, "ovp_plane_init_general")
        return dict(dx=dx[:npl], ok=ok[:npl].astype(bool), chi2=chi2[:npl], dof=dof[:npl], new_ids=nid[:npl], cp=cpn[:npl],
                    used=used[: self.n_feats].astype(bool), gen_used=gused[:GF].astype(bool), rc=rc)

    def ekf_update(self, H, col_ids, res):
        """StateHelper::EKFUpdate with a dense H (rows x cols) and per-column state ids."""
        H = np.asfortranarray(H, dtype=np.float64)
        res = np.ascontiguousarray(res, dtype=np.float64)
        col_ids = np.ascontiguousarray(col_ids, dtype=np.int32)
        n = self.cov_size()
        dx = np.zeros(n)
        info = UpdateInfo()
        _chk(lib().ovp_ekf_update(self._h, H.ctypes.data, H.shape[0], H.shape[1], H.shape[0], col_ids.ctypes.data,
                                  res.ctypes.data, dx.ctypes.data, C.byref(info)), "ovp_ekf_update")
        return dx, info

    def slam_update(self, opts: UpdateOpts, uv, clone_idx, n_meas, p_FinG, p_FinG_fej, landmark_id, plane_state_id=None, cp=None,
                    cp_fej=None, pre=None, raise_on_error=True):
        """ovp_slam_update (UpdaterSLAM::update on the device).  pre: optional list with one entry per landmark, None (rows built
        on the device) or (H [rows x cols], col_ids [cols], res [rows]) for a block the host built.
        Returns dict(dx, status [L] (0 rejected / 1 accepted / 2 accepted without its plane), chi2 [L], info, rc)."""
        sb, keep = self._slam_batch(uv, clone_idx, n_meas, p_FinG, p_FinG_fej, landmark_id, plane_state_id, cp, cp_fej, pre)
        return self._slam_call("ovp_slam_update", sb, opts, raise_on_error)

    def slam_update_general(self, opts: UpdateOpts, uv, clone_idx, cam_idx, n_meas, p_FinG, p_FinG_fej, landmark_id, plane_state_id=None,
                            cp=None, cp_fej=None, pre=None, raise_on_error=True):
        """ovp_slam_update_general: slam_update with the camera of every observation (cam_idx [L, max_meas]), every camera's tables
        from cameras_upload.  Same results."""
        sb, keep = self._slam_batch(uv, clone_idx, n_meas, p_FinG, p_FinG_fej, landmark_id, plane_state_id, cp, cp_fej, pre)
        L, M = sb.n_landmarks, sb.max_meas
        cam = np.ascontiguousarray(cam_idx, dtype=np.int32).reshape(L, M) if L else np.zeros((0, M), np.int32)
        return self._slam_call("ovp_slam_update_general", sb, opts, raise_on_error, cam)

    def _slam_call(self, fn, sb, opts, raise_on_error, cam=None):
        L = sb.n_landmarks
        n = self.cov_size()
        dx = np.zeros(n)
        status = np.zeros(max(L, 1), dtype=np.uint8)
        chi2 = np.zeros(max(L, 1))
        info = UpdateInfo()
        args = (self._h, C.byref(opts), C.byref(sb)) + ((cam.ctypes.data,) if cam is not None else ()) + (
            dx.ctypes.data, status.ctypes.data, chi2.ctypes.data, C.byref(info))
        rc = getattr(lib(), fn)(*args)
        if raise_on_error:
            _chk(rc, fn)
        return dict(dx=dx, status=status[:L], chi2=chi2[:L], info=info, rc=rc)

    @staticmethod
    def _slam_batch(uv, clone_idx, n_meas, p_FinG, p_FinG_fej, landmark_id, plane_state_id=None, cp=None, cp_fej=None, pre=None):
        n_meas = np.ascontiguousarray(n_meas, dtype=np.int32)
        L = int(n_meas.shape[0])
        uv = np.ascontiguousarray(uv, dtype=np.float32)
        uv = uv.reshape(L, -1, 2) if L else uv.reshape(0, 1, 2)
        M = uv.shape[1]
        ci = np.ascontiguousarray(clone_idx, dtype=np.int32).reshape(L, M)
        p = np.ascontiguousarray(p_FinG, dtype=np.float64).reshape(L, 3)
        pf = np.ascontiguousarray(p_FinG_fej, dtype=np.float64).reshape(L, 3)
        lm = np.ascontiguousarray(landmark_id, dtype=np.int32)
        sb = SlamBatch()
        sb.n_landmarks, sb.max_meas = L, M
        sb.uv, sb.clone_idx, sb.n_meas = uv.ctypes.data, ci.ctypes.data, n_meas.ctypes.data
        sb.p_FinG, sb.p_FinG_fej, sb.landmark_id = p.ctypes.data, pf.ctypes.data, lm.ctypes.data
        keep = [uv, ci, p, pf, lm]
        if plane_state_id is not None:
            ps = np.ascontiguousarray(plane_state_id, dtype=np.int32)
            cpa = np.ascontiguousarray(cp, dtype=np.float64).reshape(L, 3)
            cpf = np.ascontiguousarray(cp_fej, dtype=np.float64).reshape(L, 3)
            sb.plane_state_id, sb.cp, sb.cp_fej = ps.ctypes.data, cpa.ctypes.data, cpf.ctypes.data
            keep += [ps, cpa, cpf]
        if pre is not None and any(e is not None for e in pre):
            pr = np.zeros(L, dtype=np.int32)
            pc = np.zeros(L, dtype=np.int32)
            hh, ii = [], []
            for l, e in enumerate(pre):
                if e is None:
                    continue
                H, ids, res = e
                H = np.asfortranarray(H, dtype=np.float64)
                pr[l], pc[l] = H.shape
                hh += [H.ravel(order="F"), np.asarray(res, dtype=np.float64).ravel()]
                ii.append(np.asarray(ids, dtype=np.int32).ravel())
            ph = np.ascontiguousarray(np.concatenate(hh))
            pi = np.ascontiguousarray(np.concatenate(ii))
            sb.pre_rows, sb.pre_cols, sb.pre_H, sb.pre_ids = pr.ctypes.data, pc.ctypes.data, ph.ctypes.data, pi.ctypes.data
            keep += [pr, pc, ph, pi]
        sb._keep = keep
        keep.append(n_meas)
        return sb, keep

    def slam_delayed_init(self, opts: UpdateOpts, uv, clone_idx, n_meas, p_FinG, raise_on_error=True):
        """ovp_slam_delayed_init: the candidate loop of UpdaterSLAM::delayed_init on the device.  Returns dict(ok [L], chi2 [L],
        new_id [L], delta_init [L,3], dx [L, stride] in the final column layout, rc)."""
        n_meas = np.ascontiguousarray(n_meas, dtype=np.int32)
        L = int(n_meas.shape[0])
        uv = np.ascontiguousarray(uv, dtype=np.float32).reshape(L, -1, 2)
        M = uv.shape[1]
        ci = np.ascontiguousarray(clone_idx, dtype=np.int32).reshape(L, M)
        p = np.ascontiguousarray(p_FinG, dtype=np.float64).reshape(L, 3)
        fb = FeatureBatch(L, M, uv.ctypes.data, ci.ctypes.data, n_meas.ctypes.data, p.ctypes.data)
        stride = self.cov_size() + 3 * L
        ok = np.zeros(max(L, 1), dtype=np.uint8)
        chi2 = np.zeros(max(L, 1))
        nid = -np.ones(max(L, 1), dtype=np.int32)
        dl = np.zeros((max(L, 1), 3))
        dx = np.zeros((max(L, 1), stride))
        rc = lib().ovp_slam_delayed_init(self._h, C.byref(opts), C.byref(fb), ok.ctypes.data, chi2.ctypes.data, nid.ctypes.data,
                                         dl.ctypes.data, dx.ctypes.data, stride)
        if raise_on_error:
            _chk(rc, "ovp_slam_delayed_init")
        return dict(ok=ok[:L].astype(bool), chi2=chi2[:L], new_id=nid[:L], delta_init=dl[:L], dx=dx[:L], rc=rc)

    def slam_delayed_init_general(self, opts: UpdateOpts, uv, clone_idx, cam_idx, n_meas, p_FinG, raise_on_error=True):
        """ovp_slam_delayed_init_general: slam_delayed_init with the camera of every observation (cam_idx [L, max_meas]), every
        camera's tables from cameras_upload (and updated on the device by every accepted candidate).  Same results."""
        gb = self._general_batch(uv, clone_idx, cam_idx, n_meas, p_FinG)
        L = gb.n_feats
        stride = self.cov_size() + 3 * L
        ok = np.zeros(max(L, 1), dtype=np.uint8)
        chi2 = np.zeros(max(L, 1))
        nid = -np.ones(max(L, 1), dtype=np.int32)
        dl = np.zeros((max(L, 1), 3))
        dx = np.zeros((max(L, 1), stride))
        rc = lib().ovp_slam_delayed_init_general(self._h, C.byref(opts), C.byref(gb), ok.ctypes.data, chi2.ctypes.data, nid.ctypes.data,
                                                 dl.ctypes.data, dx.ctypes.data, stride)
        if raise_on_error:
            _chk(rc, "ovp_slam_delayed_init_general")
        return dict(ok=ok[:L].astype(bool), chi2=chi2[:L], new_id=nid[:L], delta_init=dl[:L], dx=dx[:L], rc=rc)

    def slam_delayed_init_planes(self, opts: UpdateOpts, uv, clone_idx, n_meas, p_FinG, cam_idx=None, plane_of_cand=None,
                                 plane_state_id=None, cp=None, cp_fej=None, p_FinG_noplane=None, raise_on_error=True):
        """ovp_slam_delayed_init_planes: the device candidate loop with the point-on-plane rows of candidates on planes of the state
        and the fallback without them decided on the device.  cam_idx None = camera 0's rows (tables of state_upload), else the
        general rows (cameras_upload).  plane_of_cand [L]: 0 = none, else 1-based slot into plane_state_id / cp / cp_fej; without
        planes (plane_state_id None) the call is the plane-free loop.  Returns dict(status [L] 0 / 1 / 2, ok, chi2, new_id,
        delta_init, dx, rc)."""
        gb = self._general_batch(uv, clone_idx, cam_idx, n_meas, p_FinG)
        if cam_idx is None:
            gb.cam_idx = None
        L = gb.n_feats
        keep = []
        dpl = None
        if plane_state_id is not None:
            sid = np.ascontiguousarray(plane_state_id, dtype=np.int32).reshape(-1)
            cpv = np.ascontiguousarray(cp, dtype=np.float64).reshape(-1, 3)
            cpf = None if cp_fej is None else np.ascontiguousarray(cp_fej, dtype=np.float64).reshape(-1, 3)
            poc = np.ascontiguousarray(np.zeros(L) if plane_of_cand is None else plane_of_cand, dtype=np.int32).reshape(-1)
            pnp = None if p_FinG_noplane is None else np.ascontiguousarray(p_FinG_noplane, dtype=np.float64).reshape(L, 3)
            keep = [sid, cpv, cpf, poc, pnp]
            dpl = DinitPlanes(int(sid.shape[0]), sid.ctypes.data, cpv.ctypes.data, None if cpf is None else cpf.ctypes.data,
                              poc.ctypes.data, None if pnp is None else pnp.ctypes.data)
        stride = self.cov_size() + 3 * L
        st = np.zeros(max(L, 1), dtype=np.uint8)
        chi2 = np.zeros(max(L, 1))
        nid = -np.ones(max(L, 1), dtype=np.int32)
        dl = np.zeros((max(L, 1), 3))
        dx = np.zeros((max(L, 1), stride))
        rc = lib().ovp_slam_delayed_init_planes(self._h, C.byref(opts), C.byref(gb), None if dpl is None else C.byref(dpl),
                                                st.ctypes.data, chi2.ctypes.data, nid.ctypes.data, dl.ctypes.data, dx.ctypes.data, stride)
        del keep
        if raise_on_error:
            _chk(rc, "ovp_slam_delayed_init_planes")
        return dict(status=st[:L].copy(), ok=st[:L] > 0, chi2=chi2[:L], new_id=nid[:L], delta_init=dl[:L], dx=dx[:L], rc=rc)

    def plane_table_download(self, n_planes):
        """The device plane table of the last slam_delayed_init_planes, as its commits left it: (cp [n, 3], cp_fej [n, 3], id [n])."""
        tab = self.debug_read("dinit_planes", (n_planes, 8))
        return tab[:, 0:3].copy(), tab[:, 3:6].copy(), tab[:, 6].astype(np.int64)

    def camera_tables_download(self, n_cams):
        """The device's camera tables: (camera 0's of state_upload [20], the n_cams cameras of cameras_upload [n_cams, 20]); layout
        [R_ItoC row-major (9) | p_IinC (3) | intrinsics (8)]."""
        return self.debug_read("cal", (20,)), self.debug_read("gen_cal", (n_cams, 20))

    def cov_initialize(self, Hx_init, H_up, col_ids, H_Linv, R_init, res_up, r_iso, chi2_threshold, do_update=True):
        """StateHelper::initialize downstream of its Givens split as one device sequence (state/StateHelper.cpp:448-487):
        returns (accepted, chi2, dx); the covariance grows by k = Hx_init.shape[0] columns when accepted."""
        Hx = np.asfortranarray(Hx_init, dtype=np.float64)
        k, cols = Hx.shape
        Hu = np.asfortranarray(H_up, dtype=np.float64).reshape(-1, cols, order="F") if H_up is not None else np.zeros((0, cols))
        rup = Hu.shape[0]
        Hi = np.asfortranarray(H_Linv, dtype=np.float64)
        Ri = np.asfortranarray(R_init, dtype=np.float64)
        ru = np.ascontiguousarray(res_up if res_up is not None else np.zeros(0), dtype=np.float64)
        ids = np.ascontiguousarray(col_ids, dtype=np.int32)
        dx = np.zeros(self.cov_size() + k)
        acc = C.c_int(0)
        chi2 = C.c_double(0.0)
        _chk(lib().ovp_cov_initialize(self._h, Hx.ctypes.data, Hu.ctypes.data if rup else None, k, rup, cols, ids.ctypes.data,
                                      Hi.ctypes.data, Ri.ctypes.data, ru.ctypes.data if rup else None, float(r_iso),
                                      float(chi2_threshold), 1 if do_update else 0, C.byref(acc), C.byref(chi2), dx.ctypes.data),
             "ovp_cov_initialize")
        return bool(acc.value), chi2.value, dx

    def triangulate(self, uv_norm, opts=None):
        """ovp_triangulate on the uploaded batch; returns dict(p_FinG [F,3], ok [F])."""
        o = opts if opts is not None else triang_defaults()
        uvn = np.ascontiguousarray(uv_norm, dtype=np.float32)
        F = self.n_feats
        p = np.zeros((max(F, 1), 3))
        ok = np.zeros(max(F, 1), dtype=np.uint8)
        _chk(lib().ovp_triangulate(self._h, C.byref(o), uvn.ctypes.data, p.ctypes.data, ok.ctypes.data), "ovp_triangulate")
        return dict(p_FinG=p[:F], ok=ok[:F].astype(bool))

    def plane_fitting(self, feat_start, p_FinG, min_inlier_num, max_cond, shuffle_variant=0):
        """ovp_plane_fitting: RANSAC + refit for a batch of planes; returns dict(abcd [P,4], inlier [F], ok [P])."""
        fs = np.ascontiguousarray(feat_start, dtype=np.int32)
        pts = np.ascontiguousarray(p_FinG, dtype=np.float64)
        P = len(fs) - 1
        b = PlaneFitBatch(P, fs.ctypes.data_as(C.POINTER(C.c_int)), pts.ctypes.data_as(C.POINTER(C.c_double)),
                          int(min_inlier_num), float(max_cond), int(shuffle_variant))
        abcd = np.zeros((max(P, 1), 4))
        inl = np.zeros(max(len(pts), 1), dtype=np.uint8)
        ok = np.zeros(max(P, 1), dtype=np.uint8)
        _chk(lib().ovp_plane_fitting(self._h, C.byref(b), abcd.ctypes.data, inl.ctypes.data, ok.ctypes.data),
             "ovp_plane_fitting")
        return dict(abcd=abcd[:P], inlier=inl[: len(pts)].astype(bool), ok=ok[:P].astype(bool))

    def plane_optimize(self, problems):
        """ovp_plane_optimize on a list of per-plane problems (dicts as ov_plane_amd.synth.make_planefit_problem returns;
        sigma / pose fields are taken from the first).  Returns a list of dict(ok, cp, p_FinG, kept, iterations)."""
        P = len(problems)
        fs = np.zeros(P + 1, dtype=np.int32)
        for k, pb in enumerate(problems):
            fs[k + 1] = fs[k] + int(pb["n_feats"])
        p0 = np.ascontiguousarray(np.concatenate([np.asarray(pb["p_FinG"], dtype=np.float64).reshape(-1, 3) for pb in problems]))
        n_obs = np.ascontiguousarray(np.concatenate([np.asarray(pb["n_obs"], dtype=np.int32) for pb in problems]))
        obs_start = np.zeros(len(n_obs), dtype=np.int32)
        obs_start[1:] = np.cumsum(n_obs)[:-1]
        cat = lambda key, w: np.ascontiguousarray(
            np.concatenate([np.asarray(pb[key], dtype=np.float64).reshape(-1, w) for pb in problems]))
        uv, Rc, pc = cat("uv_norm", 2), cat("R_GtoC", 9), cat("p_CinG", 3)
        cp = np.ascontiguousarray(np.array([pb["cp"] for pb in problems], dtype=np.float64))
        fix = np.ascontiguousarray(np.array([1 if pb["fix_plane"] else 0 for pb in problems], dtype=np.uint8))
        b = PlaneOptBatch()
        b.n_planes = P
        b.feat_start = fs.ctypes.data_as(C.POINTER(C.c_int))
        b.p_FinG = p0.ctypes.data_as(C.POINTER(C.c_double))
        b.obs_start = obs_start.ctypes.data_as(C.POINTER(C.c_int))
        b.n_obs = n_obs.ctypes.data_as(C.POINTER(C.c_int))
        b.n_obs_total = int(n_obs.sum())
        b.uv_norm = uv.ctypes.data_as(C.POINTER(C.c_double))
        b.R_GtoC = Rc.ctypes.data_as(C.POINTER(C.c_double))
        b.p_CinG = pc.ctypes.data_as(C.POINTER(C.c_double))
        b.cp = cp.ctypes.data_as(C.POINTER(C.c_double))
        b.fix_plane = fix.ctypes.data_as(C.POINTER(C.c_ubyte))
        f = problems[0]
        b.sigma_px_norm = float(f["sigma_px_norm"])
        b.sigma_c = float(f["sigma_c"])
        b.R_GtoI = (C.c_double * 9)(*np.asarray(f["R_GtoI"], dtype=np.float64).reshape(-1))
        b.p_IinG = (C.c_double * 3)(*np.asarray(f["p_IinG"], dtype=np.float64))
        b.R_ItoC = (C.c_double * 9)(*np.asarray(f["R_ItoC"], dtype=np.float64).reshape(-1))
        b.p_IinC = (C.c_double * 3)(*np.asarray(f["p_IinC"], dtype=np.float64))
        F = int(fs[-1])
        cp_out = np.zeros((P, 3))
        p_out = np.zeros((max(F, 1), 3))
        kept = np.zeros(max(F, 1), dtype=np.uint8)
        ok = np.zeros(P, dtype=np.uint8)
        its = np.zeros(P, dtype=np.int32)
        _chk(lib().ovp_plane_optimize(self._h, C.byref(b), cp_out.ctypes.data, p_out.ctypes.data, kept.ctypes.data,
                                      ok.ctypes.data, its.ctypes.data), "ovp_plane_optimize")
        return [dict(ok=bool(ok[k]), cp=cp_out[k].copy(), p_FinG=p_out[fs[k]:fs[k + 1]].copy(),
                     kept=kept[fs[k]:fs[k + 1]].astype(bool), iterations=int(its[k])) for k in range(P)]

    def plane_fit_refine(self, feat_start, uv_norm, clone_idx, cam_idx, n_meas, p_FinG, cp, fix_plane, min_inlier_num, max_cond,
                         sigma_px_norm, sigma_c, R_GtoI, p_IinG, n_clones, n_cams, refine=True, shuffle_variant=0,
                         raise_on_error=True):
        """ovp_plane_fit_refine: RANSAC fit and joint refinement of every plane of a frame in one device pass, over observations
        of any camera and tracks of any length (the poses come from the resident clone / camera tables).  Plane k owns the
        features [feat_start[k], feat_start[k+1]).  Returns dict(fit_ok [P], abcd [P,4], ok [P], cp [P,3], iterations [P],
        inlier [F], kept [F], p_FinG [F,3], poses [n_clones, n_cams, 12], rc)."""
        fs = np.ascontiguousarray(feat_start, dtype=np.int32)
        P = len(fs) - 1
        uvn = np.ascontiguousarray(uv_norm, dtype=np.float32)
        gb = self._general_batch(uvn, clone_idx, cam_idx, n_meas, p_FinG)
        F = gb.n_feats
        cpa = np.ascontiguousarray(np.asarray(cp, dtype=np.float64).reshape(-1, 3))
        fix = np.ascontiguousarray(np.asarray(fix_plane).astype(np.uint8))
        assert len(cpa) == P and len(fix) == P
        pin = PlaneFrontIn(P, fs.ctypes.data, cpa.ctypes.data, fix.ctypes.data, int(min_inlier_num), float(max_cond),
                           int(shuffle_variant), 1 if refine else 0, float(sigma_px_norm), float(sigma_c))
        pin.R_GtoI = (C.c_double * 9)(*np.asarray(R_GtoI, dtype=np.float64).reshape(-1))
        pin.p_IinG = (C.c_double * 3)(*np.asarray(p_IinG, dtype=np.float64).reshape(-1))
        r = dict(fit_ok=np.zeros(max(P, 1), dtype=np.uint8), abcd=np.zeros((max(P, 1), 4)), ok=np.zeros(max(P, 1), dtype=np.uint8),
                 cp=np.zeros((max(P, 1), 3)), iterations=np.zeros(max(P, 1), dtype=np.int32), inlier=np.zeros(max(F, 1), dtype=np.uint8),
                 kept=np.zeros(max(F, 1), dtype=np.uint8), p_FinG=np.zeros((max(F, 1), 3)),
                 poses=np.zeros((max(int(n_clones), 1), max(int(n_cams), 1), 12)))
        pout = PlaneFrontOut(*[r[k].ctypes.data for k in ("fit_ok", "abcd", "ok", "cp", "iterations", "inlier", "kept", "p_FinG",
                                                           "poses")])
        rc = lib().ovp_plane_fit_refine(self._h, C.byref(gb), uvn.ctypes.data, C.byref(pin), C.byref(pout))
        if rc != 0 and raise_on_error:
            raise OvpError(rc, "ovp_plane_fit_refine")
        return dict(fit_ok=r["fit_ok"][:P].astype(bool), abcd=r["abcd"][:P], ok=r["ok"][:P].astype(bool), cp=r["cp"][:P],
                    iterations=r["iterations"][:P], inlier=r["inlier"][:F].astype(bool), kept=r["kept"][:F].astype(bool),
                    p_FinG=r["p_FinG"][:F], poses=r["poses"], rc=rc)

    def debug_chol2(self, A, brow=None, add_identity=False, reps=0, piv_floor=0.0):
        """k_chol2 on a host matrix: dict(L [(n+1),(n+1)], z, y, piv, ms, rc).  piv_floor > 0: columns whose pivot falls below it
        are dropped (zero column in the factor, zero entry in z)."""
        lib().ovp_debug_chol2_floor.argtypes = [C.c_double]
        lib().ovp_debug_chol2_floor.restype = None
        lib().ovp_debug_chol2_floor(float(piv_floor))
        A = np.ascontiguousarray(A, dtype=np.float64)
        n = A.shape[0]
        nb = n + (1 if brow is not None else 0)
        L = np.zeros((nb, nb))
        z, y, piv = np.zeros(n), np.zeros(n), np.zeros(n)
        ms = C.c_float(0)
        b = None if brow is None else np.ascontiguousarray(brow, dtype=np.float64)
        f = lib().ovp_debug_chol2
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                      C.c_void_p, C.c_int, C.POINTER(C.c_float)]
        rc = f(self._h, A.ctypes.data, n, n, None if b is None else b.ctypes.data, int(add_identity), L.ctypes.data,
               z.ctypes.data, y.ctypes.data, piv.ctypes.data, int(reps), C.byref(ms))
        return dict(L=L, z=z, y=y, piv=piv, ms=ms.value, rc=rc)

    def sync(self):
        _chk(lib().ovp_sync(self._h), "ovp_sync")

    def stream_handle(self):
        """hipStream_t (as int) the context orders its work on; wrap it with torch.cuda.ExternalStream for collectives."""
        s = C.c_void_p()
        _chk(lib().ovp_ctx_stream(self._h, C.byref(s)), "ovp_ctx_stream")
        return int(s.value or 0)

    def timings_ms(self):
        t = np.zeros(4, dtype=np.float32)
        lib().ovp_last_timings(self._h, t.ctypes.data)
        return t

    def kernel_timer(self, enable=True, reset=False):
        ms, nl = C.c_float(0), C.c_int(0)
        lib().ovp_kernel_timer(self._h, int(enable), int(reset), C.byref(ms), C.byref(nl))
        return ms.value, nl.value

    def plane_kernel_timer(self, enable=True, reset=False):
        ms, nl = C.c_float(0), C.c_int(0)
        lib().ovp_plane_kernel_timer(self._h, int(enable), int(reset), C.byref(ms), C.byref(nl))
        return ms.value, nl.value

    def host_timing(self, reset=False):
        """Accumulated host clock of the update entry points (ms): plane loop entry -> first launch, entry -> last launch
        enqueued, wait for the device, calls; point update enqueue, wait, calls."""
        t = np.zeros(8)
        lib().ovp_host_timing(self._h, int(reset), t.ctypes.data)
        return dict(plane_pre_ms=t[0], plane_enqueue_ms=t[1], plane_wait_ms=t[2], plane_calls=int(t[3]),
                    point_enqueue_ms=t[4], point_wait_ms=t[5], point_calls=int(t[6]), plane_loop_device_ms=t[7])

    def debug_read(self, name, shape, dtype=np.float64):
        out = np.zeros(shape, dtype=dtype)
        nb = lib().ovp_debug_read(self._h, name.encode(), out.ctypes.data, out.nbytes)
        if nb < 0:
            raise OvpError(nb, "ovp_debug_read(%s)" % name)
        return out


class PreparedFrame:
    """A scene's arguments of ovp_state_upload / ovp_batch_upload / ovp_msckf_plane_update / ovp_msckf_update as prebuilt ctypes
    structs over persistent numpy buffers, and the output arrays of the two updates (see Context.prepared_frame)."""

    def __init__(self, ctx, sc, opts_plane, opts_point):
        self.ctx, self.sc = ctx, sc
        self.st = ctx.state_tables(sc)
        self.uv = np.ascontiguousarray(sc.uv, dtype=np.float32)
        self.clone_idx = np.ascontiguousarray(sc.clone_idx, dtype=np.int32)
        self.n_meas = np.ascontiguousarray(sc.n_meas, dtype=np.int32)
        self.p_FinG = np.ascontiguousarray(sc.p_FinG, dtype=np.float64)
        F = int(self.uv.shape[0])
        self.F = F
        self.fb = FeatureBatch(F, int(self.uv.shape[1]), self.uv.ctypes.data, self.clone_idx.ctypes.data, self.n_meas.ctypes.data,
                               self.p_FinG.ctypes.data)
        self.opts_plane, self.opts_point = opts_plane, opts_point
        self.npl = int(np.asarray(sc.plane_state_id).shape[0]) if sc.cp.shape[0] > 0 else 0
        n = int(sc.N)
        self.n = n
        if self.npl:
            self.plane_of_feat = np.ascontiguousarray(sc.plane_id, dtype=np.int32)
            self.cp = np.ascontiguousarray(sc.cp, dtype=np.float64)
            self.cp_fej = np.ascontiguousarray(sc.cp_fej, dtype=np.float64)
            self.sid = np.ascontiguousarray(sc.plane_state_id, dtype=np.int32)
            self.pb = PlaneBatch(self.npl, self.plane_of_feat.ctypes.data, self.cp.ctypes.data, self.cp_fej.ctypes.data, self.sid.ctypes.data)
        self.pl_dx = np.zeros((max(self.npl, 1), n))
        self.pl_ok = np.zeros(max(self.npl, 1), dtype=np.uint8)
        self.pl_chi2 = np.zeros(max(self.npl, 1))
        self.pl_dof = np.zeros(max(self.npl, 1), dtype=np.int32)
        self.pl_used = np.zeros(max(F, 1), dtype=np.uint8)
        self.dx = np.zeros(n)
        self.acc = np.zeros(max(F, 1), dtype=np.uint8)
        self.chi2 = np.zeros(max(F, 1))
        self.info = UpdateInfo()
        self._L = lib()

    def upload(self):
        """ovp_state_upload + ovp_batch_upload of the frame (the H2D copies of the timed step)."""
        h = self.ctx._h
        _chk(self._L.ovp_state_upload(h, C.byref(self.st)), "ovp_state_upload")
        _chk(self._L.ovp_batch_upload(h, C.byref(self.fb)), "ovp_batch_upload")
        self.ctx.n_feats = self.F

    def upload_state(self):
        """ovp_state_upload alone (the pose / calibration tables: a plane loop commits its corrections to them)."""
        _chk(self._L.ovp_state_upload(self.ctx._h, C.byref(self.st)), "ovp_state_upload")

    def plane_update(self):
        rc = self._L.ovp_msckf_plane_update(self.ctx._h, C.byref(self.opts_plane), C.byref(self.pb), self.pl_dx.ctypes.data,
                                            self.pl_ok.ctypes.data, self.pl_chi2.ctypes.data, self.pl_dof.ctypes.data, self.pl_used.ctypes.data)
        if rc != 0:
            raise OvpError(rc, "ovp_msckf_plane_update")

    def point_update(self):
        rc = self._L.ovp_msckf_update(self.ctx._h, C.byref(self.opts_point), self.dx.ctypes.data, self.acc.ctypes.data,
                                      self.chi2.ctypes.data, C.byref(self.info))
        if rc != 0:
            raise OvpError(rc, "ovp_msckf_update")

    def results(self):
        """(plane dict or None, point dict) shaped like Context.plane_update / Context.msckf_update, from the last calls."""
        pl = None
        if self.npl:
            pl = dict(dx=self.pl_dx[:self.npl].copy(), ok=self.pl_ok[:self.npl].astype(bool), chi2=self.pl_chi2[:self.npl].copy(),
                      dof=self.pl_dof[:self.npl].copy(), used=self.pl_used[:self.F].astype(bool), rc=0)
        pt = dict(dx=self.dx.copy(), accepted=self.acc[:self.F].astype(bool), chi2=self.chi2[:self.F].copy(), info=self.info, rc=0)
        return pl, pt
