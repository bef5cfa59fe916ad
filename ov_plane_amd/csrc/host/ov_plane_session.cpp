// A filter session over the host mirror: the slice of ov_plane::VioManager::do_feature_propagate_update (core/VioManager.cpp:
// 330-930) that sequences the updaters around a camera frame - propagate and clone (:348), marginalise the SLAM landmarks that
// lost their track (:463-485), plane initialisation (:583-588), MSCKF(+plane) update (:670), SLAM update (:676-688), SLAM
// delayed initialisation (:692), anchor change (:861), marginalisation of the oldest clone (:864-872).  Which track is used
// when (lost / about to be marginalised / long enough to become a landmark, :360-506) is the caller's tracker-side bookkeeping
// (ov_plane_amd/closed_loop.py); the covariance lives on the device for the whole session.
//
// C interface (ctypes): ovph_session_open / _feed_imu / _step / _close.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <set>
#include <vector>

#include <chrono>
#include <fstream>

#include "ov_plane_host.h"
#include "ov_plane_io.h"
#include "ov_plane_trackplane.h"
#include "ov_plane_activetracks.h"

using namespace ov_plane;
using namespace ov_type;

namespace {
struct Session {
  std::shared_ptr<State> state;
  std::shared_ptr<Propagator> prop;
  std::unique_ptr<UpdaterMSCKF> msckf;
  std::unique_ptr<UpdaterSLAM> slam;
  std::unique_ptr<UpdaterPlane> plane;
  std::unique_ptr<UpdaterZeroVelocity> zupt;              // only with try_zupt (VioManagerOptions::try_zupt)
  std::shared_ptr<ov_core::FeatureDatabase> db;           // raw tracks of the last frames: the disparity test of the detector
  int C = 0, plane_mode = 0;
  // StateOptions::gpu_plane_detection: the detector and the tracked points of the frame about to be stepped
  std::unique_ptr<TrackPlane> track;
  double track_time = -1.0;
  std::vector<size_t> track_ids;
  std::vector<float> track_uv, track_uvn;
  int detect_rc = 0, detect_planar = 0;
  // StateOptions::gpu_active_tracks: VioManager's active tracks of the last step, from the same hand-over
  std::unique_ptr<ActiveTracks> active;
  int active_rc = 0;
  ov_core::FeatureInitializerOptions featinit;  // VioManagerOptions::featinit_options
  // what a run of the reference leaves behind (ros/ROSVisualizerHelper.cpp:152-302, core/VioManager.cpp:110-118, 911-927)
  std::ofstream of_est, of_std, of_gt, of_timing;
  bool files = false;
};
double seconds_since(const std::chrono::steady_clock::time_point &t0) {
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}
}  // namespace

// Window of C clones (oldest first, 1 / cam_rate apart, the last one cam_dt before t_state), IMU value x16 at t_state, prior P
// (N = 30 + 6 C, State.cpp order: IMU | dt | extrinsics | intrinsics | clones).  opts_i: use_rk4, do_fej, plane_mode (0 none,
// 1 MSCKF plane constraints, 2 + planes into the state), plane_min_feat, max_slam_features, feat_rep_slam.
// opts_d: sigma_w, sigma_a, sigma_wb, sigma_ab, gravity, sigma_px, chi2_mult (MSCKF), chi2_mult (SLAM), sigma_c, cam_dt.
extern "C" void *ovph_session_open(int C, const double *clone_q, const double *clone_p, const double *calib_q, const double *calib_p,
                                   const double *intr, const double *imu_x16, double calib_dt, int N, const double *P, double t_state,
                                   const int *opts_i, const double *opts_d) {
  auto s = std::make_unique<Session>();
  s->C = C;
  s->plane_mode = opts_i[2];
  StateOptions so;
  so.use_rk4_integration = opts_i[0] != 0;
  so.do_fej = opts_i[1] != 0;
  so.do_calib_camera_pose = so.do_calib_camera_intrinsics = so.do_calib_camera_timeoffset = true;
  so.max_clone_size = C;
  so.max_slam_features = opts_i[4];
  so.feat_rep_slam = (LandmarkRepresentation::Representation)opts_i[5];
  so.max_state_size = N + 16 + 3 * 16 + 3 * std::max(opts_i[4], 0);
  so.max_features = 4096;
  if (s->plane_mode) {
    so.use_plane_constraint = so.use_plane_constraint_msckf = true;
    so.use_plane_constraint_slamu = so.use_plane_constraint_slamd = true;
    so.use_plane_slam_feats = s->plane_mode == 2;
    so.sigma_constraint = opts_d[8];
    so.plane_init_min_feat = so.plane_msckf_min_feat = opts_i[3];
  }
  auto state = std::make_shared<State>(so);
  s->state = state;
  {
    VectorXd v(7, 1), iv(8, 1);
    for (int k = 0; k < 4; ++k) v(k) = calib_q[k];
    for (int k = 0; k < 3; ++k) v(4 + k) = calib_p[k];
    state->_calib_IMUtoCAM.at(0)->set_value(v);
    state->_calib_IMUtoCAM.at(0)->set_fej(v);
    for (int k = 0; k < 8; ++k) iv(k) = intr[k];
    state->_cam_intrinsics.at(0)->set_value(iv);
    state->_cam_intrinsics.at(0)->set_fej(iv);
  }
  const double w0[3] = {0, 0, 0}, cam_dt = opts_d[9];
  for (int i = 0; i < C; ++i) {
    VectorXd a(7, 1);
    for (int k = 0; k < 4; ++k) a(k) = clone_q[4 * i + k];
    for (int k = 0; k < 3; ++k) a(4 + k) = clone_p[3 * i + k];
    state->_imu->pose()->set_value(a);
    state->_imu->pose()->set_fej(a);
    state->_timestamp = t_state - cam_dt * (C - i);
    StateHelper::augment_clone(state, w0);
  }
  if (state->max_covariance_size() != N) return nullptr;
  VectorXd x(16, 1), dtv(1, 1);
  for (int k = 0; k < 16; ++k) x(k) = imu_x16[k];
  state->_imu->set_value(x);
  state->_imu->set_fej(x);
  dtv(0) = calib_dt;
  state->_calib_dt_CAMtoIMU->set_value(dtv);
  state->_calib_dt_CAMtoIMU->set_fej(dtv);
  state->_timestamp = t_state;
  {
    std::vector<std::shared_ptr<Type>> all;
    all.push_back(state->_imu);
    all.push_back(state->_calib_dt_CAMtoIMU);
    all.push_back(state->_calib_IMUtoCAM.at(0));
    all.push_back(state->_cam_intrinsics.at(0));
    for (auto &c : state->_clones_IMU) all.push_back(c.second);
    MatrixXd Pm(N, N);
    memcpy(Pm.data(), P, sizeof(double) * (size_t)N * N);
    StateHelper::set_initial_covariance(state, Pm, all);
  }
  NoiseManager nm;
  nm.sigma_w = opts_d[0];
  nm.sigma_a = opts_d[1];
  nm.sigma_wb = opts_d[2];
  nm.sigma_ab = opts_d[3];
  s->prop = std::make_shared<Propagator>(nm, opts_d[4]);
  UpdaterOptions um, us;
  um.sigma_pix = us.sigma_pix = opts_d[5];
  um.chi2_multipler = opts_d[6];
  us.chi2_multipler = opts_d[7];
  ov_core::FeatureInitializerOptions fio;
  s->msckf = std::make_unique<UpdaterMSCKF>(um, fio);
  s->slam = std::make_unique<UpdaterSLAM>(us, us, fio);
  s->plane = std::make_unique<UpdaterPlane>(um, fio);
  s->featinit = fio;
  return s.release();
}

extern "C" void ovph_session_close(void *h) { delete static_cast<Session *>(h); }

// Zero-velocity updates (core/VioManager.cpp:311-331): zupt4 = max velocity, noise multiplier, max disparity, chi2 multiplier.
// The IMU readings fed afterwards also reach the detector; ovph_session_feed_tracks hands it the raw pixel tracks of a frame.
extern "C" int ovph_session_enable_zupt(void *h, const double *zupt4, const double *sigmas4, double gravity_mag) {
  auto *s = static_cast<Session *>(h);
  NoiseManager nm;
  nm.sigma_w = sigmas4[0];
  nm.sigma_a = sigmas4[1];
  nm.sigma_wb = sigmas4[2];
  nm.sigma_ab = sigmas4[3];
  UpdaterOptions uo;
  uo.chi2_multipler = zupt4[3];
  s->db = std::make_shared<ov_core::FeatureDatabase>();
  s->zupt = std::make_unique<UpdaterZeroVelocity>(uo, nm, s->db, s->prop, gravity_mag, zupt4[0], zupt4[1], zupt4[2]);
  return 0;
}

extern "C" int ovph_session_feed_tracks(void *h, double frame_time, int n, const long long *fid, const float *uv) {
  auto *s = static_cast<Session *>(h);
  if (!s->db) return 0;
  for (int i = 0; i < n; ++i) s->db->update_feature((size_t)fid[i], frame_time, 0, uv[2 * i], uv[2 * i + 1], 0.f, 0.f);
  // the detector looks one frame back: forget what is older than a few frames
  auto &all = s->db->get_internal_data();
  for (auto it = all.begin(); it != all.end();) {
    auto &f = *it->second;
    while (!f.timestamps.empty() && f.timestamps.front() < frame_time - 1.0) {
      f.timestamps.erase(f.timestamps.begin());
      f.uvs.erase(f.uvs.begin(), f.uvs.begin() + 2);
      if (f.uvs_norm.size() >= 2) f.uvs_norm.erase(f.uvs_norm.begin(), f.uvs_norm.begin() + 2);
    }
    if (f.timestamps.empty()) it = all.erase(it);
    else ++it;
  }
  return 0;
}

// StateOptions::gpu_plane_detection on: opts = ovp_trackplane_opts (NULL: the defaults).  From then on a frame whose tracked points
// were handed over by ovph_session_feed_plane_tracks takes its feature -> plane map from the detector, not from `plane` of the step.
extern "C" int ovph_session_enable_plane_detection(void *h, const ovp_trackplane_opts *opts) {
  auto *s = static_cast<Session *>(h);
  ovp_trackplane_opts o;
  ovp_trackplane_defaults(&o);
  if (opts) o = *opts;
  if (!s->state->gpu()) return -31;
  s->track.reset();
  s->track = std::make_unique<TrackPlane>(s->state->gpu(), o);
  if (!s->track->ok()) {
    s->track.reset();
    return -31;
  }
  s->state->_options.gpu_plane_detection = true;
  if (s->state->_options.gpu_device_delaunay && s->track->set_device_delaunay(true)) return -31;
  return 0;
}

// StateOptions::gpu_device_delaunay: the detector (now, or when ovph_session_enable_plane_detection makes it) triangulates on the device
extern "C" int ovph_session_set_device_delaunay(void *h, int on) {
  auto *s = static_cast<Session *>(h);
  s->state->_options.gpu_device_delaunay = on != 0;
  if (s->track && s->track->set_device_delaunay(on != 0)) return -31;
  return 0;
}

// StateOptions::gpu_active_tracks on: from then on a step whose tracked points were handed over by ovph_session_feed_plane_tracks for
// its timestamp runs VioManager::retriangulate_active_tracks (core/VioManager.cpp:757) on the device, between the SLAM delayed
// initialisation and the anchor change, and ovph_session_active_tracks returns its maps.  Camera 0's image size is the simulator's
// (752 x 480) unless ovph_session_set_image_size says otherwise.
extern "C" int ovph_session_enable_active_tracks(void *h) {
  auto *s = static_cast<Session *>(h);
  if (!s->state->gpu()) return -31;
  s->active.reset();
  s->active = std::make_unique<ActiveTracks>(s->state->gpu());
  if (!s->active->ok()) {
    s->active.reset();
    return -31;
  }
  s->state->_options.gpu_active_tracks = true;
  return 0;
}

// The ids of the planes the state holds, ascending (State::_features_PLANE); returns their number (at most `cap` are written).
extern "C" int ovph_session_plane_ids(void *h, int cap, long long *ids) {
  auto *s = static_cast<Session *>(h);
  int n = 0;
  for (const auto &p : s->state->_features_PLANE) {
    if (n < cap) ids[n] = (long long)p.first;
    ++n;
  }
  return n;
}

// StateOptions::gpu_batched_retire on (or off again): from the next step on marginalize_slam and merge_planes_and_marginalize retire
// their variables in one device pass each.
extern "C" int ovph_session_enable_batched_retire(void *h, int on) {
  auto *s = static_cast<Session *>(h);
  if (!s->state->gpu()) return -31;
  s->state->_options.gpu_batched_retire = on != 0;
  return 0;
}

// StateOptions::gpu_zupt on (or off again): from the next ovph_session_try_zupt on, UpdaterZeroVelocity::try_update gates and
// updates in one device pass (ovp_zupt_update).
extern "C" int ovph_session_enable_gpu_zupt(void *h, int on) {
  auto *s = static_cast<Session *>(h);
  if (!s->state->gpu()) return -31;
  s->state->_options.gpu_zupt = on != 0;
  return 0;
}

// StateOptions::gpu_propagate on (or off again): from the next step on, Propagator::propagate_and_clone integrates, propagates and
// clones in one device pass (ovp_propagate_and_clone).
extern "C" int ovph_session_enable_gpu_propagate(void *h, int on) {
  auto *s = static_cast<Session *>(h);
  if (!s->state->gpu()) return -31;
  s->state->_options.gpu_propagate = on != 0;
  return 0;
}

extern "C" int ovph_session_set_image_size(void *h, int width, int height) {
  auto *s = static_cast<Session *>(h);
  if (!s->active || width < 1 || height < 1) return -21;
  s->active->set_image_size(width, height);
  return 0;
}

// VioManager::get_active_tracks after the last step: *n = entries (also when cap is smaller), ids [cap], flags [cap] (bit 0: in
// active_tracks_posinG, bit 1: in active_tracks_uvd), p [3 cap], uvd [3 cap], ascending id.  Returns 0; 1 when the last step did
// not run the stage (option off, or no points handed over for its timestamp: the maps are empty); an OVP_E_* code when it failed.
extern "C" int ovph_session_active_tracks(void *h, int cap, long long *ids, unsigned char *flags, double *p, double *uvd, int *n) {
  auto *s = static_cast<Session *>(h);
  if (!n || cap < 0 || (cap > 0 && (!ids || !flags || !p || !uvd))) return -21;
  *n = 0;
  if (!s->active) return 1;
  if (s->active_rc) return s->active_rc;
  std::map<size_t, int> all;
  for (const auto &e : s->active->active_tracks_posinG) all[e.first] |= 1;
  for (const auto &e : s->active->active_tracks_uvd) all[e.first] |= 2;
  *n = (int)all.size();
  int i = 0;
  for (const auto &e : all) {
    if (i >= cap) break;
    ids[i] = (long long)e.first, flags[i] = (unsigned char)e.second;
    for (int k = 0; k < 3; ++k) {
      p[3 * i + k] = (e.second & 1) ? s->active->active_tracks_posinG.at(e.first)[k] : 0.0;
      uvd[3 * i + k] = (e.second & 2) ? s->active->active_tracks_uvd.at(e.first)[k] : 0.0;
    }
    ++i;
  }
  return s->active->active_tracks_time < 0 ? 1 : 0;
}

// the pose the last retriangulated step projected with: [R_ItoC 9 | p_IinC 3] of camera 0, [R_GtoI 9 | p_IinG 3] of the newest clone
extern "C" int ovph_session_active_tracks_pose(void *h, double *out24) {
  auto *s = static_cast<Session *>(h);
  if (!s->active || !out24) return -21;
  memcpy(out24, s->active->last_pose, sizeof(s->active->last_pose));
  return 0;
}

// every point tracked into the frame at frame_time (not only the tracks the step uses): ids, pixels, normalised coordinates
extern "C" int ovph_session_feed_plane_tracks(void *h, double frame_time, int n, const long long *fid, const float *uv,
                                              const float *uv_norm) {
  auto *s = static_cast<Session *>(h);
  if (n < 0 || (n > 0 && (!fid || !uv || !uv_norm))) return -21;
  s->track_time = frame_time;
  s->track_ids.assign(fid, fid + n);
  s->track_uv.assign(uv, uv + 2 * (size_t)n);
  s->track_uvn.assign(uv_norm, uv_norm + 2 * (size_t)n);
  return 0;
}

// [0] return code of the last frame's detection, [1] features of the last step that the detector put on a plane, [2] entries of
// the detector's map
extern "C" int ovph_session_plane_detection_info(void *h, int *out3) {
  auto *s = static_cast<Session *>(h);
  out3[0] = s->detect_rc, out3[1] = s->detect_planar, out3[2] = s->track ? (int)s->track->get_feature2plane().size() : 0;
  return 0;
}

// VioManager.cpp:311-331: returns 1 when the platform was found standing still and the zero-velocity update was applied - the
// frame is then NOT cloned and ovph_session_step must not be called for it; 0 otherwise.  x16 / posecov36 as in the step.
extern "C" int ovph_session_try_zupt(void *h, double frame_time, double *x16, double *posecov36, double *chi2) {
  auto *s = static_cast<Session *>(h);
  if (!s->zupt) return 0;
  const bool did = s->zupt->try_update(s->state, frame_time);
  if (chi2) *chi2 = s->zupt->last_chi2();
  if (did) {
    memcpy(x16, s->state->_imu->value().data(), 16 * sizeof(double));
    std::vector<std::shared_ptr<Type>> po;
    po.push_back(s->state->_imu->pose());
    MatrixXd Pp = StateHelper::get_marginal_covariance(s->state, po);
    memcpy(posecov36, Pp.data(), 36 * sizeof(double));
  }
  return did ? 1 : 0;
}

// Output files of a run, in the reference's formats: state estimate / standard deviation / groundtruth (one line per frame,
// written by ovph_session_step when it is handed the true state) and the timing CSV.  Empty or null path = not written.
extern "C" int ovph_session_open_files(void *h, const char *est, const char *stdev, const char *gt, const char *timing) {
  auto *s = static_cast<Session *>(h);
  auto open = [](std::ofstream &f, const char *p) {
    if (p && *p) f.open(p, std::ofstream::out | std::ofstream::trunc);
    return !(p && *p) || f.is_open();
  };
  if (!open(s->of_est, est) || !open(s->of_std, stdev) || !open(s->of_gt, gt) || !open(s->of_timing, timing)) return -1;
  // header line as the visualizer writes it when it opens the files (ros/ROS1Visualizer.cpp:158-167)
  const char *hdr = "# timestamp(s) q p v bg ba cam_imu_dt num_cam cam0_k cam0_d cam0_rot cam0_trans .... etc";
  if (s->of_est.is_open()) s->of_est << hdr << std::endl;
  if (s->of_std.is_open()) s->of_std << hdr << std::endl;
  if (s->of_gt.is_open()) s->of_gt << hdr << std::endl;
  if (s->of_timing.is_open()) write_timing_header(s->of_timing, s->state->_options);
  s->files = true;
  return 0;
}

extern "C" int ovph_session_feed_imu(void *h, int n, const double *imu7) {
  auto *s = static_cast<Session *>(h);
  for (int i = 0; i < n; ++i) {
    ov_core::ImuData d;
    d.timestamp = imu7[7 * i];
    for (int k = 0; k < 3; ++k) {
      d.wm[k] = imu7[7 * i + 1 + k];
      d.am[k] = imu7[7 * i + 4 + k];
    }
    s->prop->feed_imu(d, s->state->_timestamp);
    if (s->zupt) s->zupt->feed_imu(d, s->state->_timestamp);
  }
  return 0;
}

// One camera frame.  Features f = 0..F-1: id gfid[f], kind[f] (0 MSCKF track, 1 new measurement(s) of a SLAM landmark in the
// state, 2 long track that should become a SLAM landmark), n_meas[f] measurements uv / uv_norm [F][M][2] taken in the window
// slots clone_slot [F][M] (0 = oldest of the C + 1 clones after cloning, C = this frame), plane[f] (0 = free point).
// Outputs: counts[0..5] = MSCKF features left after the update (passed the gates), SLAM landmarks updated, initialised,
// marginalised because their track ended, landmarks in the state, planes in the state; IMU value [16] and pose covariance [36]
// after the frame; ids of the landmarks in the state (slam_ids, at most slam_cap).
// truth (or NULL) feeds the groundtruth file: [0..16] t, q, p, v, bg, ba of the simulator at this frame, [17] true camera time
// offset, [18..25] true intrinsics, [26..32] true extrinsics (q_ItoC, p_IinC).
// Tracker-side plane bookkeeping (core/VioManager.cpp:513-534): active_planes[n_active] = ids of the planes the tracker currently
// sees (the distinct values of its feature -> plane map over ALL live tracks, not only the ones used in this frame),
// merge_pairs[2 * n_merge] = (surviving id, old id) pairs of planes the front end merged.  With active_planes != NULL the step runs
// StateHelper::merge_planes_and_marginalize like the reference does every frame: merged planes are fused (3-row update) and
// planes nobody observes any more leave the state.  n_active < 0 = no bookkeeping handed over: every plane is kept (the caller
// guarantees they stay observed); n_active = 0 = the tracker sees no plane at all (every plane leaves) - the pointer may then be NULL.
extern "C" int ovph_session_step2(void *h, double frame_time, int F, int M, const float *uv, const float *uv_norm, const int *clone_slot,
                                  const int *n_meas, const long long *gfid, const int *kind, const int *plane, int *counts,
                                  double *x16, double *posecov36, int slam_cap, long long *slam_ids, const double *truth17,
                                  int n_active, const long long *active_planes, int n_merge, const long long *merge_pairs);

extern "C" int ovph_session_step(void *h, double frame_time, int F, int M, const float *uv, const float *uv_norm, const int *clone_slot,
                                 const int *n_meas, const long long *gfid, const int *kind, const int *plane, int *counts,
                                 double *x16, double *posecov36, int slam_cap, long long *slam_ids, const double *truth17) {
  return ovph_session_step2(h, frame_time, F, M, uv, uv_norm, clone_slot, n_meas, gfid, kind, plane, counts, x16, posecov36, slam_cap,
                            slam_ids, truth17, -1, nullptr, 0, nullptr);
}

extern "C" int ovph_session_step2(void *h, double frame_time, int F, int M, const float *uv, const float *uv_norm, const int *clone_slot,
                                  const int *n_meas, const long long *gfid, const int *kind, const int *plane, int *counts,
                                  double *x16, double *posecov36, int slam_cap, long long *slam_ids, const double *truth17,
                                  int n_active, const long long *active_planes, int n_merge, const long long *merge_pairs) {
  auto *s = static_cast<Session *>(h);
  auto &state = s->state;
  // the inputs are checked BEFORE the state is touched: a rejected call must leave the filter where it was (a propagated state
  // with an extra clone could not be stepped again: "Propagation called again at same timestep" is fatal)
  {
    const int n_window = (int)state->_clones_IMU.size() + 1;  // clones after this frame's cloning
    for (int f = 0; f < F; ++f) {
      if (n_meas[f] < 0 || n_meas[f] > M) return -21;
      for (int q = 0; q < n_meas[f]; ++q) {
        const int sl = clone_slot[(size_t)f * M + q];
        if (sl < 0 || sl >= n_window) return -21;
      }
      if (kind[f] < 0 || kind[f] > 2) return -23;
      if (kind[f] == 1 && !state->_features_SLAM.count((size_t)gfid[f])) return -22;  // the caller's bookkeeping is out of step
    }
  }
  TimingRecord tr;
  const auto t_start = std::chrono::steady_clock::now();
  auto t_prev = t_start;
  auto lap = [&](double &field) {
    field = seconds_since(t_prev);
    t_prev = std::chrono::steady_clock::now();
  };
  s->prop->propagate_and_clone(state, frame_time);  // VioManager.cpp:348
  lap(tr.prop);
  std::vector<double> times;
  for (auto &c : state->_clones_IMU) times.push_back(c.first);
  std::vector<std::shared_ptr<ov_core::Feature>> f_msckf, f_slam_up, f_slam_new, fextra, fused;
  std::map<size_t, size_t> feat2plane;
  std::set<size_t> seen_landmarks;
  for (int f = 0; f < F; ++f) {
    auto ft = std::make_shared<ov_core::Feature>();
    ft->featid = (size_t)gfid[f];
    for (int q = 0; q < n_meas[f]; ++q) {
      const int sl = clone_slot[(size_t)f * M + q];
      if (sl < 0 || sl >= (int)times.size()) return -21;
      ft->timestamps.push_back(times[sl]);
      for (int c = 0; c < 2; ++c) {
        ft->uvs.push_back(uv[((size_t)f * M + q) * 2 + c]);
        ft->uvs_norm.push_back(uv_norm[((size_t)f * M + q) * 2 + c]);
      }
    }
    if (s->plane_mode && plane && plane[f] > 0) feat2plane[ft->featid] = (size_t)plane[f];
    if (kind[f] == 1) {
      if (!state->_features_SLAM.count(ft->featid)) return -22;  // the caller's bookkeeping is out of step with the state
      seen_landmarks.insert(ft->featid);
      ft->uvs_norm.clear();  // a landmark needs no triangulation
      f_slam_up.push_back(ft);
    } else if (kind[f] == 2) {
      f_slam_new.push_back(ft);
    } else {
      f_msckf.push_back(ft);
    }
  }
  // the tracked points were handed over for THIS frame (the detector below consumes the hand-over; the active tracks share it)
  const bool have_tracks = s->track_time == frame_time;
  bool detected = false;
  std::map<size_t, std::set<size_t>> detected_merges;
  if (state->_options.gpu_plane_detection && s->track && s->track_time != frame_time) {
    // the option is on and no tracked points were handed over for THIS frame: the caller's map is not a substitute
    s->detect_rc = OVP_E_STATE;
    s->detect_planar = 0;
    feat2plane.clear();
  }
  if (state->_options.gpu_plane_detection && s->track && s->track_time == frame_time) {
    // the detector runs on the newest clone (TrackPlane.cpp:612-624) and its map stands in for the caller's
    const auto &clone = state->_clones_IMU.at(state->_timestamp);
    const double *Rgi = clone->Rot(), *pig = clone->pos(), *Ric = state->_calib_IMUtoCAM.at(0)->Rot(),
                 *pic = state->_calib_IMUtoCAM.at(0)->pos();
    double Rgc[9], pcg[3];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) Rgc[3 * r + c] = Ric[3 * r] * Rgi[c] + Ric[3 * r + 1] * Rgi[3 + c] + Ric[3 * r + 2] * Rgi[6 + c];
    for (int c = 0; c < 3; ++c) pcg[c] = pig[c] - (Rgc[c] * pic[0] + Rgc[3 + c] * pic[1] + Rgc[6 + c] * pic[2]);
    s->track->feed_pose(frame_time, Rgc, pcg);
    s->detect_rc = s->track->feed_plane_detection(frame_time, s->track_ids, s->track_uv, s->track_uvn);
    feat2plane.clear();
    s->detect_planar = 0;
    if (s->plane_mode) {
      feat2plane = s->track->get_feature2plane();
      for (int f = 0; f < F; ++f) s->detect_planar += (int)feat2plane.count((size_t)gfid[f]);
    }
    s->track_time = -1.0;
    detected = s->detect_rc == 0 && s->plane_mode == 2;
    if (detected) detected_merges = s->track->get_plane2oldplane();
  }
  // VioManager.cpp:463-485 landmarks that were not tracked into this frame leave the state
  int n_marg = 0;
  for (auto &lm : state->_features_SLAM)
    if (!seen_landmarks.count(lm.first)) {
      lm.second->should_marg = true;
      ++n_marg;
    }
  StateHelper::marginalize_slam(state);
  // :513-534 planes the front end merged are fused, planes that are no longer observed leave the state
  if (detected) {
    // the detector's own bookkeeping: the planes of its map are the active ones, its merge history says which ids were fused
    StateHelper::merge_planes_and_marginalize(state, feat2plane, detected_merges);
  } else if (n_active >= 0 && s->plane_mode == 2) {
    std::map<size_t, size_t> f2p_active = feat2plane;
    size_t fake = (size_t)-1;  // ids that cannot collide with tracker ids: only the VALUES of the map are read
    for (int k = 0; k < n_active; ++k) f2p_active[fake--] = (size_t)active_planes[k];
    std::map<size_t, std::set<size_t>> plane2oldplane;
    for (int k = 0; k < n_merge; ++k) plane2oldplane[(size_t)merge_pairs[2 * k]].insert((size_t)merge_pairs[2 * k + 1]);
    StateHelper::merge_planes_and_marginalize(state, f2p_active, plane2oldplane);
  }
  {  // :487-500 a landmark that was flagged by a failed update is gone now although it is still tracked: its single new
     // measurement would be a delayed initialisation with one observation, which :112-118 of UpdaterSLAM.cpp drops
    std::vector<std::shared_ptr<ov_core::Feature>> still;
    for (auto &ft : f_slam_up)
      if (state->_features_SLAM.count(ft->featid)) still.push_back(ft);
    f_slam_up.swap(still);
  }
  // :543-600 planar candidates first try to initialise their planes
  if (s->plane_mode == 2) {
    std::vector<std::shared_ptr<ov_core::Feature>> fplane, finit_used, rest;
    for (auto &ft : f_msckf)
      if (feat2plane.count(ft->featid)) fplane.push_back(ft);
    s->plane->init_vio_plane(state, fplane, finit_used, feat2plane);
    std::set<size_t> used;
    for (auto &ft : finit_used) used.insert(ft->featid);
    for (auto &ft : f_msckf)
      if (!used.count(ft->featid)) rest.push_back(ft);
    f_msckf.swap(rest);
  }
  lap(tr.planeinit);
  if (getenv("OVP_SESSION_DEBUG"))
    fprintf(stderr, "[session] t=%.3f n=%d msckf=%zu slam_up=%zu slam_new=%zu landmarks=%zu cap=%d\n", frame_time,
            state->max_covariance_size(), f_msckf.size(), f_slam_up.size(), f_slam_new.size(), state->_features_SLAM.size(),
            state->_options.max_state_size);
  s->msckf->update(state, f_msckf, fextra, fused, feat2plane);  // :670
  lap(tr.msckf);
  const int n_up = (int)f_slam_up.size();
  s->slam->update(state, f_slam_up, feat2plane);                // :676-688
  lap(tr.slam_update);
  const size_t before = state->_features_SLAM.size();
  s->slam->delayed_init(state, f_slam_new, feat2plane);         // :692
  lap(tr.slam_delay);
  counts[0] = (int)f_msckf.size();
  counts[1] = n_up;
  counts[2] = (int)(state->_features_SLAM.size() - before);
  counts[3] = n_marg;
  if (state->_options.gpu_active_tracks && s->active) {  // :757 retriangulate_active_tracks; its time falls into tr.marg (rT7 -> rT8)
    if (have_tracks) {
      s->active_rc = s->active->retriangulate(state, state->_timestamp, s->featinit, {0}, {s->track_ids}, {s->track_uv}, {s->track_uvn});
      s->track_time = -1.0;
    } else {
      s->active->clear();
      s->active_rc = 0;
    }
  }
  s->slam->change_anchors(state);             // :861
  StateHelper::marginalize_old_clone(state);  // :864-872
  lap(tr.marg);
  tr.total = seconds_since(t_start);
  tr.timestamp_inI = state->_timestamp + state->_calib_dt_CAMtoIMU->value()(0);  // :911-914
  if (s->of_timing.is_open()) write_timing_row(s->of_timing, state->_options, tr);
  if (s->files && truth17 && (s->of_est.is_open() || s->of_std.is_open() || s->of_gt.is_open())) {
    SimTruth st;
    memcpy(st.state_gt, truth17, sizeof(st.state_gt));
    st.calib_camimu_dt = truth17[17];
    memcpy(st.intrinsics, truth17 + 18, sizeof(st.intrinsics));
    memcpy(st.extrinsics, truth17 + 26, sizeof(st.extrinsics));
    std::ofstream null_stream;
    ROSVisualizerHelper::sim_save_total_state_to_file(state, &st, s->of_est.is_open() ? s->of_est : null_stream,
                                                      s->of_std.is_open() ? s->of_std : null_stream,
                                                      s->of_gt.is_open() ? s->of_gt : null_stream);
  }
  counts[4] = (int)state->_features_SLAM.size();
  counts[5] = (int)state->_features_PLANE.size();
  memcpy(x16, state->_imu->value().data(), 16 * sizeof(double));
  {
    std::vector<std::shared_ptr<Type>> po;
    po.push_back(state->_imu->pose());
    MatrixXd Pp = StateHelper::get_marginal_covariance(state, po);
    memcpy(posecov36, Pp.data(), 36 * sizeof(double));
  }
  int k = 0;
  for (auto &lm : state->_features_SLAM)
    if (k < slam_cap) slam_ids[k++] = (long long)lm.first;
  return 0;
}
