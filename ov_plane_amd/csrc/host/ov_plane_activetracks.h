// Host mirror of the active-track half of ov_plane::VioManager (core/VioManager.h: active_tracks_time, active_tracks_posinG,
// active_tracks_uvd, active_feat_linsys_*): retriangulate() is VioManager::retriangulate_active_tracks
// (core/VioManagerHelper.cpp:220-418) on the tracked points of one frame - no images - and get_active_tracks() the reference's
// accessor (core/VioManager.h).  The per-feature linear systems live in the device context (ovp_active_tracks_*); this class reads
// the poses, the calibration and the SLAM landmarks out of the State, hands the frame over and keeps the two maps.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <memory>
#include <unordered_map>
#include <vector>

#include "ov_plane_host.h"
#include "ovplane_hip.h"

namespace ov_plane {

class ActiveTracks {
 public:
  // ok() is false when the context has no room for the table
  explicit ActiveTracks(ovp_ctx *gpu) : _gpu(gpu) { _rc = ovp_active_tracks_create(gpu); }
  ~ActiveTracks() {
    if (_rc == 0) ovp_active_tracks_destroy(_gpu);
  }
  ActiveTracks(const ActiveTracks &) = delete;
  ActiveTracks &operator=(const ActiveTracks &) = delete;
  bool ok() const { return _rc == 0; }
  // camera 0's image size (the reference reads it from _cam_intrinsics_cameras.at(0), :399-400; the mirror's State has none)
  void set_image_size(int width, int height) { _w = width, _h = height; }

  // One frame at the clone of `time`: sensor_ids in the caller's order, and per entry the tracked ids, raw pixels uv [2n] and
  // undistorted normalised coordinates uv_norm [2n] of that camera (get_last_ids / get_last_obs, :240-241).  Returns 0 or an
  // OVP_E_* code (OVP_E_STATE without a clone at `time`, :227); after a failure the maps are empty.
  int retriangulate(const std::shared_ptr<State> &state, double time, const ov_core::FeatureInitializerOptions &featinit,
                    const std::vector<size_t> &sensor_ids, const std::vector<std::vector<size_t>> &ids,
                    const std::vector<std::vector<float>> &uv, const std::vector<std::vector<float>> &uv_norm) {
    active_tracks_posinG.clear();  // :235-236
    active_tracks_uvd.clear();
    active_tracks_time = -1;
    if (_rc) return _rc;
    auto clone_it = state->_clones_IMU.find(time);
    if (clone_it == state->_clones_IMU.end()) return OVP_E_STATE;
    if (sensor_ids.size() != ids.size() || ids.size() != uv.size() || ids.size() != uv_norm.size()) return OVP_E_ARG;
    const double *R_GtoI = clone_it->second->Rot(), *p_IinG = clone_it->second->pos();
    ovp_active_tracks_in in = {};
    std::vector<int32_t> cam_idx;
    std::vector<int64_t> feat_id;
    std::vector<float> px;
    std::vector<double> uvn;
    size_t n_cams = 1;
    for (size_t cam : sensor_ids) n_cams = std::max(n_cams, cam + 1);
    if (n_cams > (size_t)OVP_MAX_CAMERAS) return OVP_E_CAPACITY;
    std::vector<double> R_GtoC(9 * n_cams, 0.0), p_CinG(3 * n_cams, 0.0);
    for (size_t s = 0; s < sensor_ids.size(); ++s) {
      const size_t cam = sensor_ids[s];
      if (uv[s].size() != 2 * ids[s].size() || uv_norm[s].size() != 2 * ids[s].size() || !state->_calib_IMUtoCAM.count(cam)) return OVP_E_ARG;
      camera_pose(state->_calib_IMUtoCAM.at(cam)->Rot(), state->_calib_IMUtoCAM.at(cam)->pos(), R_GtoI, p_IinG, &R_GtoC[9 * cam], &p_CinG[3 * cam]);
      for (size_t i = 0; i < ids[s].size(); ++i) {
        cam_idx.push_back((int32_t)cam);
        feat_id.push_back((int64_t)ids[s][i]);
        px.push_back(uv[s][2 * i]), px.push_back(uv[s][2 * i + 1]);
        uvn.push_back(uv_norm[s][2 * i]), uvn.push_back(uv_norm[s][2 * i + 1]);  // (undistort_cv returns f32: the values stay f32-rounded)
      }
    }
    in.n_obs = (int)feat_id.size();
    in.cam_idx = cam_idx.data(), in.feat_id = feat_id.data(), in.uv = px.data(), in.uv_norm = uvn.data();
    in.n_cams = (int)n_cams, in.R_GtoC = R_GtoC.data(), in.p_CinG = p_CinG.data();
    memcpy(in.R_ItoC0, state->_calib_IMUtoCAM.at(0)->Rot(), sizeof(in.R_ItoC0));
    memcpy(in.p_IinC0, state->_calib_IMUtoCAM.at(0)->pos(), sizeof(in.p_IinC0));
    memcpy(in.R_GtoI, R_GtoI, sizeof(in.R_GtoI));
    memcpy(in.p_IinG, p_IinG, sizeof(in.p_IinG));
    in.width = _w, in.height = _h;
    in.min_dist = featinit.min_dist, in.max_dist = featinit.max_dist, in.max_cond_number = featinit.max_cond_number;
    // :342-357 the landmarks of the state
    const size_t nl = state->_features_SLAM.size();
    std::vector<int64_t> sid;
    std::vector<double> sxyz(3 * nl), aR(9 * nl, 0.0), ap(3 * nl, 0.0), cR(9 * nl, 0.0), cp(3 * nl, 0.0);
    std::vector<uint8_t> srel(nl, 0);
    for (const auto &feat : state->_features_SLAM) {
      const size_t j = sid.size();
      sid.push_back((int64_t)feat.second->_featid);
      feat.second->get_xyz(false, &sxyz[3 * j]);
      if (ov_type::LandmarkRepresentation::is_relative_representation(feat.second->_feat_representation)) {
        auto anchor = state->_clones_IMU.find(feat.second->_anchor_clone_timestamp);
        if (anchor == state->_clones_IMU.end() || !state->_calib_IMUtoCAM.count((size_t)feat.second->_anchor_cam_id)) return OVP_E_STATE;
        srel[j] = 1;
        memcpy(&aR[9 * j], anchor->second->Rot(), 9 * sizeof(double));
        memcpy(&ap[3 * j], anchor->second->pos(), 3 * sizeof(double));
        memcpy(&cR[9 * j], state->_calib_IMUtoCAM.at((size_t)feat.second->_anchor_cam_id)->Rot(), 9 * sizeof(double));
        memcpy(&cp[3 * j], state->_calib_IMUtoCAM.at((size_t)feat.second->_anchor_cam_id)->pos(), 3 * sizeof(double));
      }
    }
    in.n_slam = (int)nl;
    in.slam_id = sid.data(), in.slam_xyz = sxyz.data(), in.slam_relative = srel.data();
    in.slam_anchor_R_GtoI = aR.data(), in.slam_anchor_p_IinG = ap.data(), in.slam_anchor_R_ItoC = cR.data(), in.slam_anchor_p_IinC = cp.data();
    const size_t cap = feat_id.size() + nl + 1;
    std::vector<int64_t> oid(cap);
    std::vector<uint8_t> oflag(cap);
    std::vector<double> op(3 * cap), ouvd(3 * cap);
    ovp_active_tracks_out out = {};
    out.cap = (int)cap, out.ids = oid.data(), out.flags = oflag.data(), out.p_FinG = op.data(), out.uvd = ouvd.data();
    const int rc = ovp_active_tracks_update(_gpu, &in, &out);
    if (rc) return rc;
    memcpy(last_pose, in.R_ItoC0, 9 * sizeof(double)), memcpy(last_pose + 9, in.p_IinC0, 3 * sizeof(double));
    memcpy(last_pose + 12, in.R_GtoI, 9 * sizeof(double)), memcpy(last_pose + 21, in.p_IinG, 3 * sizeof(double));
    active_tracks_time = time;  // :228
    for (int i = 0; i < out.n; ++i) {
      if (oflag[i] & 1) active_tracks_posinG[(size_t)oid[i]] = {op[3 * i], op[3 * i + 1], op[3 * i + 2]};
      if (oflag[i] & 2) active_tracks_uvd[(size_t)oid[i]] = {ouvd[3 * i], ouvd[3 * i + 1], ouvd[3 * i + 2]};
    }
    return 0;
  }

  // VioManager::get_active_tracks (core/VioManager.h)
  void get_active_tracks(double &time, std::unordered_map<size_t, std::array<double, 3>> &feat_posinG,
                         std::unordered_map<size_t, std::array<double, 3>> &feat_tracks_uvd) const {
    time = active_tracks_time;
    feat_posinG = active_tracks_posinG;
    feat_tracks_uvd = active_tracks_uvd;
  }

  // the frame was not retriangulated (no points handed over for it): the maps are empty and say so
  void clear() {
    active_tracks_time = -1;
    active_tracks_posinG.clear();
    active_tracks_uvd.clear();
  }

  double active_tracks_time = -1;
  double last_pose[24] = {};  // what the last frame was projected with: [R_ItoC | p_IinC] of camera 0, [R_GtoI | p_IinG] of its clone
  std::unordered_map<size_t, std::array<double, 3>> active_tracks_posinG;
  std::unordered_map<size_t, std::array<double, 3>> active_tracks_uvd;

 private:
  // :262-263 R_GtoCi = R_ItoC R_GtoI, p_CiinG = p_IinG - R_GtoCi^T p_IinC (row-major)
  static void camera_pose(const double *Ric, const double *pic, const double *Rgi, const double *pig, double *Rgc, double *pcg) {
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) Rgc[3 * r + c] = Ric[3 * r] * Rgi[c] + Ric[3 * r + 1] * Rgi[3 + c] + Ric[3 * r + 2] * Rgi[6 + c];
    for (int c = 0; c < 3; ++c) pcg[c] = pig[c] - (Rgc[c] * pic[0] + Rgc[3 + c] * pic[1] + Rgc[6 + c] * pic[2]);
  }
  ovp_ctx *_gpu;
  int _rc = 0;
  int _w = 752, _h = 480;  // ext the simulator's default camera
};

}  // namespace ov_plane
