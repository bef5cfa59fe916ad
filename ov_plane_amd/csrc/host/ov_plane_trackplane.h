// Host mirror of the detection half of ov_plane::TrackPlane (track_plane/TrackPlane.h): feed_plane_detection() is
// perform_plane_detection_monocular (track_plane/TrackPlane.cpp:580-1121) on the tracked points of one frame - no images - and
// get_feature2plane() the reference's accessor.  The per-feature history and the plane maps live in the detector of the device
// context (ovp_plane_detector_*); this class hands it the frame, triangulates the points that have a position (Delaunay,
// ov_plane_delaunay.h, where the reference calls CDT) and reads the map back.  With set_device_delaunay the triangulation is the
// detector's own, on the device behind its first call: no has_est round trip and no triangles to hand over.
#pragma once
#include <array>
#include <cstdint>
#include <map>
#include <set>
#include <vector>

#include "ov_plane_delaunay.h"
#include "ovplane_hip.h"

namespace ov_plane {

class TrackPlane {
 public:
  // options: TrackPlaneOptions by name (ovp_trackplane_defaults).  ok() is false when the context has no room for a detector.
  TrackPlane(ovp_ctx *gpu, const ovp_trackplane_opts &options) : _gpu(gpu) { _rc = ovp_plane_detector_create(gpu, &options); }
  ~TrackPlane() {
    if (_rc == 0) ovp_plane_detector_destroy(_gpu);
  }
  TrackPlane(const TrackPlane &) = delete;
  TrackPlane &operator=(const TrackPlane &) = delete;
  bool ok() const { return _rc == 0; }
  // StateOptions::gpu_device_delaunay
  int set_device_delaunay(bool on) {
    if (_rc) return _rc;
    const int rc = ovp_plane_detector_set_device_delaunay(_gpu, on ? 1 : 0);
    if (rc == 0) _device_delaunay = on;
    return rc;
  }

  // the camera pose of the newest clone (hist_state and hist_calib of the reference, TrackPlane.cpp:612-624, already combined):
  // R_GtoC row-major, p_CinG
  void feed_pose(double time, const double *R_GtoC, const double *p_CinG) {
    _pose_time = time;
    for (int k = 0; k < 9; ++k) _R[k] = R_GtoC[k];
    for (int k = 0; k < 3; ++k) _p[k] = p_CinG[k];
    _have_pose = true;
  }

  // One frame: ids, pixel positions uv [2n] and their undistorted normalised coordinates uv_norm [2n].  Returns 0, an OVP_E_* code
  // (OVP_E_CAPACITY above OVP_DET_MAX_POINTS points: nothing touched), or OVP_E_STATE without the pose of `time`
  // (TrackPlane.cpp:605-606 returns there as well).
  int feed_plane_detection(double time, const std::vector<size_t> &ids, const std::vector<float> &uv, const std::vector<float> &uv_norm) {
    if (_rc) return _rc;
    if (!_have_pose || _pose_time != time) return OVP_E_STATE;
    const int n = (int)ids.size();
    if (uv.size() != 2 * ids.size() || uv_norm.size() != 2 * ids.size()) return OVP_E_ARG;
    if (n == 0) return 0;
    std::vector<int64_t> id64(ids.begin(), ids.end());
    std::vector<double> uvn(uv_norm.begin(), uv_norm.end());  // (undistort_cv returns f32: the values stay f32-rounded)
    if (_device_delaunay) {
      const int rc = ovp_plane_detect_triangulate(_gpu, n, id64.data(), uv.data(), uvn.data(), _R, _p, nullptr, nullptr);
      return rc ? rc : ovp_plane_detect_planes(_gpu, 0, nullptr);
    }
    std::vector<uint8_t> has(n);
    int rc = ovp_plane_detect_triangulate(_gpu, n, id64.data(), uv.data(), uvn.data(), _R, _p, has.data(), nullptr);
    if (rc) return rc;
    std::vector<float> vxy;
    for (int i = 0; i < n; ++i)
      if (has[i] & 1) vxy.push_back(uv[2 * i]), vxy.push_back(uv[2 * i + 1]);
    std::vector<std::array<int, 3>> tris;
    ovp_delaunay_host((int)vxy.size() / 2, vxy.data(), tris);
    static const int32_t none[3] = {0, 0, 0};
    return ovp_plane_detect_planes(_gpu, (int)tris.size(), tris.empty() ? none : &tris[0][0]);
  }

  std::map<size_t, size_t> get_feature2plane() const {
    std::map<size_t, size_t> out;
    int n = 0;
    if (_rc || ovp_plane_detector_map(_gpu, nullptr, nullptr, 0, &n) || n == 0) return out;
    std::vector<int64_t> ids(n), pl(n);
    if (ovp_plane_detector_map(_gpu, ids.data(), pl.data(), n, &n)) return out;
    for (int i = 0; i < n; ++i) out[(size_t)ids[i]] = (size_t)pl[i];
    return out;
  }

  // history of planes which have been merged into others (TrackPlane.h:145-149)
  std::map<size_t, std::set<size_t>> get_plane2oldplane() const {
    std::map<size_t, std::set<size_t>> out;
    int n = 0;
    if (_rc || ovp_plane_detector_merges(_gpu, nullptr, 0, &n) || n == 0) return out;
    std::vector<int64_t> pairs(2 * (size_t)n);
    if (ovp_plane_detector_merges(_gpu, pairs.data(), n, &n)) return out;
    for (int i = 0; i < n; ++i) out[(size_t)pairs[2 * i]].insert((size_t)pairs[2 * i + 1]);
    return out;
  }

 private:
  ovp_ctx *_gpu;
  int _rc = 0;
  bool _have_pose = false, _device_delaunay = false;
  double _pose_time = 0.0, _R[9], _p[3];
};

}  // namespace ov_plane
