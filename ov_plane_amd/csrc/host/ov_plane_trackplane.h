// Host mirror of the detection half of ov_plane::TrackPlane (track_plane/TrackPlane.h): feed_plane_detection() is
// perform_plane_detection_monocular (track_plane/TrackPlane.cpp:580-1121) on the tracked points of one frame - no images - and
// get_feature2plane() the reference's accessor.  The per-feature history and the plane maps live in the detector of the device
// context (ovp_plane_detector_*); this class hands it the frame, triangulates the points that have a position (Delaunay,
// ov_plane_delaunay.h, where the reference calls CDT) and reads the map back.  With set_device_delaunay the triangulation is the
// detector's own, on the device behind its first call: no has_est round trip and no triangles to hand over.
// The image half: feed_new_camera() is TrackPlane::feed_new_camera (:40-92) followed by the bookkeeping of feed_monocular
// (:505-567) minus detection and the epipolar check, perform_matching_klt() the cv::calcOpticalFlowPyrLK call of perform_matching
// (:1326-1330, :1352-1356); both pyramids live in the tracker of the device context (ovp_klt_*).  Detection is the caller's:
// add_points() seeds or tops up pts_last / ids_last.
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
    if (_klt_made) ovp_klt_destroy(_gpu);
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

  // ---- image front end ---------------------------------------------------------------------------------------------------------
  // TrackBase's pyr_levels (maxLevel: pyr_levels + 1 images), win_size, histogram_method (OVP_KLT_HIST_*) and the most points one
  // frame tracks; before the first image
  int set_klt_options(int pyr_levels, int win_size, int histogram_method, int max_points) {
    if (_klt_made) return OVP_E_STATE;
    _pyr_levels = pyr_levels, _win_size = win_size, _hist = histogram_method, _klt_max_points = max_points;
    return 0;
  }

  // the caller's detection (perform_detection_monocular, :1173-1297, is not built): points of the last image fed
  void add_points(const std::vector<size_t> &ids, const std::vector<float> &uv) {
    for (size_t i = 0; i < ids.size() && 2 * i + 1 < uv.size(); ++i) {
      _ids_last.push_back(ids[i]);
      _pts_last.push_back(uv[2 * i]), _pts_last.push_back(uv[2 * i + 1]);
    }
  }

  // :1326-1330 pts0 [2n] of the previous image into the current one, starting at pts1 [2n] (OPTFLOW_USE_INITIAL_FLOW); mask_klt [n]
  // is OpenCV's status, and pts1 is moved as :1352-1356 does.  Not here: the findFundamentalMat RANSAC of :1344 and, with it, the
  // "fewer than 10 points" return of :1320-1324, which exists for that RANSAC alone.
  int perform_matching_klt(const std::vector<float> &pts0, std::vector<float> &pts1, std::vector<uint8_t> &mask_klt) {
    if (pts0.size() != pts1.size() || (pts0.size() & 1)) return OVP_E_ARG;
    const int n = (int)pts0.size() / 2;
    mask_klt.assign(n, 0);
    if (n == 0) return 0;  // :1307-1309
    std::vector<float> out(2 * (size_t)n);
    const int rc = ovp_klt_track(_gpu, n, pts0.data(), pts1.data(), out.data(), mask_klt.data());
    if (rc == 0) pts1.swap(out);
    return rc;
  }

  // One camera image (8-bit, h rows of `stride` bytes) and its mask (h x w, NULL: none; a value above 127 masks the pixel):
  // :40-92 equalise and build the pyramid, then :514-567 track pts_last into it and keep a point unless x < 0, y < 0,
  // (int) x >= cols, (int) y >= rows, it lies in the mask, or its status is 0.  Returns 0 or an OVP_E_* code.
  int feed_new_camera(double time, const uint8_t *img, int w, int h, int stride, const uint8_t *mask = nullptr) {
    if (!_klt_made) {
      const int rc = ovp_klt_create(_gpu, w, h, _pyr_levels + 1, _win_size, _klt_max_points);
      if (rc) return rc;
      _klt_made = true, _klt_w = w, _klt_h = h;
    }
    if (w != _klt_w || h != _klt_h) return OVP_E_ARG;
    int rc = ovp_klt_feed_image(_gpu, img, stride, _hist);
    if (rc) return rc;
    _time_last = time;
    _match_pts.clear(), _match_mask.clear();
    if (++_n_images < 2 || _ids_last.empty()) return 0;
    std::vector<float> pts_new = _pts_last;  // :512 pts_left_new = pts_left_old
    rc = perform_matching_klt(_pts_last, pts_new, _match_mask);
    if (rc) return rc;
    _match_pts = pts_new;
    std::vector<float> good;
    std::vector<size_t> good_ids;
    for (size_t i = 0; i < _ids_last.size(); ++i) {
      const float x = pts_new[2 * i], y = pts_new[2 * i + 1];
      if (x < 0 || y < 0 || (int)x >= w || (int)y >= h) continue;            // :538-540
      if (mask && mask[(size_t)(int)y * w + (int)x] > 127) continue;          // :543-544
      if (!_match_mask[i]) continue;                                           // :546
      good.push_back(x), good.push_back(y), good_ids.push_back(_ids_last[i]);
    }
    _pts_last.swap(good), _ids_last.swap(good_ids);  // :560-567
    return 0;
  }
  const std::vector<size_t> &get_last_ids() const { return _ids_last; }
  const std::vector<float> &get_last_pts() const { return _pts_last; }          // [2n]
  const std::vector<float> &get_last_match_pts() const { return _match_pts; }   // of the points that went into the last frame
  const std::vector<uint8_t> &get_last_match_mask() const { return _match_mask; }

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
  // image front end
  bool _klt_made = false;
  int _pyr_levels = 5, _win_size = 15, _hist = OVP_KLT_HIST_HISTOGRAM, _klt_max_points = OVP_KLT_MAX_POINTS;
  int _klt_w = 0, _klt_h = 0, _n_images = 0;
  double _time_last = 0.0;
  std::vector<size_t> _ids_last;
  std::vector<float> _pts_last, _match_pts;
  std::vector<uint8_t> _match_mask;
};

}  // namespace ov_plane
