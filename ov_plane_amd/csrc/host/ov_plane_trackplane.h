// Host mirror of the detection half of ov_plane::TrackPlane (track_plane/TrackPlane.h): feed_plane_detection() is
// perform_plane_detection_monocular (track_plane/TrackPlane.cpp:580-1121) on the tracked points of one frame - no images - and
// get_feature2plane() the reference's accessor.  The per-feature history and the plane maps live in the detector of the device
// context (ovp_plane_detector_*); this class hands it the frame, triangulates the points that have a position (Delaunay,
// ov_plane_delaunay.h, where the reference calls CDT) and reads the map back.  With set_device_delaunay the triangulation is the
// detector's own, on the device behind its first call: no has_est round trip and no triangles to hand over.
// The image half: feed_new_camera() is TrackPlane::feed_new_camera (:40-92) followed by the bookkeeping of feed_monocular
// (:505-567) minus detection and the epipolar check, perform_matching_klt() the cv::calcOpticalFlowPyrLK call of perform_matching
// (:1326-1330, :1352-1356); both pyramids live in the tracker of the device context (ovp_klt_*).  add_points() seeds or tops up
// pts_last / ids_last with a caller's points; perform_detection_monocular() is :1173-1297 on the device's candidates
// (ovp_klt_detect: Grider_FAST and OpenCV are not in the reference tree, that stage is recalled and unpinned), and
// feed_new_camera(.., detect = true) feed_monocular's use of it (:477-491, :505-507).  perform_matching() is :1299-1357 in full -
// perform_matching_klt, then the epipolar check on the device (ovp_klt_epipolar: recalled and unpinned, tests/epi_ref.py) under the
// camera of set_camera() - and feed_new_camera(.., epipolar = true) feed_monocular's use of it (:510-567), the reset of :520-530
// included; get_last_uv_norm() holds the kept points' undistorted coordinates (:555).  set_intake() selects the histogram method by
// TrackBase's names - CLAHE (:66-70) included, on the device: recalled and unpinned, tests/clahe_ref.py - and downsample_cameras
// (core/VioManager.cpp:279-289): feed_new_camera() then takes the full-size image and mask and halves both on the device.
// feed_monocular() is :463-567 over ONE entry (ovp_klt_match_frame): KLT, the epipolar check, the keep rule and, under
// set_database(), database->update_feature of the survivors (:553-557) in one device pass - the same frame feed_new_camera walks
// through ovp_klt_track, ovp_klt_epipolar and its own keep rule, byte for byte.
#pragma once
#include <array>
#include <cmath>
#include <cstdint>
#include <map>
#include <set>
#include <vector>

#include "ov_plane_delaunay.h"
#include "ov_plane_featdb.h"  // the context's database, which feed_monocular() appends to on the device
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

  // ov_core::TrackBase::HistogramMethod, by its names and in its order (OVP_KLT_HIST_*)
  enum HistogramMethod { NONE, HISTOGRAM, CLAHE };
  // histogram_method and downsample_cameras of estimator_config.yaml; CLAHE's parameters are the reference's own (:67-68).  From
  // here on feed_new_camera feeds through ovp_klt_feed_image_opts, and with `downsample` it takes the FULL-SIZE image and mask
  // (core/VioManager.cpp:279-289) - the tracker's size is (w / 2, h / 2).  Before the first image.
  int set_intake(HistogramMethod method, bool downsample, double clahe_clip = 10.0, int tiles_x = 8, int tiles_y = 8) {
    if (_klt_made) return OVP_E_STATE;
    if (method != NONE && method != HISTOGRAM && method != CLAHE) return OVP_E_ARG;
    ovp_klt_intake_defaults(&_intake);
    _intake.hist_method = (int)method, _intake.downsample = downsample ? 1 : 0;
    _intake.clahe_clip = clahe_clip, _intake.clahe_tiles_x = tiles_x, _intake.clahe_tiles_y = tiles_y;
    _hist = (int)method, _intake_set = true;
    return 0;
  }

  // TrackBase's num_features, grid_x, grid_y, threshold and min_px_dist
  void set_detector_options(int num_features, int grid_x, int grid_y, int threshold, int min_px_dist) {
    _num_features = num_features, _grid_x = grid_x, _grid_y = grid_y, _threshold = threshold, _min_px_dist = min_px_dist;
  }

  // :1173-1297 on level 0 of a half of the tracker (0: the current image, 1: the previous one): walks pts [2n] / ids through the
  // occupancy grid, returns when fewer than 5 % of num_features are missing, else accepts the device's candidates in order and
  // numbers them ++currid (which starts at 0: the first id is 1).  mask: h x w, NULL for none.  Every candidate is refined on the
  // device and the masked ones are dropped afterwards; the reference drops them before the refinement, which is the same:
  // cornerSubPix treats each point on its own.
  int perform_detection_monocular(int half, const uint8_t *mask, std::vector<float> &pts, std::vector<size_t> &ids) {
    if (!_klt_made) return OVP_E_STATE;
    const int cap = _klt_max_points;
    return detection_monocular(_klt_w, _klt_h, _num_features, _grid_x, _grid_y, _min_px_dist, mask, pts, ids, _currid, _last_detected,
                               [&](std::vector<int32_t> &xy, std::vector<float> &ref) {
                                 std::vector<int32_t> resp(cap), cell(cap);
                                 xy.resize(2 * (size_t)cap), ref.resize(2 * (size_t)cap);
                                 int n = 0;
                                 const int rc = ovp_klt_detect(_gpu, half, _num_features, _grid_x, _grid_y, _threshold, &n, xy.data(), resp.data(),
                                                               ref.data(), cell.data(), cap);
                                 xy.resize(rc ? 0 : 2 * (size_t)n), ref.resize(rc ? 0 : 2 * (size_t)n);
                                 return rc;
                               });
  }

  // the host half of the above on its own (no device: tests hand the candidates in): candidates(xy_int [2n], refined [2n]) -> 0 or
  // a code, called only behind the 5 % return
  template <class Candidates>
  static int detection_monocular(int cols, int rows, int num_features, int grid_x, int grid_y, int min_px_dist, const uint8_t *mask,
                                 std::vector<float> &pts, std::vector<size_t> &ids, size_t &currid, bool &detected, Candidates &&candidates) {
    if (min_px_dist < 1 || grid_x < 1 || grid_y < 1 || pts.size() != 2 * ids.size()) return OVP_E_ARG;
    const int mpd = min_px_dist;
    const int wc = (int)((float)cols / (float)mpd), hc = (int)((float)rows / (float)mpd);  // :1180-1181 size_close
    const float size_x = (float)cols / (float)grid_x, size_y = (float)rows / (float)grid_y;
    std::vector<uint8_t> close((size_t)std::max(wc, 0) * std::max(hc, 0), 0);
    std::vector<uint8_t> upd((size_t)cols * rows, 0);
    if (mask) upd.assign(mask, mask + (size_t)cols * rows);
    std::vector<float> kp;
    std::vector<size_t> ki;
    for (size_t i = 0; i < ids.size(); ++i) {
      const float fx = pts[2 * i], fy = pts[2 * i + 1];
      const int x = (int)fx, y = (int)fy, edge = 10;
      if (x < edge || x >= cols - edge || y < edge || y >= rows - edge) continue;          // :1195-1199
      const int xc = (int)(fx / (float)mpd), yc = (int)(fy / (float)mpd);
      if (xc < 0 || xc >= wc || yc < 0 || yc >= hc) continue;                               // :1203-1207
      const int xg = (int)std::floor(fx / size_x), yg = (int)std::floor(fy / size_y);
      if (xg < 0 || xg >= grid_x || yg < 0 || yg >= grid_y) continue;                       // :1211-1215
      if (close[(size_t)yc * wc + xc] > 127) continue;                                      // :1217-1221
      if (mask && mask[(size_t)y * cols + x] > 127) continue;                               // :1224-1228
      close[(size_t)yc * wc + xc] = 255;
      if (x - mpd >= 0 && x + mpd < cols && y - mpd >= 0 && y + mpd < rows)                 // :1235-1239 the rectangle, when it fits
        for (int r = y - mpd; r <= y + mpd; ++r)
          for (int q = x - mpd; q <= x + mpd; ++q) upd[(size_t)r * cols + q] = 255;
      kp.push_back(fx), kp.push_back(fy), ki.push_back(ids[i]);
    }
    detected = false;
    if (num_features - (int)ki.size() >= num_features * (1.0 - 0.95)) {                     // :1246-1249
      std::vector<int32_t> xy;
      std::vector<float> ref;
      const int rc = candidates(xy, ref);
      if (rc) return rc;
      detected = true;
      for (size_t j = 0; 2 * j + 1 < xy.size(); ++j) {
        if (xy[2 * j] < 0 || xy[2 * j] >= cols || xy[2 * j + 1] < 0 || xy[2 * j + 1] >= rows) continue;
        if (upd[(size_t)xy[2 * j + 1] * cols + xy[2 * j]] > 127) continue;                  // Grider_FAST's mask test, on the corner's pixel
        const int xc = (int)(ref[2 * j] / (float)mpd), yc = (int)(ref[2 * j + 1] / (float)mpd);  // :1265-1281
        if (xc < 0 || xc >= wc || yc < 0 || yc >= hc || close[(size_t)yc * wc + xc] > 127) continue;
        close[(size_t)yc * wc + xc] = 255;
        kp.push_back(ref[2 * j]), kp.push_back(ref[2 * j + 1]), ki.push_back(++currid);     // :1292
      }
    }
    pts.swap(kp), ids.swap(ki);
    return 0;
  }
  bool last_detected() const { return _last_detected; }

  // a caller's own detection: points of the last image fed
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

  // undistort_cv's camera: OVP_EPI_MODE_* and its 8 intrinsics; the threshold of :1341-1344 is 2 / max(fx, fy) (mode
  // OVP_EPI_MODE_NORMALISED: the defaults' threshold, or the one of set_epipolar_options).  Under set_intake(.., downsample = true)
  // the tracked points are pixels of the halved image: the caller passes the HALVED intrinsics (fx, fy, cx, cy over 2), as the
  // reference's options loader does (core/VioManagerOptions.h:252-264).
  int set_camera(int mode, const double *intrinsics) {
    if (!intrinsics || mode < OVP_EPI_MODE_NORMALISED || mode > OVP_EPI_MODE_EQUIDISTANT) return OVP_E_ARG;
    _epi.mode = mode;
    for (int k = 0; k < 8; ++k) _epi.intrinsics[k] = intrinsics[k];
    if (mode != OVP_EPI_MODE_NORMALISED) _epi.threshold = 2.0 / std::max(intrinsics[0], intrinsics[1]);
    _camera_set = true;
    return 0;
  }
  // the RANSAC's own options (:1344 passes 0.999; max_iters and the seed are this library's); threshold <= 0 keeps the camera's
  void set_epipolar_options(double confidence, int max_iters, uint32_t seed, double threshold = 0.0) {
    _epi.confidence = confidence, _epi.max_iters = max_iters, _epi.seed = seed;
    if (threshold > 0.0) _epi.threshold = threshold;
  }

  // :1299-1357 on the host, the two device calls handed in (tests stub them): track(pts0, pts1, mask_klt) -> code is the KLT call,
  // which moves pts1; epi(pts0, pts1, mask_klt, mask_out, uvn1) -> code the epipolar check, mask_out = mask_klt & mask_rsc.
  // No points: mask_out stays empty (:1307); fewer than 10: all zeros and no KLT (:1319-1323).
  template <class Track, class Epi>
  static int matching(const std::vector<float> &pts0, std::vector<float> &pts1, std::vector<uint8_t> &mask_out, std::vector<float> &uvn1,
                      Track &&track, Epi &&epi) {
    mask_out.clear(), uvn1.clear();
    if (pts0.size() != pts1.size() || (pts0.size() & 1)) return OVP_E_ARG;
    const size_t n = pts0.size() / 2;
    if (n == 0) return 0;
    if (n < OVP_EPI_MIN_POINTS) {
      mask_out.assign(n, 0);
      return 0;
    }
    std::vector<uint8_t> mask_klt;
    int rc = track(pts0, pts1, mask_klt);
    if (rc) return rc;
    mask_out.assign(n, 0), uvn1.assign(2 * n, 0.f);
    return epi(pts0, pts1, mask_klt, mask_out, uvn1);
  }

  int perform_matching(const std::vector<float> &pts0, std::vector<float> &pts1, std::vector<uint8_t> &mask_out, std::vector<float> &uvn1) {
    return matching(
        pts0, pts1, mask_out, uvn1,
        [&](const std::vector<float> &p0, std::vector<float> &p1, std::vector<uint8_t> &mk) { return perform_matching_klt(p0, p1, mk); },
        [&](const std::vector<float> &p0, const std::vector<float> &p1, const std::vector<uint8_t> &mk, std::vector<uint8_t> &mo,
            std::vector<float> &u1) {
          return ovp_klt_epipolar(_gpu, &_epi, (int)mk.size(), p0.data(), p1.data(), mk.data(), mo.data(), nullptr, u1.data(), &_epi_info);
        });
  }

  // feed_monocular :510-567 behind the top-up, on the host: matching(pts0, pts1, mask_out, uvn1) -> code is perform_matching.  An
  // empty mask resets (:520-530); otherwise a point is kept unless x < 0, y < 0, (int) x >= w, (int) y >= h, it lies in the mask,
  // or mask_out is 0.  match_pts / match_mask: what went in, moved, and its mask.
  template <class Matching>
  static int matching_frame(int w, int h, const uint8_t *mask, std::vector<size_t> &ids_last, std::vector<float> &pts_last,
                            std::vector<float> &uvn_last, std::vector<float> &match_pts, std::vector<uint8_t> &match_mask, bool &reset,
                            Matching &&matching) {
    std::vector<float> pts_new = pts_last, uvn;  // :512
    std::vector<uint8_t> mask_ll;
    reset = false;
    uvn_last.clear(), match_pts.clear(), match_mask.clear();
    const int rc = matching(pts_last, pts_new, mask_ll, uvn);
    if (rc) return rc;
    if (mask_ll.empty()) {  // :520-530
      pts_last.clear(), ids_last.clear();
      reset = true;
      return 0;
    }
    std::vector<float> good, good_n;
    std::vector<size_t> good_ids;
    for (size_t i = 0; i < ids_last.size(); ++i) {
      const float x = pts_new[2 * i], y = pts_new[2 * i + 1];
      if (x < 0 || y < 0 || (int)x >= w || (int)y >= h) continue;            // :538-540
      if (mask && mask[(size_t)(int)y * w + (int)x] > 127) continue;          // :543-544
      if (!mask_ll[i]) continue;                                               // :546
      good.push_back(x), good.push_back(y), good_ids.push_back(ids_last[i]);
      if (2 * i + 1 < uvn.size()) good_n.push_back(uvn[2 * i]), good_n.push_back(uvn[2 * i + 1]);  // :555
    }
    if (uvn.size() == pts_new.size()) match_pts = pts_new;  // (the KLT ran)
    match_mask = mask_ll;
    pts_last.swap(good), ids_last.swap(good_ids), uvn_last.swap(good_n);    // :560-567
    return 0;
  }

  // One camera image (8-bit, h rows of `stride` bytes) and its mask (h x w, NULL: none; a value above 127 masks the pixel):
  // :40-92 equalise and build the pyramid, then :514-567 track pts_last into it and keep a point unless x < 0, y < 0,
  // (int) x >= cols, (int) y >= rows, it lies in the mask, or its status is 0.  Returns 0 or an OVP_E_* code.
  // detect: feed_monocular :477-567 minus the epipolar check - without points, detection on this image and return (:477-491);
  // otherwise pts_last is topped up on the previous image under its mask (:505-507) before it is tracked.
  // epipolar: perform_matching in full decides (:510-567): fewer than 10 points keep nothing, none resets (last_reset()), and
  // get_last_uv_norm() holds the kept points' undistorted coordinates.  Off by default: nothing existing changes.
  // Under set_intake(.., downsample = true) img and mask are the full-size ones, w x h their size, and everything behind the
  // halving - tracker, mask tests, points - is in pixels of the (w / 2) x (h / 2) image.
  int feed_new_camera(double time, const uint8_t *img, int w, int h, int stride, const uint8_t *mask = nullptr, bool detect = false,
                      bool epipolar = false) {
    std::vector<uint8_t> mask_halved;
    bool finished = false;
    int rc = feed_front(time, img, w, h, stride, mask, detect, mask_halved, finished);
    if (rc || finished) return rc;
    _uvn_last.clear(), _last_reset = false;
    if (epipolar && _n_images >= 2)
      return matching_frame(w, h, mask, _ids_last, _pts_last, _uvn_last, _match_pts, _match_mask, _last_reset,
                            [&](const std::vector<float> &p0, std::vector<float> &p1, std::vector<uint8_t> &mo, std::vector<float> &u1) {
                              return perform_matching(p0, p1, mo, u1);
                            });
    if (_n_images < 2 || _ids_last.empty()) return 0;
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
  // the feature database feed_monocular() appends the kept points to on the device (NULL: none).  The entry appends to the database
  // of its context, so only that one can be attached: OVP_E_ARG for a database of another context, OVP_E_STATE for one whose create failed.
  int set_database(FeatureDatabase *database) {
    if (database && database->context() != _gpu) return OVP_E_ARG;
    if (database && database->status() != 0) return OVP_E_STATE;
    _database = database;
    return 0;
  }

  // feed_monocular :463-567 over ovp_klt_match_frame - image and mask as feed_new_camera takes them, detect as there.  epipolar:
  // perform_matching's check decides; without it the status alone, and uv_norm (get_last_uv_norm) comes from the undistortion
  // alone when a camera is set.  With a database the kept points' observations are appended at `time` in the same device pass
  // (a camera is needed: OVP_E_ARG without one).  The empty-set rules are feed_new_camera's: no points with the check resets
  // (:520-530), fewer than ten keep nothing and run no KLT (:1319-1323).
  int feed_monocular(double time, const uint8_t *img, int w, int h, int stride, const uint8_t *mask = nullptr, bool detect = false,
                     bool epipolar = false) {
    std::vector<uint8_t> mask_halved;
    bool finished = false;
    int rc = feed_front(time, img, w, h, stride, mask, detect, mask_halved, finished);
    if (rc || finished) return rc;
    _uvn_last.clear(), _last_reset = false;
    const size_t n = _ids_last.size();
    if (epipolar && _n_images >= 2) {
      if (n == 0) {  // :1307 an empty mask -> :520-530
        _last_reset = true;
        return 0;
      }
      if (n < OVP_EPI_MIN_POINTS) {  // :1319-1323 all zeros, no KLT
        _match_mask.assign(n, 0);
        _pts_last.clear(), _ids_last.clear();
        return 0;
      }
    }
    if (_n_images < 2 || n == 0) return 0;
    std::vector<int64_t> id64(_ids_last.begin(), _ids_last.end());
    std::vector<uint8_t> keep(n), mask_epi(n);
    std::vector<float> pts_new(2 * n), uvn(2 * n);
    ovp_klt_frame_in in = {};
    in.n = (int)n, in.pts_prev = _pts_last.data(), in.ids = id64.data(), in.timestamp = time;
    in.mask = mask, in.mask_stride = w;
    in.epi = (epipolar || _camera_set) ? &_epi : nullptr;
    in.check = epipolar ? 1 : 0, in.to_database = _database ? 1 : 0;
    ovp_klt_frame_out out = {};
    out.keep = keep.data(), out.pts_out = pts_new.data(), out.mask_epi = mask_epi.data(), out.uvn = uvn.data();
    rc = ovp_klt_match_frame(_gpu, &in, &out);
    if (rc) return rc;
    if (epipolar) _epi_info = out.info;
    std::vector<float> good, good_n;
    std::vector<size_t> good_ids;
    for (size_t i = 0; i < n; ++i) {
      if (!keep[i]) continue;
      good.push_back(pts_new[2 * i]), good.push_back(pts_new[2 * i + 1]), good_ids.push_back(_ids_last[i]);
      if (in.epi) good_n.push_back(uvn[2 * i]), good_n.push_back(uvn[2 * i + 1]);  // :555
    }
    _match_pts = pts_new, _match_mask = mask_epi;
    _pts_last.swap(good), _ids_last.swap(good_ids), _uvn_last.swap(good_n);  // :560-567
    return 0;
  }
  const std::vector<size_t> &get_last_ids() const { return _ids_last; }
  const std::vector<float> &get_last_pts() const { return _pts_last; }          // [2n]
  const std::vector<float> &get_last_match_pts() const { return _match_pts; }   // of the points that went into the last frame
  const std::vector<uint8_t> &get_last_match_mask() const { return _match_mask; }
  const std::vector<float> &get_last_uv_norm() const { return _uvn_last; }     // [2n] of the kept points, with the check on
  const ovp_epipolar_info &get_last_epipolar_info() const { return _epi_info; }
  bool last_reset() const { return _last_reset; }

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
  // the front of a frame, shared by feed_new_camera and feed_monocular: the tracker on first use, the image's intake (:40-92), the
  // mask's halving and feed_monocular's use of the detection (:477-491, :505-507).  w, h and mask become the tracker's; finished:
  // the frame ended with the first detection.
  int feed_front(double time, const uint8_t *img, int &w, int &h, int stride, const uint8_t *&mask, bool detect,
                 std::vector<uint8_t> &mask_halved, bool &finished) {
    const bool halve = _intake_set && _intake.downsample;
    const int src_w = w, src_h = h;
    if (halve) w = src_w / 2, h = src_h / 2;
    if (!_klt_made) {
      const int rc = ovp_klt_create(_gpu, w, h, _pyr_levels + 1, _win_size, _klt_max_points);
      if (rc) return rc;
      _klt_made = true, _klt_w = w, _klt_h = h;
    }
    if (w != _klt_w || h != _klt_h) return OVP_E_ARG;
    int rc;
    if (_intake_set) {
      ovp_klt_intake in = _intake;
      in.src_width = src_w, in.src_height = src_h;
      rc = ovp_klt_feed_image_opts(_gpu, img, stride, &in);
    } else {
      rc = ovp_klt_feed_image(_gpu, img, stride, _hist);
    }
    if (rc) return rc;
    if (halve && mask) {  // core/VioManager.cpp:284-288
      mask_halved.resize((size_t)w * h);
      rc = ovp_klt_halve(_gpu, mask, src_w, src_w, src_h, mask_halved.data());
      if (rc) return rc;
      mask = mask_halved.data();
    }
    _time_last = time;
    _match_pts.clear(), _match_mask.clear();
    ++_n_images;
    if (detect) {
      std::vector<uint8_t> mask_prev;
      mask_prev.swap(_mask_last);
      if (mask) _mask_last.assign(mask, mask + (size_t)w * h);
      if (_ids_last.empty()) {
        finished = true;
        return perform_detection_monocular(0, mask, _pts_last, _ids_last);
      }
      rc = perform_detection_monocular(1, mask_prev.empty() ? nullptr : mask_prev.data(), _pts_last, _ids_last);
      if (rc) return rc;
    }
    return 0;
  }

  ovp_ctx *_gpu;
  int _rc = 0;
  bool _have_pose = false, _device_delaunay = false;
  double _pose_time = 0.0, _R[9], _p[3];
  // image front end
  bool _klt_made = false;
  int _pyr_levels = 5, _win_size = 15, _hist = OVP_KLT_HIST_HISTOGRAM, _klt_max_points = OVP_KLT_MAX_POINTS;
  int _klt_w = 0, _klt_h = 0, _n_images = 0;
  ovp_klt_intake _intake = {};  // set_intake
  bool _intake_set = false;
  double _time_last = 0.0;
  std::vector<size_t> _ids_last;
  std::vector<float> _pts_last, _match_pts;
  std::vector<uint8_t> _match_mask;
  // detection
  int _num_features = 200, _grid_x = 12, _grid_y = 12, _threshold = 15, _min_px_dist = 15;
  size_t _currid = 0;
  bool _last_detected = false;
  std::vector<uint8_t> _mask_last;  // img_mask_last: the previous image's mask, for the top-up
  // epipolar check
  ovp_epipolar_opts _epi = [] {
    ovp_epipolar_opts o;
    ovp_epipolar_defaults(&o);
    return o;
  }();
  ovp_epipolar_info _epi_info = {};
  std::vector<float> _uvn_last;
  bool _last_reset = false;
  bool _camera_set = false;            // set_camera was called: feed_monocular undistorts without the check as well
  FeatureDatabase *_database = nullptr;  // set_database
};

}  // namespace ov_plane
