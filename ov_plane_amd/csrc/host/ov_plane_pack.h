// The one packing layer between the host mirror and the C-ABI: every array and C struct the updaters hand to the device is
// filled here.  The first part is pure (no ovp_* call: it compiles and runs without the device library, tests/host_pack_main.cpp);
// the functions at the bottom issue the uploads and the triangulation and live in ov_plane_pack.cpp.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <vector>

#include "ov_plane_host.h"

namespace ov_plane {

typedef std::vector<std::shared_ptr<ov_core::Feature>> FeatureVec;

// update/UpdaterMSCKF.cpp:74-100, :101-118, update/UpdaterSLAM.cpp:80-118, :391-419, update/UpdaterPlane.cpp:76-107 (ext
// Feature::clean_old_measurements): only the measurements taken at a clone time of the window stay.  clones: any map keyed by
// the clone timestamps.  uvs_norm of another length than uvs is dropped.
template <class ClonesByTime> void keep_window_measurements(ov_core::Feature &ft, const ClonesByTime &clones) {
  std::vector<float> uv2, uvn2;
  std::vector<double> ts2;
  std::vector<int> cam2;
  const bool has_norm = ft.uvs_norm.size() == ft.uvs.size();
  for (size_t k = 0; k < ft.timestamps.size(); ++k)
    if (clones.count(ft.timestamps[k])) {
      ts2.push_back(ft.timestamps[k]);
      if (!ft.cam_ids.empty()) cam2.push_back(ft.cam_of(k));
      uv2.push_back(ft.uvs[2 * k]);
      uv2.push_back(ft.uvs[2 * k + 1]);
      if (has_norm) {
        uvn2.push_back(ft.uvs_norm[2 * k]);
        uvn2.push_back(ft.uvs_norm[2 * k + 1]);
      }
    }
  ft.timestamps = ts2;
  ft.cam_ids = cam2;
  ft.uvs = uv2;
  ft.uvs_norm = uvn2;
}

// The clone window in the order of the device tables: slot i of ovp_state_upload is clones[i]
struct CloneWindow {
  std::map<double, int> clone_slot;  // timestamp -> slot
  std::vector<std::shared_ptr<ov_type::PoseJPL>> clones;
  explicit CloneWindow(const std::map<double, std::shared_ptr<ov_type::PoseJPL>> &clones_IMU) {
    for (const auto &c : clones_IMU) {
      clone_slot[c.first] = (int)clones.size();
      clones.push_back(c.second);
    }
  }
  int size() const { return (int)clones.size(); }
};

// The window's poses as the arrays of ovp_state_tables (and of the frame trace), at their values of now
struct CloneTables {
  std::vector<double> q, p, q_fej, p_fej;
  std::vector<int> id;
  explicit CloneTables(const CloneWindow &w) : q(4 * w.size()), p(3 * w.size()), q_fej(4 * w.size()), p_fej(3 * w.size()), id(w.size()) {
    for (int i = 0; i < w.size(); ++i) {
      memcpy(&q[4 * i], w.clones[i]->quat(), 4 * sizeof(double));
      memcpy(&p[3 * i], w.clones[i]->pos(), 3 * sizeof(double));
      memcpy(&q_fej[4 * i], w.clones[i]->quat_fej(), 4 * sizeof(double));
      memcpy(&p_fej[3 * i], w.clones[i]->pos_fej(), 3 * sizeof(double));
      id[i] = w.clones[i]->id();
    }
  }
};

// Which measurements of a feature a batch carries
enum class Meas {
  ALL,
  NONE,        // the feature keeps its row (and its p_FinG) but takes no part: "off batch"
  CAM0_CAPPED  // the first OVP_MAX_MEAS measurements of camera 0: enough for a position estimate of a track the batch cannot carry
};

// What differs between the packing sites.  The defaults are those of a camera-0 feature batch.
struct PackSite {
  std::function<Meas(const ov_core::Feature &)> which;  // unset: ALL
  int min_M = 1;         // the row width is max(min_M, longest selection)
  int pad = -1;          // clone_idx behind a feature's measurements (-1 in feature batches, 0 in general ones)
  bool uv_norm = false;  // uv carries uvs_norm instead of uvs (zeros for a feature whose uvs_norm has another length than uvs)
  bool with_uvn = false; // uvn is filled as well (uvs_norm, zeros as above); otherwise it stays empty
  int empty_rows = 0;    // rows the arrays are sized for when there is no feature (the entries that want non-null pointers)
};

// how many measurements of a feature a rule selects (they are taken in the feature's order)
inline int n_selected(const ov_core::Feature &f, Meas m) {
  if (m == Meas::ALL) return (int)f.timestamps.size();
  int n = 0;
  for (size_t k = 0; m == Meas::CAM0_CAPPED && k < f.timestamps.size() && n < OVP_MAX_MEAS; ++k) n += f.cam_of(k) == 0 ? 1 : 0;
  return n;
}

// SoA form of a range of features: measurement k of feature f at [f * M + k]
struct FeaturePack {
  int F = 0, M = 1;
  std::vector<float> uv, uvn;
  std::vector<int> cidx, cam, nm;
  std::vector<double> pf;
  ovp_feature_batch as_feature_batch() const { return ovp_feature_batch{F, M, uv.data(), cidx.data(), nm.data(), pf.data()}; }
  ovp_general_batch as_general_batch(bool with_cam = true, bool with_p = true) const {
    return ovp_general_batch{F, M, uv.data(), cidx.data(), with_cam ? cam.data() : nullptr, nm.data(), with_p ? pf.data() : nullptr};
  }
};

inline FeaturePack pack_features(const std::vector<const ov_core::Feature *> &feats, const std::map<double, int> &clone_slot,
                                 const PackSite &site = PackSite()) {
  FeaturePack g;
  g.F = (int)feats.size();
  std::vector<Meas> rule(feats.size(), Meas::ALL);
  g.M = site.min_M;
  const size_t rows = (size_t)std::max(g.F, site.empty_rows);
  g.nm.assign(rows, 0);
  for (size_t f = 0; f < feats.size(); ++f) {
    if (site.which) rule[f] = site.which(*feats[f]);
    g.nm[f] = n_selected(*feats[f], rule[f]);
    g.M = std::max(g.M, g.nm[f]);
  }
  const size_t M = (size_t)g.M;
  g.uv.assign(rows * M * 2, 0.f);
  if (site.with_uvn) g.uvn.assign(rows * M * 2, 0.f);
  g.cidx.assign(rows * M, site.pad);
  g.cam.assign(rows * M, 0);
  g.pf.assign(rows * 3, 0.0);
  for (size_t f = 0; f < feats.size(); ++f) {
    const ov_core::Feature &ft = *feats[f];
    const bool has_norm = ft.uvs_norm.size() == ft.uvs.size();
    size_t o = f * M;
    for (size_t s = 0; o < f * M + (size_t)g.nm[f]; ++s) {  // s: the feature's measurement, o: its place in the row
      if (rule[f] == Meas::CAM0_CAPPED && ft.cam_of(s) != 0) continue;
      g.cidx[o] = clone_slot.at(ft.timestamps[s]);
      g.cam[o] = ft.cam_of(s);
      if (!site.uv_norm || has_norm) memcpy(&g.uv[2 * o], site.uv_norm ? &ft.uvs_norm[2 * s] : &ft.uvs[2 * s], 2 * sizeof(float));
      if (site.with_uvn && has_norm) memcpy(&g.uvn[2 * o], &ft.uvs_norm[2 * s], 2 * sizeof(float));
      ++o;
    }
    memcpy(&g.pf[3 * f], ft.p_FinG, 3 * sizeof(double));
  }
  return g;
}

// the ranges the sites pack: a whole vector, a part of it, the features at some indices
inline std::vector<const ov_core::Feature *> feature_range(const FeatureVec &fv, size_t begin = 0, size_t end = (size_t)-1) {
  std::vector<const ov_core::Feature *> r;
  for (size_t f = begin; f < std::min(end, fv.size()); ++f) r.push_back(fv[f].get());
  return r;
}
template <class Index> std::vector<const ov_core::Feature *> feature_range(const FeatureVec &fv, const std::vector<Index> &idx) {
  std::vector<const ov_core::Feature *> r;
  for (Index f : idx) r.push_back(fv[(size_t)f].get());
  return r;
}

inline ovp_update_opts make_update_opts(const UpdaterOptions &u, const StateOptions &s) {
  return ovp_update_opts{u.sigma_pix,
                         u.chi2_multipler,
                         s.sigma_constraint,
                         s.do_fej ? 1 : 0,
                         s.do_calib_camera_pose ? 1 : 0,
                         s.do_calib_camera_intrinsics ? 1 : 0,
                         0};
}

inline ovp_triang_opts make_triang_opts(const ov_core::FeatureInitializerOptions &fio) {
  ovp_triang_opts to;
  to.refine_features = fio.refine_features ? 1 : 0;
  to.triangulate_1d = fio.triangulate_1d ? 1 : 0;
  to.reserved = 0;
  to.max_runs = fio.max_runs;
  to.init_lamda = fio.init_lamda;
  to.max_lamda = fio.max_lamda;
  to.min_dx = fio.min_dx;
  to.min_dcost = fio.min_dcost;
  to.lam_mult = fio.lam_mult;
  to.min_dist = fio.min_dist;
  to.max_dist = fio.max_dist;
  to.max_baseline = fio.max_baseline;
  to.max_cond_number = fio.max_cond_number;
  return to;
}

// whether a feature arrives with normalised measurements, i.e. without a position (empty uvs_norm = p_FinG was handed over)
inline bool wants_triangulation(const ov_core::Feature &f) { return !f.uvs_norm.empty() && f.uvs_norm.size() == f.uvs.size(); }
inline bool any_wants_triangulation(const FeatureVec &fv) {
  return std::any_of(fv.begin(), fv.end(), [](const std::shared_ptr<ov_core::Feature> &f) { return wants_triangulation(*f); });
}

// ---- what follows talks to the device (ov_plane_pack.cpp) ----------------------------------------------------------------

// pose tables of the clone window + camera 0's calibration -> device (ovp_state_upload), at the values of now
void upload_state_tables(const std::shared_ptr<State> &state, const CloneWindow &window);
// every camera's calibration -> device (ovp_cameras_upload): the tables of the general entries
void upload_camera_tables(const std::shared_ptr<State> &state);

// update/UpdaterMSCKF.cpp:120-166, update/UpdaterSLAM.cpp:120-166, update/UpdaterPlane.cpp:126-149: the features that arrive with
// normalised measurements are triangulated (+ refined) against the uploaded clone window and get their p_FinG; those that fail
// leave `features`.  Features whose position was handed over (no uvs_norm) pass through.  Two passes: the camera-0 batch
// (ovp_batch_upload + ovp_triangulate), then - for the features `general` names - every camera's views, each with its own
// extrinsics (ovp_cameras_upload + ovp_triangulate_general), whose result replaces the first pass's.
struct TriangulationSite {
  std::function<Meas(const ov_core::Feature &)> mono;    // measurements the camera-0 pass sees (unset: all)
  std::function<bool(const ov_core::Feature &)> general;  // takes the second pass, given that it has uvs_norm (unset: none)
  bool general_pixels = false;  // the general batch carries the pixels and p_FinG beside uvs_norm (UpdaterMSCKF), or uvs_norm alone
  bool general_M_of_mono = false;  // its row width is at least the camera-0 batch's (UpdaterSLAM), or that of its own features
  bool flag_failures = true;    // a failure gets to_delete (:161-165); UpdaterPlane only takes it out of its candidate set
};
void triangulate_on_device(const std::shared_ptr<State> &state, const CloneWindow &window, const ov_core::FeatureInitializerOptions &fio,
                           FeatureVec &features, const TriangulationSite &site);

// Camera-0 pose of every clone for the host plane fit (update/UpdaterMSCKF.cpp:122-141): R_GtoCi = R_ItoC R_GtoIi,
// p_CiinG = p_IiinG - R_GtoCi^T p_IinC; stateI = [q_GtoI, p_IinG], calib0 = [q_ItoC, p_IinC] of PlaneFitting::optimize_plane
struct ClonesInCamera0 {
  PlaneFitting::ClonesCam clones_cam;
  double stateI[7], calib0[7];
};
ClonesInCamera0 clones_in_camera0(const std::shared_ptr<State> &state);

}  // namespace ov_plane
