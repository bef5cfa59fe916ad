// The device-facing half of ov_plane_pack.h: table uploads and the triangulation block every updater opens with.
#include "ov_plane_pack.h"

#include <cstdio>
#include <cstdlib>

namespace ov_plane {

static void pack_check(int rc, const char *what) {
  if (rc == 0) return;
  fprintf(stderr, "ov_plane(gpu): %s failed: %s\n", what, ovp_error_string(rc));
  std::exit(EXIT_FAILURE);
}

void upload_state_tables(const std::shared_ptr<State> &state, const CloneWindow &window) {
  const CloneTables t(window);
  ovp_state_tables st;
  st.n_state = ovp_cov_size(state->gpu());
  st.n_clones = window.size();
  st.clone_q = t.q.data();
  st.clone_p = t.p.data();
  st.clone_q_fej = t.q_fej.data();
  st.clone_p_fej = t.p_fej.data();
  st.clone_id = t.id.data();
  auto calib = state->_calib_IMUtoCAM.at(0);
  auto intr = state->_cam_intrinsics.at(0);
  memcpy(st.calib_q, calib->quat(), 4 * sizeof(double));
  memcpy(st.calib_p, calib->pos(), 3 * sizeof(double));
  st.calib_id = calib->id();
  memcpy(st.intrinsics, intr->value().data(), 8 * sizeof(double));
  st.intr_id = intr->id();
  st.cam_fisheye = (state->_cam_fisheye.count(0) && state->_cam_fisheye.at(0)) ? 1 : 0;
  pack_check(ovp_state_upload(state->gpu(), &st), "ovp_state_upload");  // (the tables are staged inside the call)
}

void upload_camera_tables(const std::shared_ptr<State> &state) {
  std::vector<ovp_camera_tables> cams(state->_options.num_cameras);
  for (int k = 0; k < state->_options.num_cameras; ++k) {
    auto calib = state->_calib_IMUtoCAM.at(k);
    auto intr = state->_cam_intrinsics.at(k);
    memcpy(cams[k].calib_q, calib->quat(), 4 * sizeof(double));
    memcpy(cams[k].calib_p, calib->pos(), 3 * sizeof(double));
    cams[k].calib_id = calib->id();
    memcpy(cams[k].intrinsics, intr->value().data(), 8 * sizeof(double));
    cams[k].intr_id = intr->id();
    cams[k].fisheye = (state->_cam_fisheye.count(k) && state->_cam_fisheye.at(k)) ? 1 : 0;
  }
  pack_check(ovp_cameras_upload(state->gpu(), (int)cams.size(), cams.data()), "ovp_cameras_upload");
}

// StateOptions::gpu_featdb: the camera-0 batch comes from the device database - every feature whole, none for the general pass
static bool featdb_can_carry(const FeatureVec &features, const TriangulationSite &site) {
  for (const auto &f : features) {
    if (!wants_triangulation(*f) || (site.mono && site.mono(*f) != Meas::ALL)) return false;
    if (site.general && site.general(*f)) return false;
  }
  return true;
}

// false: the database does not hold every feature of the call with an observation in the window (the gather refused, nothing was
// touched) - the caller packs and uploads as without the option
static bool triangulate_from_featdb(const std::shared_ptr<State> &state, const CloneWindow &window,
                                    const ov_core::FeatureInitializerOptions &fio, FeatureVec &features, const TriangulationSite &site) {
  std::vector<int64_t> ids;
  for (const auto &f : features) ids.push_back((int64_t)f->featid);
  std::vector<double> times;
  for (const auto &c : window.clone_slot) times.push_back(c.first);  // ascending: slot i of the tables is times[i]
  const int rg = state->_featdb->gather(ids, times);
  if (rg == OVP_E_ARG) return false;
  pack_check(rg, "ovp_featdb_gather");
  std::vector<double> pf;
  std::vector<uint8_t> okv;
  pack_check(state->_featdb->triangulate(make_triang_opts(fio), pf, okv, (int)ids.size()), "ovp_featdb_triangulate");
  FeatureVec kept;
  for (size_t f = 0; f < features.size(); ++f) {
    if (!okv[f]) {
      if (site.flag_failures) features[f]->to_delete = true;  // :161-165
      continue;
    }
    memcpy(features[f]->p_FinG, &pf[3 * f], 3 * sizeof(double));
    kept.push_back(features[f]);
  }
  features = kept;
  return true;
}

void triangulate_on_device(const std::shared_ptr<State> &state, const CloneWindow &window, const ov_core::FeatureInitializerOptions &fio,
                           FeatureVec &features, const TriangulationSite &site) {
  if (!any_wants_triangulation(features)) return;
  if (state->_options.gpu_featdb && state->_featdb && featdb_can_carry(features, site) &&
      triangulate_from_featdb(state, window, fio, features, site))
    return;
  PackSite mono;
  mono.which = site.mono;
  mono.with_uvn = true;
  const FeaturePack b = pack_features(feature_range(features), window.clone_slot, mono);
  const ovp_feature_batch fb = b.as_feature_batch();
  pack_check(ovp_batch_upload(state->gpu(), &fb), "ovp_batch_upload");
  const ovp_triang_opts to = make_triang_opts(fio);
  std::vector<double> pf((size_t)b.F * 3);
  std::vector<uint8_t> okv(b.F, 0);
  pack_check(ovp_triangulate(state->gpu(), &to, b.uvn.data(), pf.data(), okv.data()), "ovp_triangulate");
  std::vector<size_t> gidx;
  for (size_t f = 0; site.general && f < features.size(); ++f)
    if (features[f]->uvs_norm.size() == features[f]->uvs.size() && site.general(*features[f])) gidx.push_back(f);
  if (!gidx.empty()) {
    upload_camera_tables(state);
    PackSite gen;
    gen.pad = 0;
    gen.min_M = site.general_M_of_mono ? b.M : 1;
    gen.uv_norm = !site.general_pixels;
    gen.with_uvn = site.general_pixels;
    const FeaturePack g = pack_features(feature_range(features, gidx), window.clone_slot, gen);
    const ovp_general_batch gb = g.as_general_batch(true, site.general_pixels);
    std::vector<double> gpf(gidx.size() * 3, 0.0);
    std::vector<uint8_t> gok(gidx.size(), 0);
    pack_check(ovp_triangulate_general(state->gpu(), &to, &gb, site.general_pixels ? g.uvn.data() : g.uv.data(), gpf.data(), gok.data()),
               "ovp_triangulate_general");
    for (size_t i = 0; i < gidx.size(); ++i) {
      okv[gidx[i]] = gok[i];
      memcpy(&pf[3 * gidx[i]], &gpf[3 * i], 3 * sizeof(double));
    }
  }
  FeatureVec kept;
  for (size_t f = 0; f < features.size(); ++f) {
    const bool had_norm = !features[f]->uvs_norm.empty();
    if (had_norm && !okv[f]) {
      if (site.flag_failures) features[f]->to_delete = true;  // :161-165
      continue;
    }
    if (had_norm) memcpy(features[f]->p_FinG, &pf[3 * f], 3 * sizeof(double));
    kept.push_back(features[f]);
  }
  features = kept;
}

ClonesInCamera0 clones_in_camera0(const std::shared_ptr<State> &state) {
  ClonesInCamera0 c;
  auto calib = state->_calib_IMUtoCAM.at(0);
  for (const auto &cl : state->_clones_IMU) {
    PlaneFitting::ClonePose cpose;
    const double *Ri = cl.second->Rot(), *Rc = calib->Rot(), *pi = cl.second->pos(), *pc = calib->pos();
    for (int i = 0; i < 3; ++i)
      for (int k = 0; k < 3; ++k) cpose.R[3 * i + k] = Rc[3 * i] * Ri[k] + Rc[3 * i + 1] * Ri[3 + k] + Rc[3 * i + 2] * Ri[6 + k];
    for (int i = 0; i < 3; ++i) cpose.p[i] = pi[i] - (cpose.R[i] * pc[0] + cpose.R[3 + i] * pc[1] + cpose.R[6 + i] * pc[2]);
    c.clones_cam[0][cl.first] = cpose;
  }
  memcpy(c.stateI, state->_imu->quat(), 4 * sizeof(double));
  memcpy(c.stateI + 4, state->_imu->pos(), 3 * sizeof(double));
  memcpy(c.calib0, calib->quat(), 4 * sizeof(double));
  memcpy(c.calib0 + 4, calib->pos(), 3 * sizeof(double));
  return c;
}

}  // namespace ov_plane
