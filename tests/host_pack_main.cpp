// The pure half of csrc/host/ov_plane_pack.h on features made by hand, every packed array against values written out here.
// Links nothing of the device; tests/test_host_pack_cpu.py builds it with the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ov_plane_pack.h"
#include "ov_types.h"
#include "ovplane_hip.h"

using namespace ov_plane;
using ov_core::Feature;

#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                           \
    }                                                         \
  } while (0)

static const int NC = 70;  // clones at t = 100, 101, ...: slot i <-> time 100 + i
static double t_of(int slot) { return 100.0 + slot; }
struct View {
  int slot;  // < 0: a time outside the window
  int cam;
};
// measurement k of feature id: pixel (16 id + k, 16 id + k + 0.5), normalised (id + k / 128, -(id + k / 128))
static float px(int id, int k) { return 16.f * id + k; }
static float nx(int id, int k) { return id + k / 128.f; }
enum Norm { NORM_ABSENT, NORM_PRESENT, NORM_SHORT };
static std::shared_ptr<Feature> feat(int id, const std::vector<View> &views, Norm norm, bool with_cam_ids = true) {
  auto f = std::make_shared<Feature>();
  f->featid = id;
  for (size_t k = 0; k < views.size(); ++k) {
    f->timestamps.push_back(views[k].slot < 0 ? 50.0 + k : t_of(views[k].slot));
    if (with_cam_ids) f->cam_ids.push_back(views[k].cam);
    f->uvs.push_back(px(id, k));
    f->uvs.push_back(px(id, k) + 0.5f);
    if (norm != NORM_ABSENT && !(norm == NORM_SHORT && k + 1 == views.size())) {
      f->uvs_norm.push_back(nx(id, k));
      f->uvs_norm.push_back(-nx(id, k));
    }
  }
  f->p_FinG[0] = id;
  f->p_FinG[1] = id + 0.25;
  f->p_FinG[2] = -id;
  return f;
}
static std::vector<View> cam0_track(int n, int first_slot = 0) {
  std::vector<View> v;
  for (int k = 0; k < n; ++k) v.push_back({first_slot + k, 0});
  return v;
}
// row f of a pack carries exactly the measurements `sel` of `ft` (uv: pixels or normalised), pad behind them, zeros in uv
static void check_row(const FeaturePack &g, int f, const Feature &ft, const std::vector<size_t> &sel, int pad, bool uv_is_norm,
                      bool uv_zero = false) {
  const int id = (int)ft.featid;
  CHECK(g.nm[f] == (int)sel.size());
  for (int k = 0; k < g.M; ++k) {
    const size_t o = (size_t)f * g.M + k;
    if (k < (int)sel.size()) {
      CHECK(g.cidx[o] == (int)(ft.timestamps[sel[k]] - 100.0));
      CHECK(g.cam[o] == ft.cam_of(sel[k]));
      const float u = uv_zero ? 0.f : uv_is_norm ? nx(id, (int)sel[k]) : px(id, (int)sel[k]);
      const float v = uv_zero ? 0.f : uv_is_norm ? -nx(id, (int)sel[k]) : px(id, (int)sel[k]) + 0.5f;
      CHECK(g.uv[2 * o] == u && g.uv[2 * o + 1] == v);
    } else {
      CHECK(g.cidx[o] == pad && g.cam[o] == 0 && g.uv[2 * o] == 0.f && g.uv[2 * o + 1] == 0.f);
    }
  }
  CHECK(g.pf[3 * f] == id && g.pf[3 * f + 1] == id + 0.25 && g.pf[3 * f + 2] == -id);
}
static std::vector<size_t> first_n(size_t n) {
  std::vector<size_t> s;
  for (size_t k = 0; k < n; ++k) s.push_back(k);
  return s;
}

int main() {
  // ---- the clone window and its tables ----
  std::map<double, std::shared_ptr<ov_type::PoseJPL>> clones_IMU;
  for (int i = NC - 1; i >= 0; --i) {  // (inserted backwards: the slots follow the timestamps)
    auto c = std::make_shared<ov_type::PoseJPL>();
    VectorXd v(7, 1), vf(7, 1);
    const double val[7] = {0, 0, 0, 1, 1.0 * i, 2.0 * i, 3.0 * i}, fej[7] = {0, 1, 0, 0, -1.0 * i, 0.5 * i, 7};
    for (int k = 0; k < 7; ++k) v(k) = val[k], vf(k) = fej[k];
    c->set_value(v);
    c->set_fej(vf);
    c->set_local_id(15 + 6 * i);
    clones_IMU[t_of(i)] = c;
  }
  const CloneWindow w(clones_IMU);
  CHECK(w.size() == NC && (int)w.clone_slot.size() == NC);
  CHECK(w.clone_slot.at(100.0) == 0 && w.clone_slot.at(101.0) == 1 && w.clone_slot.at(169.0) == 69);
  CHECK(w.clones[3] == clones_IMU.at(103.0));
  const CloneTables t(w);
  CHECK(t.q.size() == 4 * NC && t.p.size() == 3 * NC && t.q_fej.size() == 4 * NC && t.p_fej.size() == 3 * NC && t.id.size() == NC);
  CHECK(t.q[4 * 2 + 3] == 1 && t.q[4 * 2] == 0 && t.p[3 * 2] == 2 && t.p[3 * 2 + 1] == 4 && t.p[3 * 2 + 2] == 6);
  CHECK(t.q_fej[4 * 2 + 1] == 1 && t.q_fej[4 * 2 + 3] == 0 && t.p_fej[3 * 2] == -2 && t.p_fej[3 * 2 + 1] == 1 && t.p_fej[3 * 2 + 2] == 7);
  CHECK(t.id[0] == 15 && t.id[2] == 27 && t.id[69] == 15 + 6 * 69);

  // ---- an empty range: nothing, or one zero row for the entries that want pointers ----
  {
    const FeaturePack g = pack_features({}, w.clone_slot);
    CHECK(g.F == 0 && g.M == 1 && g.uv.empty() && g.uvn.empty() && g.cidx.empty() && g.cam.empty() && g.nm.empty() && g.pf.empty());
    PackSite s;
    s.pad = 0;
    s.empty_rows = 1;
    const FeaturePack e = pack_features({}, w.clone_slot, s);
    CHECK(e.F == 0 && e.M == 1 && e.uv == std::vector<float>({0.f, 0.f}) && e.cidx == std::vector<int>({0}) && e.cam == std::vector<int>({0}));
    CHECK(e.nm == std::vector<int>({0}) && e.pf == std::vector<double>({0, 0, 0}) && e.uvn.empty());
    const ovp_general_batch gb = e.as_general_batch();
    CHECK(gb.n_feats == 0 && gb.max_meas == 1 && gb.uv && gb.clone_idx && gb.cam_idx && gb.n_meas && gb.p_FinG);
  }

  // ---- the window clean-up: nothing left, exactly one left, uvs_norm of the wrong length ----
  {
    auto gone = feat(1, {{-1, 0}, {-1, 1}, {-1, 0}}, NORM_PRESENT);
    keep_window_measurements(*gone, clones_IMU);
    CHECK(gone->timestamps.empty() && gone->uvs.empty() && gone->uvs_norm.empty() && gone->cam_ids.empty());
    auto one = feat(2, {{-1, 0}, {5, 1}, {-1, 0}}, NORM_PRESENT);
    keep_window_measurements(*one, w.clone_slot);  // (any map keyed by the clone times)
    CHECK(one->timestamps == std::vector<double>({105.0}) && one->cam_ids == std::vector<int>({1}));
    CHECK(one->uvs == std::vector<float>({33.f, 33.5f}) && one->uvs_norm == std::vector<float>({nx(2, 1), -nx(2, 1)}));
    auto no_cams = feat(3, {{4, 0}, {-1, 0}, {6, 0}}, NORM_ABSENT, false);
    keep_window_measurements(*no_cams, clones_IMU);
    CHECK(no_cams->timestamps == std::vector<double>({104.0, 106.0}) && no_cams->cam_ids.empty() && no_cams->uvs_norm.empty());
    CHECK(no_cams->uvs == std::vector<float>({48.f, 48.5f, 50.f, 50.5f}));
    auto bad_norm = feat(4, {{0, 0}, {1, 0}, {2, 0}}, NORM_SHORT);
    CHECK(bad_norm->uvs_norm.size() == 4 && !wants_triangulation(*bad_norm));
    keep_window_measurements(*bad_norm, clones_IMU);
    CHECK(bad_norm->timestamps.size() == 3 && bad_norm->uvs.size() == 6 && bad_norm->uvs_norm.empty());
    // the packer on what is left: a feature without measurements keeps its row
    const FeatureVec fv{gone, one, no_cams};
    const FeaturePack g = pack_features(feature_range(fv), w.clone_slot);
    CHECK(g.F == 3 && g.M == 2 && g.uv.size() == 12 && g.cidx.size() == 6 && g.uvn.empty());
    CHECK(g.cidx == std::vector<int>({-1, -1, 5, -1, 4, 6}) && g.cam == std::vector<int>({0, 0, 1, 0, 0, 0}) && g.nm == std::vector<int>({0, 1, 2}));
    CHECK(g.uv == std::vector<float>({0, 0, 0, 0, 33.f, 33.5f, 0, 0, 48.f, 48.5f, 50.f, 50.5f}));
    CHECK(g.pf == std::vector<double>({1, 1.25, -1, 2, 2.25, -2, 3, 3.25, -3}));
    CHECK(wants_triangulation(*one) && !wants_triangulation(*no_cams) && !wants_triangulation(*gone));
    CHECK(any_wants_triangulation(fv) && !any_wants_triangulation(FeatureVec{gone, no_cams}));
  }

  // ---- tracks of OVP_MAX_MEAS and OVP_MAX_MEAS + 1 views ----
  const auto fits = [](const Feature &f) { return f.only_camera0() && (int)f.timestamps.size() <= OVP_MAX_MEAS ? Meas::ALL : Meas::NONE; };
  {
    const FeatureVec fv{feat(5, cam0_track(OVP_MAX_MEAS, 3), NORM_ABSENT), feat(6, cam0_track(OVP_MAX_MEAS + 1), NORM_ABSENT)};
    const FeaturePack all = pack_features(feature_range(fv), w.clone_slot);
    CHECK(all.F == 2 && all.M == OVP_MAX_MEAS + 1);
    check_row(all, 0, *fv[0], first_n(OVP_MAX_MEAS), -1, false);
    check_row(all, 1, *fv[1], first_n(OVP_MAX_MEAS + 1), -1, false);
    CHECK(all.cidx[0] == 3 && all.cidx[OVP_MAX_MEAS - 1] == 34 && all.cidx[OVP_MAX_MEAS] == -1 && all.cidx[2 * OVP_MAX_MEAS + 1] == 32);
    PackSite s;  // the batch of the update: the long one is present without measurements
    s.which = fits;
    const FeaturePack b = pack_features(feature_range(fv), w.clone_slot, s);
    CHECK(b.M == OVP_MAX_MEAS);
    check_row(b, 0, *fv[0], first_n(OVP_MAX_MEAS), -1, false);
    check_row(b, 1, *fv[1], {}, -1, false);
    s.which = [](const Feature &) { return Meas::CAM0_CAPPED; };  // the triangulation rule: its first OVP_MAX_MEAS views
    const FeaturePack c = pack_features(feature_range(fv), w.clone_slot, s);
    CHECK(c.M == OVP_MAX_MEAS);
    check_row(c, 1, *fv[1], first_n(OVP_MAX_MEAS), -1, false);
    const ovp_feature_batch fb = c.as_feature_batch();
    CHECK(fb.n_feats == 2 && fb.max_meas == OVP_MAX_MEAS && fb.uv == c.uv.data() && fb.clone_idx == c.cidx.data() && fb.n_meas == c.nm.data() &&
          fb.p_FinG == c.pf.data());
  }

  // ---- tracks of OVP_GEN_MAX_MEAS and OVP_GEN_MAX_MEAS + 1 views, the general batches' pad ----
  {
    const FeatureVec fv{feat(7, cam0_track(OVP_GEN_MAX_MEAS + 1), NORM_ABSENT), feat(8, cam0_track(OVP_GEN_MAX_MEAS, 6), NORM_ABSENT)};
    PackSite s;
    s.pad = 0;
    const FeaturePack g = pack_features(feature_range(fv), w.clone_slot, s);
    CHECK(g.F == 2 && g.M == OVP_GEN_MAX_MEAS + 1 && g.cidx.size() == 2 * (OVP_GEN_MAX_MEAS + 1));
    check_row(g, 0, *fv[0], first_n(OVP_GEN_MAX_MEAS + 1), 0, false);
    check_row(g, 1, *fv[1], first_n(OVP_GEN_MAX_MEAS), 0, false);
    CHECK(g.cidx[OVP_GEN_MAX_MEAS] == 64 && g.cidx[OVP_GEN_MAX_MEAS + 1] == 6 && g.cidx[2 * OVP_GEN_MAX_MEAS + 1] == 0);
    const FeaturePack one = pack_features(feature_range(fv, std::vector<int>{1}), w.clone_slot, s);  // the features at some indices
    CHECK(one.F == 1 && one.M == OVP_GEN_MAX_MEAS);
    check_row(one, 0, *fv[1], first_n(OVP_GEN_MAX_MEAS), 0, false);
    const FeaturePack part = pack_features(feature_range(fv, 0, 1), w.clone_slot, s);  // a part of the vector
    CHECK(part.F == 1 && part.M == OVP_GEN_MAX_MEAS + 1 && part.pf[0] == 7);
  }

  // ---- no cam_ids beside two cameras' views in the same clone; the least row width ----
  {
    const FeatureVec fv{feat(9, {{2, 0}}, NORM_ABSENT, false), feat(10, {{4, 0}, {4, 1}, {5, 0}, {5, 1}}, NORM_ABSENT)};
    const FeaturePack g = pack_features(feature_range(fv), w.clone_slot);
    CHECK(g.M == 4 && g.cidx == std::vector<int>({2, -1, -1, -1, 4, 4, 5, 5}) && g.cam == std::vector<int>({0, 0, 0, 0, 0, 1, 0, 1}));
    CHECK(g.uv[8] == 160.f && g.uv[11] == 161.5f && g.uv[15] == 163.5f);
    ovp_general_batch gb = g.as_general_batch(false, false);
    CHECK(gb.n_feats == 2 && gb.max_meas == 4 && gb.uv == g.uv.data() && gb.clone_idx == g.cidx.data() && gb.n_meas == g.nm.data());
    CHECK(gb.cam_idx == nullptr && gb.p_FinG == nullptr);
    gb = g.as_general_batch(true, true);
    CHECK(gb.cam_idx == g.cam.data() && gb.p_FinG == g.pf.data());
    PackSite s;
    s.min_M = 2;
    const FeaturePack two = pack_features(feature_range(fv, 0, 1), w.clone_slot, s);
    CHECK(two.F == 1 && two.M == 2 && two.cidx == std::vector<int>({2, -1}) && two.nm == std::vector<int>({1}));
    CHECK(fits(*fv[0]) == Meas::ALL && fits(*fv[1]) == Meas::NONE);
  }

  // ---- the triangulation rule on a camera-1-first feature: camera 0's views only, at most OVP_MAX_MEAS of them ----
  {
    std::vector<View> v;
    for (int c = 0; c < 40; ++c) {
      v.push_back({c, 1});
      v.push_back({c, 0});
    }
    auto f = feat(11, v, NORM_PRESENT);
    std::vector<size_t> sel;
    for (int k = 0; k < OVP_MAX_MEAS; ++k) sel.push_back(2 * k + 1);
    CHECK(n_selected(*f, Meas::CAM0_CAPPED) == OVP_MAX_MEAS && n_selected(*f, Meas::NONE) == 0 && n_selected(*f, Meas::ALL) == 80);
    PackSite s;
    s.which = [](const Feature &) { return Meas::CAM0_CAPPED; };
    s.with_uvn = true;
    const FeaturePack g = pack_features({f.get()}, w.clone_slot, s);
    CHECK(g.M == OVP_MAX_MEAS && g.uvn.size() == g.uv.size());
    check_row(g, 0, *f, sel, -1, false);
    for (int k = 0; k < OVP_MAX_MEAS; ++k) CHECK(g.cidx[k] == k && g.uvn[2 * k] == nx(11, 2 * k + 1) && g.uvn[2 * k + 1] == -nx(11, 2 * k + 1));
  }

  // ---- uvs_norm absent, present, of the wrong length: in uvn beside the pixels, or in uv ----
  {
    const FeatureVec fv{feat(12, cam0_track(2), NORM_ABSENT), feat(13, cam0_track(3, 1), NORM_PRESENT), feat(14, cam0_track(3), NORM_SHORT)};
    PackSite s;
    s.with_uvn = true;
    const FeaturePack a = pack_features(feature_range(fv), w.clone_slot, s);
    CHECK(a.M == 3);
    for (int f = 0; f < 3; ++f) check_row(a, f, *fv[f], first_n(fv[f]->timestamps.size()), -1, false);
    CHECK(a.uvn == std::vector<float>({0, 0, 0, 0, 0, 0, nx(13, 0), -nx(13, 0), nx(13, 1), -nx(13, 1), nx(13, 2), -nx(13, 2), 0, 0, 0, 0, 0, 0}));
    PackSite n;
    n.pad = 0;
    n.uv_norm = true;
    const FeaturePack b = pack_features(feature_range(fv), w.clone_slot, n);
    CHECK(b.uvn.empty());
    check_row(b, 0, *fv[0], first_n(2), 0, true, true);
    check_row(b, 1, *fv[1], first_n(3), 0, true);
    check_row(b, 2, *fv[2], first_n(3), 0, true, true);
    CHECK(b.uv == a.uvn && b.cidx == std::vector<int>({0, 1, 0, 1, 2, 3, 0, 1, 2}) && a.cidx == std::vector<int>({0, 1, -1, 1, 2, 3, 0, 1, 2}));
  }

  // ---- the two option structs, field by field ----
  {
    ov_core::FeatureInitializerOptions fio;
    fio.triangulate_1d = true;
    fio.refine_features = false;
    fio.max_runs = 7;
    fio.init_lamda = 1.5;
    fio.max_lamda = 2.5;
    fio.min_dx = 3.5;
    fio.min_dcost = 4.5;
    fio.lam_mult = 5.5;
    fio.min_dist = 6.5;
    fio.max_dist = 7.5;
    fio.max_baseline = 8.5;
    fio.max_cond_number = 9.5;
    ovp_triang_opts to = make_triang_opts(fio);
    CHECK(to.refine_features == 0 && to.triangulate_1d == 1 && to.reserved == 0 && to.max_runs == 7 && to.init_lamda == 1.5 && to.max_lamda == 2.5);
    CHECK(to.min_dx == 3.5 && to.min_dcost == 4.5 && to.lam_mult == 5.5 && to.min_dist == 6.5 && to.max_dist == 7.5 && to.max_baseline == 8.5);
    CHECK(to.max_cond_number == 9.5);
    to = make_triang_opts(ov_core::FeatureInitializerOptions());
    CHECK(to.refine_features == 1 && to.triangulate_1d == 0 && to.max_runs == 5 && to.max_dist == 60);
    UpdaterOptions uo;
    uo.sigma_pix = 1.25;
    uo.chi2_multipler = 2.25;
    uo.sigma_pix_sq = 99;
    StateOptions so;
    so.sigma_constraint = 0.125;
    so.do_fej = true;
    so.do_calib_camera_pose = false;
    so.do_calib_camera_intrinsics = true;
    ovp_update_opts o = make_update_opts(uo, so);
    CHECK(o.sigma_px == 1.25 && o.chi2_multiplier == 2.25 && o.sigma_constraint == 0.125 && o.do_fej == 1 && o.do_calib_camera_pose == 0);
    CHECK(o.do_calib_camera_intrinsics == 1 && o.skip_plane_used == 0);
    so.do_fej = false;
    so.do_calib_camera_pose = true;
    so.do_calib_camera_intrinsics = false;
    o = make_update_opts(uo, so);
    CHECK(o.do_fej == 0 && o.do_calib_camera_pose == 1 && o.do_calib_camera_intrinsics == 0 && o.skip_plane_used == 0);
  }
  printf("host pack ok\n");
  return 0;
}
