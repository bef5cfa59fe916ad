// ov_plane::FeatureDatabase: ext ov_core::FeatureDatabase under the reference's method names, over the device database of the C-ABI
// (ovp_featdb_*, include/ovplane_hip.h).  update_feature takes a frame's observations at once; every list is in ascending feature
// id.  select() is core/VioManager.cpp:373-506 on the published class table (ov_plane_featdb_select.h: pure host code).
#pragma once
#include <cmath>
#include <limits>

#include "ov_plane_featdb_select.h"
#include "ovplane_hip.h"

namespace ov_plane {

class FeatureDatabase {
 public:
  struct Table {
    std::vector<int64_t> ids;
    std::vector<int> cls, count, cleaned;
    std::vector<uint8_t> flags;
    int totals[4] = {0, 0, 0, 0};
  };
  struct Feature {
    int64_t featid = -1;
    bool to_delete = false;
    std::vector<double> timestamps;
    std::vector<float> uvs, uvs_norm;  // [2 n]
  };

  FeatureDatabase(ovp_ctx* ctx, int max_slots = OVP_FEATDB_MAX_SLOTS, int max_meas = OVP_MAX_MEAS)
      : ctx_(ctx), S_(max_slots), M_(max_meas), rc_(ovp_featdb_create(ctx, max_slots, max_meas)) {}
  ~FeatureDatabase() {
    if (rc_ == 0) (void)ovp_featdb_destroy(ctx_);
  }
  FeatureDatabase(const FeatureDatabase&) = delete;
  FeatureDatabase& operator=(const FeatureDatabase&) = delete;
  int status() const { return rc_; }  // of the create
  ovp_ctx* context() const { return ctx_; }

  int update_feature(double timestamp, const std::vector<int64_t>& ids, const std::vector<float>& uv, const std::vector<float>& uv_norm) {
    if (uv.size() != 2 * ids.size() || uv_norm.size() != 2 * ids.size()) return OVP_E_ARG;
    return ovp_featdb_append(ctx_, timestamp, (int)ids.size(), ids.data(), uv.data(), uv_norm.data());
  }
  int classify(const std::vector<double>& clone_times, double t_now, double marg_time, int max_clone_size, bool want_marg, Table& t) {
    ovp_featdb_classify_in in;
    ovp_featdb_classify_defaults(&in);
    in.clone_times = clone_times.data(), in.n_clones = (int)clone_times.size(), in.max_clone_size = max_clone_size;
    in.t_now = t_now, in.marg_time = marg_time, in.want_marg = want_marg ? 1 : 0;
    t.ids.resize(S_), t.cls.resize(S_), t.count.resize(S_), t.cleaned.resize(S_), t.flags.resize(S_);
    ovp_featdb_classify_out out;
    out.cap = S_, out.n = 0;
    out.ids = t.ids.data(), out.cls = t.cls.data(), out.count = t.count.data(), out.cleaned = t.cleaned.data(), out.flags = t.flags.data();
    const int rc = ovp_featdb_classify(ctx_, &in, &out);
    const int n = rc ? 0 : out.n;
    t.ids.resize(n), t.cls.resize(n), t.count.resize(n), t.cleaned.resize(n), t.flags.resize(n);
    for (int k = 0; k < 4; ++k) t.totals[k] = out.totals[k];
    return rc;
  }
  // (timestamp, remove = false, skip_deleted = true)
  int features_not_containing_newer(double timestamp, std::vector<int64_t>& out) { return query(timestamp, false, out); }
  int features_containing(double timestamp, std::vector<int64_t>& out) { return query(timestamp, true, out); }
  // core/VioManager.cpp:373-506; state_times: the clone times after cloning, ascending (the oldest is margtimestep, state/State.h:70)
  int select(const std::vector<double>& state_times, double t_now, int max_clone_size, const std::vector<int64_t>& landmarks,
             int max_slam_features, bool slam_delay_ok, FeatDbSelection& sel, Table* table = nullptr) {
    Table t;
    const bool want = (int)state_times.size() > max_clone_size || state_times.size() > 5;  // :379
    const double marg = state_times.empty() ? std::numeric_limits<double>::infinity() : state_times.front();
    const int rc = classify(state_times, t_now, marg, max_clone_size, want, t);
    if (rc) return rc;
    sel = featdb_select(t.ids, t.cls, landmarks, max_slam_features, slam_delay_ok);
    if (table) *table = t;
    return 0;
  }
  int mark_deleted(const std::vector<int64_t>& ids) { return ovp_featdb_mark_deleted(ctx_, (int)ids.size(), ids.data()); }
  int gather(const std::vector<int64_t>& ids, const std::vector<double>& clone_times, const std::vector<int>* old_index = nullptr) {
    if (old_index && old_index->size() != ids.size()) return OVP_E_ARG;
    return ovp_featdb_gather(ctx_, (int)ids.size(), ids.data(), old_index ? old_index->data() : nullptr, clone_times.data(),
                             (int)clone_times.size());
  }
  int triangulate(const ovp_triang_opts& o, std::vector<double>& p_FinG, std::vector<uint8_t>& ok, int n_feats) {
    p_FinG.assign(3 * (size_t)std::max(n_feats, 1), 0.0), ok.assign((size_t)std::max(n_feats, 1), 0);
    return ovp_featdb_triangulate(ctx_, &o, p_FinG.data(), ok.data());
  }
  int cleanup() { return ovp_featdb_cleanup(ctx_, 1, std::nan("")); }
  int cleanup_measurements(double timestamp) { return ovp_featdb_cleanup(ctx_, 0, timestamp); }
  // false: the database does not hold the id (the reference's nullptr)
  bool get_feature(int64_t id, Feature& f) {
    int cnt = -1, del = 0;
    f.timestamps.assign(M_, 0.0), f.uvs.assign(2 * (size_t)M_, 0.f), f.uvs_norm.assign(2 * (size_t)M_, 0.f);
    if (ovp_featdb_get(ctx_, id, nullptr, &cnt, &del, f.timestamps.data(), f.uvs.data(), f.uvs_norm.data(), M_) || cnt < 0) return false;
    f.featid = id, f.to_delete = del != 0;
    f.timestamps.resize(cnt), f.uvs.resize(2 * (size_t)cnt), f.uvs_norm.resize(2 * (size_t)cnt);
    return true;
  }

 private:
  int query(double t, bool containing, std::vector<int64_t>& out) {
    Table tb;
    const double inf = std::numeric_limits<double>::infinity();
    const int rc = classify({}, containing ? -inf : t, containing ? t : inf, 1 << 30, containing, tb);
    out.clear();
    for (size_t i = 0; i < tb.ids.size(); ++i)
      if (tb.cls[i] == (containing ? OVP_FEATDB_MARG : OVP_FEATDB_LOST)) out.push_back(tb.ids[i]);
    return rc;
  }
  ovp_ctx* ctx_;
  int S_, M_, rc_;
};

}  // namespace ov_plane
