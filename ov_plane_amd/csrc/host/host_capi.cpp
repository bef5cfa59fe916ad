// Harness over the host mirror (tests only need C symbols to drive the C++ classes from ctypes).  An entry builds an
// ov_plane::State the way VioManager would (clone by clone through StateHelper::augment_clone), installs the given covariance, wraps
// the measurements in ov_core::Feature objects and calls the class under test.
//
// The harness holds no state of its own: what used to be armed for "the next call" travels in the ovph_run_opts the entry is handed
// (host_capi.h), its per-call results (camera 1, the shard range) come back in the same struct, and the struct's pointers are
// borrowed for that call only.  build_harness_state is the one place here that makes a State, export_state the one place that
// copies one out.
#include <cstddef>
#include <chrono>
#include <cstring>

#include "host_capi.h"
#include "ov_plane_host.h"
#include "ov_plane_trackplane.h"

using namespace ov_plane;
using namespace ov_type;

extern "C" void ovph_run_opts_defaults(ovph_run_opts *o) {
  memset(o, 0, sizeof(*o));
  o->size = sizeof(*o);
  o->fit_min_feat = 20;
  o->fit_max_cond = 100.0;
  o->comm_world = 1;
  o->seq_plane_min_feat = 20;
  o->seq_sigma_c = 0.01;
}
extern "C" int ovph_run_opts_size(void) { return (int)sizeof(ovph_run_opts); }
extern "C" int ovph_run_opts_layout(int *offsets, int cap) {
#define OVPH_OFF(m) (int)offsetof(ovph_run_opts, m)
  const int off[] = {OVPH_OFF(size), OVPH_OFF(fisheye), OVPH_OFF(uv_norm), OVPH_OFF(fit_planes), OVPH_OFF(fit_min_feat),
                     OVPH_OFF(fit_max_cond), OVPH_OFF(fit_variant), OVPH_OFF(slam_rep), OVPH_OFF(slam_anchor), OVPH_OFF(feat_rep_slam),
                     OVPH_OFF(slam_plane), OVPH_OFF(cam1_q), OVPH_OFF(cam1_p), OVPH_OFF(cam1_intr), OVPH_OFF(cam_of_meas),
                     OVPH_OFF(general_features), OVPH_OFF(general_planes), OVPH_OFF(general_plane_init), OVPH_OFF(fused_plane_fit),
                     OVPH_OFF(general_slam), OVPH_OFF(dinit_planes), OVPH_OFF(batched_retire), OVPH_OFF(featdb), OVPH_OFF(p_noplane), OVPH_OFF(comm), OVPH_OFF(comm_rank),
                     OVPH_OFF(comm_world), OVPH_OFF(device), OVPH_OFF(seq_traj), OVPH_OFF(seq_posecov), OVPH_OFF(seq_uv_norm),
                     OVPH_OFF(seq_plane), OVPH_OFF(seq_plane_mode), OVPH_OFF(seq_plane_min_feat), OVPH_OFF(seq_sigma_c),
                     OVPH_OFF(seq_planes_in_state), OVPH_OFF(last_shard), OVPH_OFF(last_cam1)};
#undef OVPH_OFF
  const int n = (int)(sizeof(off) / sizeof(off[0]));
  for (int i = 0; i < n && i < cap; ++i) offsets[i] = off[i];
  return n;
}

// These two wrap statics of UpdaterSLAM itself, not harness state: its update takes the dense form (the one a batch the device entry
// refuses falls back to) until switched off again; path of the last UpdaterSLAM::update / delayed_init (UpdaterSLAM::Route: 1 device
// general, 2 device mono, 3 dense host, 4 per-candidate host loop, 5 device loop with plane candidates, 0 none)
extern "C" void ovph_set_slam_force_dense(int on) { UpdaterSLAM::force_dense_for_tests(on != 0); }
extern "C" int ovph_last_slam_route() { return UpdaterSLAM::last_route(); }

namespace ov_plane {
struct StateTestAccess {
  static void replace_last_variable(std::shared_ptr<State> state, std::shared_ptr<Type> v) { state->_variables.back() = v; }
};
}  // namespace ov_plane

namespace {
// the options an entry works with: the caller's (results are written back into them) or, for NULL, defaults in `local`;
// nullptr when the caller's struct is not this build's
ovph_run_opts *use_opts(ovph_run_opts *given, ovph_run_opts *local) {
  if (!given) {
    ovph_run_opts_defaults(local);
    return local;
  }
  return given->size == sizeof(ovph_run_opts) ? given : nullptr;
}

struct HarnessState {
  std::shared_ptr<State> state;
  std::vector<double> times;  // of the clones, oldest first
  std::vector<std::shared_ptr<Landmark>> landmarks;
  std::vector<std::shared_ptr<Vec>> planes;
  std::vector<std::shared_ptr<Type>> order;  // imu, dt, calib0, intr0, [calib1, intr1], clones, landmarks, planes (= synth.state_layout)
};

// What a State is built from.  Where the entries differ, the difference is a member here.
struct StateSpec {
  int C = 0;
  const double *clone_q = nullptr, *clone_p = nullptr;          // [C][4], [C][3], oldest first
  const double *clone_q_fej = nullptr, *clone_p_fej = nullptr;  // nullptr: first estimate = value
  const double *calib_q = nullptr, *calib_p = nullptr, *intr = nullptr;  // camera 0; nullptr: what State's constructor gave it
  bool second_camera = false;  // camera 1 of the options (cam1_q / cam1_p / cam1_intr), its variables behind camera 0's
  bool set_fej = true;         // false (ovph_format_state_files): values only, no first estimate is written anywhere
  // IMU value at t_state (propagation / ZUPT / sequence entries).  With it the window ends one camera period (0.1) before t_state
  // - clone i at t_state - 0.1 (C - i) - and the state's time and camera time offset are set; without it clone i is at 100 + 0.1 i
  // and neither is touched.
  const double *imu_x16 = nullptr, *imu_x16_fej = nullptr;
  double calib_dt = 0.0, t_state = 0.0;
  int n_slam = 0;  // SLAM landmarks, GLOBAL_3D, ids 9000 + k
  const double *slam_p = nullptr, *slam_p_fej = nullptr;  // nullptr: first estimate = value
  int n_planes = 0;  // planes of the state
  const double *cp = nullptr, *cp_fej = nullptr;  // nullptr: first estimate = value
  const size_t *plane_ids = nullptr;              // nullptr: k + 1
  int N = 0;  // size the covariance must come out at, and the covariance
  const double *P = nullptr;
};

VectorXd vec_of(const double *a, int na, const double *b = nullptr, int nb = 0) {
  VectorXd v(na + nb, 1);
  for (int k = 0; k < na; ++k) v(k) = a[k];
  for (int k = 0; k < nb; ++k) v(na + k) = b[k];
  return v;
}

// The only place of this file that makes a State.
int build_harness_state(HarnessState &hs, StateOptions &so, const StateSpec &sp, const ovph_run_opts &o) {
  if (sp.second_camera) so.num_cameras = 2;
  hs.state = std::make_shared<State>(so);
  auto &state = hs.state;
  auto put = [&](const std::shared_ptr<Type> &var, const VectorXd &v, const VectorXd &vf) {
    var->set_value(v);
    if (sp.set_fej) var->set_fej(vf);
  };
  state->_cam_fisheye[0] = o.fisheye != 0;
  if (sp.second_camera) {
    const VectorXd v1 = vec_of(o.cam1_q, 4, o.cam1_p, 3), iv1 = vec_of(o.cam1_intr, 8);
    put(state->_calib_IMUtoCAM.at(1), v1, v1);
    put(state->_cam_intrinsics.at(1), iv1, iv1);
    state->_cam_fisheye[1] = false;
  }
  if (sp.calib_q) {
    const VectorXd v = vec_of(sp.calib_q, 4, sp.calib_p, 3), iv = vec_of(sp.intr, 8);
    put(state->_calib_IMUtoCAM.at(0), v, v);
    put(state->_cam_intrinsics.at(0), iv, iv);
  }
  // clones, oldest first, through the reference's own entry point
  const double w0[3] = {0, 0, 0};
  const double *qf = sp.clone_q_fej ? sp.clone_q_fej : sp.clone_q, *pf = sp.clone_p_fej ? sp.clone_p_fej : sp.clone_p;
  hs.times.resize(sp.C);
  for (int i = 0; i < sp.C; ++i) {
    put(state->_imu->pose(), vec_of(sp.clone_q + 4 * i, 4, sp.clone_p + 3 * i, 3), vec_of(qf + 4 * i, 4, pf + 3 * i, 3));
    hs.times[i] = sp.imu_x16 ? sp.t_state - 0.1 * (sp.C - i) : 100.0 + 0.1 * i;
    state->_timestamp = hs.times[i];
    StateHelper::augment_clone(state, w0);
  }
  // 3-dof variables: grow the covariance through StateHelper::clone of the IMU position (sizes match; the block is overwritten
  // below), then swap the cloned Vec for the variable type the updaters expect at the same id, or relabel its value
  for (int k = 0; k < sp.n_slam; ++k) {
    std::shared_ptr<Type> t = StateHelper::clone(state, state->_imu->p());
    auto lm = std::make_shared<Landmark>(3);
    lm->set_local_id(t->id());
    lm->_featid = 9000 + k;
    lm->set_from_xyz(sp.slam_p + 3 * k, false);
    lm->set_from_xyz((sp.slam_p_fej ? sp.slam_p_fej : sp.slam_p) + 3 * k, true);
    StateTestAccess::replace_last_variable(state, lm);
    state->_features_SLAM[lm->_featid] = lm;
    hs.landmarks.push_back(lm);
  }
  for (int k = 0; k < sp.n_planes; ++k) {
    auto pl = std::dynamic_pointer_cast<Vec>(StateHelper::clone(state, state->_imu->p()));
    if (!pl) return -10;
    put(pl, vec_of(sp.cp + 3 * k, 3), vec_of((sp.cp_fej ? sp.cp_fej : sp.cp) + 3 * k, 3));
    state->_features_PLANE[sp.plane_ids ? sp.plane_ids[k] : (size_t)(k + 1)] = pl;
    hs.planes.push_back(pl);
  }
  if (state->max_covariance_size() != sp.N) return -11;
  if (sp.imu_x16) {
    put(state->_imu, vec_of(sp.imu_x16, 16), vec_of(sp.imu_x16_fej, 16));
    const VectorXd dtv = vec_of(&sp.calib_dt, 1);
    put(state->_calib_dt_CAMtoIMU, dtv, dtv);
    state->_timestamp = sp.t_state;
  }
  auto &order = hs.order;
  order.push_back(state->_imu);
  order.push_back(state->_calib_dt_CAMtoIMU);
  order.push_back(state->_calib_IMUtoCAM.at(0));
  order.push_back(state->_cam_intrinsics.at(0));
  if (sp.second_camera) {
    order.push_back(state->_calib_IMUtoCAM.at(1));
    order.push_back(state->_cam_intrinsics.at(1));
  }
  for (auto &c : state->_clones_IMU) order.push_back(c.second);
  for (auto &l : hs.landmarks) order.push_back(l);
  for (auto &p : hs.planes) order.push_back(p);
  MatrixXd Pm(sp.N, sp.N);
  memcpy(Pm.data(), sp.P, sizeof(double) * (size_t)sp.N * sp.N);
  StateHelper::set_initial_covariance(state, Pm, order);
  return 0;
}

// Feature f of the batch gets id id0 + f.  cam_of [F][M]: camera of every measurement, or nullptr.  uv_norm [F][M][2]: features as
// the tracker hands them over - normalised measurements, no position yet; else p_FinG [F][3] (or nullptr)
std::vector<std::shared_ptr<ov_core::Feature>> make_features(const HarnessState &hs, int F, int M, const float *uv, const int *clone_idx,
                                                             const int *n_meas, const double *p_FinG, size_t id0, const int *cam_of,
                                                             const float *uv_norm) {
  std::vector<std::shared_ptr<ov_core::Feature>> fv;
  for (int f = 0; f < F; ++f) {
    auto ft = std::make_shared<ov_core::Feature>();
    ft->featid = id0 + f;
    for (int k = 0; k < n_meas[f]; ++k) {
      ft->timestamps.push_back(hs.times[clone_idx[(size_t)f * M + k]]);
      ft->uvs.push_back(uv[((size_t)f * M + k) * 2]);
      ft->uvs.push_back(uv[((size_t)f * M + k) * 2 + 1]);
      if (cam_of) ft->cam_ids.push_back(cam_of[(size_t)f * M + k]);
    }
    if (uv_norm) {
      for (int k = 0; k < n_meas[f]; ++k) {
        ft->uvs_norm.push_back(uv_norm[((size_t)f * M + k) * 2]);
        ft->uvs_norm.push_back(uv_norm[((size_t)f * M + k) * 2 + 1]);
      }
    } else if (p_FinG) {
      memcpy(ft->p_FinG, p_FinG + 3 * f, 3 * sizeof(double));
    }
    fv.push_back(ft);
  }
  return fv;
}

// A device database on the state's context holding every measurement of `fv`, fed as a tracker would: one update_feature per
// clone time, oldest first, the features in the vector's order.
int attach_fed_database(HarnessState &hs, const std::vector<std::shared_ptr<ov_core::Feature>> &fv) {
  if (fv.size() > OVP_FEATDB_MAX_SLOTS) return OVP_E_CAPACITY;
  auto db = std::make_shared<FeatureDatabase>(hs.state->gpu(), std::max<int>(1, (int)fv.size()), OVP_MAX_MEAS);
  if (db->status()) return db->status();
  for (double t : hs.times) {
    std::vector<int64_t> ids;
    std::vector<float> uv, uvn;
    for (const auto &ft : fv)
      for (size_t k = 0; k < ft->timestamps.size(); ++k)
        if (ft->timestamps[k] == t && ft->cam_of(k) == 0 && ft->uvs_norm.size() == ft->uvs.size()) {
          ids.push_back((int64_t)ft->featid);
          uv.insert(uv.end(), {ft->uvs[2 * k], ft->uvs[2 * k + 1]});
          uvn.insert(uvn.end(), {ft->uvs_norm[2 * k], ft->uvs_norm[2 * k + 1]});
        }
    if (int rc = db->update_feature(t, ids, uv, uvn)) return rc;
  }
  hs.state->_featdb = db;
  return 0;
}

// Where export_state copies the state to; a nullptr member is skipped.  P is column-major at the state's size, which goes to n.
struct StateOut {
  double *clone_q = nullptr, *clone_p = nullptr, *calib_q = nullptr, *calib_p = nullptr, *intr = nullptr;
  double *slam_p = nullptr, *cp = nullptr, *P = nullptr;
  int *n = nullptr;
};

// The only place of this file that copies clones, calibration, intrinsics, landmarks, planes and the covariance out; camera 1 of a
// state that has one goes to o.last_cam1.
void export_state(const HarnessState &hs, const StateOut &out, ovph_run_opts &o) {
  auto &state = hs.state;
  int i = 0;
  for (auto &c : state->_clones_IMU) {
    if (out.clone_q) memcpy(out.clone_q + 4 * i, c.second->quat(), 4 * sizeof(double));
    if (out.clone_p) memcpy(out.clone_p + 3 * i, c.second->pos(), 3 * sizeof(double));
    ++i;
  }
  if (out.calib_q) memcpy(out.calib_q, state->_calib_IMUtoCAM.at(0)->quat(), 4 * sizeof(double));
  if (out.calib_p) memcpy(out.calib_p, state->_calib_IMUtoCAM.at(0)->pos(), 3 * sizeof(double));
  if (out.intr) memcpy(out.intr, state->_cam_intrinsics.at(0)->value().data(), 8 * sizeof(double));
  for (size_t k = 0; k < hs.landmarks.size() && out.slam_p; ++k)
    memcpy(out.slam_p + 3 * k, hs.landmarks[k]->value().data(), 3 * sizeof(double));
  for (size_t k = 0; k < hs.planes.size() && out.cp; ++k) memcpy(out.cp + 3 * k, hs.planes[k]->value().data(), 3 * sizeof(double));
  const int n2 = state->max_covariance_size();
  if (out.P) {
    MatrixXd Pn = StateHelper::get_full_covariance(state);
    memcpy(out.P, Pn.data(), sizeof(double) * (size_t)n2 * n2);
  }
  if (out.n) *out.n = n2;
  if (state->_options.num_cameras > 1) {
    memcpy(o.last_cam1, state->_calib_IMUtoCAM.at(1)->quat(), 4 * sizeof(double));
    memcpy(o.last_cam1 + 4, state->_calib_IMUtoCAM.at(1)->pos(), 3 * sizeof(double));
    memcpy(o.last_cam1 + 7, state->_cam_intrinsics.at(1)->value().data(), 8 * sizeof(double));
  }
}

NoiseManager noise_of(const double *sigmas4 /* w a wb ab */) {
  NoiseManager nm;
  nm.sigma_w = sigmas4[0];
  nm.sigma_a = sigmas4[1];
  nm.sigma_wb = sigmas4[2];
  nm.sigma_ab = sigmas4[3];
  return nm;
}

template <class Sink> void feed_imu_rows(Sink &sink, int n_imu, const double *imu /* rows (t, wm, am) */) {
  for (int i = 0; i < n_imu; ++i) {
    ov_core::ImuData d;
    d.timestamp = imu[7 * i];
    for (int k = 0; k < 3; ++k) {
      d.wm[k] = imu[7 * i + 1 + k];
      d.am[k] = imu[7 * i + 4 + k];
    }
    sink.feed_imu(d);
  }
}
}  // namespace

// UpdaterMSCKF::update.  In-state planes carry the ids plane_ids_state; the estimates of the planes outside the state are handed
// over unless the options ask the updater to fit them (fit_planes).  Options read: fisheye, uv_norm, fit_*, cam1_* / cam_of_meas,
// general_features, general_planes, fused_plane_fit, comm / comm_rank / comm_world / device; written: last_shard, last_cam1.
extern "C" int ovph_run_msckf_update(int C, const double *clone_q, const double *clone_p, const double *clone_q_fej,
                                     const double *clone_p_fej, const double *calib_q, const double *calib_p,
                                     const double *intr, int n_planes_in_state, const double *cp_state,
                                     const double *cp_state_fej, const size_t *plane_ids_state, int n_planes_out,
                                     const double *cp_out, const size_t *plane_ids_out, int N, const double *P, int F, int M,
                                     const float *uv, const int *clone_idx, const int *n_meas, const double *p_FinG,
                                     const int *plane_of_feat /* reference plane id or 0 */, double sigma_px,
                                     double chi2_mult, double sigma_c, int do_fej,
                                     /* outputs */ double *out_clone_q, double *out_clone_p, double *out_calib_q,
                                     double *out_calib_p, double *out_intr, double *out_cp_state, double *out_P,
                                     unsigned char *feat_kept, unsigned char *feat_used, unsigned char *feat_deleted,
                                     ovph_run_opts *opts) {
  ovph_run_opts dflt, *op = use_opts(opts, &dflt);
  if (!op) return OVPH_E_OPTS;
  ovph_run_opts &o = *op;
  StateOptions so;
  so.do_fej = do_fej != 0;
  so.do_calib_camera_pose = so.do_calib_camera_intrinsics = so.do_calib_camera_timeoffset = true;
  so.max_clone_size = C;
  so.use_plane_constraint = so.use_plane_constraint_msckf = true;
  so.sigma_constraint = sigma_c;
  if (o.fit_planes) {
    so.plane_msckf_min_feat = o.fit_min_feat;
    so.plane_msckf_max_cond = o.fit_max_cond;
    so.planefit_shuffle_variant = o.fit_variant;
  }
  so.max_state_size = N + 8;
  so.max_features = F + 8;
  so.gpu_device = o.device;
  so.gpu_general_features = o.general_features != 0;
  so.gpu_general_planes = o.general_planes != 0;
  so.gpu_fused_plane_fit = o.fused_plane_fit != 0;
  so.gpu_featdb = o.featdb != 0;
  StateSpec sp;
  sp.C = C, sp.clone_q = clone_q, sp.clone_p = clone_p, sp.clone_q_fej = clone_q_fej, sp.clone_p_fej = clone_p_fej;
  sp.calib_q = calib_q, sp.calib_p = calib_p, sp.intr = intr, sp.second_camera = o.cam1_q != nullptr;
  sp.n_planes = n_planes_in_state, sp.cp = cp_state, sp.cp_fej = cp_state_fej, sp.plane_ids = plane_ids_state;
  sp.N = N, sp.P = P;
  HarnessState hs;
  if (int rc = build_harness_state(hs, so, sp, o)) return rc;
  auto &state = hs.state;
  if (!o.fit_planes)  // otherwise UpdaterMSCKF::update fits / refines the planes itself (UpdaterMSCKF.cpp:196-400)
    for (int k = 0; k < n_planes_out; ++k)
      state->_plane_estimates_cp_inG[plane_ids_out[k]] = {cp_out[3 * k], cp_out[3 * k + 1], cp_out[3 * k + 2]};
  // unlike ovph_run_updater, the camera of a measurement is handed on whenever it is given, second camera or not
  auto fv = make_features(hs, F, M, uv, clone_idx, n_meas, p_FinG, 5000, o.cam_of_meas, o.uv_norm);
  const auto all = fv;
  if (so.gpu_featdb)  // the tracker's side of StateOptions::gpu_featdb: the same observations, clone time by clone time
    if (int rc = attach_fed_database(hs, fv)) return rc;
  std::vector<std::shared_ptr<ov_core::Feature>> fextra, fused;
  std::map<size_t, size_t> feat2plane;
  for (int f = 0; f < F; ++f)
    if (plane_of_feat[f] > 0) feat2plane[5000 + f] = (size_t)plane_of_feat[f];
  UpdaterOptions uo;
  uo.sigma_pix = sigma_px;
  uo.chi2_multipler = chi2_mult;
  ov_core::FeatureInitializerOptions fio;
  UpdaterMSCKF updater(uo, fio);
  if (o.comm || o.comm_world > 1) updater.set_communicator(o.comm, o.comm_rank, o.comm_world);
  updater.update(state, fv, fextra, fused, feat2plane);
  updater.last_shard(o.last_shard[0], o.last_shard[1]);
  StateOut out;
  out.clone_q = out_clone_q, out.clone_p = out_clone_p, out.calib_q = out_calib_q, out.calib_p = out_calib_p, out.intr = out_intr;
  out.cp = out_cp_state, out.P = out_P;
  export_state(hs, out, o);
  for (int f = 0; f < F; ++f) {
    feat_kept[f] = 0;
    feat_used[f] = 0;
    feat_deleted[f] = all[f]->to_delete ? 1 : 0;
  }
  for (auto &ft : fv) feat_kept[ft->featid - 5000] = 1;
  for (auto &ft : fused) feat_used[ft->featid - 5000] = 1;
  return 0;
}

// Harness for StateHelper::initialize: state with C clones (first estimate = value) and the calibration State's constructor gives,
// covariance P (N x N), a new Vec(k) variable.  order_ids[n_order] select the measuring variables by Type::id() (clones /
// calibration / intrinsics).  Options read: fisheye.
extern "C" int ovph_run_initialize(int C, const double *clone_q, const double *clone_p, int N, const double *P, int n_order,
                                   const int *order_ids, int rows, int cols, const double *H_R, int k, const double *H_L,
                                   const double *res, double r_iso, double chi2_mult, const double *new_value0,
                                   double *out_P /* (N+k)^2 */, double *out_new_value, double *out_clone_q,
                                   double *out_clone_p, double *out_calib_p, double *out_intr, ovph_run_opts *opts) {
  ovph_run_opts dflt, *op = use_opts(opts, &dflt);
  if (!op) return OVPH_E_OPTS;
  StateOptions so;
  so.do_calib_camera_pose = so.do_calib_camera_intrinsics = so.do_calib_camera_timeoffset = true;
  so.max_clone_size = C;
  so.max_state_size = N + 16;
  so.max_features = 16;
  StateSpec sp;
  sp.C = C, sp.clone_q = clone_q, sp.clone_p = clone_p, sp.N = N, sp.P = P;
  HarnessState hs;
  if (int rc = build_harness_state(hs, so, sp, *op)) return rc;
  auto &state = hs.state;
  std::vector<std::shared_ptr<Type>> H_order;
  for (int i = 0; i < n_order; ++i) {
    std::shared_ptr<Type> found;
    for (auto &v : hs.order)
      if (v->id() == order_ids[i]) found = v;
    if (!found) return -12;
    H_order.push_back(found);
  }
  MatrixXd HR(rows, cols), HL(rows, k), R = MatrixXd::Zero(rows, rows);
  VectorXd r(rows, 1);
  memcpy(HR.data(), H_R, sizeof(double) * (size_t)rows * cols);
  memcpy(HL.data(), H_L, sizeof(double) * (size_t)rows * k);
  memcpy(r.data(), res, sizeof(double) * rows);
  for (int i = 0; i < rows; ++i) R(i, i) = r_iso;
  auto nv = std::make_shared<Vec>(k);
  const VectorXd v0 = vec_of(new_value0, k);
  nv->set_value(v0);
  nv->set_fej(v0);
  const bool ok = StateHelper::initialize(state, nv, H_order, HR, HL, R, r, chi2_mult, true);
  memcpy(out_new_value, nv->value().data(), sizeof(double) * k);
  StateOut out;
  out.clone_q = out_clone_q, out.clone_p = out_clone_p, out.calib_p = out_calib_p, out.intr = out_intr, out.P = out_P;
  export_state(hs, out, *op);
  return ok ? 1 : 0;
}

// mode 3: UpdaterMSCKF::update on a state that also holds SLAM landmarks (ids 9000 + k, planes from the options' slam_plane) and
// n_planes in-state planes (ids 1..n_planes); the features carry normalised measurements, the updater triangulates, fits and
// refines (fit_planes must be on).
// mode 0: UpdaterSLAM::update (feature f observes landmark f, n_slam == F); mode 1: UpdaterSLAM::delayed_init (n_slam == 0,
// out_new_p [F*3] / out_new_id [F] describe the landmarks that joined the state); mode 2: UpdaterPlane::init_vio_plane
// (n_planes in-state planes must be 0; cp_out_est [n_planes_out*3] are the upstream plane estimates with ids 1..n).
// Options read: fisheye, uv_norm, fit_*, cam1_* / cam_of_meas (a stereo state and the camera of every measurement), fused_plane_fit,
// general_slam, dinit_planes, general_plane_init; slam_rep / slam_anchor (mode 0), feat_rep_slam / p_noplane (mode 1), slam_plane
// (mode 3); written: last_cam1.
extern "C" int ovph_run_updater(int mode, int C, const double *clone_q, const double *clone_p, const double *clone_q_fej,
                                const double *clone_p_fej, const double *calib_q, const double *calib_p, const double *intr,
                                int n_slam, const double *slam_p, const double *slam_p_fej, int n_planes, const double *cp,
                                const double *cp_fej, int n_planes_out, const double *cp_out_est, int N, const double *P, int F,
                                int M, const float *uv, const int *clone_idx, const int *n_meas, const double *p_FinG,
                                const int *plane_of_feat, double sigma_px, double chi2_mult, double sigma_c, int do_fej,
                                double const_init_multi, double const_init_chi2, int n_cap,
                                /* outputs */ double *out_clone_q, double *out_clone_p, double *out_calib_q, double *out_calib_p,
                                double *out_intr, double *out_slam_p, double *out_cp, double *out_P, int *out_n,
                                unsigned char *feat_kept, unsigned char *feat_deleted, unsigned char *lm_should_marg,
                                int *slam_to_plane, double *out_new_p, int *out_new_id, ovph_run_opts *opts) {
  ovph_run_opts dflt, *op = use_opts(opts, &dflt);
  if (!op) return OVPH_E_OPTS;
  ovph_run_opts &o = *op;
  StateOptions so;
  so.do_fej = do_fej != 0;
  so.do_calib_camera_pose = so.do_calib_camera_intrinsics = so.do_calib_camera_timeoffset = true;
  so.max_clone_size = C;
  so.use_plane_constraint = so.use_plane_constraint_msckf = so.use_plane_constraint_slamu = so.use_plane_constraint_slamd = true;
  so.sigma_constraint = sigma_c;
  so.const_init_multi = const_init_multi;
  so.const_init_chi2 = const_init_chi2;
  if (o.fit_planes) {
    so.plane_init_min_feat = so.plane_msckf_min_feat = o.fit_min_feat;
    so.plane_init_max_cond = so.plane_msckf_max_cond = o.fit_max_cond;
    so.planefit_shuffle_variant = o.fit_variant;
  }
  so.max_state_size = n_cap;
  so.max_features = F + 8;
  so.gpu_fused_plane_fit = o.fused_plane_fit != 0;
  so.gpu_general_slam = o.general_slam != 0;
  so.gpu_dinit_planes = o.dinit_planes != 0;
  so.gpu_general_plane_init = o.general_plane_init != 0;
  StateSpec sp;
  sp.C = C, sp.clone_q = clone_q, sp.clone_p = clone_p, sp.clone_q_fej = clone_q_fej, sp.clone_p_fej = clone_p_fej;
  sp.calib_q = calib_q, sp.calib_p = calib_p, sp.intr = intr, sp.second_camera = o.cam1_q != nullptr;
  sp.n_slam = n_slam, sp.slam_p = slam_p, sp.slam_p_fej = slam_p_fej, sp.n_planes = n_planes, sp.cp = cp, sp.cp_fej = cp_fej;
  sp.N = N, sp.P = P;
  HarnessState hs;
  if (int rc = build_harness_state(hs, so, sp, o)) return rc;
  auto &state = hs.state;
  const size_t id0 = (mode == 0) ? 9000 : 5000;
  auto fv = make_features(hs, F, M, uv, clone_idx, n_meas, p_FinG, id0, sp.second_camera ? o.cam_of_meas : nullptr, o.uv_norm);
  auto all = fv;
  if (o.p_noplane && mode == 1)
    for (int f = 0; f < F; ++f) {
      fv[f]->has_p_FinG_original = true;
      memcpy(fv[f]->p_FinG_original, o.p_noplane + 3 * f, 3 * sizeof(double));
    }
  std::map<size_t, size_t> feat2plane;
  for (int f = 0; f < F; ++f)
    if (plane_of_feat && plane_of_feat[f] > 0) feat2plane[id0 + f] = (size_t)plane_of_feat[f];
  UpdaterOptions uo, ua;
  uo.sigma_pix = sigma_px;
  uo.chi2_multipler = chi2_mult;
  ua = uo;
  ov_core::FeatureInitializerOptions fio;
  StateOut out;
  out.clone_q = out_clone_q, out.clone_p = out_clone_p, out.calib_q = out_calib_q, out.calib_p = out_calib_p, out.intr = out_intr;
  out.slam_p = out_slam_p, out.cp = out_cp, out.P = out_P, out.n = out_n;
  if (mode == 3) {
    for (int k = 0; k < n_slam && o.slam_plane; ++k)
      if (o.slam_plane[k] > 0) feat2plane[9000 + k] = (size_t)o.slam_plane[k];
    UpdaterMSCKF up(uo, fio);
    std::vector<std::shared_ptr<ov_core::Feature>> fextra, fused;
    up.update(state, fv, fextra, fused, feat2plane);
    std::set<size_t> left;
    for (auto &ft : fv) left.insert(ft->featid);
    export_state(hs, out, o);
    for (int f = 0; f < F; ++f) {
      feat_kept[f] = left.count(id0 + f) ? 1 : 0;
      feat_deleted[f] = all[f]->to_delete ? 1 : 0;
      slam_to_plane[f] = -1;
    }
    for (int k = 0; k < n_slam && k < F; ++k) {
      auto it = state->_features_SLAM_to_PLANE.find(9000 + k);
      if (it != state->_features_SLAM_to_PLANE.end()) slam_to_plane[k] = (int)it->second;
    }
    return 0;
  }
  if (mode == 0 && o.slam_rep != 0) {
    // re-express the landmarks (built as GLOBAL_3D from their global value / first estimate) in the requested representation
    auto calib = state->_calib_IMUtoCAM.at(0);
    auto anchor = state->_clones_IMU.at(hs.times[o.slam_anchor]);
    for (auto &lm : hs.landmarks) {
      double pg[3], pgf[3], pa[3], paf[3], t[3];
      lm->get_xyz(false, pg);
      lm->get_xyz(true, pgf);
      lm->_feat_representation = (LandmarkRepresentation::Representation)o.slam_rep;
      if (LandmarkRepresentation::is_relative_representation(lm->_feat_representation)) {
        lm->_anchor_cam_id = 0;
        lm->_anchor_clone_timestamp = hs.times[o.slam_anchor];
        for (int pass = 0; pass < 2; ++pass) {
          const double *R = pass ? anchor->Rot_fej() : anchor->Rot(), *pp = pass ? anchor->pos_fej() : anchor->pos();
          const double *src = pass ? pgf : pg;
          double *dst = pass ? paf : pa;
          const double d[3] = {src[0] - pp[0], src[1] - pp[1], src[2] - pp[2]};
          for (int i = 0; i < 3; ++i) t[i] = R[3 * i] * d[0] + R[3 * i + 1] * d[1] + R[3 * i + 2] * d[2];
          for (int i = 0; i < 3; ++i)
            dst[i] = calib->Rot()[3 * i] * t[0] + calib->Rot()[3 * i + 1] * t[1] + calib->Rot()[3 * i + 2] * t[2] + calib->pos()[i];
        }
        lm->set_from_xyz(pa, false);
        lm->set_from_xyz(paf, true);
      } else {
        lm->set_from_xyz(pg, false);
        lm->set_from_xyz(pgf, true);
      }
    }
  }
  if (mode == 0) {
    UpdaterSLAM up(uo, ua, fio);
    up.update(state, fv, feat2plane);
  } else if (mode == 1) {
    UpdaterSLAM up(uo, ua, fio);
    state->_options.feat_rep_slam = (LandmarkRepresentation::Representation)o.feat_rep_slam;
    up.delayed_init(state, fv, feat2plane);
    for (int f = 0; f < F; ++f) {
      out_new_id[f] = -1;
      auto it = state->_features_SLAM.find(id0 + f);
      if (it == state->_features_SLAM.end()) continue;
      out_new_id[f] = it->second->id();
      memcpy(out_new_p + 3 * f, it->second->value().data(), (size_t)it->second->size() * sizeof(double));
    }
  } else {
    if (!o.fit_planes)  // otherwise init_vio_plane triangulates, fits and refines itself (UpdaterPlane.cpp:76-290)
      for (int k = 0; k < n_planes_out; ++k)
        state->_plane_estimates_cp_inG[(size_t)(k + 1)] = {cp_out_est[3 * k], cp_out_est[3 * k + 1], cp_out_est[3 * k + 2]};
    UpdaterPlane up(uo, fio);
    std::vector<std::shared_ptr<ov_core::Feature>> used;
    up.init_vio_plane(state, fv, used, feat2plane);
    for (int k = 0; k < n_planes_out; ++k) {
      out_new_id[k] = -1;
      auto it = state->_features_PLANE.find((size_t)(k + 1));
      if (it == state->_features_PLANE.end()) continue;
      out_new_id[k] = it->second->id();
      memcpy(out_new_p + 3 * k, it->second->value().data(), 3 * sizeof(double));
    }
  }
  export_state(hs, out, o);
  for (int f = 0; f < F; ++f) {
    feat_kept[f] = 0;
    feat_deleted[f] = all[f]->to_delete ? 1 : 0;
    slam_to_plane[f] = -1;
    auto it = state->_features_SLAM_to_PLANE.find(id0 + f);
    if (it != state->_features_SLAM_to_PLANE.end()) slam_to_plane[f] = (int)it->second;
  }
  for (auto &ft : fv) feat_kept[ft->featid - id0] = 1;
  for (size_t k = 0; k < hs.landmarks.size(); ++k) lm_should_marg[k] = hs.landmarks[k]->should_marg ? 1 : 0;
  return 0;
}

// Propagator::propagate_and_clone harness: state with C clones (first estimate = value; State's own calibration), IMU state
// x16 / x16_fej, covariance P, n_imu readings rows (t, wm, am).  state->_timestamp = t_state, camera time offset calib_dt;
// propagates to `timestamp`.
// gpu_propagate: StateOptions::gpu_propagate (ovph_run_propagate_opt; ovph_run_propagate is the same call with the option off);
// out_new_clone_id: Type::id() of the clone registered at `timestamp`; out_ms: host clock around propagate_and_clone (may be NULL)
static int run_propagate(int C, const double *clone_q, const double *clone_p, const double *imu_x16, const double *imu_x16_fej,
                         double calib_dt, int N, const double *P, int n_imu, const double *imu, double t_state, double timestamp,
                         const double *sigmas4 /* w a wb ab */, double gravity_mag, int use_rk4, int imu_avg, int do_fej,
                         /* outputs */ double *out_x16, double *out_x16_fej, double *out_Phi, double *out_Qd, double *out_last_w,
                         double *out_P /* (N+6)^2 */, double *out_new_clone7, int gpu_propagate, int *out_new_clone_id,
                         double *out_ms) {
  ovph_run_opts o;
  ovph_run_opts_defaults(&o);
  StateOptions so;
  so.gpu_propagate = gpu_propagate != 0;
  so.do_fej = do_fej != 0;
  so.do_calib_camera_pose = so.do_calib_camera_intrinsics = so.do_calib_camera_timeoffset = true;
  so.max_clone_size = C + 1;
  so.use_rk4_integration = use_rk4 != 0;
  so.imu_avg = imu_avg != 0;
  so.max_state_size = N + 16;
  so.max_features = 16;
  StateSpec sp;
  sp.C = C, sp.clone_q = clone_q, sp.clone_p = clone_p, sp.N = N, sp.P = P;
  sp.imu_x16 = imu_x16, sp.imu_x16_fej = imu_x16_fej, sp.calib_dt = calib_dt, sp.t_state = t_state;
  HarnessState hs;
  if (int rc = build_harness_state(hs, so, sp, o)) return rc;
  auto &state = hs.state;
  Propagator prop(noise_of(sigmas4), gravity_mag);
  feed_imu_rows(prop, n_imu, imu);
  const auto t_start = std::chrono::steady_clock::now();
  prop.propagate_and_clone(state, timestamp);
  if (out_ms) *out_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
  memcpy(out_x16, state->_imu->value().data(), 16 * sizeof(double));
  memcpy(out_x16_fej, state->_imu->fej().data(), 16 * sizeof(double));
  memcpy(out_Phi, prop.last_Phi(), 225 * sizeof(double));
  memcpy(out_Qd, prop.last_Qd(), 225 * sizeof(double));
  memcpy(out_last_w, prop.last_w(), 3 * sizeof(double));
  if (state->max_covariance_size() != N + 6) return -12;
  StateOut out;
  out.P = out_P;
  export_state(hs, out, o);
  auto nc = state->_clones_IMU.at(timestamp);
  memcpy(out_new_clone7, nc->value().data(), 7 * sizeof(double));
  if (out_new_clone_id) *out_new_clone_id = nc->id();
  return 0;
}

extern "C" int ovph_run_propagate(int C, const double *clone_q, const double *clone_p, const double *imu_x16, const double *imu_x16_fej,
                                  double calib_dt, int N, const double *P, int n_imu, const double *imu, double t_state,
                                  double timestamp, const double *sigmas4 /* w a wb ab */, double gravity_mag, int use_rk4,
                                  int imu_avg, int do_fej,
                                  /* outputs */ double *out_x16, double *out_x16_fej, double *out_Phi, double *out_Qd, double *out_last_w,
                                  double *out_P /* (N+6)^2 */, double *out_new_clone7) {
  return run_propagate(C, clone_q, clone_p, imu_x16, imu_x16_fej, calib_dt, N, P, n_imu, imu, t_state, timestamp, sigmas4, gravity_mag,
                       use_rk4, imu_avg, do_fej, out_x16, out_x16_fej, out_Phi, out_Qd, out_last_w, out_P, out_new_clone7, 0, nullptr,
                       nullptr);
}

extern "C" int ovph_run_propagate_opt(int C, const double *clone_q, const double *clone_p, const double *imu_x16,
                                      const double *imu_x16_fej, double calib_dt, int N, const double *P, int n_imu, const double *imu,
                                      double t_state, double timestamp, const double *sigmas4, double gravity_mag, int use_rk4,
                                      int imu_avg, int do_fej, double *out_x16, double *out_x16_fej, double *out_Phi, double *out_Qd,
                                      double *out_last_w, double *out_P, double *out_new_clone7, int gpu_propagate, int *out_new_clone_id,
                                      double *out_ms) {
  return run_propagate(C, clone_q, clone_p, imu_x16, imu_x16_fej, calib_dt, N, P, n_imu, imu, t_state, timestamp, sigmas4, gravity_mag,
                       use_rk4, imu_avg, do_fej, out_x16, out_x16_fej, out_Phi, out_Qd, out_last_w, out_P, out_new_clone7, gpu_propagate,
                       out_new_clone_id, out_ms);
}

// UpdaterZeroVelocity::try_update harness: the state of ovph_run_propagate, n_calls (1 or 2) consecutive camera times
// timestamps[k]; the feature database holds n_tracks tracks seen at t_state (uv0), timestamps[0] (uv1) and, with two calls,
// timestamps[1] (uv1 again).  Outputs per call: accepted, chi2; final IMU value, calib_dt, covariance, state timestamp, and
// how many measurements the database still holds at timestamps[0] (cleanup_measurements_exact on the second acceptance).
// gpu_zupt: StateOptions::gpu_zupt (ovph_run_zupt_opt; ovph_run_zupt is the same call with the option off); n_calls may exceed 2
// when the stream covers that many camera periods (tools/zupt_timing.py).
static int run_zupt(int C, const double *clone_q, const double *clone_p, const double *imu_x16, const double *imu_x16_fej,
                    double calib_dt, int N, const double *P, int n_imu, const double *imu, double t_state, int n_calls,
                    const double *timestamps, const double *sigmas4, double gravity_mag, int do_fej, double noise_mult,
                    double chi2_mult, double max_velocity, double max_disparity, int n_tracks, const float *uv0, const float *uv1,
                    /* outputs */ int *out_accepted, double *out_chi2, double *out_x16, double *out_calib_dt, double *out_P,
                    double *out_timestamp, int *out_meas_at_t1, int gpu_zupt, double *out_try_update_ms) {
  ovph_run_opts o;
  ovph_run_opts_defaults(&o);
  StateOptions so;
  so.do_fej = do_fej != 0;
  so.gpu_zupt = gpu_zupt != 0;
  so.do_calib_camera_pose = so.do_calib_camera_intrinsics = so.do_calib_camera_timeoffset = true;
  so.max_clone_size = C + 1;
  so.max_state_size = N + 16;
  so.max_features = 16;
  StateSpec sp;
  sp.C = C, sp.clone_q = clone_q, sp.clone_p = clone_p, sp.N = N, sp.P = P;
  sp.imu_x16 = imu_x16, sp.imu_x16_fej = imu_x16_fej, sp.calib_dt = calib_dt, sp.t_state = t_state;
  HarnessState hs;
  if (int rc = build_harness_state(hs, so, sp, o)) return rc;
  auto &state = hs.state;
  NoiseManager nm = noise_of(sigmas4);
  auto prop = std::make_shared<Propagator>(nm, gravity_mag);
  auto db = std::make_shared<ov_core::FeatureDatabase>();
  for (int f = 0; f < n_tracks; ++f) {
    db->update_feature(100 + f, t_state, 0, uv0[2 * f], uv0[2 * f + 1], 0.f, 0.f);
    for (int k = 0; k < n_calls; ++k) db->update_feature(100 + f, timestamps[k], 0, uv1[2 * f], uv1[2 * f + 1], 0.f, 0.f);
  }
  UpdaterOptions uo;
  uo.chi2_multipler = chi2_mult;
  UpdaterZeroVelocity zupt(uo, nm, db, prop, gravity_mag, max_velocity, noise_mult, max_disparity);
  feed_imu_rows(zupt, n_imu, imu);
  for (int k = 0; k < n_calls; ++k) {
    const auto t_in = std::chrono::steady_clock::now();
    out_accepted[k] = zupt.try_update(state, timestamps[k]) ? 1 : 0;
    if (out_try_update_ms) out_try_update_ms[k] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_in).count();
    out_chi2[k] = zupt.last_chi2();
  }
  memcpy(out_x16, state->_imu->value().data(), 16 * sizeof(double));
  *out_calib_dt = state->_calib_dt_CAMtoIMU->value()(0);
  if (state->max_covariance_size() != N) return -12;
  StateOut out;
  out.P = out_P;
  export_state(hs, out, o);
  *out_timestamp = state->_timestamp;
  *out_meas_at_t1 = (int)db->features_containing(timestamps[0]).size();
  return 0;
}

extern "C" int ovph_run_zupt(int C, const double *clone_q, const double *clone_p, const double *imu_x16, const double *imu_x16_fej,
                             double calib_dt, int N, const double *P, int n_imu, const double *imu, double t_state, int n_calls,
                             const double *timestamps, const double *sigmas4, double gravity_mag, int do_fej, double noise_mult,
                             double chi2_mult, double max_velocity, double max_disparity, int n_tracks, const float *uv0,
                             const float *uv1,
                             /* outputs */ int *out_accepted, double *out_chi2, double *out_x16, double *out_calib_dt, double *out_P,
                             double *out_timestamp, int *out_meas_at_t1) {
  return run_zupt(C, clone_q, clone_p, imu_x16, imu_x16_fej, calib_dt, N, P, n_imu, imu, t_state, n_calls, timestamps, sigmas4,
                  gravity_mag, do_fej, noise_mult, chi2_mult, max_velocity, max_disparity, n_tracks, uv0, uv1, out_accepted, out_chi2,
                  out_x16, out_calib_dt, out_P, out_timestamp, out_meas_at_t1, 0, nullptr);
}

extern "C" int ovph_run_zupt_opt(int C, const double *clone_q, const double *clone_p, const double *imu_x16, const double *imu_x16_fej,
                                 double calib_dt, int N, const double *P, int n_imu, const double *imu, double t_state, int n_calls,
                                 const double *timestamps, const double *sigmas4, double gravity_mag, int do_fej, double noise_mult,
                                 double chi2_mult, double max_velocity, double max_disparity, int n_tracks, const float *uv0,
                                 const float *uv1,
                                 /* outputs */ int *out_accepted, double *out_chi2, double *out_x16, double *out_calib_dt,
                                 double *out_P, double *out_timestamp, int *out_meas_at_t1, int gpu_zupt,
                                 double *out_try_update_ms /* [n_calls] host clock around each try_update, or NULL */) {
  return run_zupt(C, clone_q, clone_p, imu_x16, imu_x16_fej, calib_dt, N, P, n_imu, imu, t_state, n_calls, timestamps, sigmas4,
                  gravity_mag, do_fej, noise_mult, chi2_mult, max_velocity, max_disparity, n_tracks, uv0, uv1, out_accepted, out_chi2,
                  out_x16, out_calib_dt, out_P, out_timestamp, out_meas_at_t1, gpu_zupt, out_try_update_ms);
}

// StateHelper::marginalize_slam + merge_planes_and_marginalize harness.  State: clones, n_slam landmarks (should_marg flags),
// n_planes in-state planes (ids 1..n), every first estimate = value.  merge_pairs [n_pairs x 2] = (old id, new id);
// active_planes = ids observed by features.
// Outputs: final P / n, for every plane id 1..n+8 its Type::id() (or -1) and value, landmark ids (or -1).  Options read: fisheye,
// batched_retire.
extern "C" int ovph_run_state_maintenance(int C, const double *clone_q, const double *clone_p, const double *calib_q,
                                          const double *calib_p, const double *intr, int n_slam, const double *slam_p,
                                          const unsigned char *should_marg, int n_planes, const double *cp, int N, const double *P,
                                          int n_pairs, const int *merge_pairs, int n_active, const int *active_planes,
                                          double sigma_plane_merge, double plane_merge_chi2, double plane_merge_deg_max,
                                          double *out_P, int *out_n, int *out_plane_state_id /* [n_planes+8] */,
                                          double *out_plane_cp /* [(n_planes+8)*3] */, int *out_slam_state_id,
                                          int *out_slam_to_plane, ovph_run_opts *opts) {
  ovph_run_opts dflt, *op = use_opts(opts, &dflt);
  if (!op) return OVPH_E_OPTS;
  StateOptions so;
  so.do_calib_camera_pose = so.do_calib_camera_intrinsics = so.do_calib_camera_timeoffset = true;
  so.max_clone_size = C;
  so.use_plane_constraint = true;
  so.sigma_plane_merge = sigma_plane_merge;
  so.plane_merge_chi2 = plane_merge_chi2;
  so.plane_merge_deg_max = plane_merge_deg_max;
  so.gpu_batched_retire = op->batched_retire != 0;
  so.max_state_size = N + 8;
  so.max_features = 16;
  StateSpec sp;
  sp.C = C, sp.clone_q = clone_q, sp.clone_p = clone_p, sp.calib_q = calib_q, sp.calib_p = calib_p, sp.intr = intr;
  sp.n_slam = n_slam, sp.slam_p = slam_p, sp.n_planes = n_planes, sp.cp = cp, sp.N = N, sp.P = P;
  HarnessState hs;
  if (int rc = build_harness_state(hs, so, sp, *op)) return rc;
  auto &state = hs.state;
  for (int k = 0; k < n_slam; ++k) {
    hs.landmarks[k]->should_marg = should_marg[k] != 0;
    state->_features_SLAM_to_PLANE[hs.landmarks[k]->_featid] = 1;
  }
  StateHelper::marginalize_slam(state);
  std::map<size_t, size_t> feat2plane;
  for (int k = 0; k < n_active; ++k) feat2plane[7000 + k] = (size_t)active_planes[k];
  std::map<size_t, std::set<size_t>> plane2oldplane;
  for (int k = 0; k < n_pairs; ++k) plane2oldplane[(size_t)merge_pairs[2 * k + 1]].insert((size_t)merge_pairs[2 * k]);
  StateHelper::merge_planes_and_marginalize(state, feat2plane, plane2oldplane);
  StateOut out;
  out.P = out_P, out.n = out_n;
  export_state(hs, out, *op);
  for (int k = 0; k < n_planes + 8; ++k) {
    out_plane_state_id[k] = -1;
    auto it = state->_features_PLANE.find((size_t)(k + 1));
    if (it == state->_features_PLANE.end()) continue;
    out_plane_state_id[k] = it->second->id();
    memcpy(out_plane_cp + 3 * k, it->second->value().data(), 3 * sizeof(double));
  }
  for (int k = 0; k < n_slam; ++k) {
    auto it = state->_features_SLAM.find(hs.landmarks[k]->_featid);
    out_slam_state_id[k] = (it == state->_features_SLAM.end()) ? -1 : it->second->id();
    out_slam_to_plane[k] = state->_features_SLAM_to_PLANE.count(hs.landmarks[k]->_featid) ? 1 : 0;
  }
  return 0;
}

// UpdaterPlane::nullspace_project_inplace / measurement_compress_inplace and the UpdaterHelper twins on dense inputs
// (column-major).  Returns the number of rows left; outputs overwrite the leading rows of the inputs (ld unchanged).
extern "C" int ovph_run_plane_givens(int op /* 0 nullspace, 1 compress */, int rows, int hf_cols, double *H_f, int cols,
                                     double *H_x, int cp_cols, double *H_cp, double *res) {
  MatrixXd Hf(rows, std::max(hf_cols, 1)), Hx(rows, cols), Hcp(rows, std::max(cp_cols, 1));
  VectorXd r(rows, 1);
  if (hf_cols) memcpy(Hf.data(), H_f, sizeof(double) * (size_t)rows * hf_cols);
  memcpy(Hx.data(), H_x, sizeof(double) * (size_t)rows * cols);
  if (cp_cols) memcpy(Hcp.data(), H_cp, sizeof(double) * (size_t)rows * cp_cols);
  memcpy(r.data(), res, sizeof(double) * rows);
  if (op == 0) {
    if (cp_cols) UpdaterPlane::nullspace_project_inplace(Hf, Hx, Hcp, r);
    else UpdaterHelper::nullspace_project_inplace(Hf, Hx, r);
  } else {
    if (cp_cols) UpdaterPlane::measurement_compress_inplace(Hx, Hcp, r);
    else UpdaterHelper::measurement_compress_inplace(Hx, r);
  }
  const int ro = Hx.rows();
  for (int j = 0; j < cols; ++j)
    for (int i = 0; i < ro; ++i) H_x[(size_t)j * rows + i] = Hx(i, j);
  for (int j = 0; j < cp_cols; ++j)
    for (int i = 0; i < ro; ++i) H_cp[(size_t)j * rows + i] = Hcp(i, j);
  for (int i = 0; i < ro; ++i) res[i] = r(i);
  return ro;
}

// Closed loop over several camera frames with the reference's own call order (core/VioManager.cpp:348 propagate_and_clone,
// :670 UpdaterMSCKF::update, :864-866 marginalize_old_clone): state with C clones, IMU state, covariance P (N = 30 + 6 C).
// Frame k: propagate + clone to frame_time[k], update with that frame's features (slots index the C+1 clones of the window,
// oldest first; positions given), marginalize the oldest clone.  Outputs the final filter state and covariance.
// Options read: seq_traj, seq_posecov, seq_uv_norm, seq_plane, seq_plane_mode, seq_plane_min_feat, seq_sigma_c, fisheye; written:
// seq_planes_in_state.
extern "C" int ovph_run_sequence(int C, const double *clone_q, const double *clone_p, const double *clone_q_fej,
                                 const double *clone_p_fej, const double *calib_q, const double *calib_p, const double *intr,
                                 const double *imu_x16, const double *imu_x16_fej, double calib_dt, int N, const double *P,
                                 int n_imu, const double *imu, double t_state, const double *sigmas4, double gravity_mag,
                                 int use_rk4, int do_fej, int K, const double *frame_time, const int *feat_offset /* [K+1] */,
                                 int M, const float *uv, const int *clone_slot, const int *n_meas, const double *p_FinG,
                                 double sigma_px, double chi2_mult,
                                 /* outputs */ double *out_clone_q, double *out_clone_p, double *out_x16, double *out_calib_q,
                                 double *out_calib_p, double *out_intr, double *out_dt, double *out_P, int *n_kept_per_frame,
                                 ovph_run_opts *opts) {
  ovph_run_opts dflt, *op = use_opts(opts, &dflt);
  if (!op) return OVPH_E_OPTS;
  ovph_run_opts &o = *op;
  StateOptions so;
  so.do_fej = do_fej != 0;
  so.do_calib_camera_pose = so.do_calib_camera_intrinsics = so.do_calib_camera_timeoffset = true;
  so.max_clone_size = C;
  so.use_rk4_integration = use_rk4 != 0;
  so.max_state_size = N + 16 + 3 * 16;
  so.max_features = 4096;
  const int plane_mode = o.seq_plane ? o.seq_plane_mode : 0;
  if (plane_mode) {
    so.use_plane_constraint = so.use_plane_constraint_msckf = true;
    so.use_plane_constraint_slamu = so.use_plane_constraint_slamd = true;
    so.use_plane_slam_feats = plane_mode == 2;
    so.sigma_constraint = o.seq_sigma_c;
    so.plane_init_min_feat = so.plane_msckf_min_feat = o.seq_plane_min_feat;
  }
  StateSpec sp;
  sp.C = C, sp.clone_q = clone_q, sp.clone_p = clone_p, sp.clone_q_fej = clone_q_fej, sp.clone_p_fej = clone_p_fej;
  sp.calib_q = calib_q, sp.calib_p = calib_p, sp.intr = intr, sp.N = N, sp.P = P;
  sp.imu_x16 = imu_x16, sp.imu_x16_fej = imu_x16_fej, sp.calib_dt = calib_dt, sp.t_state = t_state;
  HarnessState hs;
  if (int rc = build_harness_state(hs, so, sp, o)) return rc;
  auto &state = hs.state;
  Propagator prop(noise_of(sigmas4), gravity_mag);
  feed_imu_rows(prop, n_imu, imu);
  UpdaterOptions uo;
  uo.sigma_pix = sigma_px;
  uo.chi2_multipler = chi2_mult;
  ov_core::FeatureInitializerOptions fio;
  UpdaterMSCKF updater(uo, fio);
  UpdaterPlane updater_plane(uo, fio);
  std::map<size_t, size_t> feat2plane;
  for (int k = 0; k < K; ++k) {
    feat2plane.clear();
    prop.propagate_and_clone(state, frame_time[k]);  // VioManager.cpp:348
    std::vector<double> times;
    for (auto &c : state->_clones_IMU) times.push_back(c.first);
    std::vector<std::shared_ptr<ov_core::Feature>> fv, fextra, fused;
    for (int f = feat_offset[k]; f < feat_offset[k + 1]; ++f) {
      auto ft = std::make_shared<ov_core::Feature>();
      ft->featid = 1000 + f;
      for (int q = 0; q < n_meas[f]; ++q) {
        ft->timestamps.push_back(times.at(clone_slot[(size_t)f * M + q]));
        ft->uvs.push_back(uv[((size_t)f * M + q) * 2]);
        ft->uvs.push_back(uv[((size_t)f * M + q) * 2 + 1]);
      }
      if (o.seq_uv_norm) {
        for (int q = 0; q < 2 * n_meas[f]; ++q) ft->uvs_norm.push_back(o.seq_uv_norm[(size_t)f * M * 2 + q]);
      } else {
        memcpy(ft->p_FinG, p_FinG + 3 * f, 3 * sizeof(double));
      }
      fv.push_back(ft);
      if (plane_mode && o.seq_plane[f] > 0) feat2plane[ft->featid] = (size_t)o.seq_plane[f];
    }
    if (plane_mode == 2) {  // VioManager.cpp:543-600: planar candidates first try to initialise their planes
      std::vector<std::shared_ptr<ov_core::Feature>> fplane, finit_used;
      for (auto &ft : fv)
        if (feat2plane.count(ft->featid)) fplane.push_back(ft);
      updater_plane.init_vio_plane(state, fplane, finit_used, feat2plane);
      std::set<size_t> used;
      for (auto &ft : finit_used) used.insert(ft->featid);
      std::vector<std::shared_ptr<ov_core::Feature>> rest;
      for (auto &ft : fv)
        if (!used.count(ft->featid)) rest.push_back(ft);
      fv.swap(rest);
    }
    updater.update(state, fv, fextra, fused, feat2plane);  // VioManager.cpp:670
    n_kept_per_frame[k] = (int)fv.size();
    StateHelper::marginalize_old_clone(state);  // VioManager.cpp:864-866
    if (o.seq_traj) memcpy(o.seq_traj + 16 * (size_t)k, state->_imu->value().data(), 16 * sizeof(double));
    if (o.seq_posecov) {
      std::vector<std::shared_ptr<Type>> po;
      po.push_back(state->_imu->pose());
      MatrixXd Pp = StateHelper::get_marginal_covariance(state, po);
      memcpy(o.seq_posecov + 36 * (size_t)k, Pp.data(), 36 * sizeof(double));
    }
  }
  o.seq_planes_in_state = (int)state->_features_PLANE.size();
  if ((int)state->_clones_IMU.size() != C) return -13;
  memcpy(out_x16, state->_imu->value().data(), 16 * sizeof(double));
  *out_dt = state->_calib_dt_CAMtoIMU->value()(0);
  StateOut out;
  out.clone_q = out_clone_q, out.clone_p = out_clone_p, out.calib_q = out_calib_q, out.calib_p = out_calib_p, out.intr = out_intr;
  // plane_mode 2: planes joined the state, the covariance is larger than the caller's buffer and is not returned
  const bool fits = state->max_covariance_size() == N;
  if (plane_mode != 2 && fits) out.P = out_P;
  export_state(hs, out, o);
  return (plane_mode == 2 || fits) ? 0 : -12;
}


// ---- on-disk formats (ov_plane_io.h) ---------------------------------------------------------------------------------
#include "ov_plane_io.h"

#include <fstream>
#include <sstream>

// no device needed: timing CSV (header + one row) into buf; returns the length
extern "C" int ovph_format_timing(int use_plane, int max_slam, const double *vals9, char *buf, int cap) {
  ov_plane::StateOptions so;
  so.use_plane_constraint = use_plane != 0;
  so.max_slam_features = max_slam;
  ov_plane::TimingRecord r;
  r.timestamp_inI = vals9[0];
  r.track = vals9[1];
  r.prop = vals9[2];
  r.planeinit = vals9[3];
  r.msckf = vals9[4];
  r.slam_update = vals9[5];
  r.slam_delay = vals9[6];
  r.marg = vals9[7];
  r.total = vals9[8];
  std::ostringstream os;
  ov_plane::write_timing_header(os, so);
  ov_plane::write_timing_row(os, so, r);
  const std::string s = os.str();
  if ((int)s.size() + 1 > cap) return -1;
  memcpy(buf, s.c_str(), s.size() + 1);
  return (int)s.size();
}

// no device needed: returns the number of poses (<= cap) copied to out [cap][8], or -1
extern "C" int ovph_load_trajectory(const char *path, double *out, int cap) {
  std::vector<std::array<double, 8>> poses;
  if (!ov_plane::load_trajectory(path, poses)) return -1;
  const int n = std::min((int)poses.size(), cap);
  for (int i = 0; i < n; ++i) memcpy(out + 8 * i, poses[i].data(), 8 * sizeof(double));
  return (int)poses.size();
}

// per-frame trace of every following UpdaterMSCKF::update (point update) into `path`; NULL / "" stops tracing
extern "C" int ovph_update_trace(const char *path) { return ov_plane::open_update_trace(path ? path : "") ? 0 : -1; }

// no device needed: reads every frame of `in` with the C++ reader and writes it back to `out` with the C++ writer
extern "C" int ovph_trace_copy(const char *in, const char *out) {
  std::ifstream is(in, std::ios::binary);
  std::ofstream os(out, std::ios::binary);
  if (!is.is_open() || !os.is_open()) return -1;
  int n = 0;
  ov_plane::FrameTrace f;
  while (is.peek() != EOF) {
    if (!ov_plane::read_frame_trace(is, f, n == 0)) return -2;
    if (!ov_plane::write_frame_trace(os, f, n == 0)) return -3;
    ++n;
  }
  return n;
}

// needs the device: a state as ovph_run_msckf_update builds it (no planes) but with values only - no first estimate is set -, one
// line of each of the three files
extern "C" int ovph_format_state_files(int C, const double *clone_q, const double *clone_p, const double *calib_q, const double *calib_p,
                                       const double *intr, int N, const double *P, double timestamp, double dt, int with_gt,
                                       char *est, char *sd, char *gt, int cap) {
  using namespace ov_plane;
  ovph_run_opts o;
  ovph_run_opts_defaults(&o);
  StateOptions so;
  so.do_calib_camera_pose = so.do_calib_camera_intrinsics = so.do_calib_camera_timeoffset = true;
  so.max_clone_size = C;
  so.max_state_size = N + 8;
  so.max_features = 16;
  StateSpec sp;
  sp.C = C, sp.clone_q = clone_q, sp.clone_p = clone_p, sp.calib_q = calib_q, sp.calib_p = calib_p, sp.intr = intr;
  sp.set_fej = false, sp.N = N, sp.P = P;
  HarnessState hs;
  if (int rc = build_harness_state(hs, so, sp, o)) return rc;
  auto &state = hs.state;
  state->_calib_dt_CAMtoIMU->set_value(vec_of(&dt, 1));
  state->_timestamp = timestamp;
  SimTruth sim;
  for (int k = 0; k < 17; ++k) sim.state_gt[k] = 0.5 + 0.125 * k;
  sim.calib_camimu_dt = 0.0123456;
  for (int k = 0; k < 8; ++k) sim.intrinsics[k] = intr[k] + 1.0;
  for (int k = 0; k < 7; ++k) sim.extrinsics[k] = 0.1 * (k + 1);
  std::ostringstream oe, os, og;
  ROSVisualizerHelper::sim_save_total_state_to_file(state, with_gt ? &sim : nullptr, oe, os, og);
  const std::string a = oe.str(), b = os.str(), c = og.str();
  if ((int)a.size() + 1 > cap || (int)b.size() + 1 > cap || (int)c.size() + 1 > cap) return -1;
  memcpy(est, a.c_str(), a.size() + 1);
  memcpy(sd, b.c_str(), b.size() + 1);
  memcpy(gt, c.c_str(), c.size() + 1);
  return 0;
}

// UpdaterHelper::get_feature_jacobian_full for ONE feature held in landmark representation `rep` anchored in clone slot
// anchor_ci (ext LandmarkRepresentation 0..5).  Outputs column-major: H_f [rows x hf_cols], H_x [rows x cols], res [rows],
// order ids / sizes of the H_x columns.  Needs the device only because a State owns a context.  Options read: fisheye.
extern "C" int ovph_feature_jacobian_rep(int C, const double *clone_q, const double *clone_p, const double *clone_q_fej,
                                         const double *clone_p_fej, const double *calib_q, const double *calib_p, const double *intr,
                                         int N, const double *P, int m, const float *uv, const int *clone_idx, const double *p_FinG,
                                         int rep, int anchor_ci, double sigma_px, int do_fej, double *H_f, double *H_x, double *res,
                                         int *rows_out, int *cols_out, int *hf_cols_out, int *order_id, int *order_size, int *n_order,
                                         ovph_run_opts *opts) {
  ovph_run_opts dflt, *op = use_opts(opts, &dflt);
  if (!op) return OVPH_E_OPTS;
  StateOptions so;
  so.do_fej = do_fej != 0;
  so.do_calib_camera_pose = so.do_calib_camera_intrinsics = so.do_calib_camera_timeoffset = true;
  so.max_clone_size = C;
  so.max_state_size = N + 8;
  so.max_features = 16;
  StateSpec sp;
  sp.C = C, sp.clone_q = clone_q, sp.clone_p = clone_p, sp.clone_q_fej = clone_q_fej, sp.clone_p_fej = clone_p_fej;
  sp.calib_q = calib_q, sp.calib_p = calib_p, sp.intr = intr, sp.N = N, sp.P = P;
  HarnessState hs;
  if (int rc = build_harness_state(hs, so, sp, *op)) return rc;
  auto &state = hs.state;
  UpdaterHelper::UpdaterHelperFeature feat;
  feat.featid = 5000;
  for (int k = 0; k < m; ++k) {
    feat.timestamps.push_back(hs.times[clone_idx[k]]);
    feat.uvs.push_back(uv[2 * k]);
    feat.uvs.push_back(uv[2 * k + 1]);
  }
  memcpy(feat.p_FinG, p_FinG, 3 * sizeof(double));
  memcpy(feat.p_FinG_fej, p_FinG, 3 * sizeof(double));
  feat.feat_representation = (LandmarkRepresentation::Representation)rep;
  if (LandmarkRepresentation::is_relative_representation(feat.feat_representation)) {
    feat.anchor_cam_id = 0;
    feat.anchor_clone_timestamp = hs.times[anchor_ci];
    auto anchor = state->_clones_IMU.at(feat.anchor_clone_timestamp);
    auto calib = state->_calib_IMUtoCAM.at(0);
    const double *Ra = anchor->Rot(), *pa = anchor->pos(), *Rc = calib->Rot(), *pc = calib->pos();
    const double d[3] = {p_FinG[0] - pa[0], p_FinG[1] - pa[1], p_FinG[2] - pa[2]};
    double t[3];
    for (int i = 0; i < 3; ++i) t[i] = Ra[3 * i] * d[0] + Ra[3 * i + 1] * d[1] + Ra[3 * i + 2] * d[2];
    for (int i = 0; i < 3; ++i) feat.p_FinA[i] = Rc[3 * i] * t[0] + Rc[3 * i + 1] * t[1] + Rc[3 * i + 2] * t[2] + pc[i];
    memcpy(feat.p_FinA_fej, feat.p_FinA, 3 * sizeof(double));
  }
  MatrixXd Hf, Hx;
  VectorXd r;
  std::vector<std::shared_ptr<Type>> order;
  UpdaterHelper::get_feature_jacobian_full(state, feat, sigma_px, 1.0, Hf, Hx, r, order);
  *rows_out = Hf.rows();
  *cols_out = Hx.cols();
  *hf_cols_out = Hf.cols();
  memcpy(H_f, Hf.data(), sizeof(double) * (size_t)Hf.rows() * Hf.cols());
  memcpy(H_x, Hx.data(), sizeof(double) * (size_t)Hx.rows() * Hx.cols());
  memcpy(res, r.data(), sizeof(double) * (size_t)r.rows());
  *n_order = (int)order.size();
  for (size_t k = 0; k < order.size(); ++k) {
    order_id[k] = order[k]->id();
    order_size[k] = order[k]->size();
  }
  return 0;
}

// UpdaterSLAM::change_anchors on a state whose first landmark is held in the anchored representation `rep` (2..4) and anchored
// in the oldest clone, with one clone more than max_clone_size in the window: the landmark moves to the newest clone.
// lm_p_FinA / lm_p_FinA_fej: its position in the old anchor camera frame.  Outputs: landmark value / fej (representation
// parameters), its new anchor clone slot, the covariance.  Options read: fisheye.
extern "C" int ovph_run_change_anchors(int C, const double *clone_q, const double *clone_p, const double *clone_q_fej,
                                       const double *clone_p_fej, const double *calib_q, const double *calib_p, const double *intr,
                                       int n_slam, const double *slam_p, int N, const double *P, int rep, const double *lm_p_FinA,
                                       const double *lm_p_FinA_fej, int do_fej, double *out_value, double *out_fej, int *out_anchor_ci,
                                       double *out_P, ovph_run_opts *opts) {
  ovph_run_opts dflt, *op = use_opts(opts, &dflt);
  if (!op) return OVPH_E_OPTS;
  StateOptions so;
  so.do_fej = do_fej != 0;
  so.do_calib_camera_pose = so.do_calib_camera_intrinsics = so.do_calib_camera_timeoffset = true;
  so.max_clone_size = C - 1;
  so.max_state_size = N + 8;
  so.max_features = 16;
  StateSpec sp;
  sp.C = C, sp.clone_q = clone_q, sp.clone_p = clone_p, sp.clone_q_fej = clone_q_fej, sp.clone_p_fej = clone_p_fej;
  sp.calib_q = calib_q, sp.calib_p = calib_p, sp.intr = intr, sp.n_slam = n_slam, sp.slam_p = slam_p, sp.N = N, sp.P = P;
  HarnessState hs;
  if (int rc = build_harness_state(hs, so, sp, *op)) return rc;
  auto &state = hs.state;
  auto lm = hs.landmarks.at(0);
  lm->_feat_representation = (LandmarkRepresentation::Representation)rep;
  lm->_anchor_cam_id = 0;
  lm->_anchor_clone_timestamp = hs.times[0];
  lm->set_from_xyz(lm_p_FinA, false);
  lm->set_from_xyz(lm_p_FinA_fej, true);
  UpdaterOptions uo, ua;
  ov_core::FeatureInitializerOptions fio;
  UpdaterSLAM up(uo, ua, fio);
  up.change_anchors(state);
  for (int k = 0; k < 3; ++k) {
    out_value[k] = lm->value()(k);
    out_fej[k] = lm->fej()(k);
  }
  *out_anchor_ci = -1;
  for (int i = 0; i < C; ++i)
    if (hs.times[i] == lm->_anchor_clone_timestamp) *out_anchor_ci = i;
  StateOut out;
  out.P = out_P;
  export_state(hs, out, *op);
  return lm->has_had_anchor_change ? 0 : -20;
}

// TrackPlane's image half on a sequence of frames (host_capi.h)
extern "C" int ovph_run_klt_sequence(int device, int width, int height, int n_frames, const uint8_t *frames, const uint8_t *mask,
                                     int pyr_levels, int win_size, int hist_method, int n_pts, const int64_t *ids, const float *uv,
                                     int32_t *n_kept, int64_t *kept_ids, float *kept_uv, int32_t *n_match, float *match_uv,
                                     uint8_t *match_mask) {
  ovp_ctx *gpu = nullptr;
  int rc = ovp_ctx_create(device, 64, 4, 8, nullptr, &gpu);
  if (rc) return rc;
  {
    ovp_trackplane_opts to;
    ovp_trackplane_defaults(&to);
    TrackPlane tp(gpu, to);
    rc = tp.ok() ? tp.set_klt_options(pyr_levels, win_size, hist_method, std::max(n_pts, 1)) : OVP_E_STATE;
    const size_t px = (size_t)width * height;
    for (int f = 0; f < n_frames && rc == 0; ++f) {
      rc = tp.feed_new_camera(0.1 * f, frames + px * f, width, height, width, mask);
      if (rc) break;
      if (f == 0) {
        std::vector<size_t> id(ids, ids + n_pts);
        std::vector<float> p(uv, uv + 2 * (size_t)n_pts);
        tp.add_points(id, p);
      }
      const auto &ki = tp.get_last_ids();
      const auto &kp = tp.get_last_pts();
      const auto &mp = tp.get_last_match_pts();
      const auto &mm = tp.get_last_match_mask();
      n_kept[f] = (int32_t)ki.size(), n_match[f] = (int32_t)mm.size();
      for (size_t i = 0; i < ki.size(); ++i) kept_ids[(size_t)f * n_pts + i] = (int64_t)ki[i];
      if (!kp.empty()) memcpy(kept_uv + 2 * (size_t)f * n_pts, kp.data(), sizeof(float) * kp.size());
      if (!mp.empty()) memcpy(match_uv + 2 * (size_t)f * n_pts, mp.data(), sizeof(float) * mp.size());
      if (!mm.empty()) memcpy(match_mask + (size_t)f * n_pts, mm.data(), mm.size());
    }
  }
  ovp_ctx_destroy(gpu);
  return rc;
}

// TrackPlane's image half with the epipolar check on, on a sequence of frames (host_capi.h)
extern "C" int ovph_run_klt_epipolar_sequence(int device, int width, int height, int n_frames, const uint8_t *frames, const uint8_t *mask,
                                              int pyr_levels, int win_size, int hist_method, int n_pts, const int64_t *ids, const float *uv,
                                              int mode, const double *intrinsics8, int max_iters, uint32_t seed, int32_t *n_kept,
                                              int64_t *kept_ids, float *kept_uv, float *kept_uvn, int32_t *reset) {
  ovp_ctx *gpu = nullptr;
  int rc = ovp_ctx_create(device, 64, 4, 8, nullptr, &gpu);
  if (rc) return rc;
  {
    ovp_trackplane_opts to;
    ovp_trackplane_defaults(&to);
    TrackPlane tp(gpu, to);
    rc = tp.ok() ? tp.set_klt_options(pyr_levels, win_size, hist_method, std::max(n_pts, 1)) : OVP_E_STATE;
    if (rc == 0) rc = tp.set_camera(mode, intrinsics8);
    tp.set_epipolar_options(0.999, max_iters, seed);
    const size_t px = (size_t)width * height;
    for (int f = 0; f < n_frames && rc == 0; ++f) {
      rc = tp.feed_new_camera(0.1 * f, frames + px * f, width, height, width, mask, false, true);
      if (rc) break;
      if (f == 0) {
        std::vector<size_t> id(ids, ids + n_pts);
        std::vector<float> p(uv, uv + 2 * (size_t)n_pts);
        tp.add_points(id, p);
      }
      const auto &ki = tp.get_last_ids();
      const auto &kp = tp.get_last_pts();
      const auto &kn = tp.get_last_uv_norm();
      n_kept[f] = (int32_t)ki.size(), reset[f] = tp.last_reset() ? 1 : 0;
      for (size_t i = 0; i < ki.size(); ++i) kept_ids[(size_t)f * n_pts + i] = (int64_t)ki[i];
      if (!kp.empty()) memcpy(kept_uv + 2 * (size_t)f * n_pts, kp.data(), sizeof(float) * kp.size());
      if (!kn.empty()) memcpy(kept_uvn + 2 * (size_t)f * n_pts, kn.data(), sizeof(float) * kn.size());
    }
  }
  ovp_ctx_destroy(gpu);
  return rc;
}

// TrackPlane::feed_monocular over the fused entry, with a feature database attached, on a sequence of frames (host_capi.h)
extern "C" int ovph_run_klt_frame_sequence(int device, int width, int height, int n_frames, const uint8_t *frames, const uint8_t *mask,
                                           const double *times, int pyr_levels, int win_size, int hist_method, int n_pts,
                                           const int64_t *ids, const float *uv, int mode, const double *intrinsics8, int check,
                                           int max_iters, uint32_t seed, int max_slots, int max_meas, int32_t *n_kept, int64_t *kept_ids,
                                           float *kept_uv, float *kept_uvn, int32_t *reset, int32_t *db_slot, int32_t *db_count,
                                           double *db_ts, float *db_uv, float *db_uvn) {
  ovp_ctx *gpu = nullptr;
  int rc = ovp_ctx_create(device, 64, 4, 8, nullptr, &gpu);
  if (rc) return rc;
  {
    ovp_trackplane_opts to;
    ovp_trackplane_defaults(&to);
    TrackPlane tp(gpu, to);
    ov_plane::FeatureDatabase db(gpu, max_slots, max_meas);
    rc = tp.ok() ? db.status() : OVP_E_STATE;
    if (rc == 0) rc = tp.set_klt_options(pyr_levels, win_size, hist_method, std::max(n_pts, 1));
    if (rc == 0) rc = tp.set_camera(mode, intrinsics8);
    tp.set_epipolar_options(0.999, max_iters, seed);
    if (rc == 0) rc = tp.set_database(&db);
    const size_t px = (size_t)width * height;
    for (int f = 0; f < n_frames && rc == 0; ++f) {
      rc = tp.feed_monocular(times[f], frames + px * f, width, height, width, mask, false, check != 0);
      if (rc) break;
      if (f == 0) {  // the caller's detection: its points, and their first observation (:477-491)
        std::vector<size_t> id(ids, ids + n_pts);
        std::vector<float> p(uv, uv + 2 * (size_t)n_pts);
        tp.add_points(id, p);
        rc = db.update_feature(times[0], std::vector<int64_t>(ids, ids + n_pts), p, p);
        if (rc) break;
      }
      const auto &ki = tp.get_last_ids();
      const auto &kp = tp.get_last_pts();
      const auto &kn = tp.get_last_uv_norm();
      n_kept[f] = (int32_t)ki.size(), reset[f] = tp.last_reset() ? 1 : 0;
      for (size_t i = 0; i < ki.size(); ++i) kept_ids[(size_t)f * n_pts + i] = (int64_t)ki[i];
      if (!kp.empty()) memcpy(kept_uv + 2 * (size_t)f * n_pts, kp.data(), sizeof(float) * kp.size());
      if (!kn.empty()) memcpy(kept_uvn + 2 * (size_t)f * n_pts, kn.data(), sizeof(float) * kn.size());
    }
    for (int i = 0; i < n_pts && rc == 0; ++i) {  // the database's read-back
      int del = 0;
      rc = ovp_featdb_get(gpu, ids[i], db_slot + i, db_count + i, &del, db_ts + (size_t)i * max_meas, db_uv + 2 * (size_t)i * max_meas,
                          db_uvn + 2 * (size_t)i * max_meas, max_meas);
    }
  }
  ovp_ctx_destroy(gpu);
  return rc;
}

// TrackPlane's image half with its own detection on a sequence of frames (host_capi.h)
extern "C" int ovph_run_klt_detect_sequence(int device, int width, int height, int n_frames, const uint8_t *frames, const uint8_t *mask,
                                            int pyr_levels, int win_size, int hist_method, int max_points, const int32_t *detector5,
                                            int32_t *n_kept, int64_t *kept_ids, float *kept_uv) {
  ovp_ctx *gpu = nullptr;
  int rc = ovp_ctx_create(device, 64, 4, 8, nullptr, &gpu);
  if (rc) return rc;
  {
    ovp_trackplane_opts to;
    ovp_trackplane_defaults(&to);
    TrackPlane tp(gpu, to);
    rc = tp.ok() ? tp.set_klt_options(pyr_levels, win_size, hist_method, max_points) : OVP_E_STATE;
    tp.set_detector_options(detector5[0], detector5[1], detector5[2], detector5[3], detector5[4]);
    const size_t px = (size_t)width * height;
    for (int f = 0; f < n_frames && rc == 0; ++f) {
      rc = tp.feed_new_camera(0.1 * f, frames + px * f, width, height, width, mask, true);
      if (rc) break;
      const auto &ki = tp.get_last_ids();
      const auto &kp = tp.get_last_pts();
      if ((int)ki.size() > max_points) {
        rc = OVP_E_CAPACITY;
        break;
      }
      n_kept[f] = (int32_t)ki.size();
      for (size_t i = 0; i < ki.size(); ++i) kept_ids[(size_t)f * max_points + i] = (int64_t)ki[i];
      if (!kp.empty()) memcpy(kept_uv + 2 * (size_t)f * max_points, kp.data(), sizeof(float) * kp.size());
    }
  }
  ovp_ctx_destroy(gpu);
  return rc;
}

// TrackPlane's image half under the intake options, with its own detection, on a sequence of frames (host_capi.h)
extern "C" int ovph_run_klt_intake_sequence(int device, int width, int height, int n_frames, const uint8_t *frames, const uint8_t *mask,
                                            int pyr_levels, int win_size, int hist_method, int downsample, double clahe_clip, int tiles_x,
                                            int tiles_y, int max_points, const int32_t *detector5, int32_t *n_kept, int64_t *kept_ids,
                                            float *kept_uv) {
  ovp_ctx *gpu = nullptr;
  int rc = ovp_ctx_create(device, 64, 4, 8, nullptr, &gpu);
  if (rc) return rc;
  {
    ovp_trackplane_opts to;
    ovp_trackplane_defaults(&to);
    TrackPlane tp(gpu, to);
    rc = tp.ok() ? tp.set_klt_options(pyr_levels, win_size, hist_method, max_points) : OVP_E_STATE;
    if (rc == 0) rc = tp.set_intake((TrackPlane::HistogramMethod)hist_method, downsample != 0, clahe_clip, tiles_x, tiles_y);
    tp.set_detector_options(detector5[0], detector5[1], detector5[2], detector5[3], detector5[4]);
    const size_t px = (size_t)width * height;
    for (int f = 0; f < n_frames && rc == 0; ++f) {
      rc = tp.feed_new_camera(0.1 * f, frames + px * f, width, height, width, mask, true);
      if (rc) break;
      const auto &ki = tp.get_last_ids();
      const auto &kp = tp.get_last_pts();
      if ((int)ki.size() > max_points) {
        rc = OVP_E_CAPACITY;
        break;
      }
      n_kept[f] = (int32_t)ki.size();
      for (size_t i = 0; i < ki.size(); ++i) kept_ids[(size_t)f * max_points + i] = (int64_t)ki[i];
      if (!kp.empty()) memcpy(kept_uv + 2 * (size_t)f * max_points, kp.data(), sizeof(float) * kp.size());
    }
  }
  ovp_ctx_destroy(gpu);
  return rc;
}

// ov_plane::FeatureDatabase (ov_plane_featdb.h) on a sequence of frames, on a context of its own (host_capi.h)
extern "C" int ovph_run_featdb_sequence(int device, int max_slots, int max_meas, int n_frames, const double *times, const int32_t *n_obs,
                                        const int64_t *ids, const float *uv, const float *uv_norm, int max_clone_size,
                                        int max_slam_features, int64_t *out, long cap, long *used) {
  ovp_ctx *gpu = nullptr;
  int rc = ovp_ctx_create(device, 32, 32, 64, nullptr, &gpu);
  if (rc) return rc;
  long at = 0;
  auto put = [&](int64_t v) {
    if (at < cap) out[at] = v;
    ++at;
  };
  auto put_list = [&](const std::vector<int64_t> &v) {
    put((int64_t)v.size());
    for (int64_t x : v) put(x);
  };
  {
    FeatureDatabase db(gpu, max_slots, max_meas);
    rc = db.status();
    std::vector<int64_t> landmarks;
    size_t o = 0;
    for (int f = 0; f < n_frames && !rc; ++f) {
      const size_t n = (size_t)n_obs[f];
      rc = db.update_feature(times[f], std::vector<int64_t>(ids + o, ids + o + n), std::vector<float>(uv + 2 * o, uv + 2 * (o + n)),
                             std::vector<float>(uv_norm + 2 * o, uv_norm + 2 * (o + n)));
      o += n;
      if (rc) break;
      const std::vector<double> window(times + std::max(0, f - max_clone_size), times + f + 1);
      FeatDbSelection s;
      FeatureDatabase::Table t;
      if ((rc = db.select(window, times[f], max_clone_size, landmarks, max_slam_features, true, s, &t))) break;
      put_list(t.ids);
      for (const std::vector<int> *v : {&t.cls, &t.count, &t.cleaned}) put_list(std::vector<int64_t>(v->begin(), v->end()));
      put_list(std::vector<int64_t>(t.flags.begin(), t.flags.end()));
      for (int k = 0; k < 4; ++k) put(t.totals[k]);
      for (const std::vector<int64_t> *v : {&s.lost, &s.marg, &s.maxtracks, &s.slam_delayed, &s.slam_update, &s.landmarks_marg}) put_list(*v);
      // the two queries under the reference's names, and one feature read back
      std::vector<int64_t> q;
      if ((rc = db.features_not_containing_newer(times[f], q))) break;
      put_list(q);
      if ((rc = db.features_containing(window.front(), q))) break;
      put_list(q);
      FeatureDatabase::Feature ft;
      const bool have = !t.ids.empty() && db.get_feature(t.ids.front(), ft);
      put(have ? (int64_t)ft.timestamps.size() : -1);
      put(have && ft.to_delete ? 1 : 0);
      // what the updaters do with the selection, then :855-869
      std::vector<int64_t> next;
      for (int64_t lm : landmarks)
        if (!std::count(s.landmarks_marg.begin(), s.landmarks_marg.end(), lm)) next.push_back(lm);
      next.insert(next.end(), s.slam_delayed.begin(), s.slam_delayed.end());
      landmarks = next;
      std::vector<int64_t> chosen = s.lost;
      for (const std::vector<int64_t> *v : {&s.marg, &s.maxtracks, &s.slam_delayed, &s.slam_update}) chosen.insert(chosen.end(), v->begin(), v->end());
      if ((rc = db.mark_deleted(chosen))) break;
      if ((rc = db.cleanup())) break;
      if ((int)window.size() > max_clone_size && (rc = db.cleanup_measurements(window.front()))) break;
    }
  }
  ovp_ctx_destroy(gpu);
  if (used) *used = at;
  return rc ? rc : (at > cap ? OVP_E_CAPACITY : 0);
}
