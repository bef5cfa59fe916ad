// C-ABI shim, part 6 (see ovp_ctx.h): general point features - observations of any camera, tracks longer than OVP_MAX_MEAS.
// The device form of ovp_msckf_dense_blocks (update/UpdaterMSCKF.cpp:695-764 for the features the batch format cannot carry) and
// the triangulation of such features over every camera (update/UpdaterMSCKF.cpp:120-166).  Kernels: csrc/k_feat_gen.hip,
// csrc/k_triang.hip (k_triangulate_gen).
#include "ovp_ctx.h"

extern "C" int ovp_cameras_upload(ovp_ctx* c, int n_cams, const ovp_camera_tables* cams) {
  if (!c || !cams || n_cams < 1 || n_cams > OVP_MAX_CAMERAS) return OVP_E_ARG;
  if (!c->gen_cal) HIPCHK(dalloc(&c->gen_cal, (size_t)20 * OVP_MAX_CAMERAS));
  HIPCHK(hipStreamSynchronize(c->stream));  // (the previous tables may still be on their way: gen_cal_h is the source of the copy)
  for (int k = 0; k < n_cams; ++k) {
    double* cal = c->gen_cal_h + 20 * k;
    quat_2_rot(cams[k].calib_q, cal);
    memcpy(cal + 9, cams[k].calib_p, sizeof(double) * 3);
    memcpy(cal + 12, cams[k].intrinsics, sizeof(double) * 8);
    c->gen_calib_id[k] = cams[k].calib_id;
    c->gen_intr_id[k] = cams[k].intr_id;
    c->gen_fisheye[k] = cams[k].fisheye ? 1 : 0;
  }
  HIPCHK(hipMemcpyAsync(c->gen_cal, c->gen_cal_h, sizeof(double) * 20 * n_cams, hipMemcpyHostToDevice, c->stream));
  c->gen_ncams = n_cams;
  return 0;
}

// argument checks of a general batch against the context's tables (host only, nothing enqueued)
int check_general_batch(const ovp_ctx* c, const ovp_general_batch* b, bool need_p, const int* only) {
  if (!b || b->n_feats < 0) return OVP_E_ARG;
  if (b->n_feats == 0) return 0;
  if (b->max_meas < 1 || !b->uv || !b->clone_idx || !b->cam_idx || !b->n_meas || (need_p && !b->p_FinG)) return OVP_E_ARG;
  for (int f = 0; f < b->n_feats; ++f) {
    if (only && !only[f]) continue;
    const int m = b->n_meas[f];
    if (m > OVP_GEN_MAX_MEAS) return OVP_E_CAPACITY;
    if (m < 0 || m > b->max_meas) return OVP_E_ARG;
    for (int k = 0; k < m; ++k) {
      const size_t o = (size_t)f * b->max_meas + k;
      if (b->clone_idx[o] < 0 || b->clone_idx[o] >= c->fp.n_clones) return OVP_E_ARG;
      if (b->cam_idx[o] < 0 || b->cam_idx[o] >= c->gen_ncams) return OVP_E_ARG;
    }
  }
  return 0;
}

static int gen_scratch(ovp_ctx* c, size_t bytes) {
  if (bytes <= c->gen_cap) return 0;
  HIPCHK(hipStreamSynchronize(c->stream));
  if (c->gen_buf) HIPCHK(hipFree(c->gen_buf));
  c->gen_buf = nullptr;
  c->gen_cap = 0;
  const size_t cap = bytes + bytes / 2 + 4096;
  HIPCHK(hipMalloc(&c->gen_buf, cap));
  c->gen_cap = cap;
  return 0;
}

static inline size_t al64(size_t v) { return (v + 63) & ~(size_t)63; }

extern "C" int ovp_msckf_general_features(ovp_ctx* c, const ovp_update_opts* o, const ovp_general_batch* b, uint8_t* accepted,
                                          double* chi2) {
  if (!c || !o || !b) return OVP_E_ARG;
  if (!c->have_state || !c->have_cov || c->gen_ncams < 1) return OVP_E_STATE;
  {
    const int rc = check_general_batch(c, b, true);
    if (rc) return rc;
  }
  const int n = c->n, F = b->n_feats, M = b->max_meas;
  const unsigned calmask = (o->do_calib_camera_pose ? 0x3Fu : 0u) | (o->do_calib_camera_intrinsics ? (0xFFu << 6) : 0u);
  for (int k = 0; k < c->gen_ncams; ++k) {  // calibration columns of every camera the options estimate
    if ((calmask & 0x3Fu) && (c->gen_calib_id[k] < 0 || c->gen_calib_id[k] + 6 > n)) return OVP_E_ARG;
    if ((calmask >> 6) && (c->gen_intr_id[k] < 0 || c->gen_intr_id[k] + 8 > n)) return OVP_E_ARG;
  }
  c->dense_cols.clear();  // (a second call replaces the pending pair, as ovp_msckf_dense_blocks does)
  if (F == 0) return 0;
  // involved state columns of every feature (UpdaterHelper.cpp:205-277) and their union, ascending; a feature's local columns are
  // its columns in the same order
  std::vector<int> stamp((size_t)n, -1), upos((size_t)n, -1), q((size_t)F);
  std::vector<std::vector<int>> fcols((size_t)F);
  std::vector<char> in_union((size_t)n, 0);
  for (int f = 0; f < F; ++f) {
    std::vector<int>& cf = fcols[f];
    auto add = [&](int col) {
      if (stamp[col] != f) {
        stamp[col] = f;
        cf.push_back(col);
        in_union[col] = 1;
      }
    };
    for (int k = 0; k < b->n_meas[f]; ++k) {
      const size_t ob = (size_t)f * M + k;
      const int cid = c->h_clone_id[b->clone_idx[ob]], cam = b->cam_idx[ob];
      for (int j = 0; j < 6; ++j) add(cid + j);
      for (int j = 0; j < 14; ++j)
        if ((calmask >> j) & 1) add(j < 6 ? c->gen_calib_id[cam] + j : c->gen_intr_id[cam] + (j - 6));
    }
    std::sort(cf.begin(), cf.end());
    q[f] = (int)cf.size();
  }
  std::vector<int> uni;
  for (int col = 0; col < n; ++col)
    if (in_union[col]) {
      upos[col] = (int)uni.size();
      uni.push_back(col);
    }
  const int nu = (int)uni.size();
  std::vector<int> loc((size_t)F * nu, -1);
  std::vector<long long> hp_off((size_t)F);
  long long hp_tot = 0;
  for (int f = 0; f < F; ++f) {
    for (int j = 0; j < q[f]; ++j) loc[(size_t)f * nu + upos[fcols[f][j]]] = j;
    hp_off[f] = hp_tot;
    hp_tot += (long long)(q[f] + 1) * 2 * b->n_meas[f];
  }
  // inputs: one pinned block, one copy [uv | clone_idx | cam_idx | n_meas | p_FinG | upos | loc | q | hp_off]; results behind them
  const size_t FM = (size_t)F * M;
  const size_t o_uv = 0, o_ci = al64(o_uv + sizeof(float) * 2 * FM), o_cam = al64(o_ci + sizeof(int) * FM),
               o_nm = al64(o_cam + sizeof(int) * FM), o_p = al64(o_nm + sizeof(int) * F), o_up = al64(o_p + sizeof(double) * 3 * F),
               o_loc = al64(o_up + sizeof(int) * n), o_q = al64(o_loc + sizeof(int) * loc.size()),
               o_off = al64(o_q + sizeof(int) * F), in_bytes = al64(o_off + sizeof(long long) * F);
  // device scratch [A | b | chi2 | accept | hp]: the first four come back to the host in one copy
  const size_t s_A = 0, s_b = s_A + sizeof(double) * (size_t)nu * nu, s_chi2 = s_b + sizeof(double) * nu,
               s_acc = s_chi2 + sizeof(double) * F, out_bytes = al64(s_acc + F), s_hp = out_bytes,
               scratch = s_hp + sizeof(double) * (size_t)hp_tot;
  void *ah = nullptr, *ad = nullptr;
  {
    const int rca = ovp_io_arena(c, in_bytes + out_bytes, &ah, &ad);
    if (rca) return rca;
    const int rcs = gen_scratch(c, scratch);
    if (rcs) return rcs;
  }
  char* h = (char*)ah;
  memcpy(h + o_uv, b->uv, sizeof(float) * 2 * FM);
  memcpy(h + o_ci, b->clone_idx, sizeof(int) * FM);
  memcpy(h + o_cam, b->cam_idx, sizeof(int) * FM);
  memcpy(h + o_nm, b->n_meas, sizeof(int) * F);
  memcpy(h + o_p, b->p_FinG, sizeof(double) * 3 * F);
  memcpy(h + o_up, upos.data(), sizeof(int) * n);
  memcpy(h + o_loc, loc.data(), sizeof(int) * loc.size());
  memcpy(h + o_q, q.data(), sizeof(int) * F);
  memcpy(h + o_off, hp_off.data(), sizeof(long long) * F);
  HIPCHK(hipMemcpyAsync(ad, ah, in_bytes, hipMemcpyHostToDevice, c->stream));
  char* d = (char*)ad;
  char* sd = (char*)c->gen_buf;
  ovp::GenParams g;
  memset(&g, 0, sizeof(g));
  g.fp = c->fp;
  g.fp.do_fej = o->do_fej;
  g.fp.calmask = calmask;
  g.fp.white_px = 1.0 / o->sigma_px;
  for (int k = 0; k < OVP_MAX_CAMERAS; ++k) {
    g.cam_fisheye[k] = c->gen_fisheye[k];
    g.cam_calib_id[k] = c->gen_calib_id[k];
    g.cam_intr_id[k] = c->gen_intr_id[k];
  }
  g.cam_cal = c->gen_cal;
  g.uv = (const float*)(d + o_uv);
  g.clone_idx = (const int*)(d + o_ci);
  g.cam_idx = (const int*)(d + o_cam);
  g.n_meas = (const int*)(d + o_nm);
  g.p_FinG = (const double*)(d + o_p);
  g.n_feats = F;
  g.max_meas = M;
  g.P = c->P;
  g.ldp = c->ld;
  g.chi2_table = c->chi2_table;
  g.chi2_mult = o->chi2_multiplier;
  g.upos = (const int*)(d + o_up);
  g.loc = (const int*)(d + o_loc);
  g.q = (const int*)(d + o_q);
  g.hp_off = (const long long*)(d + o_off);
  g.nu = nu;
  g.hp = (double*)(sd + s_hp);
  g.chi2 = (double*)(sd + s_chi2);
  g.accept = (unsigned char*)(sd + s_acc);
  HIPCHK(ovp_launch_feat_gen(&g, c->stream));
  HIPCHK(ovp_launch_gen_pair(&g, (double*)(sd + s_A), (double*)(sd + s_b), c->stream));
  HIPCHK(hipMemcpyAsync(h + in_bytes, sd, out_bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  const char* r = h + in_bytes;
  const double* x2 = (const double*)(r + s_chi2);
  const unsigned char* acc = (const unsigned char*)(r + s_acc);
  int n_acc = 0;
  for (int f = 0; f < F; ++f) {
    if (accepted) accepted[f] = acc[f] ? 1 : 0;
    if (chi2) chi2[f] = x2[f];
    n_acc += acc[f] ? 1 : 0;
  }
  if (n_acc > 0) {  // the pending pair the next point update of the context adds to its own (ovp_api_point.hip)
    const double* A = (const double*)(r + s_A);
    const double* bb = (const double*)(r + s_b);
    c->dense_cols = uni;
    c->dense_A.assign(A, A + (size_t)nu * nu);
    c->dense_b.assign(bb, bb + nu);
  }
  return 0;
}

extern "C" int ovp_triangulate_general(ovp_ctx* c, const ovp_triang_opts* o, const ovp_general_batch* b, const float* uv_norm,
                                       double* p_FinG_out, uint8_t* ok) {
  if (!c || !o || !b || !uv_norm || !ok) return OVP_E_ARG;
  if (!c->have_state || c->gen_ncams < 1) return OVP_E_STATE;
  {
    const int rc = check_general_batch(c, b, false);
    if (rc) return rc;
  }
  const int F = b->n_feats, M = b->max_meas;
  if (F == 0) return 0;
  // arena: [uv_norm | clone_idx | cam_idx | n_meas] in, [p_FinG | ok] out
  const size_t FM = (size_t)F * M;
  const size_t o_uv = 0, o_ci = al64(sizeof(float) * 2 * FM), o_cam = al64(o_ci + sizeof(int) * FM), o_nm = al64(o_cam + sizeof(int) * FM),
               o_p = al64(o_nm + sizeof(int) * F), o_ok = o_p + sizeof(double) * 3 * F, total = al64(o_ok + F);
  void *ah = nullptr, *ad = nullptr;
  {
    const int rca = ovp_io_arena(c, total, &ah, &ad);
    if (rca) return rca;
  }
  char *h = (char*)ah, *d = (char*)ad;
  memcpy(h + o_uv, uv_norm, sizeof(float) * 2 * FM);
  memcpy(h + o_ci, b->clone_idx, sizeof(int) * FM);
  memcpy(h + o_cam, b->cam_idx, sizeof(int) * FM);
  memcpy(h + o_nm, b->n_meas, sizeof(int) * F);
  HIPCHK(hipMemcpyAsync(d, h, o_p, hipMemcpyHostToDevice, c->stream));
  ovp::TriParams tp;
  memset(&tp, 0, sizeof(tp));
  tp.uvn = (const float*)(d + o_uv);
  tp.clone_idx = (const int*)(d + o_ci);
  tp.n_meas = (const int*)(d + o_nm);
  tp.n_feats = F;
  tp.max_meas = M;
  tp.clone_R = c->clone_R;
  tp.clone_p = c->clone_p;
  tp.cal = c->gen_cal;
  tp.refine_features = o->refine_features;
  tp.triangulate_1d = o->triangulate_1d;
  tp.max_runs = o->max_runs;
  tp.init_lamda = o->init_lamda;
  tp.max_lamda = o->max_lamda;
  tp.min_dx = o->min_dx;
  tp.min_dcost = o->min_dcost;
  tp.lam_mult = o->lam_mult;
  tp.min_dist = o->min_dist;
  tp.max_dist = o->max_dist;
  tp.max_baseline = o->max_baseline;
  tp.max_cond_number = o->max_cond_number;
  tp.p_FinG = (double*)(d + o_p);
  tp.ok = (unsigned char*)(d + o_ok);
  HIPCHK(ovp_launch_triangulate_gen(&tp, (const int*)(d + o_cam), c->stream));
  HIPCHK(hipMemcpyAsync(h + o_p, d + o_p, total - o_p, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (p_FinG_out) memcpy(p_FinG_out, h + o_p, sizeof(double) * 3 * F);
  memcpy(ok, h + o_ok, F);
  return 0;
}
