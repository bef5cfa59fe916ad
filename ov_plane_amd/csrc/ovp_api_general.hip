// C-ABI shim, part 6 (see ovp_ctx.h): general point features - observations of any camera, tracks longer than OVP_MAX_MEAS.
// The device form of ovp_msckf_dense_blocks (update/UpdaterMSCKF.cpp:695-764 for the features the batch format cannot carry) and
// the triangulation of such features over every camera (update/UpdaterMSCKF.cpp:120-166).  Kernels: csrc/k_feat_gen.hip,
// csrc/k_triang.hip (k_triangulate_gen).
#include "ovp_ctx.h"

extern "C" int ovp_cameras_upload(ovp_ctx* c, int n_cams, const ovp_camera_tables* cams) {
  if (!c || !cams || n_cams < 1 || n_cams > OVP_MAX_CAMERAS) return OVP_E_ARG;
  HIPCHK(c->gen_cal.alloc((size_t)20 * OVP_MAX_CAMERAS));
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
int check_general_batch(const ovp_ctx* c, const ovp_general_batch* b, bool need_p, const int* only, bool any_length) {
  if (!b || b->n_feats < 0) return OVP_E_ARG;
  if (b->n_feats == 0) return 0;
  if (b->max_meas < 1 || (!b->uv && !any_length) || !b->clone_idx || !b->cam_idx || !b->n_meas || (need_p && !b->p_FinG)) return OVP_E_ARG;
  for (int f = 0; f < b->n_feats; ++f) {
    if (only && !only[f]) continue;
    const int m = b->n_meas[f];
    if (m > OVP_GEN_MAX_MEAS && !any_length) return OVP_E_CAPACITY;
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
  if (bytes <= c->gen_buf.capacity()) return 0;
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(c->gen_buf.reserve(bytes, bytes / 2 + 4096));
  return 0;
}

extern "C" int ovp_msckf_general_features(ovp_ctx* c, const ovp_update_opts* o, const ovp_general_batch* b, uint8_t* accepted,
                                          double* chi2) {
  if (!c || !o || !b) return OVP_E_ARG;
  if (!c->have_state || !c->have_cov || c->gen_ncams < 1) return OVP_E_STATE;
  {
    const int rc = check_general_batch(c, b, true);
    if (rc) return rc;
  }
  const int n = c->n, F = b->n_feats, M = b->max_meas;
  const CalCols cc(c, o);
  if (cc.check(n, true)) return OVP_E_ARG;  // calibration columns of every camera the options estimate
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
        if (cc.on(j)) add(cc.col_of(cam, j));
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
  StageLayout lay;
  const size_t o_uv = lay.take(sizeof(float) * 2 * FM), o_ci = lay.take(sizeof(int) * FM), o_cam = lay.take(sizeof(int) * FM),
               o_nm = lay.take(sizeof(int) * F), o_p = lay.take(sizeof(double) * 3 * F), o_up = lay.take(sizeof(int) * n),
               o_loc = lay.take(sizeof(int) * loc.size()), o_q = lay.take(sizeof(int) * F),
               o_off = lay.take(sizeof(long long) * F), in_bytes = lay.bytes();
  // device scratch [A | b | chi2 | accept | hp]: the first four come back to the host in one copy
  const size_t s_A = 0, s_b = s_A + sizeof(double) * (size_t)nu * nu, s_chi2 = s_b + sizeof(double) * nu,
               s_acc = s_chi2 + sizeof(double) * F, out_bytes = StageLayout::al(s_acc + F), s_hp = out_bytes,
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
  g.fp.calmask = cc.mask;
  g.fp.white_px = 1.0 / o->sigma_px;
  cc.fill_cameras_and_columns(g);
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
  c->io.done();
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
  StageLayout lay;
  const size_t o_uv = lay.take(sizeof(float) * 2 * FM), o_ci = lay.take(sizeof(int) * FM), o_cam = lay.take(sizeof(int) * FM),
               o_nm = lay.take(sizeof(int) * F), o_p = lay.take(sizeof(double) * 3 * F + F), o_ok = o_p + sizeof(double) * 3 * F,
               total = lay.bytes();  // (ok directly behind p_FinG: the two come back in one copy)
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
  c->io.done();
  if (p_FinG_out) memcpy(p_FinG_out, h + o_p, sizeof(double) * 3 * F);
  memcpy(ok, h + o_ok, F);
  return 0;
}

// PlaneFitting::plane_fitting + optimize_plane for every plane of a frame (update/UpdaterMSCKF.cpp:262-401) as one device sequence
// (k_planefit.hip): the inputs cross the bus in one copy, the lists that link the RANSAC to the refinement stay on the device
// (gen_buf), the results come back in one copy behind one synchronisation.
extern "C" int ovp_plane_fit_refine(ovp_ctx* c, const ovp_general_batch* b, const float* uv_norm, const ovp_planefront_in* in,
                                    const ovp_planefront_out* out) {
  if (!c || !b || !in || !out) return OVP_E_ARG;
  if (!c->have_state || c->gen_ncams < 1) return OVP_E_STATE;
  const int P = in->n_planes;
  if (P < 0) return OVP_E_ARG;
  if (P == 0) return 0;
  if (!in->feat_start || !in->cp || !in->fix_plane) return OVP_E_ARG;
  const int F = b->n_feats, M = b->max_meas, NC = c->fp.n_clones, NK = c->gen_ncams;
  if (F < 0 || in->feat_start[0] != 0 || in->feat_start[P] != F) return OVP_E_ARG;
  for (int k = 0; k < P; ++k) {
    if (in->feat_start[k + 1] < in->feat_start[k]) return OVP_E_ARG;
    if (in->feat_start[k + 1] - in->feat_start[k] > 256) return OVP_E_CAPACITY;  // one thread per feature of a plane
  }
  if (F > 0 && !uv_norm) return OVP_E_ARG;
  {
    const int rc = check_general_batch(c, b, true, nullptr, true);
    if (rc) return rc;
  }
  size_t O = 0;
  for (int f = 0; f < F; ++f) O += (size_t)b->n_meas[f];
  if (O > (size_t)0x7fffffff) return OVP_E_CAPACITY;
  // the free planes, compacted for the RANSAC
  std::vector<int> free_slot((size_t)P, -1), rs_fs(1, 0);
  for (int k = 0; k < P; ++k)
    if (!in->fix_plane[k]) {
      free_slot[k] = (int)rs_fs.size() - 1;
      rs_fs.push_back(rs_fs.back() + in->feat_start[k + 1] - in->feat_start[k]);
    }
  const int NF = (int)rs_fs.size() - 1, FR = rs_fs.back();
  const size_t FM = (size_t)F * M, n_sets = (size_t)NF * 200 * 5;
  StageLayout lay, wlay;
  // arena: inputs ...
  const size_t o_fs = lay.take(sizeof(int) * (P + 1)), o_slot = lay.take(sizeof(int) * P), o_rfs = lay.take(sizeof(int) * (NF + 1)),
               o_rpts = lay.take(sizeof(double) * 3 * FR), o_sets = lay.take(sizeof(int) * n_sets), o_nm = lay.take(sizeof(int) * F),
               o_ci = lay.take(sizeof(int) * FM), o_cam = lay.take(sizeof(int) * FM), o_uv = lay.take(sizeof(float) * 2 * FM),
               o_p = lay.take(sizeof(double) * 3 * F), o_cp = lay.take(sizeof(double) * 3 * P), o_fix = lay.take((size_t)P);
  const size_t in_bytes = lay.bytes();
  // ... and results
  const size_t o_pose = lay.take(sizeof(double) * 12 * NC * NK), o_abcd = lay.take(sizeof(double) * 4 * NF), o_rinl = lay.take((size_t)FR),
               o_rok = lay.take((size_t)NF), o_cfs = lay.take(sizeof(int) * (P + 1)), o_src = lay.take(sizeof(int) * F),
               o_cpo = lay.take(sizeof(double) * 3 * P), o_po = lay.take(sizeof(double) * 3 * F), o_kept = lay.take((size_t)F),
               o_ok = lay.take((size_t)P), o_it = lay.take(sizeof(int) * P);
  const size_t total = lay.bytes();
  // device only: the refinement's lists
  const size_t w_p0 = wlay.take(sizeof(double) * 3 * F), w_no = wlay.take(sizeof(int) * F), w_is = wlay.take(sizeof(int) * (P + 1)),
               w_iob = wlay.take(sizeof(int) * O), w_ilf = wlay.take(sizeof(int) * O), w_fi0 = wlay.take(sizeof(int) * F),
               w_uv = wlay.take(sizeof(double) * 2 * O), w_R = wlay.take(sizeof(double) * 9 * O), w_pc = wlay.take(sizeof(double) * 3 * O),
               w_cp0 = wlay.take(sizeof(double) * 3 * P);
  const size_t work = wlay.bytes();
  void *ah = nullptr, *ad = nullptr;
  {
    const int rca = ovp_io_arena(c, total, &ah, &ad);
    if (rca) return rca;
    const int rcs = gen_scratch(c, work);
    if (rcs) return rcs;
  }
  char *h = (char*)ah, *d = (char*)ad, *w = (char*)c->gen_buf;
  memcpy(h + o_fs, in->feat_start, sizeof(int) * (P + 1));
  memcpy(h + o_slot, free_slot.data(), sizeof(int) * P);
  memcpy(h + o_rfs, rs_fs.data(), sizeof(int) * (NF + 1));
  for (int k = 0; k < P; ++k) {
    const int r = free_slot[k];
    if (r < 0) continue;
    const int f0 = in->feat_start[k], n = in->feat_start[k + 1] - f0;
    double* pts = (double*)(h + o_rpts) + 3 * (size_t)rs_fs[r];
    int* sets = (int*)(h + o_sets) + (size_t)r * 200 * 5;
    memcpy(pts, b->p_FinG + 3 * (size_t)f0, sizeof(double) * 3 * n);
    ovp_planefit_sets(pts, n, in->min_inlier_num, in->shuffle_variant, sets);
    if (n < 4) sets[0] = -1;  // update/UpdaterMSCKF.cpp:320-321: the RANSAC reports the plane as failed
  }
  if (F > 0) {
    memcpy(h + o_nm, b->n_meas, sizeof(int) * F);
    memcpy(h + o_ci, b->clone_idx, sizeof(int) * FM);
    memcpy(h + o_cam, b->cam_idx, sizeof(int) * FM);
    memcpy(h + o_uv, uv_norm, sizeof(float) * 2 * FM);
    memcpy(h + o_p, b->p_FinG, sizeof(double) * 3 * F);
  }
  memcpy(h + o_cp, in->cp, sizeof(double) * 3 * P);
  memcpy(h + o_fix, in->fix_plane, (size_t)P);
  HIPCHK(hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, c->stream));
  ovp::PlaneFrontJob j;
  memset(&j, 0, sizeof(j));
  j.n_planes = P;
  j.n_free = NF;
  j.n_clones = NC;
  j.n_cams = NK;
  j.max_meas = M;
  j.refine = in->refine ? 1 : 0;
  j.clone_R = c->clone_R;
  j.clone_p = c->clone_p;
  j.cam_cal = c->gen_cal;
  j.poses = (double*)(d + o_pose);
  j.rs_feat_start = (const int*)(d + o_rfs);
  j.rs_pts = (const double*)(d + o_rpts);
  j.rs_sets = (const int*)(d + o_sets);
  j.min_inlier_num = in->min_inlier_num;
  j.max_cond = in->max_cond;
  j.rs_abcd = (double*)(d + o_abcd);
  j.rs_inlier = (unsigned char*)(d + o_rinl);
  j.rs_ok = (unsigned char*)(d + o_rok);
  j.feat_start = (const int*)(d + o_fs);
  j.free_slot = (const int*)(d + o_slot);
  j.n_meas = (const int*)(d + o_nm);
  j.clone_idx = (const int*)(d + o_ci);
  j.cam_idx = (const int*)(d + o_cam);
  j.uvn = (const float*)(d + o_uv);
  j.p_in = (const double*)(d + o_p);
  j.cp_in = (const double*)(d + o_cp);
  j.fix_plane = (const unsigned char*)(d + o_fix);
  j.c_feat_start = (int*)(d + o_cfs);
  j.c_src = (int*)(d + o_src);
  j.c_p0 = (double*)(w + w_p0);
  j.c_n_obs = (int*)(w + w_no);
  j.item_start = (int*)(w + w_is);
  j.item_ob = (int*)(w + w_iob);
  j.item_lf = (int*)(w + w_ilf);
  j.feat_item0 = (int*)(w + w_fi0);
  j.it_uv = (double*)(w + w_uv);
  j.it_R = (double*)(w + w_R);
  j.it_p = (double*)(w + w_pc);
  j.cp0 = (double*)(w + w_cp0);
  j.sigma_px_norm = in->sigma_px_norm;
  j.sigma_c = in->sigma_c;
  // current camera: camera 0 of the tables at the pose given   (PlaneFitting.cpp:444-453)
  const double* cal0 = c->gen_cal_h;
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 3; ++k) {
      double sum = 0.0;
      for (int q = 0; q < 3; ++q) sum += cal0[3 * i + q] * in->R_GtoI[3 * q + k];
      j.R_GtoC[3 * i + k] = sum;
    }
  for (int i = 0; i < 3; ++i) {
    double sum = 0.0;
    for (int q = 0; q < 3; ++q) sum += j.R_GtoC[3 * q + i] * cal0[9 + q];
    j.p_CinG[i] = in->p_IinG[i] - sum;
  }
  j.cp_out = (double*)(d + o_cpo);
  j.c_p_out = (double*)(d + o_po);
  j.c_kept = (unsigned char*)(d + o_kept);
  j.ok = (unsigned char*)(d + o_ok);
  j.iterations = (int*)(d + o_it);
  HIPCHK(ovp_launch_planefront(&j, c->stream));
  const size_t out_end = j.refine ? total : o_cfs;  // (fit only: nothing behind the RANSAC's results was written)
  HIPCHK(hipMemcpyAsync(h + o_pose, d + o_pose, out_end - o_pose, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->io.done();
  if (out->poses) memcpy(out->poses, h + o_pose, sizeof(double) * 12 * NC * NK);
  const double* r_abcd = (const double*)(h + o_abcd);
  const unsigned char *r_inl = (const unsigned char*)(h + o_rinl), *r_ok = (const unsigned char*)(h + o_rok);
  const int *cfs = (const int*)(h + o_cfs), *src = (const int*)(h + o_src), *its = (const int*)(h + o_it);
  const double *d_cpo = (const double*)(h + o_cpo), *d_po = (const double*)(h + o_po);
  const unsigned char *d_kept = (const unsigned char*)(h + o_kept), *d_ok = (const unsigned char*)(h + o_ok);
  if (out->p_out && F > 0) memcpy(out->p_out, b->p_FinG, sizeof(double) * 3 * F);
  if (out->kept && F > 0) memset(out->kept, 0, (size_t)F);
  for (int k = 0; k < P; ++k) {
    const int r = free_slot[k], f0 = in->feat_start[k], n = in->feat_start[k + 1] - f0;
    const bool fitted = r < 0 || r_ok[r] != 0;
    if (out->fit_ok) out->fit_ok[k] = fitted ? 1 : 0;
    if (out->abcd)
      for (int a = 0; a < 4; ++a) out->abcd[4 * k + a] = r >= 0 ? r_abcd[4 * r + a] : 0.0;
    if (out->inlier)
      for (int i = 0; i < n; ++i) out->inlier[f0 + i] = r < 0 ? 1 : r_inl[rs_fs[r] + i];
    bool ok = fitted;
    if (j.refine) {
      ok = d_ok[k] != 0;
      for (int g = cfs[k]; g < cfs[k + 1]; ++g) {
        const int f = src[g];
        if (out->kept) out->kept[f] = d_kept[g] ? 1 : 0;
        if (out->p_out) memcpy(out->p_out + 3 * (size_t)f, d_po + 3 * (size_t)g, sizeof(double) * 3);
      }
    } else if (out->kept) {
      for (int i = 0; i < n; ++i) out->kept[f0 + i] = r < 0 ? 1 : r_inl[rs_fs[r] + i];
    }
    if (out->ok) out->ok[k] = ok ? 1 : 0;
    if (out->iterations) out->iterations[k] = j.refine ? its[k] : 0;
    if (out->cp_out)
      for (int a = 0; a < 3; ++a) {
        double v = in->cp[3 * k + a];  // the input when the plane is not ok
        if (ok && j.refine) v = d_cpo[3 * k + a];
        else if (ok && r >= 0) v = -r_abcd[4 * r + a] * r_abcd[4 * r + 3];  // UpdaterMSCKF.cpp:352
        out->cp_out[3 * k + a] = v;
      }
  }
  return 0;
}
