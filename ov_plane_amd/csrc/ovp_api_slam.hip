// C-ABI shim, part 5 (see ovp_ctx.h): SLAM landmarks (update/UpdaterSLAM.cpp:66-682) and triangulation.
#include "ovp_ctx.h"
#include "ovp_slam_plan.h"

// ---- triangulation ----------------------------------------------------------------
extern "C" void ovp_triang_defaults(ovp_triang_opts* o) {
  if (!o) return;
  o->refine_features = 1;
  o->max_runs = 5;
  o->init_lamda = 1e-3;
  o->max_lamda = 1e10;
  o->min_dx = 1e-6;
  o->min_dcost = 1e-6;
  o->lam_mult = 10.0;
  o->min_dist = 0.10;
  o->max_dist = 60.0;
  o->max_baseline = 40.0;
  o->max_cond_number = 10000.0;
  o->triangulate_1d = 0;
  o->reserved = 0;
}

extern "C" int ovp_triangulate(ovp_ctx* c, const ovp_triang_opts* o, const float* uv_norm, double* p_FinG_out, uint8_t* ok) {
  if (!c || !o || !uv_norm || !ok) return OVP_E_ARG;
  if (!c->have_state || !c->have_batch) return OVP_E_STATE;
  const size_t F = (size_t)c->n_feats, M = (size_t)c->max_meas;
  if (F == 0) return 0;
  // arena: [uv_norm | -> p_FinG | ok]
  StageLayout lay;
  const size_t b_uv = sizeof(float) * F * M * 2;
  lay.take(b_uv);
  const size_t o_p = lay.take(sizeof(double) * 3 * F), o_ok = lay.take(F), total = lay.bytes();
  void *ah = nullptr, *ad = nullptr;
  {
    const int rca = ovp_io_arena(c, total, &ah, &ad);
    if (rca) return rca;
  }
  memcpy(ah, uv_norm, b_uv);
  HIPCHK(hipMemcpyAsync(ad, ah, b_uv, hipMemcpyHostToDevice, c->stream));
  ovp::TriParams tp;
  tp.uvn = (const float*)ad;
  tp.clone_idx = c->fp.clone_idx;
  tp.n_meas = c->fp.n_meas;
  tp.n_feats = (int)F;
  tp.max_meas = (int)M;
  fill_tri_params(tp, c, o);
  tp.p_FinG = c->p_FinG;  // the library's own buffer even when the batch was bound to caller memory
  tp.ok = (unsigned char*)ad + o_ok;
  HIPCHK(ovp_launch_triangulate(&tp, c->stream));
  c->fp.p_FinG = c->p_FinG;
  // results into the pinned block (the positions stay in the batch's buffer on the device as linearisation points)
  HIPCHK(hipMemcpyAsync((char*)ah + o_p, c->p_FinG, sizeof(double) * 3 * F, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync((char*)ah + o_ok, (char*)ad + o_ok, F, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->io.done();
  if (p_FinG_out) memcpy(p_FinG_out, (char*)ah + o_p, sizeof(double) * 3 * F);
  memcpy(ok, (char*)ah + o_ok, F);
  return 0;
}

// ---- the two SLAM entries: plan on the host (ovp_slam_plan.h: checks, column lists, capacity - pure), then stage, enqueue, unpack ---
static_assert(SLAM_PLAN_MAX_MEAS_DEV == OVP_MAX_MEAS_DEV && SLAM_PLAN_LDG_CAP == OVP_LDG_CAP && OVP_MAX_CAMERAS == OVP_GEN_MAX_CAMS &&
                  SLAM_PLAN_IDV_CAP == sizeof(ovp::DinitParams::idv) / sizeof(int) &&
                  SLAM_PLAN_IDG_CAP == sizeof(ovp::DinitGenParams::idg) / sizeof(int),
              "ovp_slam_plan.h plans against the kernels' capacities");

// what the plans read from the context and the options
static SlamEnv slam_env(const ovp_ctx* c, const ovp_update_opts* o) {
  const CalCols cc(c, o);
  SlamEnv e;
  e.n = c->n;
  e.n_max = c->n_max;
  e.clone_id = c->h_clone_id.data();
  e.n_clones = (int)c->h_clone_id.size();
  e.calmask = cc.mask;
  for (int k = 0; k < 14; ++k) e.calcol[k] = cc.col[k];
  e.gen_ncams = c->gen_ncams;
  for (int k = 0; k < OVP_MAX_CAMERAS; ++k) e.gen_calib_id[k] = c->gen_calib_id[k], e.gen_intr_id[k] = c->gen_intr_id[k];
  return e;
}

static size_t slam_res_doubles(const ovp_ctx* c) { return 4 + (size_t)c->n_max + 8; }  // a result block: [res 4 | dx n_max | 8]

// ---- UpdaterSLAM::update on the device (update/UpdaterSLAM.cpp:424-673; csrc/k_slam.hip) ------------------------------------
// Rows and gate of every landmark in ONE launch against the resident covariance (no download of P, no host gate), the accepted rows
// stacked on the device, StateHelper::EKFUpdate on that stack (S-form up to 80 rows, information form above), one synchronisation.
// cam_idx == nullptr: ovp_slam_update (camera 0's tables of ovp_state_upload); otherwise ovp_slam_update_general: observation a of
// landmark l by camera cam_idx[l * max_meas + a], every camera's tables (camera 0 included) from ovp_cameras_upload.
struct SlamOut { double* dx; uint8_t* status; double* chi2; ovp_update_info* info; };

// offsets inside the pinned staging block and its device copy, and the shape of what comes back:
// [result block | per-landmark chi2 L | status L]
struct SlamStage {
  size_t p, p_fej, cp, cp_fej, preH, uv, ci, nm, lm, ps, r0, gp, gi, pr, pc, po, pio, pid, cam, cm, bytes;
  size_t res_doubles, status, lres_bytes;
};

static SlamStage slam_stage_layout(const SlamUpdatePlan& p, int n, size_t res_doubles) {
  const size_t L = (size_t)p.L, LM = L * p.M;
  StageLayout lay;
  SlamStage st;
  st.p = lay.take(sizeof(double) * 3 * L);
  st.p_fej = lay.take(sizeof(double) * 3 * L);
  st.cp = lay.take(sizeof(double) * 3 * L);
  st.cp_fej = lay.take(sizeof(double) * 3 * L);
  st.preH = lay.take(sizeof(double) * (p.preH + 1));
  st.uv = lay.take(sizeof(float) * 2 * LM);
  st.ci = lay.take(sizeof(int) * LM);
  st.nm = lay.take(sizeof(int) * L);
  st.lm = lay.take(sizeof(int) * L);
  st.ps = lay.take(sizeof(int) * L);
  st.r0 = lay.take(sizeof(int) * L);
  st.gp = lay.take(sizeof(int) * n);
  st.gi = lay.take(sizeof(int) * p.gcols);
  st.pr = lay.take(sizeof(int) * L);
  st.pc = lay.take(sizeof(int) * L);
  st.po = lay.take(sizeof(int) * L);
  st.pio = lay.take(sizeof(int) * L);
  st.pid = lay.take(sizeof(int) * (p.preI + 1));
  st.cam = lay.take(p.gen ? sizeof(int) * LM : 0);  // (general only)
  st.cm = lay.take(p.gen ? sizeof(int) * L : 0);
  st.bytes = lay.bytes();
  st.res_doubles = res_doubles;
  StageLayout lres;  // per-landmark results: [chi2 | status]
  lres.take(sizeof(double) * L);
  st.status = lres.take(L);
  st.lres_bytes = lres.bytes();
  return st;
}

// the pinned block h: zeros wherever the batch has nothing (cp / cp_fej of a call without planes, the pre_* tables of a call
// without host-built blocks, the cameras of a landmark with a host-built block or without observations)
static void slam_stage_fill(const SlamUpdatePlan& p, const ovp_slam_batch* b, const int* cam_idx, const SlamStage& st, char* h) {
  const size_t L = (size_t)p.L, M = (size_t)p.M;
  memset(h, 0, st.bytes);
  if (p.any_built) {
    memcpy(h + st.p, b->p_FinG, sizeof(double) * 3 * L);
    memcpy(h + st.p_fej, b->p_FinG_fej, sizeof(double) * 3 * L);
    memcpy(h + st.uv, b->uv, sizeof(float) * 2 * L * M);
    memcpy(h + st.ci, b->clone_idx, sizeof(int) * L * M);
  }
  if (p.gen) {
    int* cam = (int*)(h + st.cam);
    for (size_t l = 0; l < L; ++l)
      for (size_t a = 0; a < M; ++a) cam[l * M + a] = p.cam_mask[l] && (int)a < b->n_meas[l] ? cam_idx[l * M + a] : 0;
    memcpy(h + st.cm, p.cam_mask.data(), sizeof(int) * L);
  }
  if (b->cp) memcpy(h + st.cp, b->cp, sizeof(double) * 3 * L);
  if (b->cp_fej) memcpy(h + st.cp_fej, b->cp_fej, sizeof(double) * 3 * L);
  memcpy(h + st.nm, b->n_meas, sizeof(int) * L);
  memcpy(h + st.lm, b->landmark_id, sizeof(int) * L);
  for (size_t l = 0; l < L; ++l) ((int*)(h + st.ps))[l] = b->plane_state_id ? b->plane_state_id[l] : -1;
  memcpy(h + st.r0, p.row0.data(), sizeof(int) * L);
  memcpy(h + st.gp, p.gpos.data(), sizeof(int) * p.gpos.size());
  memcpy(h + st.gi, p.gids.data(), sizeof(int) * p.gcols);
  if (p.any_pre) {
    memcpy(h + st.pr, b->pre_rows, sizeof(int) * L);
    memcpy(h + st.pc, b->pre_cols, sizeof(int) * L);
    memcpy(h + st.po, p.pre_off.data(), sizeof(int) * L);
    memcpy(h + st.pio, p.pre_ids_off.data(), sizeof(int) * L);
    memcpy(h + st.preH, b->pre_H, sizeof(double) * p.preH);
    memcpy(h + st.pid, b->pre_ids, sizeof(int) * p.preI);
  }
}

// one pinned staging block -> one copy; the device buffers of the stacked system (Hd = H^T [gcols][m_total], resd), of the
// per-landmark results and of the blocks that do not fit LDS
static int slam_stage_upload(ovp_ctx* c, const SlamUpdatePlan& p, const ovp_slam_batch* b, const int* cam_idx, SlamStage* st) {
  *st = slam_stage_layout(p, c->n, slam_res_doubles(c));
  int rc = plane2_buffers(c, st->bytes, st->res_doubles * sizeof(double) + st->lres_bytes + 64);
  if (rc) return rc;
  char* h = c->pl_stage.begin(st->bytes, &rc);
  if (!h) return rc;
  slam_stage_fill(p, b, cam_idx, *st, h);
  HIPCHK(c->Hd.reserve((size_t)p.gcols * p.m_total, 64));
  HIPCHK(c->resd.reserve((size_t)p.m_total, 64));
  HIPCHK(c->slam_res.reserve(st->lres_bytes, 4096));
  if (!p.h_in_lds) HIPCHK(c->slam_hscr.reserve((size_t)p.L * p.rows_max * p.cols_max, 64));
  HIPCHK(c->pl_stage.send(st->bytes, c->stream, Fence::CallerWaits));
  return 0;
}

// S-form (k_init.hip) up to 80 stacked rows: scratch [res 4 | dx n_max | 8 | chi2 L | status L] M_all | Linv | y in smallbuf, so
// that everything the host wants comes back in ONE copy.  The plan says whether the stack fits the kernel; OVP_EKF_INFO_FORM and
// the capacity of smallbuf are the caller's conditions.
struct SlamScratch { bool sform; double *res, *M, *Li, *y; };
static SlamScratch slam_scratch(const ovp_ctx* c, const SlamUpdatePlan& p, const SlamStage& st) {
  SlamScratch k;
  k.res = c->smallbuf;
  k.M = (double*)((char*)(k.res + st.res_doubles) + st.lres_bytes);
  k.Li = k.M + (size_t)c->n * p.m_total;
  k.y = k.Li + (size_t)p.m_total * p.m_total;
  k.sform = !ekf_info_form_only() && p.sform_fits && (size_t)(k.y + p.m_total + 8 - c->smallbuf) <= c->smallbuf.capacity();
  return k;
}

static ovp::SlamParams slam_params(const ovp_ctx* c, const ovp_update_opts* o, const SlamUpdatePlan& p, const SlamStage& st,
                                   const SlamScratch& k) {
  const char* d = c->pl_stage.dev();
  ovp::SlamParams sp;
  memset(&sp, 0, sizeof(sp));
  sp.fp = c->fp;
  sp.fp.uv = (const float*)(d + st.uv);
  sp.fp.clone_idx = (const int*)(d + st.ci);
  sp.fp.n_meas = (const int*)(d + st.nm);
  sp.fp.p_FinG = (const double*)(d + st.p);
  sp.fp.n_feats = p.L;
  sp.fp.max_meas = p.M;
  sp.fp.do_fej = o->do_fej;
  CalCols(c, o).fill(sp.fp);
  sp.fp.white_px = 1.0 / o->sigma_px;
  sp.fp.chi2_mult = o->chi2_multiplier;
  sp.fp.chi2_table = c->chi2_table;
  sp.fp.P = c->P;
  sp.fp.n = c->n;
  sp.fp.ldp = c->ld;
  sp.p_fej = (const double*)(d + st.p_fej);
  sp.lm_id = (const int*)(d + st.lm);
  sp.plane_sid = (const int*)(d + st.ps);
  sp.cp = (const double*)(d + st.cp);
  sp.cp_fej = (const double*)(d + st.cp_fej);
  sp.white_c = 1.0 / o->sigma_constraint;
  if (p.any_pre) {
    sp.pre_rows = (const int*)(d + st.pr);
    sp.pre_cols = (const int*)(d + st.pc);
    sp.pre_off = (const int*)(d + st.po);
    sp.pre_ids_off = (const int*)(d + st.pio);
    sp.pre_H = (const double*)(d + st.preH);
    sp.pre_ids = (const int*)(d + st.pid);
  }
  sp.row0 = (const int*)(d + st.r0);
  sp.gpos = (const int*)(d + st.gp);
  sp.Ht = c->Hd;
  sp.m_total = p.m_total;
  sp.gcols = p.gcols;
  sp.res_out = c->resd;
  sp.Hscr = c->slam_hscr;
  sp.rows_max = p.rows_max;
  sp.cols_max = p.cols_max;
  sp.h_in_lds = p.h_in_lds;
  if (k.sform) {
    sp.chi2 = k.res + st.res_doubles;
    sp.status = (unsigned char*)(k.res + st.res_doubles) + st.status;
    sp.Mall = k.M;
  } else {
    sp.chi2 = (double*)c->slam_res;
    sp.status = (unsigned char*)c->slam_res + st.status;
  }
  return sp;
}

static ovp::SlamGenParams slam_gen_params(const ovp_ctx* c, const ovp_update_opts* o, const ovp::SlamParams& sp, const SlamStage& st) {
  const char* d = c->pl_stage.dev();
  ovp::SlamGenParams gp;
  memset(&gp, 0, sizeof(gp));
  gp.sp = sp;
  gp.cam_idx = (const int*)(d + st.cam);
  gp.cam_mask = (const int*)(d + st.cm);
  CalCols(c, o).fill_cameras_and_columns(gp);
  return gp;
}

// rows + gate of every landmark, accepted rows into the stack
static int slam_enqueue_gate(ovp_ctx* c, const ovp_update_opts* o, const SlamUpdatePlan& p, const SlamStage& st, const SlamScratch& k) {
  const ovp::SlamParams sp = slam_params(c, o, p, st, k);
  const size_t lds = ovp_slam_gate_lds(p.rows_max, p.cols_max, p.h_in_lds);
  if (p.gen) {
    const ovp::SlamGenParams gp = slam_gen_params(c, o, sp, st);
    HIPCHK(ovp_launch_slam_gate_gen(&gp, p.L, lds, c->stream));
  } else {
    HIPCHK(ovp_launch_slam_gate(&sp, p.L, lds, c->stream));
  }
  return 0;
}

// hl = the per-landmark part of the result block, [chi2 L | status L at o_status]
static void slam_finish_landmarks(const SlamUpdatePlan& p, const ovp_slam_batch* b, const char* hl, size_t o_status, const SlamOut& out) {
  const int L = p.L;
  if (out.chi2) memcpy(out.chi2, hl, sizeof(double) * L);
  if (out.status) memcpy(out.status, hl + o_status, L);
  if (!out.info) return;
  out.info->n_cols = p.gcols;
  for (int l = 0; l < L; ++l) {
    const unsigned char st = ((const unsigned char*)(hl + o_status))[l];
    if (!st) continue;
    out.info->n_accepted++;
    const int rows_l = (l + 1 < L ? p.row0[l + 1] : p.m_total) - p.row0[l];
    const bool pre = p.any_pre && b->pre_rows[l] > 0;
    out.info->n_rows += (st == 2 && !pre) ? 2 * b->n_meas[l] : rows_l;
  }
}

// StateHelper::EKFUpdate on the stack, S-form: two launches, one copy back
static int slam_tail_sform(ovp_ctx* c, const SlamUpdatePlan& p, const ovp_slam_batch* b, const SlamStage& st, const SlamScratch& k,
                           const SlamOut& out) {
  hipStream_t s = c->stream;
  const int n = c->n, rows = p.m_total;
  const int* dgid = (const int*)(c->pl_stage.dev() + st.gi);
  HIPCHK(ovp_launch_init_core(c->P, c->ld, n, dgid, p.gcols, c->Hd, 0, rows, k.M, c->resd /* unused: k = 0 */, c->resd, c->resd, 1.0,
                              1e300, k.Li, k.y, k.res, s));
  HIPCHK(ovp_launch_init_update(c->P, c->P_tmp, c->ld, n, k.M, rows, 0, rows, k.Li, k.y, k.res, k.res + 4, s));
  const int rf = ovp_fetch_to_hres(c, k.res, st.res_doubles * sizeof(double) + st.lres_bytes, s);
  if (rf) return rf;
  c->pl_stage.done();
  const double* hres = (const double*)c->pl_hres.payload();
  slam_finish_landmarks(p, b, (const char*)(hres + st.res_doubles), st.status, out);
  if (out.info) {
    out.info->not_spd = hres[1] > 0.5 ? 0 : 1;
    out.info->neg_diag = hres[2] != 0.0;
  }
  if (!(hres[1] > 0.5)) return OVP_E_NOTSPD;  // S = H P H^T + I lost definiteness: P is not a covariance; nothing was written
  c->P.swap(c->P_tmp);
  if (out.dx) memcpy(out.dx, hres + 4, sizeof(double) * n);
  return hres[2] != 0.0 ? OVP_E_NEGDIAG : 0;
}

// information form: A = H^T H, b = H^T r on the call's columns, scattered to the state
static int slam_tail_info(ovp_ctx* c, const SlamUpdatePlan& p, const ovp_slam_batch* b, const SlamStage& st, const SlamOut& out) {
  hipStream_t s = c->stream;
  const int n = c->n, gcols = p.gcols, m_total = p.m_total;
  const int* dgid = (const int*)(c->pl_stage.dev() + st.gi);
  char* hl = (char*)c->pl_hres.payload() + st.res_doubles * sizeof(double);
  // nothing accepted: no update at all (update/UpdaterSLAM.cpp:661-663) - the information form of an empty stack would still
  // rewrite the covariance as chol(P) chol(P)^T, equal to P only to rounding.  The statuses decide it, so they are fetched first.
  HIPCHK(hipMemcpyAsync(hl, c->slam_res, st.lres_bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  {
    bool any = false;
    for (int l = 0; l < p.L; ++l) any = any || ((const unsigned char*)(hl + st.status))[l] != 0;
    if (!any) {
      c->pl_stage.done();
      slam_finish_landmarks(p, b, hl, st.status, out);
      return 0;
    }
  }
  HIPCHK(c->Acc.alloc((size_t)c->n_max * c->n_max));
  HIPCHK(c->bcc.alloc((size_t)c->n_max));
  HIPCHK(hipMemsetAsync(c->flags, 0, sizeof(int) * 4, s));
  HIPCHK(ovp_launch_gemm(0, 1, gcols, gcols, m_total, c->Hd, m_total, c->Hd, m_total, c->Acc, gcols, 0, s));
  HIPCHK(ovp_launch_gemm(0, 0, gcols, 1, m_total, c->Hd, m_total, c->resd, 1, c->bcc, 1, 0, s));
  HIPCHK(hipMemsetAsync(c->Ab, 0, sizeof(double) * (size_t)(n + 1) * c->ld, s));
  HIPCHK(ovp_launch_scatter_gram(c->Acc, c->bcc, gcols, dgid, c->Ab, c->ld, n, s));
  {
    std::vector<int> ids(p.gids);
    std::sort(ids.begin(), ids.end());
    const int rs = set_substate(c, ids);
    if (rs) return rs;
  }
  const int rc = ekf_from_gram(c, PointTail());
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(c->h_dx, c->dx, sizeof(double) * n, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(c->h_flags, c->flags, sizeof(int) * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  c->pl_stage.done();
  slam_finish_landmarks(p, b, hl, st.status, out);
  if (c->h_flags[0]) {  // positive semi-definite prior: S-form instead of the factor of P
    const int rs = ekf_sform(c);
    if (rs) return rs;
  }
  if (out.dx) memcpy(out.dx, c->h_dx, sizeof(double) * n);
  if (out.info) {
    out.info->not_spd = c->h_flags[0];
    out.info->neg_diag = c->h_flags[1];
  }
  if (c->h_flags[0]) return OVP_E_NOTSPD;
  if (c->h_flags[1]) return OVP_E_NEGDIAG;
  return 0;
}

static int slam_update_impl(ovp_ctx* c, const ovp_update_opts* o, const ovp_slam_batch* b, const int* cam_idx, const SlamOut& out) {
  drop_kept_factor(c);  // (writes the covariance: a kept factor no longer belongs to it)
  if (!c || !o || !b || b->n_landmarks < 0) return OVP_E_ARG;
  if (!c->have_state || !c->have_cov) return OVP_E_STATE;
  c->slam_dbg_rows = 0;  // (a call that fails before its gate leaves nothing for ovp_debug_read "slam_*")
  c->slam_dbg_sform = false;
  c->slam_dbg_h_in_lds = 0;
  c->slam_dbg_cols.clear();
  const int L = b->n_landmarks;
  if (out.info) memset(out.info, 0, sizeof(*out.info));
  if (out.dx) memset(out.dx, 0, sizeof(double) * c->n);
  if (L == 0) return 0;
  SlamUpdatePlan plan;
  int rc = plan_slam_update(slam_env(c, o), b, cam_idx, &plan);
  if (rc) return rc;
  if (plan.nothing) {
    if (out.status) memset(out.status, 0, L);
    if (out.chi2) memset(out.chi2, 0, sizeof(double) * L);
    return 0;
  }
  SlamStage st;
  rc = slam_stage_upload(c, plan, b, cam_idx, &st);
  if (rc) return rc;
  const SlamScratch k = slam_scratch(c, plan, st);
  c->slam_dbg_rows = plan.m_total;  // (what ovp_debug_read "slam_*" reads back)
  c->slam_dbg_n = c->n;
  c->slam_dbg_sform = k.sform;
  c->slam_dbg_h_in_lds = plan.h_in_lds;
  c->slam_dbg_M = (size_t)(k.M - (double*)c->smallbuf);
  c->slam_dbg_cols = plan.gids;
  rc = slam_enqueue_gate(c, o, plan, st, k);
  if (rc) return rc;
  return k.sform ? slam_tail_sform(c, plan, b, st, k, out) : slam_tail_info(c, plan, b, st, out);
}

extern "C" int ovp_slam_update(ovp_ctx* c, const ovp_update_opts* o, const ovp_slam_batch* b, double* dx_host, uint8_t* status_host,
                               double* chi2_host, ovp_update_info* info) {
  return slam_update_impl(c, o, b, nullptr, SlamOut{dx_host, status_host, chi2_host, info});
}

extern "C" int ovp_slam_update_general(ovp_ctx* c, const ovp_update_opts* o, const ovp_slam_batch* b, const int* cam_idx,
                                       double* dx_host, uint8_t* status_host, double* chi2_host, ovp_update_info* info) {
  if (!c || !o || !b || !cam_idx || c->gen_ncams < 1) return OVP_E_ARG;  // (every camera from the tables of ovp_cameras_upload)
  return slam_update_impl(c, o, b, cam_idx, SlamOut{dx_host, status_host, chi2_host, info});
}

// ---- UpdaterSLAM::delayed_init, candidate loop on the device (update/UpdaterSLAM.cpp:204-364; csrc/k_dinit.hip) -----------------
// The candidate arrays come from an ovp_feature_batch (cam_idx == nullptr: camera 0's tables of ovp_state_upload, ovp_slam_delayed_init)
// or from an ovp_general_batch (ovp_slam_delayed_init_general: every camera's tables from ovp_cameras_upload; a candidate's columns are
// the clone blocks of its distinct clones in first-seen order, then the estimated calibration columns of each of its cameras in
// camera order; every commit updates camera 0's table of ovp_state_upload AND every camera of ovp_cameras_upload).
//
// with_planes (ovp_slam_delayed_init_planes; csrc/k_dinit.hip k_dinit_rows_pl / k_dinit_rows_gen_pl, csrc/k_init.hip *_sk): a
// candidate on a plane of the state (pl->plane_of_cand) is enqueued as TWO attempts on the same three-column slot - A with its m
// point-on-plane rows and the plane's columns at p_FinG, B without them at p_FinG_noplane; B's four kernels read A's result block
// on the device and do nothing but forward it when A was accepted, so the loop stays one enqueue.  The planes live in a device
// table [cp | cp_fej | id] inside the staging block, and every commit adds the accepted correction to every closest point.
// ok_host then carries the status codes of ovp_slam_update (0 / 1 / 2).  Without with_planes nothing here differs from before.
struct DinitCands { int L, M; const float* uv; const int *clone_idx, *cam_idx, *n_meas; const double* p; };
struct DinitOut { uint8_t* ok; double* chi2; int* new_id; double* delta_init; double* dx; int dx_stride; };

// offsets inside the staging block: the candidates as a feature batch, every attempt's column list [NA][cols_max], (general) the
// cameras, (with planes) the fallback's linearisation points and the plane table
struct DinitStage { size_t p, uv, ci, nm, id, cam, p2, pt, bytes, res_doubles; };

static DinitStage dinit_stage_layout(const DinitPlan& p, size_t res_doubles) {
  const size_t L = (size_t)p.L, LM = L * p.M;
  StageLayout lay;
  DinitStage st;
  st.p = lay.take(sizeof(double) * 3 * L);
  st.uv = lay.take(sizeof(float) * 2 * LM);
  st.ci = lay.take(sizeof(int) * LM);
  st.nm = lay.take(sizeof(int) * L);
  st.id = lay.take(sizeof(int) * p.att.size() * p.cols_max);
  st.cam = lay.take(p.gen ? sizeof(int) * LM : 0);
  st.p2 = lay.take(p.with_planes ? sizeof(double) * 3 * L : 0);
  st.pt = lay.take(sizeof(double) * OVP_DINIT_PLTAB * (size_t)p.n_pl);
  st.bytes = lay.bytes();
  st.res_doubles = res_doubles;
  return st;
}

static void dinit_stage_fill(const DinitPlan& p, const DinitCands& b, const ovp_dinit_planes* pl, const DinitStage& st, char* h) {
  const size_t L = (size_t)p.L, LM = L * p.M;
  memcpy(h + st.p, b.p, sizeof(double) * 3 * L);
  memcpy(h + st.uv, b.uv, sizeof(float) * 2 * LM);
  memcpy(h + st.ci, b.clone_idx, sizeof(int) * LM);
  memcpy(h + st.nm, b.n_meas, sizeof(int) * L);
  if (p.gen) memcpy(h + st.cam, b.cam_idx, sizeof(int) * LM);
  for (size_t a = 0; a < p.att.size(); ++a) dinit_attempt_ids(p, pl, (int)a, (int*)(h + st.id) + a * p.cols_max);
  if (!p.with_planes) return;
  memcpy(h + st.p2, pl && pl->p_FinG_noplane ? pl->p_FinG_noplane : b.p, sizeof(double) * 3 * L);
  double* tab = (double*)(h + st.pt);
  for (int q = 0; q < p.n_pl; ++q) {
    double* e = tab + (size_t)q * OVP_DINIT_PLTAB;
    for (int k = 0; k < 3; ++k) e[k] = pl->cp[3 * q + k], e[3 + k] = (pl->cp_fej ? pl->cp_fej : pl->cp)[3 * q + k];
    e[6] = (double)pl->plane_state_id[q];
    e[7] = 0.0;
  }
}

// device scratch of the loop inside c->dinit_buf: [result blocks NA x res_doubles | Ht | Mall | Linv | y | Hinv 9 | Rk 9 | resid]
struct DinitScratch { double *res0, *Ht, *M, *Li, *y, *Hinv, *Rk, *resid; };

static int dinit_stage_upload(ovp_ctx* c, const DinitPlan& p, const DinitCands& b, const ovp_dinit_planes* pl, DinitStage* st,
                              DinitScratch* k) {
  const size_t NA = p.att.size(), rows_max = (size_t)p.rows_max, n_end = (size_t)p.n0 + 3 * p.L;
  *st = dinit_stage_layout(p, slam_res_doubles(c));
  int rc = plane2_buffers(c, st->bytes, sizeof(double) * st->res_doubles * NA + 64);
  if (rc) return rc;
  char* h = c->pl_stage.begin(st->bytes, &rc);
  if (!h) return rc;
  dinit_stage_fill(p, b, pl, *st, h);
  if (p.with_planes) {  // the plane table of the last call inside pl_stage (ovp_debug_read "dinit_planes")
    c->dinit_pltab_off = st->pt;
    c->dinit_nplanes = p.n_pl;
  }
  const size_t need = st->res_doubles * NA + (size_t)p.cols_max * rows_max + n_end * rows_max + rows_max * rows_max + rows_max + 32 +
                      rows_max + 64;
  HIPCHK(c->dinit_buf.reserve(need, 1024));
  k->res0 = c->dinit_buf;
  k->Ht = k->res0 + st->res_doubles * NA;
  k->M = k->Ht + (size_t)p.cols_max * rows_max;
  k->Li = k->M + n_end * rows_max;
  k->y = k->Li + rows_max * rows_max;
  k->Hinv = k->y + rows_max + 8;
  k->Rk = k->Hinv + 12;
  k->resid = k->Rk + 12;
  HIPCHK(c->pl_stage.send(st->bytes, c->stream, Fence::CallerWaits));
  return 0;
}

// the three parameter structs of a call: everything but the per-attempt fields (dinit_enqueue_attempt)
static ovp::DinitParams dinit_params(const ovp_ctx* c, const ovp_update_opts* o, const DinitPlan& p, const DinitStage& st,
                                     const DinitScratch& k) {
  const char* d = c->pl_stage.dev();
  ovp::DinitParams dp;
  memset(&dp, 0, sizeof(dp));
  dp.fp = c->fp;
  dp.fp.uv = (const float*)(d + st.uv);
  dp.fp.clone_idx = (const int*)(d + st.ci);
  dp.fp.n_meas = (const int*)(d + st.nm);
  dp.fp.p_FinG = (const double*)(d + st.p);
  dp.fp.n_feats = p.L;
  dp.fp.max_meas = p.M;
  dp.fp.do_fej = o->do_fej;
  CalCols(c, o).fill(dp.fp);
  dp.fp.white_px = 1.0 / o->sigma_px;
  dp.fp.ldp = c->ld;
  dp.n_max = c->n_max;
  dp.P = c->P;
  dp.clone_R = c->clone_R;
  dp.clone_p = c->clone_p;
  dp.cal = c->cal;
  dp.Ht = k.Ht;
  dp.Hinv = k.Hinv;
  dp.Rk = k.Rk;
  dp.resid = k.resid;
  return dp;
}

static ovp::DinitGenParams dinit_gen_params(const ovp_ctx* c, const ovp_update_opts* o, const DinitStage& st) {  // (general only)
  ovp::DinitGenParams gp;
  memset(&gp, 0, sizeof(gp));
  CalCols(c, o).fill_cameras_and_columns(gp);
  gp.n_cams = c->gen_ncams;
  gp.cam_idx = (const int*)(c->pl_stage.dev() + st.cam);
  return gp;
}

static ovp::DinitPlaneParams dinit_plane_params(const ovp_ctx* c, const ovp_update_opts* o, const DinitPlan& p, const DinitStage& st) {
  ovp::DinitPlaneParams pp;  // (with planes only)
  memset(&pp, 0, sizeof(pp));
  pp.tab = (double*)(c->pl_stage.dev() + st.pt);
  pp.n_planes = p.n_pl;
  pp.white_c = 1.0 / o->sigma_constraint;
  return pp;
}

struct DinitCall { ovp::DinitParams dp; ovp::DinitGenParams gp; ovp::DinitPlaneParams pp; };

// the rows kernel of the call's kind: camera 0 or any camera, without or with the plane table
static hipError_t dinit_launch_rows(const DinitPlan& p, DinitCall& k, size_t lds, hipStream_t s) {
  if (p.gen) {
    k.gp.dp = k.dp;
    return p.with_planes ? ovp_launch_dinit_rows_gen_pl(&k.gp, &k.pp, lds, s) : ovp_launch_dinit_rows_gen(&k.gp, lds, s);
  }
  return p.with_planes ? ovp_launch_dinit_rows_pl(&k.dp, &k.pp, lds, s) : ovp_launch_dinit_rows(&k.dp, lds, s);
}

// one attempt: the previous attempt's commit and this one's rows, M = P[:, ids] H^T, the gate + initialize_invertible, the update
static int dinit_enqueue_attempt(ovp_ctx* c, const ovp_update_opts* o, const DinitPlan& p, const DinitStage& st, const DinitScratch& b,
                                 int a, DinitCall& k) {
  hipStream_t s = c->stream;
  const DinitAttempt& t = p.att[a];
  const char* d = c->pl_stage.dev();
  const int n = p.n0 + 3 * t.l, rup = t.rows - 3;
  const bool second = t.skip_blk >= 0;  // attempt B: attempt A has committed the previous candidate
  const double* skip = second ? b.res0 + st.res_doubles * t.skip_blk : nullptr;
  k.dp.cand = t.l;
  k.dp.m_obs = t.m;
  k.dp.n = n;
  k.dp.prev_res = (a && !second) ? b.res0 + st.res_doubles * (a - 1) : nullptr;
  k.dp.ids = (const int*)(d + st.id) + (size_t)a * p.cols_max;
  k.dp.res = b.res0 + st.res_doubles * a;
  k.dp.fp.p_FinG = (const double*)(d + (second ? st.p2 : st.p));
  k.pp.slot = t.slot;
  k.pp.skip = skip;
  const int* hids = (const int*)(c->pl_stage.host() + st.id) + (size_t)a * p.cols_max;
  if (p.gen) {
    k.gp.cols = t.cols;
    memcpy(k.gp.idg, hids, sizeof(int) * t.cols);
    memcpy(k.gp.ocol, p.ocol[t.l].data(), sizeof(k.gp.ocol));
    memcpy(k.gp.ccol, p.ccol[t.l].data(), sizeof(k.gp.ccol));
  } else {
    memcpy(k.dp.idv, hids, sizeof(int) * t.cols);
  }
  const size_t lds = p.with_planes ? ovp_dinit_pl_rows_lds(t.rows, t.cols)
                                   : (p.gen ? ovp_dinit_gen_rows_lds(t.m, t.cols) : ovp_dinit_rows_lds(t.m, p.ncal));
  HIPCHK(dinit_launch_rows(p, k, lds, s));
  HIPCHK(ovp_launch_init_m_sk(skip, c->P, c->ld, n, k.dp.ids, t.cols, b.Ht, t.rows, b.M, s));  // M = P[:, ids] H_all^T on many workgroups
  // chi2 of the update rows with dof = all rows (StateHelper.cpp:471), initialize_invertible, update in place
  const double thr = o->chi2_multiplier * ovp_chi2_quantile_095(t.rows);
  HIPCHK(ovp_launch_init_core_sk(skip, c->P, c->ld, n, k.dp.ids, t.cols, b.Ht, 3, rup, b.M, b.Hinv, b.Rk, b.resid, 1.0, thr, b.Li, b.y,
                                 k.dp.res, s));
  HIPCHK(ovp_launch_init_update_sk(skip, (int)st.res_doubles, c->P, c->P, c->ld, n + 3, b.M, t.rows, 3, rup, b.Li, b.y, k.dp.res,
                                   k.dp.res + 4, s));
  return 0;
}

// behind the last attempt: its commit alone
static int dinit_enqueue_commit(ovp_ctx* c, const DinitPlan& p, const DinitStage& st, const DinitScratch& b, DinitCall& k) {
  k.dp.cand = -1;
  k.dp.n = p.n0 + 3 * p.L;
  k.dp.prev_res = b.res0 + st.res_doubles * (p.att.size() - 1);
  k.dp.fp.p_FinG = (const double*)(c->pl_stage.dev() + st.p);
  k.pp.slot = 0;
  k.pp.skip = nullptr;
  HIPCHK(dinit_launch_rows(p, k, 64, c->stream));
  return 0;
}

// hres = the attempts' result blocks on the host.  Final layout: the inert blocks of the rejected candidates go (last first), the
// accepted ones move up; status 0 / 1 / 2, delta_init and every accepted candidate's dx row at the final ids.
static int dinit_unpack(ovp_ctx* c, const DinitPlan& p, const double* hres, size_t res_doubles, const DinitOut& out) {
  const int L = p.L, n0 = p.n0;
  std::vector<int> final_id(L, -1);
  int n_acc = 0, negdiag = 0;
  for (int l = 0; l < L; ++l) {
    const double* r = hres + res_doubles * p.blk_final[l];  // (the block of the attempt that decided: B carries A's when A stood)
    if (r[1] > 0.5) final_id[l] = n0 + 3 * n_acc++;
    if (r[1] > 0.5 && r[2] != 0.0) negdiag = 1;
  }
  for (int l = L - 1; l >= 0; --l)
    if (final_id[l] < 0) {
      const int rc = ovp_cov_marginalize(c, n0 + 3 * l, 3);
      if (rc) return rc;
    }
  for (int l = 0; l < L; ++l) {
    const double* r = hres + res_doubles * p.blk_final[l];
    const bool ok = r[1] > 0.5;
    // with planes: 1 = accepted (with its plane rows if it had a plane), 2 = accepted by the fallback without them
    const bool by_B = p.blk_final[l] != p.blk_A[l] && !(hres[res_doubles * p.blk_A[l] + 1] > 0.5);
    if (out.ok) out.ok[l] = ok ? (by_B ? 2 : 1) : 0;
    if (out.chi2) out.chi2[l] = r[0];
    if (out.new_id) out.new_id[l] = final_id[l];
    if (out.delta_init)
      for (int k = 0; k < 3; ++k) out.delta_init[3 * l + k] = ok ? r[4 + c->n_max + k] : 0.0;
    if (out.dx) {
      double* dx = out.dx + (size_t)l * out.dx_stride;
      memset(dx, 0, sizeof(double) * out.dx_stride);
      if (ok) {
        memcpy(dx, r + 4, sizeof(double) * n0);
        for (int g = 0; g <= l; ++g)  // the landmarks that were state variables at that point, at their final ids
          if (final_id[g] >= 0)
            for (int k = 0; k < 3; ++k) dx[final_id[g] + k] = r[4 + n0 + 3 * g + k];
      }
    }
  }
  return negdiag ? OVP_E_NEGDIAG : 0;
}

static int slam_delayed_init_impl(ovp_ctx* c, const ovp_update_opts* o, const DinitCands& b, const DinitOut& out, bool with_planes = false,
                                  const ovp_dinit_planes* pl = nullptr) {
  drop_kept_factor(c);  // (writes the covariance: a kept factor no longer belongs to it)
  if (!c || !o || b.L < 0) return OVP_E_ARG;
  if (!c->have_state || !c->have_cov) return OVP_E_STATE;
  if (b.L == 0) return 0;
  DinitPlan plan;
  // (a dx row is checked against its stride only when dx is wanted; a negative stride is then too short like any other)
  int rc = plan_delayed_init(slam_env(c, o), b.L, b.M, b.uv, b.clone_idx, b.cam_idx, b.n_meas, b.p, pl, with_planes,
                             out.dx ? std::max(out.dx_stride, 0) : -1, &plan);
  if (rc) return rc;
  DinitStage st;
  DinitScratch k;
  rc = dinit_stage_upload(c, plan, b, pl, &st, &k);
  if (rc) return rc;
  DinitCall call{dinit_params(c, o, plan, st, k), dinit_gen_params(c, o, st), dinit_plane_params(c, o, plan, st)};
  const int NA = (int)plan.att.size();
  for (int a = 0; a < NA; ++a) {
    rc = dinit_enqueue_attempt(c, o, plan, st, k, a, call);
    if (rc) return rc;
  }
  rc = dinit_enqueue_commit(c, plan, st, k, call);
  if (rc) return rc;
  rc = ovp_fetch_to_hres(c, k.res0, sizeof(double) * st.res_doubles * NA, c->stream);
  if (rc) return rc;
  c->pl_stage.done();
  c->n = plan.n0 + 3 * plan.L;
  return dinit_unpack(c, plan, (const double*)c->pl_hres.payload(), st.res_doubles, out);
}

// A null batch: ovp_slam_delayed_init and _planes drop the kept factor before they return OVP_E_ARG, _general returns without
// dropping it.  Kept as it is; the three entries have always differed in this.
extern "C" int ovp_slam_delayed_init(ovp_ctx* c, const ovp_update_opts* o, const ovp_feature_batch* b, uint8_t* ok_host,
                                     double* chi2_host, int* new_id, double* delta_init, double* dx_host, int dx_stride) {
  if (!b) {
    drop_kept_factor(c);
    return OVP_E_ARG;
  }
  return slam_delayed_init_impl(c, o, DinitCands{b->n_feats, b->max_meas, b->uv, b->clone_idx, nullptr, b->n_meas, b->p_FinG},
                                DinitOut{ok_host, chi2_host, new_id, delta_init, dx_host, dx_stride});
}

extern "C" int ovp_slam_delayed_init_planes(ovp_ctx* c, const ovp_update_opts* o, const ovp_general_batch* b, const ovp_dinit_planes* pl,
                                            uint8_t* status_host, double* chi2_host, int* new_id, double* delta_init, double* dx_host,
                                            int dx_stride) {
  if (!c || !o || !b || (b->cam_idx && c->gen_ncams < 1)) {
    drop_kept_factor(c);
    return OVP_E_ARG;
  }
  return slam_delayed_init_impl(c, o, DinitCands{b->n_feats, b->max_meas, b->uv, b->clone_idx, b->cam_idx, b->n_meas, b->p_FinG},
                                DinitOut{status_host, chi2_host, new_id, delta_init, dx_host, dx_stride}, true, pl);
}

extern "C" int ovp_slam_delayed_init_general(ovp_ctx* c, const ovp_update_opts* o, const ovp_general_batch* b, uint8_t* ok_host,
                                             double* chi2_host, int* new_id, double* delta_init, double* dx_host, int dx_stride) {
  if (!c || !o || !b || !b->cam_idx || c->gen_ncams < 1) return OVP_E_ARG;  // (every camera from the tables of ovp_cameras_upload)
  return slam_delayed_init_impl(c, o, DinitCands{b->n_feats, b->max_meas, b->uv, b->clone_idx, b->cam_idx, b->n_meas, b->p_FinG},
                                DinitOut{ok_host, chi2_host, new_id, delta_init, dx_host, dx_stride});
}
