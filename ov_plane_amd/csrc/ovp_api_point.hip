// C-ABI shim, part 2 (see ovp_ctx.h): the point update - UpdaterMSCKF::update downstream of the plane loop
// (update/UpdaterMSCKF.cpp:671-814, state/StateHelper.cpp:121-202) and StateHelper::EKFUpdate with a dense host H.
#include "ovp_ctx.h"
#include "ovp_point_plan.h"

// Results go to the host without a copy command: the last kernel of an update writes the result block into the pinned mirror
// (c->h_res_block, a Mailbox) and then the sequence number of its channel 0; ovp_msckf_fetch_results waits on that channel.

// ---- the update step ---------------------------------------------------------------------------
// States above the tile factorization's limit (N > 288: e.g. 30 clones plus 50 landmarks).  A measurement batch never
// touches all of such a state: A = H^T H is non-zero on ns <= 288 involved columns s only.  With G = P[:, s]:
//     P+ = P - G (A - A Pss+ A) G^T ,   Pss+ = (Pss^-1 + A)^-1   (from (I + P A)^-1 = I - P+ A restricted to s),
// so the factorizations run on the ns x ns problem through the same tile kernels and the rest is three MFMA products.
static bool substate_ok(const ovp_ctx* c) { return c->n > OVP_TILECHOL_NMAX && c->sub_ns > 0 && c->sub_ns <= OVP_TILECHOL_NMAX; }

int set_substate(ovp_ctx* c, const std::vector<int>& ids) {
  c->sub_ns = 0;
  if (c->n <= OVP_TILECHOL_NMAX || ids.empty() || (int)ids.size() > OVP_TILECHOL_NMAX) return 0;
  HIPCHK(c->sub_ids.alloc(OVP_TILECHOL_NMAX + 16));
  HIPCHK(c->sub_buf.alloc((size_t)6 * OVP_TILECHOL_NMAX * OVP_TILECHOL_NMAX));
  HIPCHK(hipMemcpyAsync(c->sub_ids, ids.data(), sizeof(int) * ids.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));  // ids is the caller's temporary
  c->sub_ns = (int)ids.size();
  return 0;
}

// k_chol2 in mode 0: the dense lower-triangular factor of A (n x n, leading dimension ld for both) into Ldense
static ovp::Chol2Job dense_chol2_job(const double* A, int n, int ld, int* flag, double* Ldense) {
  ovp::Chol2Job j;
  memset(&j, 0, sizeof(j));
  j.A = A;
  j.n = n;
  j.ld = ld;
  j.mode = 0;
  j.flag = flag;
  j.Ldense = Ldense;
  j.ldo = ld;
  return j;
}

// Positive SEMI-definite A (state/StateHelper.cpp:159-187 never factors P, so the reference updates such a covariance - right after
// StateHelper::clone the newest pose is an exact copy, :346-396).  ANY factor with L0 L0^T = A serves the identities the updates
// stand on (P_k = L0 (I + L0^T A_k L0)^-1 L0^T is the matrix inversion lemma, no inverse of P in it): the pivot-dropping Cholesky
// of the unit-diagonal form, L0 = D Lc with zero columns where A determines nothing.  unit: n x n scratch, dvec: n doubles.
static int pivot_dropping_factor(ovp_ctx* c, const double* A, int n, int ld, double* unit, double* dvec, double* Lout, hipStream_t s) {
  HIPCHK(ovp_launch_unit_diag(A, n, ld, unit, dvec, s));
  ovp::Chol2Job j = dense_chol2_job(unit, n, ld, c->flags, Lout);
  j.piv_floor = 1e-12;  // regular pivots of the unit-diagonal form are >= 1 / cond (1e-8 at worst), dropped ones rounding noise
  HIPCHK(ovp_launch_chol2(&j, nullptr, nullptr, s));
  HIPCHK(ovp_launch_scale_rows(Lout, n, ld, dvec, s));
  return 0;
}

int chol_of_P(ovp_ctx* c, hipStream_t s, bool psd) {
  const int n = c->n, ld = c->ld;
  if (psd && n <= ovp_chol2_max_n() + 1)  // (plane loop, second attempt)
    return pivot_dropping_factor(c, c->P, n, ld, c->W1, c->pl_crow, c->L, s);
  if (n <= ovp_chol2_max_n() + 1) {  // dense factor from the second-generation kernel
    const ovp::Chol2Job j = dense_chol2_job(c->P, n, ld, c->flags, c->L);
    return (int)ovp_launch_chol2(&j, nullptr, nullptr, s);
  }
  if (n <= OVP_TILECHOL_NMAX) return (int)ovp_launch_tilechol(c->P, c->L, nullptr, nullptr, n, ld, c->flags, 0, s);
  if (substate_ok(c)) return 0;  // the sub-state update factors Pss, not P
  return (int)ovp_launch_chol(c->P, c->L, n, ld, c->flags, 0, s);
}

// chol(T) behind an update: tile-packed factor + inverted diagonal blocks for k_fwdsub.  The second-generation kernel (k_chol2:
// fused elimination, role hand-over through LDS counters instead of workgroup barriers) took over from k_tilechol in round 3
// (the first generation serves the sizes above k_chol2's register budget).
hipError_t chol_of_T(ovp_ctx* c, const double* T, int n, int ld, int add_identity, const int* cond, hipStream_t s) {
  if (n > ovp_chol2_max_n() + 1)
    return ovp_launch_tilechol_unless(T, nullptr, c->Dinv, c->Ltp, n, ld, c->flags, add_identity, cond, s);
  return ovp_launch_chol2_packed(T, c->Dinv, c->Ltp, n, ld, c->flags, add_identity, cond, s);
}

static int ekf_substate(ovp_ctx* c, bool psd = false) {
  const int n = c->n, ld = c->ld, ns = c->sub_ns, lds = OVP_TILECHOL_NMAX;
  const size_t sz = (size_t)OVP_TILECHOL_NMAX * OVP_TILECHOL_NMAX;
  double *S_P = c->sub_buf, *S_A = S_P + sz, *S_L = S_A + sz, *S_W = S_L + sz, *S_T = S_W + sz, *S_Y = S_T + sz;
  hipStream_t s = c->stream;
  HIPCHK(ovp_launch_gather_block(c->P, ld, c->sub_ids, ns, S_P, lds, s));
  HIPCHK(ovp_launch_gather_block(c->Ab, ld, c->sub_ids, ns, S_A, lds, s));
  // Pss+ = Ls (I + Ls^T A Ls)^-1 Ls^T exactly as the full-state path does it
  if (psd) {
    // second attempt behind a failed chol(Pss): positive SEMI-definite prior (an exact stochastic clone) - any factor with
    // Ls Ls^T = Pss serves the identity above
    const int rp = pivot_dropping_factor(c, S_P, ns, lds, S_W, c->dx, S_L, s);
    if (rp) return rp;
  } else {
    HIPCHK(ovp_launch_tilechol(S_P, S_L, nullptr, nullptr, ns, lds, c->flags, 0, s));
  }
  HIPCHK(ovp_launch_gemm4(0, 0, ns, ns, ns, S_A, lds, S_L, lds, S_W, lds, 0, 0, s));
  HIPCHK(ovp_launch_gemm4(1, 0, ns, ns, ns, S_L, lds, S_W, lds, S_T, lds, 1, 1, s));
  HIPCHK(ovp_launch_tilechol(S_T, nullptr, c->Dinv, c->Ltp, ns, lds, c->flags, 0, s));
  HIPCHK(ovp_launch_fwdsub(c->Ltp, c->Dinv, S_L, S_Y, ns, lds, 0, s));
  HIPCHK(ovp_launch_gemm4(1, 0, ns, ns, ns, S_Y, lds, S_Y, lds, S_P, lds, 0, 1, s));
  // Lambda = A - A Pss+ A
  HIPCHK(ovp_launch_gemm4(0, 0, ns, ns, ns, S_A, lds, S_P, lds, S_W, lds, 0, 0, s));
  HIPCHK(ovp_launch_gemm4(0, 0, ns, ns, ns, S_W, lds, S_A, lds, S_T, lds, 0, 1, s));
  HIPCHK(ovp_launch_mat_sub(S_A, S_T, S_T, ns, ns, lds, s));
  // P -= G Lambda G^T   (G in Y, G Lambda in W1, the product in T)
  HIPCHK(ovp_launch_gather_cols(c->P, ld, c->sub_ids, n, ns, c->Y, ld, s));
  HIPCHK(ovp_launch_gemm4(0, 0, n, ns, ns, c->Y, ld, S_T, lds, c->W1, ld, 0, 0, s));
  HIPCHK(ovp_launch_gemm4(0, 1, n, n, ns, c->W1, ld, c->Y, ld, c->T, ld, 0, 1, s));
  HIPCHK(ovp_launch_sub_sym_unless(c->P, c->T, n, ld, c->flags, s));  // (a failed factorization leaves the resident covariance alone)
  return 0;
}

// The update's last kernel: dx = P+ b, the boost amounts off the diagonal, the negative-diagonal check.  publish: its last block
// also writes [flags | dx] into the pinned host block and posts channel 0 (no separate launch, no copy command).
static int point_publish_dx(ovp_ctx* c, const double* boost, int boost_n, const int* cancel, bool publish) {
  const int n = c->n;
  const double* b = c->Ab + (size_t)n * c->ld;
  if (!publish)
    return (int)ovp_launch_dx_rows_boost(c->P, n, c->ld, b, c->dx, c->flags + 1, nullptr, nullptr, nullptr, 0, nullptr, 0u, boost, boost_n,
                                         cancel, c->stream);
  const int words = (int)((16 + sizeof(double) * (size_t)n + 7) / 8);
  SeqChannel& ch = c->h_res_block.channel(0);
  const unsigned seq = ch.arm();
  HIPCHK(ovp_launch_dx_rows_boost(c->P, n, c->ld, b, c->dx, c->flags + 1, c->ticket, c->res_block, c->h_res_block.dev(c->h_flags), words,
                                  ch.word_dev(), seq, boost, boost_n, cancel, c->stream));
  c->point.pub_armed = true;
  return 0;
}

// The second half of an information-form update: the pair [A | b] is in c->Ab and the factor t names is on its way on c->stream.
// Its form follows the state's size and the sub-state set_substate left in the context, for every caller alike; a PointPlan's
// `tail` / `sub_ns` say beforehand what that will be (set_substate on the plan's column list) and are there for the read-back.
static int point_enqueue_tail(ovp_ctx* c, const PointTail& t, bool publish) {
  const int n = c->n, ld = c->ld;
  c->kept = KeptFactor();  // P is about to change
  if (n <= OVP_TILECHOL_NMAX) {
    // W1 = A L ;  T = I + L^T W1 ;  Lt = chol(T) (+ inverses of its diagonal blocks).  L: chol(P), or the dense factor the plane
    // loop left (any M with M M^T = P gives P+ = M (I + M^T A M)^-1 M^T); with the reversed-order factor T is the identity outside
    // its leading nl columns
    const double* Lf = t.factor ? t.factor : (const double*)c->L;
    const int nl = t.nl > 0 ? t.nl : n;
    HIPCHK(ovp_launch_gemm4(0, 0, n, nl, n, c->Ab, ld, Lf, ld, c->W1, ld, 0, 0, c->stream));
    HIPCHK(ovp_launch_gemm4(1, 0, nl, nl, n, Lf, ld, c->W1, ld, c->T, ld, 1, 1, c->stream));
    HIPCHK(chol_of_T(c, c->T, nl, ld, 0, nullptr, c->stream));
    // V = Lt^-1 L^T ;  P+ = V^T V ;  dx = P+ b
    HIPCHK(ovp_launch_fwdsub_lead(c->Ltp, c->Dinv, Lf, c->Y, n, ld, t.dense, nl, c->stream));
    // (skipped on the device when a factorization failed: the resident covariance then stays what it was, OVP_E_NOTSPD)
    HIPCHK(ovp_launch_gemm4c(1, 0, n, n, n, c->Y, ld, c->Y, ld, c->P, ld, 0, 1, c->flags, c->stream));
    return point_publish_dx(c, t.boost, t.boost_n, c->flags, publish);
  }
  if (substate_ok(c)) {
    int rc = ekf_substate(c);
    if (rc) return rc;
    return point_publish_dx(c, nullptr, 0, nullptr, publish);
  }
  // large-state fallback when the measurements touch more than 288 columns: global-memory factorization
  HIPCHK(ovp_launch_gemm(0, 0, n, n, n, c->Ab, ld, c->L, ld, c->W1, ld, 0, c->stream));
  HIPCHK(ovp_launch_gemm(1, 0, n, n, n, c->L, ld, c->W1, ld, c->T, ld, 1, c->stream));
  HIPCHK(ovp_launch_chol(c->T, c->Lt, n, ld, c->flags, 0, c->stream));
  HIPCHK(ovp_launch_trsm_right_lt(c->L, c->Lt, c->Y, n, ld, c->stream));
  HIPCHK(ovp_launch_cov_finish(c->Y, n, ld, c->Ab + (size_t)n * ld, c->P, ld, c->dx, c->flags + 1, c->stream));
  return 0;
}

// for the entries that bring a pair of their own (ovp_ekf_update's information form, ovp_slam_update): chol(P) on the main stream
int ekf_from_gram(ovp_ctx* c, const PointTail& t) {
  const int rc = chol_of_P(c, c->stream);
  return rc ? rc : point_enqueue_tail(c, t, false);
}

// Update of a covariance that is positive SEMI-definite (an exact stochastic clone before the next propagation, a zero-variance
// prior): P has no Cholesky factor, but the reference's own form needs none (state/StateHelper.cpp:159-187):
//   P+ = P - P H^T (H P H^T + I)^-1 H P,   with H := La^T, La La^T = A the (pivot-dropping) Cholesky factor of the information
// matrix of the batch - H^T H = A and H^T r = b is all the update depends on.  S = I + La^T P La is positive definite whatever P is.
// Runs after a failed chol(P) (flags[0]): the pair [A | b] is still in c->Ab, P was not touched (ovp_launch_gemm4c cancel flag).
// the retry's ending: dx = P+ b, correction and flags to the host, the flag words cleared for the next update
static int sform_finish(ovp_ctx* c) {
  hipStream_t s = c->stream;
  const int rc = point_publish_dx(c, nullptr, 0, nullptr, false);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(c->h_dx, c->dx, sizeof(double) * c->n, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(c->h_flags, c->flags, sizeof(int) * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  HIPCHK(hipMemsetAsync(c->flags, 0, sizeof(int) * 4, s));
  return 0;
}

int ekf_sform(ovp_ctx* c) {
  const int n = c->n, ld = c->ld;
  hipStream_t s = c->stream;
  if (n > OVP_TILECHOL_NMAX || n > ovp_chol2_max_n()) {
    // above the tile factorization: the sub-state update once more, on the pivot-dropping factor of the involved block
    if (!substate_ok(c) || c->sub_ns > ovp_chol2_max_n()) return OVP_E_NOTSPD;
    HIPCHK(hipMemsetAsync(c->flags, 0, sizeof(int) * 4, s));
    const int rs = ekf_substate(c, true);
    return rs ? rs : sform_finish(c);
  }
  HIPCHK(hipMemsetAsync(c->flags, 0, sizeof(int) * 4, s));
  HIPCHK(hipMemsetAsync(c->W1, 0, sizeof(double) * (size_t)n * ld, s));
  HIPCHK(ovp_launch_max_diag(c->Ab, n, ld, c->smallbuf, s));
  ovp::Chol2Job j = dense_chol2_job(c->Ab, n, ld, c->flags + 3, c->W1);  // La (lower triangular, zero columns where a pivot was dropped)
  j.piv_floor = 1e-13;  // directions that carry less than 1e-13 of the largest diagonal entry count as unobserved
  j.floor_scale = c->smallbuf;
  HIPCHK(ovp_launch_chol2(&j, nullptr, nullptr, s));
  HIPCHK(ovp_launch_gemm4(0, 0, n, n, n, c->P, ld, c->W1, ld, c->Y, ld, 0, 0, s));   // Wm = P La
  HIPCHK(ovp_launch_gemm4(1, 0, n, n, n, c->W1, ld, c->Y, ld, c->T, ld, 1, 1, s));   // S = I + La^T Wm
  HIPCHK(ovp_launch_tilechol(c->T, nullptr, c->Dinv, c->Ltp, n, ld, c->flags, 0, s));
  HIPCHK(ovp_launch_fwdsub(c->Ltp, c->Dinv, c->Y, c->L, n, ld, 1, s));               // V = Ls^-1 Wm^T
  HIPCHK(ovp_launch_gemm4(1, 0, n, n, n, c->L, ld, c->L, ld, c->T, ld, 0, 1, s));    // V^T V
  HIPCHK(ovp_launch_sub_sym(c->P, c->T, n, ld, s));
  return sform_finish(c);
}

int fill_feat_params(ovp_ctx* c, const ovp_update_opts* o) {
  const int n = c->n, F = c->n_feats;
  ovp::FeatParams& fp = c->fp;
  fp.n_feats = F;
  fp.max_meas = c->max_meas;
  fp.do_fej = o->do_fej;
  const CalCols cc(c, o);
  if (cc.check(n, false)) return OVP_E_ARG;
  cc.fill(fp);
  fp.white_px = 1.0 / o->sigma_px;
  fp.chi2_mult = o->chi2_multiplier;
  fp.chi2_table = c->chi2_table;
  fp.P = c->P;
  fp.n = n;
  fp.ldp = c->ld;
  fp.G = c->G;
  fp.Bscr = c->Bscr;
  fp.ldg = c->ldg;
  fp.rec = c->rec;
  // per-feature results straight into the pinned host block (same layout as res_block): they cross PCIe while K1 runs
  fp.chi2 = (double*)c->h_res_block.dev(c->h_chi2);
  fp.accept = (unsigned char*)c->h_res_block.dev(c->h_accept);
  fp.dbg_cycles = c->dbg_cycles;
  fp.slot = nullptr;
  fp.n_out = 0;
  fp.skip = nullptr;
  fp.range_lo = c->range_lo < 0 ? 0 : c->range_lo;
  fp.range_hi = c->range_lo < 0 ? 0x7fffffff : c->range_hi;
  if (o->skip_plane_used) {
    if (!c->pl_used_valid || !c->pl_used) return OVP_E_STATE;  // no plane update ran on this batch
    fp.skip = c->pl_used;
  }
  return 0;
}

// ---- the first half: plan (ovp_point_plan.h), then enqueue by stages ---------------------------------------------------------------
// the three switches of the point update; read per call: the tests flip them inside one process
static PointSwitches point_switches() {
  PointSwitches sw;
  const char* overlap_env = getenv("OVP_OVERLAP_MODE");
  sw.overlap = overlap_env ? atoi(overlap_env) : 0;
  sw.no_flip = getenv("OVP_POINT_NO_FLIP") != nullptr;
  sw.no_boost = getenv("OVP_POINT_NO_BOOST") != nullptr;
  return sw;
}

// what the planner reads: the context, and the options as fill_feat_params left them in c->fp
static PointEnv point_env(ovp_ctx* c) {
  PointEnv e;
  e.n = c->n, e.F = c->n_feats, e.max_meas = c->max_meas;
  e.clone_id = c->h_clone_id.data(), e.n_clones = (int)c->h_clone_id.size();
  e.calmask = c->fp.calmask, e.calib_id = c->calib_id, e.intr_id = c->intr_id;
  e.dense_cols = c->dense_cols.data(), e.n_dense = (int)c->dense_cols.size();
  e.range_lo = c->range_lo, e.range_hi = c->range_hi;
  e.used = c->h_pl_used.data();
  e.used_valid = c->fp.skip != nullptr && c->pl_used_valid && (int)c->h_pl_used.size() == e.F;
  e.have_factor = c->kept.have && c->Lkeep, e.factor_boosted = c->kept.boost;
  e.rows_per_chunk = c->rows_per_chunk, e.n_split = c->n_split;
  e.tilechol_nmax = OVP_TILECHOL_NMAX, e.chol2_max_n = ovp_chol2_max_n();
  e.fused_max_tiles = OVP_TC_MAX_TILES, e.fused_max_meas = OVP_FEAT_CHOL_MAX_MEAS;  // (what ovp_feat_chol_supported compares against)
  e.side_capacity = ovp_feat_chol_side_capacity();
  e.sw = point_switches();
  return e;
}

static PointTail point_tail(ovp_ctx* c, const PointPlan& p) {
  PointTail t;
  if (p.chol_p == CHOLP_NONE) t.factor = c->Lkeep;
  t.nl = p.nl, t.dense = p.dense;
  t.boost = p.boost == BOOST_CHOL ? (const double*)c->boost : p.boost == BOOST_LOOP ? (const double*)c->boost_vec : nullptr;
  t.boost_n = p.boost_n;
  return t;
}

// From the fork on the side stream may hold work of the update; its regular join is the second half's (or, with K2 over there, the
// end of the first).  A failing exit in between makes the main stream wait here, before anything else is enqueued on it.
struct SideJoin {
  ovp_ctx* c;
  bool armed = false;
  ~SideJoin() {
    if (!armed) return;
    (void)hipEventRecord(c->ev_join, c->stream2);
    (void)hipStreamWaitEvent(c->stream, c->ev_join, 0);
  }
};

// order and boost of a chol(P) of this update (CholJob / Chol2Job share the fields)
template <class Job>
static void point_chol_order(ovp_ctx* c, const PointPlan& p, Job* j) {
  j->flip = p.flip ? 1 : 0;
  if (p.boost != BOOST_CHOL) return;
  j->boost = c->boost;
  j->boost_n = p.boost_n;
  j->boost_rel = 1e-9;
}

// chol(P) outside the feature launch forks the side stream at fork_ev: as k_chol2 over there, in front of K1 (ev_join behind it) - or
// on the main stream behind K1, and K2 goes over there (it is the shorter of the two branches: the join then never stalls the main
// stream, and the cross-queue wake-up latency sits at the START of the side branch, off the critical path)
static int point_enqueue_chol_p(ovp_ctx* c, const PointPlan& p, hipEvent_t fork_ev, SideJoin* side) {
  HIPCHK(hipEventRecord(fork_ev, c->stream));
  side->armed = true;
  HIPCHK(hipStreamWaitEvent(c->stream2, fork_ev, 0));
  if (p.chol_p == CHOLP_BEHIND_K1) return chol_of_P(c, c->stream);
  ovp::Chol2Job j = dense_chol2_job(c->P, c->n, c->ld, c->flags, c->L);
  point_chol_order(c, p, &j);
  HIPCHK(ovp_launch_chol2(&j, nullptr, nullptr, c->stream2));
  HIPCHK(hipEventRecord(c->ev_join, c->stream2));
  return 0;
}

// K1: gate and rows of every feature.  The fused shape carries chol(P) in workgroup 0 (cj.n > 0) or leaves that workgroup idle.
static int point_enqueue_k1(ovp_ctx* c, const PointPlan& p) {
  if (p.k1 == K1_ONE_WAVE) return (int)ovp_launch_feat_gate(&c->fp, c->stream);
  ovp::CholJob cj{c->P, c->L, nullptr, nullptr, p.k1 == K1_FUSED_CHOL ? c->n : 0, c->ld, c->flags, 0, nullptr, 0, 0.0};
  point_chol_order(c, p, &cj);
  return (int)ovp_launch_feat_chol(&c->fp, &cj, c->stream);
}

// K2 on the Fa features that own rows of rec / G (or a clear of the pair), then the pending dense pair
static int point_enqueue_pair(ovp_ctx* c, const PointPlan& p, hipStream_t s) {
  const int n = c->n;
  if (!p.clear_Ab) {
    int nsplit = p.nsplit;
    HIPCHK(ovp_launch_gram_pair(c->rec, c->fp.n_clones, p.Fa, c->rows_per_chunk, p.used_chunks, c->gramS, c->G, 3 * p.Fa, c->ldg, n + 1,
                                c->n_split, c->part, &nsplit, s));
    HIPCHK(ovp_launch_reduce_gram(c->gramS, c->fp.n_clones, p.used_chunks, c->gramR, s));
    HIPCHK(ovp_launch_assemble(c->gramR, c->fp.n_clones, 1, c->part, nsplit, c->colmap, n, c->Ab, c->ld, s));
  } else {
    HIPCHK(hipMemsetAsync(c->Ab, 0, sizeof(double) * (size_t)(n + 1) * c->ld, s));
  }
  if (p.add_pair) {
    // the pair of the dense blocks accepted by ovp_msckf_dense_blocks joins the batch's (same update, update/UpdaterMSCKF.cpp:767-814)
    const int m = (int)c->dense_cols.size();
    HIPCHK(c->Acc.alloc((size_t)c->n_max * c->n_max));
    HIPCHK(c->bcc.alloc((size_t)c->n_max));
    HIPCHK(hipMemcpyAsync(c->Acc, c->dense_A.data(), sizeof(double) * (size_t)m * m, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->bcc, c->dense_b.data(), sizeof(double) * m, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->idbuf, c->dense_cols.data(), sizeof(int) * m, hipMemcpyHostToDevice, s));
    HIPCHK(ovp_launch_scatter_gram_add(c->Acc, c->bcc, m, c->idbuf, c->Ab, c->ld, n, s));
    HIPCHK(hipStreamSynchronize(s));  // (the host vectors are pageable and about to be cleared; slow path)
    c->dense_cols.clear();
  }
  return 0;
}

static int point_enqueue_build(ovp_ctx* c, const PointPlan& p) {
  SideJoin side{c};
  if (c->n > OVP_TILECHOL_NMAX) {
    const int rs = set_substate(c, p.sub_ids);
    if (rs) return rs;
  }
  if (p.boost == BOOST_CHOL) HIPCHK(c->boost.alloc(64));
  // Events on the main stream are kept to a minimum (each one costs microseconds between dependent kernels): with the kernel timer
  // on, ev_k0 / ev_k1 bracket K1 and ev_k1 doubles as the fork point behind it; otherwise one untimed fork event.
  if (c->ktimer) HIPCHK(hipEventRecord(c->ev_k0, c->stream));
  int rc = p.chol_p == CHOLP_SIDE ? point_enqueue_chol_p(c, p, c->ev_fork, &side) : 0;
  if (!rc) rc = point_enqueue_k1(c, p);
  if (rc) return rc;
  if (c->ktimer) c->point.k1_timed = true;
  const bool k2_aside = p.chol_p == CHOLP_BEHIND_K1;
  if (k2_aside) rc = point_enqueue_chol_p(c, p, c->ktimer ? c->ev_k1 : c->ev_fork, &side);
  else if (c->ktimer) HIPCHK(hipEventRecord(c->ev_k1, c->stream));
  if (!rc) rc = point_enqueue_pair(c, p, k2_aside ? c->stream2 : c->stream);
  if (rc) return rc;
  if (k2_aside) {
    // the Gram pair must be complete on the main stream when this call returns (the caller may all-reduce it there)
    HIPCHK(hipEventRecord(c->ev_join, c->stream2));
    HIPCHK(hipStreamWaitEvent(c->stream, c->ev_join, 0));
  }
  side.armed = false;
  c->point.tail = point_tail(c, p);
  c->point.join_owed = p.join;
  return 0;
}

extern "C" int ovp_msckf_build_gate_gram_async(ovp_ctx* c, const ovp_update_opts* o) {
  if (!c || !o) return OVP_E_ARG;
  if (!c->have_state || !c->have_cov || !c->have_batch) return OVP_E_STATE;
  if (c->fp.n_clones < 1) return OVP_E_STATE;
  {
    int rc = fill_feat_params(c, o);
    if (rc) return rc;
  }
  c->point.tail = PointTail();  // (pub_armed and k1_timed are the fetch's to clear)
  c->point.join_owed = false;
  PointPlan p;
  plan_point_update(point_env(c), c->h_slot.get(), &p);
  const int route[8] = {p.k1, p.chol_p, p.tail, p.flip ? 1 : 0, p.nl, p.boost_n, p.Fa, p.sub_ns};
  memcpy(c->point_route, route, sizeof(route));
  if (p.slots) {  // K1 reads a feature's slot from host-mapped memory at the start of its wave
    c->fp.slot = c->h_slot.dev();
    c->fp.n_out = p.Fa;
  }
  // (the flag words were cleared by the previous ovp_msckf_fetch_results, or at creation)
  return point_enqueue_build(c, p);
}

// Dense blocks beside the batch (see ovplane_hip.h): gates on the host against the marginal of the involved columns, pair kept for
// the point update that follows.
extern "C" int ovp_msckf_dense_blocks(ovp_ctx* c, double chi2_multiplier, int n_blocks, const int* rows, const int* cols, const double* H,
                                      const int* col_ids, const double* res, uint8_t* accepted, double* chi2) {
  if (!c || n_blocks < 0 || (n_blocks > 0 && (!rows || !cols || !H || !col_ids || !res))) return OVP_E_ARG;
  if (!c->have_cov) return OVP_E_STATE;
  c->dense_cols.clear();
  if (n_blocks == 0) return 0;
  // union of the columns, in ascending order
  std::vector<int> uni;
  {
    size_t oc = 0;
    for (int k = 0; k < n_blocks; ++k) {
      if (rows[k] < 1 || cols[k] < 1) return OVP_E_ARG;
      for (int j = 0; j < cols[k]; ++j) {
        const int id = col_ids[oc + j];
        if (id < 0 || id >= c->n) return OVP_E_ARG;
        uni.push_back(id);
      }
      oc += cols[k];
    }
    std::sort(uni.begin(), uni.end());
    uni.erase(std::unique(uni.begin(), uni.end()), uni.end());
  }
  const int m = (int)uni.size();
  std::vector<int> ones((size_t)m, 1), pos((size_t)c->n, -1);
  for (int i = 0; i < m; ++i) pos[uni[i]] = i;
  std::vector<double> Pm((size_t)m * m);
  {
    const int rm = ovp_cov_marginal(c, uni.data(), ones.data(), m, Pm.data());
    if (rm) return rm;
  }
  std::vector<double> A((size_t)m * m, 0.0), b((size_t)m, 0.0);
  size_t oH = 0, oc = 0, orr = 0;
  int n_acc = 0;
  for (int k = 0; k < n_blocks; ++k) {
    const int r = rows[k], q = cols[k];
    const double* Hk = H + oH;        // column-major r x q
    const int* idk = col_ids + oc;
    const double* rk = res + orr;
    oH += (size_t)r * q;
    oc += q;
    orr += r;
    // S = H Pm H^T + I (lower triangle), chi2 = |L^-1 r|^2
    std::vector<double> HP((size_t)r * q, 0.0), S((size_t)r * r, 0.0), y((size_t)r);
    for (int j = 0; j < q; ++j)
      for (int l = 0; l < q; ++l) {
        const double p = Pm[(size_t)pos[idk[l]] * m + pos[idk[j]]];
        if (p == 0.0) continue;
        for (int i = 0; i < r; ++i) HP[(size_t)j * r + i] += Hk[(size_t)l * r + i] * p;
      }
    for (int a = 0; a < r; ++a)
      for (int i = a; i < r; ++i) {
        double v = (i == a) ? 1.0 : 0.0;
        for (int j = 0; j < q; ++j) v += HP[(size_t)j * r + i] * Hk[(size_t)j * r + a];
        S[(size_t)a * r + i] = v;
      }
    double x2 = 0.0;
    bool spd = true;
    for (int j = 0; j < r && spd; ++j) {
      double d = S[(size_t)j * r + j];
      for (int l = 0; l < j; ++l) d -= S[(size_t)l * r + j] * S[(size_t)l * r + j];
      if (!(d > 0.0)) {
        spd = false;
        break;
      }
      d = sqrt(d);
      S[(size_t)j * r + j] = d;
      double rj = rk[j];
      for (int l = 0; l < j; ++l) rj -= S[(size_t)l * r + j] * y[l];
      y[j] = rj / d;
      x2 += y[j] * y[j];
      for (int i = j + 1; i < r; ++i) {
        double v = S[(size_t)j * r + i];
        for (int l = 0; l < j; ++l) v -= S[(size_t)l * r + i] * S[(size_t)l * r + j];
        S[(size_t)j * r + i] = v / d;
      }
    }
    if (!spd) x2 = INFINITY;
    const bool ok = x2 <= chi2_multiplier * ovp_chi2_quantile_095(r);
    if (accepted) accepted[k] = ok ? 1 : 0;
    if (chi2) chi2[k] = x2;
    if (!ok) continue;
    ++n_acc;
    for (int j = 0; j < q; ++j) {
      const int pj = pos[idk[j]];
      double bj = 0.0;
      for (int i = 0; i < r; ++i) bj += Hk[(size_t)j * r + i] * rk[i];
      b[pj] += bj;
      for (int l = 0; l < q; ++l) {
        double v = 0.0;
        for (int i = 0; i < r; ++i) v += Hk[(size_t)j * r + i] * Hk[(size_t)l * r + i];
        A[(size_t)pos[idk[l]] * m + pj] += v;
      }
    }
  }
  if (n_acc > 0) {
    c->dense_cols = uni;
    c->dense_A = A;
    c->dense_b = b;
  }
  return 0;
}

extern "C" int ovp_gram_buffer(ovp_ctx* c, double** Ab_dev, int* n_rows, int* ld) {
  if (!c || !Ab_dev) return OVP_E_ARG;
  *Ab_dev = c->Ab;
  if (n_rows) *n_rows = c->n + 1;
  if (ld) *ld = c->ld;
  return 0;
}

extern "C" int ovp_ekf_update_from_gram_async(ovp_ctx* c) {
  if (!c) return OVP_E_ARG;
  if (!c->have_cov) return OVP_E_STATE;
  const PointPending pend = c->point;  // (consumed here: a second call without a build runs the plain tail)
  c->point.tail = PointTail();
  c->point.join_owed = false;
  if (pend.join_owed) HIPCHK(hipStreamWaitEvent(c->stream, c->ev_join, 0));
  int rc = point_enqueue_tail(c, pend.tail, true);
  if (rc) return rc;
  if (c->ktimer) {
    HIPCHK(hipEventRecord(c->ev_t[3], c->stream));
    c->timed = true;
  }
  return 0;
}

extern "C" int ovp_msckf_fetch_results(ovp_ctx* c, double* dx_host, uint8_t* accepted_host, double* chi2_host,
                                       ovp_update_info* info) {
  if (!c) return OVP_E_ARG;
  const int n = c->n, F = c->n_feats;
  {
    // [flags | dx] are published by the last block of the dx kernel (or, on the fallback path, by a publish kernel);
    // chi2 / accept were written into the pinned block by K1 itself
    SeqChannel& ch = c->h_res_block.channel(0);
    if (!c->point.pub_armed) {
      const size_t words = (16 + sizeof(double) * (size_t)n + 7) / 8;
      const unsigned seq = ch.arm();
      // (also clears the four flag words of the device block for the next update)
      HIPCHK(ovp_launch_publish_block(c->res_block, c->h_res_block.dev(c->h_flags), 8 * words, ch.word_dev(), seq, 2, c->stream));
    }
    c->point.pub_armed = false;
    const int rw = ch.wait(c->stream);
    if (rw) return rw;
  }
  if (c->h_flags[0]) {
    // chol(P) failed: the prior is only positive semi-definite.  Same update in the reference's S-form (no factor of P needed).
    int rs = ekf_sform(c);
    if (rs) return rs;
  }
  if (dx_host) memcpy(dx_host, c->h_dx, sizeof(double) * n);
  if (accepted_host && F) memcpy(accepted_host, c->h_accept, (size_t)F);
  if (chi2_host && F) memcpy(chi2_host, c->h_chi2, sizeof(double) * F);
  if (c->timed) {
    hipEventSynchronize(c->ev_t[3]);  // recorded behind the publishing kernel: may trail the sequence word by a moment
    // stage times while the kernel timer is on: [0] K1, [1] unused (K2 runs beside chol(P)), [2] chol(P) || K2 and the EKF
    // update, [3] total from the start of K1
    hipEventElapsedTime(&c->last_ms[0], c->ev_k0, c->ev_k1);
    c->last_ms[1] = 0.f;
    hipEventElapsedTime(&c->last_ms[2], c->ev_k1, c->ev_t[3]);
    hipEventElapsedTime(&c->last_ms[3], c->ev_k0, c->ev_t[3]);
    c->timed = false;
  }
  if (c->point.k1_timed) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, c->ev_k0, c->ev_k1) == hipSuccess) {
      c->ktime_ms += ms;
      c->klaunches += 1;
    }
    c->point.k1_timed = false;
  }
  if (info) {
    memset(info, 0, sizeof(*info));
    // n_meas may live in caller-owned device memory (bind_device): read it back once per batch for the row count
    if (F && !c->h_nmeas_valid) {
      c->h_nmeas.resize(F);
      HIPCHK(hipMemcpy(c->h_nmeas.data(), c->fp.n_meas, sizeof(int) * F, hipMemcpyDeviceToHost));
      c->h_nmeas_valid = true;
    }
    for (int f = 0; f < F; ++f)
      if (c->h_accept[f]) {
        info->n_accepted++;
        info->n_rows += 2 * c->h_nmeas[f] - 3;
      }
    info->n_cols = 0;
    info->not_spd = c->h_flags[0];
    info->neg_diag = c->h_flags[1];
  }
  if (c->h_flags[0]) return OVP_E_NOTSPD;
  if (c->h_flags[1]) return OVP_E_NEGDIAG;
  return 0;
}

extern "C" int ovp_msckf_update(ovp_ctx* c, const ovp_update_opts* o, double* dx_host, uint8_t* accepted_host,
                                double* chi2_host, ovp_update_info* info) {
  const double t0 = host_now_ms();
  int rc = ovp_msckf_build_gate_gram_async(c, o);
  if (rc) return rc;
  rc = ovp_ekf_update_from_gram_async(c);
  if (rc) return rc;
  const double t1 = host_now_ms();
  rc = ovp_msckf_fetch_results(c, dx_host, accepted_host, chi2_host, info);
  c->host_acc[4] += t1 - t0;
  c->host_acc[5] += host_now_ms() - t1;
  c->host_acc[6] += 1.0;
  return rc;
}

// ---- StateHelper::EKFUpdate with a dense host H ------------------------------------------------
extern "C" int ovp_ekf_update(ovp_ctx* c, const double* H_host, int rows, int cols, int ld, const int* col_ids,
                              const double* res_host, double* dx_host, ovp_update_info* info) {
  drop_kept_factor(c);  // (writes the covariance: a kept factor no longer belongs to it)
  if (!c || !H_host || !col_ids || !res_host || rows < 1 || cols < 1 || ld < rows) return OVP_E_ARG;
  if (!c->have_cov) return OVP_E_STATE;
  if (cols > c->n) return OVP_E_ARG;
  const int n = c->n;
  for (int j = 0; j < cols; ++j)
    if (col_ids[j] < 0 || col_ids[j] >= n) return OVP_E_ARG;
  // few rows (a frame's landmark re-observations, a zero-velocity update): the reference's own S-form on the kernels of
  // csrc/k_init.hip - S = H P H^T + I in LDS, P+ = P - W W^T - instead of two N x N factorizations
  if (!ekf_info_form_only() && ovp_init_fits(0, rows, cols) && cols <= c->n_max) {
    hipStream_t s = c->stream;
    const size_t oHt = 0, oRes = oHt + (size_t)cols * rows, oId = oRes + rows + 8;
    const size_t bytes = oId * sizeof(double) + sizeof(int) * (size_t)cols + 64;
    const size_t res_doubles = 4 + (size_t)c->n_max + 8;
    int rc = plane2_buffers(c, bytes, res_doubles * sizeof(double));
    if (rc) return rc;
    double* h = (double*)c->pl_stage.begin(bytes, &rc);
    if (!h) return rc;
    const double* d = (const double*)c->pl_stage.dev();
    for (int a = 0; a < cols; ++a) memcpy(h + oHt + (size_t)a * rows, H_host + (size_t)a * ld, sizeof(double) * rows);  // = H^T row-major
    memcpy(h + oRes, res_host, sizeof(double) * rows);
    memcpy(h + oId, col_ids, sizeof(int) * cols);
    const int* did = (const int*)(d + oId);
    double* dres = c->smallbuf;
    double* dM = dres + res_doubles;
    double* dLi = dM + (size_t)n * rows;
    double* dy = dLi + (size_t)rows * rows;
    if ((size_t)(dy + rows + 8 - c->smallbuf) > c->smallbuf.capacity()) return OVP_E_CAPACITY;
    HIPCHK(c->pl_stage.send(bytes, s, Fence::CallerWaits));
    HIPCHK(ovp_launch_init_m(c->P, c->ld, n, did, cols, d + oHt, rows, dM, s));
    HIPCHK(ovp_launch_init_core(c->P, c->ld, n, did, cols, d + oHt, 0, rows, dM, d + oRes /* unused: k = 0 */, d + oRes, d + oRes, 1.0,
                                1e300, dLi, dy, dres, s));
    HIPCHK(ovp_launch_init_update(c->P, c->P_tmp, c->ld, n, dM, rows, 0, rows, dLi, dy, dres, dres + 4, s));
    double* hres = (double*)c->pl_hres.payload();
    {
      const int rf = ovp_fetch_to_hres(c, dres, sizeof(double) * (4 + (size_t)n), s);
      if (rf) return rf;
      c->pl_stage.done();
    }
    if (info) {
      memset(info, 0, sizeof(*info));
      info->n_rows = rows;
      info->n_cols = cols;
      info->not_spd = hres[1] > 0.5 ? 0 : 1;
      info->neg_diag = hres[2] != 0.0;
    }
    if (!(hres[1] > 0.5)) return OVP_E_NOTSPD;  // S = H P H^T + I lost definiteness: P is not a covariance; nothing was written
    c->P.swap(c->P_tmp);
    if (dx_host) memcpy(dx_host, hres + 4, sizeof(double) * n);
    return hres[2] != 0.0 ? OVP_E_NEGDIAG : 0;
  }
  const size_t need = (size_t)ld * cols;
  HIPCHK(c->Hd.reserve(need, 0));
  HIPCHK(c->resd.reserve((size_t)rows, 64));
  HIPCHK(c->Acc.alloc((size_t)c->n_max * c->n_max));
  HIPCHK(c->bcc.alloc((size_t)c->n_max));
  HIPCHK(hipMemsetAsync(c->flags, 0, sizeof(int) * 4, c->stream));
  HIPCHK(hipMemcpyAsync(c->Hd, H_host, sizeof(double) * need, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->resd, res_host, sizeof(double) * rows, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->idbuf, col_ids, sizeof(int) * cols, hipMemcpyHostToDevice, c->stream));
  // column-major H [rows x cols, ld] == row-major H^T [cols x rows, ld]:  A = H^T H, b = H^T r
  HIPCHK(ovp_launch_gemm(0, 1, cols, cols, rows, c->Hd, ld, c->Hd, ld, c->Acc, cols, 0, c->stream));
  HIPCHK(ovp_launch_gemm(0, 0, cols, 1, rows, c->Hd, ld, c->resd, 1, c->bcc, 1, 0, c->stream));
  HIPCHK(hipMemsetAsync(c->Ab, 0, sizeof(double) * (size_t)(n + 1) * c->ld, c->stream));
  HIPCHK(ovp_launch_scatter_gram(c->Acc, c->bcc, cols, c->idbuf, c->Ab, c->ld, n, c->stream));
  {
    std::vector<int> ids(col_ids, col_ids + cols);
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    int rs = set_substate(c, ids);
    if (rs) return rs;
  }
  int rc = ekf_from_gram(c, PointTail());
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(c->h_dx, c->dx, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(c->h_flags, c->flags, sizeof(int) * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (c->h_flags[0]) {  // positive semi-definite prior: S-form instead of the factor of P
    int rs = ekf_sform(c);
    if (rs) return rs;
  }
  if (dx_host) memcpy(dx_host, c->h_dx, sizeof(double) * n);
  if (info) {
    memset(info, 0, sizeof(*info));
    info->n_rows = rows;
    info->n_cols = cols;
    info->not_spd = c->h_flags[0];
    info->neg_diag = c->h_flags[1];
  }
  if (c->h_flags[0]) return OVP_E_NOTSPD;
  if (c->h_flags[1]) return OVP_E_NEGDIAG;
  return 0;
}

