// C-ABI shim, part 4 (see ovp_ctx.h): the per-plane loop of UpdaterMSCKF::update (update/UpdaterMSCKF.cpp:411-649,
// update/UpdaterPlane.cpp:296-552) and UpdaterPlane::init_vio_plane.  ovp_msckf_plane_update_general: the same loop with the on-plane
// features of a general batch (any camera, tracks of up to OVP_GEN_MAX_MEAS views) stacked behind the batch's, as
// update/UpdaterHelper.cpp:335-344 and :448-512 stack them whatever camera saw them and however long the track is.
#include "ovp_ctx.h"
#include "k_plane_init2.h"

// the loop's per-plane results and the buffers of a plane's front end (the per-call tables travel in c->pl_stage, plane_stage_upload)
static int plane_buffers(ovp_ctx* c, int NP) {
  const size_t ld = (size_t)c->ld, np = (size_t)NP, n_max = (size_t)c->n_max;
  HIPCHK(c->pl_res.reserve(4 * np, 4 * 8));  // NP + 8 planes
  HIPCHK(c->pl_dx.reserve(n_max * np, n_max * 8));
  HIPCHK(c->pl_cst.alloc(((size_t)c->f_max + 1) * 10));  // (+ the record of a plane's general features)
  HIPCHK(c->pl_An.alloc((n_max + 1) * ld));
  HIPCHK(c->pl_bn.alloc(n_max));
  HIPCHK(c->pl_scal.alloc(8));
  return 0;
}

// ---- UpdaterMSCKF::update, per-plane loop: the host structures, the result kernels, the buffers; the loop itself
// (plane_loop) is further down, behind the column-order route into it ----
struct PlaneJobH { int pl, start, nf, rows_total, rows_live, rows_u, n_involved, in_state, sid, n_inv_cols, ns_pl; double thr;
                   int g_start, ng; /* general features: range in the list of the call */
                   int dof; /* what plane_dof reports: rows_u, initialisation: all rows_c (StateHelper::initialize's chi2) */ };

// The loop as the front of a plane initialisation (ovp_plane_init_general): every plane of the call is outside the state, its
// constraint rows carry const_init_multi, the gate is StateHelper::initialize's, and behind the last plane the accepted ones are
// appended to the resident covariance (k_plane_init2.hip).
struct PlaneInitView {
  double multi = 1.0, chi2 = 1.0;  // const_init_multi, const_init_chi2
  double* keep = nullptr;          // device [n_planes][3][nk + 4]: the plane rows of every plane's extended pair
  int* slot = nullptr;             // device [2 n_planes]: numbering of the accepted planes
  int extra = 0;                   // doubles behind the loop's 4 n_planes results, published with them: [d cp | plane-by-plane corrections]
  double* P = nullptr;             // the resident covariance and its size
  int n_state = 0;
  const int* d_ids = nullptr;      // device: loop column -> state column
};

// What tells the routes into the plane loop apart, as arguments: ovp_msckf_plane_update and ovp_msckf_plane_update_general fill in the
// general batch, plane_update_ordered the column order, the retry on a positive semi-definite prior sets psd.  None of it is kept in
// the context, so no call can leave any of it behind for the next.
struct PlaneLoopView {
  bool ordered = false;               // the loop runs in its own column order (plane_update_ordered: remapped tables, c->P = permuted copy)
  bool marginal = false;              // ... on a marginal: the rest of the state follows by push-through (k_plane_sub_accum per plane)
  const int* nl = nullptr;            // ordered: [plane] leading columns involved up to and including that plane (loop order)
  double* scatter_dst = nullptr;      // full order: where the covariance product of the loop is un-permuted to
  const int* scatter_ids = nullptr;   // ... and the inverse id table (device) for that
  bool boost = false;                 // full order: the columns behind the involved ones carry the diagonal boost (c->boost_vec)
  double t_entry = 0.0;               // host clock at the entry point (ovp_host_timing)
  bool psd = false;                   // second attempt of a loop whose chol(P) failed: pivot-dropping factor of the PSD prior
  const ovp_general_batch* gen = nullptr;  // general on-plane features (k_plane_feat_gen.hip), nullptr = none
  const int* plane_of_gen = nullptr;  // [gen->n_feats] 1-based plane slot, 0 = not on a plane
  const int* gen_pos = nullptr;       // [n_state] state column -> column in the loop's order, nullptr = identity
  int n_state = 0;
  unsigned char* gen_used = nullptr;  // [gen->n_feats] out: consumed by an accepted plane
  const PlaneInitView* init = nullptr;  // the loop initialises its planes (nullptr: it updates with them)
};
// the caller's result arrays of a plane entry point (each may be nullptr)
struct PlaneOut { double* dx_planes; uint8_t* plane_ok; double* plane_chi2; int* plane_dof; uint8_t* feat_used; };

// column of calibration column k of camera `cam` (ovp_cameras_upload) in the loop's column order (pos: PlaneLoopView::gen_pos)
static inline int gen_cam_col(const CalCols& cc, const int* pos, int n_pos, int cam, int k) {
  const int id = cc.col_of(cam, k);
  if (!pos) return id;
  return (id >= 0 && id < n_pos) ? pos[id] : -1;
}
// The plane loop's results go to the host as the point update's do (ovp_mailbox.h): ONE kernel behind the
// loop writes [chi2, decision, ... per plane | dx per plane | consumed features | flags] into mapped pinned memory and then a
// sequence number the host spins on - instead of four copy commands (a blit kernel of ~4 us each on the stream) and a stream
// synchronisation (interrupt + wake-up).  It also clears the device flags for the next call (was a fill command).
__global__ __launch_bounds__(1024) void k_publish_plane_results(const double* __restrict__ res, int n_res, const double* __restrict__ dx,
                                                               int n_dx, const unsigned char* __restrict__ used, int n_used,
                                                               int* __restrict__ flags, double* __restrict__ dst_res,
                                                               double* __restrict__ dst_dx, unsigned char* __restrict__ dst_used,
                                                               int* __restrict__ dst_flags, volatile unsigned* seq_host, unsigned seq) {
  const int t = threadIdx.x;
  for (int i = t; i < n_res; i += 1024) dst_res[i] = res[i];
  for (int i = t; i < n_dx; i += 1024) dst_dx[i] = dx[i];
  {
    // (8 bytes at a time: `used` and its mirror are 8-byte aligned, the tail byte by byte)
    const int w = n_used >> 3;
    const unsigned long long* us = reinterpret_cast<const unsigned long long*>(used);
    unsigned long long* ud = reinterpret_cast<unsigned long long*>(dst_used);
    for (int i = t; i < w; i += 1024) ud[i] = us[i];
    for (int i = 8 * w + t; i < n_used; i += 1024) dst_used[i] = used[i];
  }
  if (t < 4) dst_flags[t] = flags[t];
  __threadfence_system();
  __syncthreads();
  if (t == 0) *seq_host = seq;
  if (t < 4) flags[t] = 0;
}

// A device block -> the start of the pinned result block (c->pl_hres), by a kernel + sequence word instead of a copy command and a
// stream synchronisation (the entry points with a handful of results: SLAM update, delayed initialisation, initialize, dense update).
// A source the kernel cannot take (misaligned, 2 GiB) goes by copy + synchronisation; a block the caller reserved no payload for
// (plane2_buffers) is an error - it would run over the channels' line.
int ovp_fetch_to_hres(ovp_ctx* c, const void* dsrc, size_t bytes, hipStream_t s) {
  Mailbox& m = c->pl_hres;
  if (bytes > m.payload_capacity()) return OVP_E_CAPACITY;
  if ((((size_t)dsrc) & 7) || bytes > (size_t)0x7fffffff) {
    HIPCHK(hipMemcpyAsync(m.payload(), dsrc, bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
  }
  SeqChannel& ch = m.channel(0);
  const unsigned seq = ch.arm();
  HIPCHK(ovp_launch_publish_block(dsrc, m.dev(m.payload()), bytes, ch.word_dev(), seq, 0, s));
  return ch.wait(s);
}
static int ensure_pl_used(ovp_ctx* c) {
  HIPCHK(c->pl_used.alloc((size_t)c->f_max + 16));
  return 0;
}

int plane2_buffers(ovp_ctx* c, size_t stage_bytes, size_t res_bytes) {
  const int ld = c->ld;
  if (!c->pl_xflag) {  // first use (pl_xflag comes last: a call that failed half-way is taken up again by the next)
    const size_t nn = (size_t)(c->n_max + 1) * ld;
    HIPCHK(c->pl_Tbuf.alloc(2 * nn));
    HIPCHK(c->pl_crow.alloc((size_t)c->n_max + 16));
    HIPCHK(c->pl_dxlast.alloc((size_t)c->n_max + 16));
    HIPCHK(c->pl_cur.alloc(4));
    HIPCHK(c->pl_range_done.alloc(4));
    HIPCHK(hipMemset(c->pl_range_done, 0, 16));
    HIPCHK(c->pl_xbuf.alloc((size_t)9 * 18 * 256));
    HIPCHK(c->pl_xy.alloc((size_t)c->n_max + 32));
    HIPCHK(c->pl_xflag.alloc(64));
    HIPCHK(hipMemset(c->pl_xflag, 0, sizeof(unsigned) * 64));
  }
  HIPCHK(c->pl_stage.reserve(stage_bytes, 4096, c->stream));
  // (res_bytes is the callers' size of the whole result block, the line of the sequence word included)
  const size_t payload = res_bytes > Mailbox::LINE ? res_bytes - Mailbox::LINE : 0;
  if (payload > c->pl_hres.payload_capacity()) {
    HIPCHK(hipStreamSynchronize(c->stream));  // a kernel of an earlier call may still write the old block
    HIPCHK(c->pl_hres.reserve(payload, 4096));
  }
  return 0;
}

// ---- a selection of state columns as a state of its own (the plane loop in its own order) ----
// Device block [ids | inverse | clone ids | column map] of the selection `ids` (pos = its inverse, -1 = not selected), staged in the
// context's pinned block and sent on stream s; the kernels then address the selection through these tables instead of the state's.
struct SubTables {
  const int* d_ids = nullptr;
  const int* d_inv = nullptr;
  int* d_clone_id = nullptr;
  ovp::ColMap* d_colmap = nullptr;
  int calib_sub = -1, intr_sub = -1;
  std::vector<int> clone_sub;
};
static int sub_tables_upload(ovp_ctx* c, const ovp_update_opts* o, const std::vector<int>& ids, const std::vector<int>& pos,
                             SubTables* t, hipStream_t s) {
  const int n = c->n, C = c->fp.n_clones, ns = (int)ids.size();
  const size_t o_ids = 0, o_inv = sizeof(int) * (size_t)(c->n_max + 16), o_tab = 2 * o_inv;
  const size_t tab_bytes = sizeof(int) * (size_t)(c->c_max + 16) + sizeof(ovp::ColMap) * (size_t)c->n_max;
  const size_t blk_bytes = o_tab + tab_bytes;
  HIPCHK(c->pl_sub_tab.alloc(blk_bytes));
  int rc = 0;
  char* hb = c->pl_sub_tab.begin(blk_bytes, &rc);
  if (!hb) return rc;
  memset(hb, 0, blk_bytes);
  int* h_ids = (int*)(hb + o_ids);
  int* h_inv = (int*)(hb + o_inv);
  int* t_clone = (int*)(hb + o_tab);
  ovp::ColMap* t_cm = (ovp::ColMap*)(hb + o_tab + sizeof(int) * (size_t)(c->c_max + 16));
  memcpy(h_ids, ids.data(), sizeof(int) * (size_t)ns);
  for (int col = 0; col < n; ++col) h_inv[col] = pos[col] >= 0 ? pos[col] : 0;
  t->clone_sub.assign((size_t)C, 0);
  for (int i = 0; i < C; ++i) {
    t->clone_sub[i] = t_clone[i] = pos[c->h_clone_id[i]];
    for (int k = 0; k < 6; ++k) {
      ovp::ColMap& m = t_cm[t->clone_sub[i] + k];
      m.kind = 1;
      m.idx = i;
      m.off = k;
    }
  }
  t->calib_sub = (c->calib_id >= 0 && c->calib_id + 6 <= n && pos[c->calib_id] >= 0) ? pos[c->calib_id] : -1;
  t->intr_sub = (c->intr_id >= 0 && c->intr_id + 8 <= n && pos[c->intr_id] >= 0) ? pos[c->intr_id] : -1;
  if (t->calib_sub >= 0 && o->do_calib_camera_pose)
    for (int k = 0; k < 6; ++k) {
      t_cm[t->calib_sub + k].kind = 2;
      t_cm[t->calib_sub + k].idx = k;
    }
  if (t->intr_sub >= 0 && o->do_calib_camera_intrinsics)
    for (int k = 0; k < 8; ++k) {
      t_cm[t->intr_sub + k].kind = 2;
      t_cm[t->intr_sub + k].idx = 6 + k;
    }
  HIPCHK(c->pl_sub_tab.send(blk_bytes, s, Fence::Event));
  char* db = c->pl_sub_tab.dev();
  t->d_ids = (const int*)(db + o_ids);
  t->d_inv = (const int*)(db + o_inv);
  t->d_clone_id = (int*)(db + o_tab);
  t->d_colmap = (ovp::ColMap*)(db + o_tab + sizeof(int) * (size_t)(c->c_max + 16));
  return 0;
}
// the context's view of the state while a selection stands in for it, and back
struct SubSaved {
  int n, calib_id, intr_id;
  const double* P;  // the resident block (c->P on entry)
  int* clone_id;
  ovp::ColMap* colmap;
  const int* fp_clone_id;
  std::vector<int> h_clone_id;
};
// (the selection's covariance was gathered into c->P_tmp: the two buffers change places for as long as it stands in, and nothing
// in between addresses c->P_tmp)
static SubSaved sub_enter(ovp_ctx* c, const SubTables& t, int ns) {
  SubSaved sv{c->n, c->calib_id, c->intr_id, c->P, c->clone_id, c->colmap, c->fp.clone_id, c->h_clone_id};
  c->n = ns;
  c->P.swap(c->P_tmp);
  c->calib_id = t.calib_sub;
  c->intr_id = t.intr_sub;
  c->clone_id = t.d_clone_id;
  c->fp.clone_id = c->clone_id;
  c->colmap = t.d_colmap;
  c->h_clone_id = t.clone_sub;
  return sv;
}
static void sub_leave(ovp_ctx* c, const SubSaved& sv) {
  c->n = sv.n;
  if (c->P.get() != sv.P) c->P.swap(c->P_tmp);  // (the resident block comes back whatever happened to the pair in between)
  c->calib_id = sv.calib_id;
  c->intr_id = sv.intr_id;
  c->clone_id = sv.clone_id;
  c->fp.clone_id = sv.fp_clone_id;
  c->colmap = sv.colmap;
  c->h_clone_id = sv.h_clone_id;
}

static hipError_t ensure_events(std::vector<OvpEvent>& ev, size_t count) {  // the kernel timers' events, created on first use
  if (ev.size() < count) ev.resize(count);
  for (OvpEvent& e : ev)
    if (hipError_t err = e.create()) return err;
  return hipSuccess;
}

// sub_enter / sub_leave as a scope: every way out restores the context's view of the state
struct SubScope {
  ovp_ctx* c;
  SubSaved sv;
  bool in = false;
  void enter(const SubTables& t, int ns) {
    sv = sub_enter(c, t, ns);
    in = true;
  }
  ~SubScope() {
    if (in) sub_leave(c, sv);
  }
};

// A column order by first involvement: ids = the state columns in that order, pos = its inverse (-1 = not placed).
struct ColumnOrder {
  int n;  // state size the ids are checked against
  std::vector<int> ids, pos;
  bool bad_id = false;
  ColumnOrder(int n_, int pos_size) : n(n_), pos((size_t)pos_size, -1) { ids.reserve((size_t)n_); }
  void place(int id, int sz) {
    if (id < 0 || id + sz > n) {
      bad_id = true;
      return;
    }
    for (int k = 0; k < sz; ++k)
      if (pos[id + k] < 0) {
        pos[id + k] = (int)ids.size();
        ids.push_back(id + k);
      }
  }
  void place_clones_and_calibration(const ovp_ctx* c, const ovp_update_opts* o) {
    for (int i = 0; i < c->fp.n_clones; ++i) place(c->h_clone_id[i], 6);
    if (o->do_calib_camera_pose) place(c->calib_id, 6);
    if (o->do_calib_camera_intrinsics) place(c->intr_id, 8);
  }
};

// The rest of the state behind an update on the selection s (ns columns, device ids d_ids) by the push-through identity:
//   Lambda = A - A Pss+ A ;  P -= G Lambda G^T ;  dx = G u     (A = the pair accumulated in c->pl_Asum, G = P0[:, s])
// push_through_lambda leaves Lambda in c->T and G in c->Y (the caller's dx product reads it there), push_through_commit updates P.
static int push_through_lambda(ovp_ctx* c, const double* Pss_new, const int* d_ids, int ns, hipStream_t s) {
  const int n = c->n, ld = c->ld;
  HIPCHK(ovp_launch_gemm4(0, 0, ns, ns, ns, c->pl_Asum, ld, Pss_new, ld, c->W1, ld, 0, 0, s));
  HIPCHK(ovp_launch_gemm4(0, 0, ns, ns, ns, c->W1, ld, c->pl_Asum, ld, c->T, ld, 0, 1, s));
  HIPCHK(ovp_launch_mat_sub(c->pl_Asum, c->T, c->T, ns, ns, ld, s));
  HIPCHK(ovp_launch_gather_cols(c->P, ld, d_ids, n, ns, c->Y, ld, s));
  return 0;
}
static int push_through_commit(ovp_ctx* c, int ns, hipStream_t s) {
  const int n = c->n, ld = c->ld;
  HIPCHK(ovp_launch_gemm4(0, 0, n, ns, ns, c->Y, ld, c->T, ld, c->W1, ld, 0, 0, s));
  HIPCHK(ovp_launch_gemm4(0, 1, n, n, ns, c->W1, ld, c->Y, ld, c->L, ld, 0, 1, s));
  HIPCHK(ovp_launch_sub_sym(c->P, c->L, n, ld, s));
  return 0;
}

static int plane_loop(ovp_ctx* c, const ovp_update_opts* o, const ovp_plane_batch* pb, const PlaneLoopView& v, const PlaneOut& out);
static int plane_init_tail(ovp_ctx* c, const PlaneLoopView& v, int NP, bool solve, bool columns, const int* flags);

// ---- the plane loop in the loop's own column order (update/UpdaterMSCKF.cpp:413-649 has no size limit) --------------------------
// A plane's rows touch the clones, the calibration, its own closest point when it is a state variable and the SLAM landmarks lying
// on it (out-of-state planes).  Two things follow:
//  (1) LEADING BLOCK.  With P0 = L0 L0^T in the order [clones + calibration | the planes' own columns in processing order |
//      everything no plane of the call involves (IMU, dt, other landmarks)], A_k is zero outside the columns involved so far and L0
//      is lower triangular, so L0^T A_k L0 is zero outside that LEADING block: T_k = blockdiag(T_lead, I).  Plane k's products and
//      its factorization run on nl_k = 6 C + calibration + (own columns of the planes up to k) columns instead of n (config 3:
//      194 .. 224 of 240 - 13 to 14 tile steps of k_chol2 instead of 15, and shorter ones); only dx = L0[:, 0:nl] y and the commit
//      see all n rows.  The covariance is permuted once in front of the loop and once behind it.
//  (2) SUB-STATE.  Above the factorization's limit (n > 287) the loop runs on the marginal P0[s, s] of the involved columns s
//      (ns <= 287; same order) - same kernels, the state tables addressed through remapped column ids - and the rest of the state
//      follows from the push-through identity (k_plane_sub_accum for dx, the point path's  P -= G (A - A Pss+ A) G^T  for P).
// vin: the entry's view (entry time, general features); the column order is added here.
static int plane_update_ordered(ovp_ctx* c, const ovp_update_opts* o, const ovp_plane_batch* pb, const PlaneLoopView& vin,
                                const PlaneOut& out) {
  const int n = c->n, ld = c->ld, NP = pb->n_planes;
  const int n_slam = pb->n_slam > 0 ? pb->n_slam : 0;
  if (n_slam > 0 && (!pb->slam_plane || !pb->slam_state_id || !pb->slam_p || !pb->slam_p_fej)) return OVP_E_ARG;
  // ---- column order: first involvement ----
  ColumnOrder co(n, n);
  std::vector<int>& ids = co.ids;
  std::vector<int>& pos = co.pos;
  co.place_clones_and_calibration(c, o);
  if (vin.gen)  // general on-plane features: their cameras' calibration columns are involved, and every accepted plane corrects
    for (int k = 0; k < c->gen_ncams; ++k) {  // the table of every uploaded camera (k_plane_gen_commit) - all of them take part
      if (o->do_calib_camera_pose) co.place(c->gen_calib_id[k], 6);
      if (o->do_calib_camera_intrinsics) co.place(c->gen_intr_id[k], 8);
    }
  for (int q = 0; q < n_slam; ++q)
    if (pb->slam_plane[q] < 1 || pb->slam_plane[q] > NP || pb->slam_state_id[q] < 0 || pb->slam_state_id[q] + 3 > n) return OVP_E_ARG;
  std::vector<int> nl((size_t)(NP > 0 ? NP : 1), 0);
  for (int k = 0; k < NP; ++k) {
    if (pb->plane_state_id[k] >= 0) co.place(pb->plane_state_id[k], 3);
    else
      for (int q = 0; q < n_slam; ++q)
        if (pb->slam_plane[q] == k + 1) co.place(pb->slam_state_id[q], 3);
    nl[k] = (int)ids.size();
  }
  if (co.bad_id) return OVP_E_ARG;
  const int n_inv = (int)ids.size();
  const bool full = n <= ovp_chol2_max_n();  // the whole state fits one factorization: the rest rides along behind the leading block
  if (!full && n_inv > ovp_chol2_max_n()) return OVP_E_CAPACITY;  // the planes of this call involve more columns than one factorization holds
  if (full)
    for (int col = 0; col < n; ++col)
      if (pos[col] < 0) {
        pos[col] = (int)ids.size();
        ids.push_back(col);
      }
  const int ns = (int)ids.size();
  hipStream_t s = c->stream;
  if (!full) {
    HIPCHK(c->pl_Asum.alloc((size_t)c->n_max * ld));
    HIPCHK(c->pl_U.reserve((size_t)NP * ld, (size_t)8 * ld));
  }
  std::vector<int> sid_sub(NP > 0 ? NP : 1, -1), slam_sub(n_slam > 0 ? n_slam : 1, 0);
  for (int k = 0; k < NP; ++k) sid_sub[k] = pb->plane_state_id[k] >= 0 ? pos[pb->plane_state_id[k]] : -1;
  for (int q = 0; q < n_slam; ++q) {
    // a landmark listed on a plane that IS in the state takes no part in the loop (UpdaterMSCKF.cpp:240-241): park it on column 0
    // (in the full order every column has a position; on a marginal the landmark's columns may be absent)
    const int p0 = (pb->slam_state_id[q] >= 0 && pb->slam_state_id[q] + 3 <= n) ? pos[pb->slam_state_id[q]] : -1;
    if (p0 < 0 && pb->plane_state_id[pb->slam_plane[q] - 1] < 0) return OVP_E_ARG;
    slam_sub[q] = p0 >= 0 ? p0 : 0;
  }
  if (c->pl_ktimer) {
    HIPCHK(ensure_events(c->pl_ev_loop, 2));
    HIPCHK(hipEventRecord(c->pl_ev_loop[0], s));
  }
  // ---- remapped tables: [ids | inverse | clone ids | column map] ----
  SubTables st;
  {
    const int rt = sub_tables_upload(c, o, ids, pos, &st, s);
    if (rt) return rt;
  }
  const int* d_ids = st.d_ids;
  PlaneLoopView v = vin;
  v.ordered = true;
  v.marginal = !full;
  v.nl = nl.data();
  v.scatter_dst = full ? c->P : nullptr;  // full order: the loop's covariance product is un-permuted straight into the resident P
  v.scatter_ids = st.d_inv;
  if (vin.gen) {
    v.gen_pos = pos.data();
    v.n_state = n;
  }
  // full order: the columns behind the involved ones take a diagonal boost that the un-permutation behind the loop takes off
  // again (k_gather_block_boost) - an exact stochastic clone then factors at the first attempt
  PlaneInitView iv;
  if (vin.init) {  // (c->P: still the resident block, the loop's view of the state is entered below)
    iv = *vin.init;
    iv.P = c->P;
    iv.n_state = n;
    iv.d_ids = d_ids;
    v.init = &iv;
  }
  v.boost = full && n_inv < ns;
  if (v.boost) {
    HIPCHK(c->boost_vec.alloc((size_t)c->n_max + 16));
    HIPCHK(ovp_launch_gather_block_boost(c->P, ld, d_ids, ns, c->P_tmp, ld, n_inv, 1e-9, c->boost_vec, s));
  } else {
    HIPCHK(ovp_launch_gather_block(c->P, ld, d_ids, ns, c->P_tmp, ld, s));
  }
  if (!full) {
    HIPCHK(hipMemsetAsync(c->pl_Asum, 0, sizeof(double) * (size_t)ns * ld, s));
    HIPCHK(hipMemsetAsync(c->pl_U, 0, sizeof(double) * (size_t)NP * ld, s));
  }
  // ---- the loop in the new order ----
  ovp_plane_batch pbs = *pb;
  pbs.plane_state_id = sid_sub.data();
  pbs.slam_state_id = slam_sub.data();
  std::vector<double> dx_sub((size_t)ns * (NP > 0 ? NP : 1), 0.0);
  double* const dx_planes = out.dx_planes;
  {
    SubScope sub{c};
    sub.enter(st, ns);
    const PlaneOut out_sub{dx_sub.data(), out.plane_ok, out.plane_chi2, out.plane_dof, out.feat_used};
    const int rc = plane_loop(c, o, &pbs, v, out_sub);
    if (rc) return rc;  // the resident covariance was not touched (the device tables may have been: a loop that fails after
                        // accepting planes has marked them invalid, have_state = false - INTEGRATION.md section 5)
  }
  if (!full) {
    // ---- the rest of the state (c->P_tmp: the marginal after the loop) ----
    if (const int r = push_through_lambda(c, c->P_tmp, d_ids, ns, s)) return r;
    if (dx_planes && NP > 0) {
      // rows = planes: DX (NP x n) = U (NP x ns) G^T
      HIPCHK(ovp_launch_gemm4(0, 1, NP, n, ns, c->pl_U, ld, c->Y, ld, c->Lt, ld, 0, 0, s));
      HIPCHK(hipMemcpy2DAsync(dx_planes, sizeof(double) * n, c->Lt, sizeof(double) * ld, sizeof(double) * n, NP, hipMemcpyDeviceToHost, s));
    }
    if (const int r = push_through_commit(c, ns, s)) return r;
    if (v.init && NP > 0)  // (a loop whose factorization failed has returned above: the decisions stand)
      if (const int r = plane_init_tail(c, v, NP, /*solve=*/false, /*columns=*/true, nullptr)) return r;
    HIPCHK(hipStreamSynchronize(s));
  }
  if (dx_planes)  // the involved entries straight from the loop (on a marginal the product above agrees with them to rounding)
    for (int k = 0; k < NP; ++k)
      for (int i = 0; i < ns; ++i) dx_planes[(size_t)k * n + ids[i]] = dx_sub[(size_t)k * ns + i];
  return 0;
}

// ---- the loop body, in stages -----------------------------------------------------------------------------------------------
// L0 = chol(P) runs on the side stream beside the first plane's front end (plane_prelaunch).  Every way out of plane_loop behind the
// fork - HIPCHK returns included - makes the loop's stream wait for the side stream: the next call must not race a factorization
// that is still writing c->L / c->flags.
struct ForkGuard {
  hipStream_t s;
  hipEvent_t ev_join;
  hipStream_t side;
  bool forked;
  ~ForkGuard() {
    if (!forked) return;
    (void)hipEventRecord(ev_join, side);  // (a second record behind whatever the side stream got: harmless when the first one made it)
    (void)hipStreamWaitEvent(s, ev_join, 0);
  }
};
static hipError_t join_chol(ForkGuard& fork) {
  if (!fork.forked) return hipSuccess;
  fork.forked = false;
  return hipStreamWaitEvent(fork.s, fork.ev_join, 0);
}
// a refusal behind the fork: chol(P) has run - a flag it may have raised (singular prior) must not outlive the call
static int plane_bail(ovp_ctx* c, ForkGuard& fork, int code) {
  (void)join_chol(fork);
  (void)hipMemsetAsync(c->flags, 0, sizeof(int) * 4, fork.s);
  return code;
}

struct PlanePre { ovp::FeatParams fp; int n_slam = 0; size_t res_bytes = 0, tstride = 0; double t_first = 0.0; bool any_candidate = false; };
// What does not depend on the grouping goes to the device first: the fills and chol(P) (~70 us) run while the host sorts the features
// by plane and builds the per-plane tables (~40 us at config 3, during which the stream used to be idle).
static int plane_prelaunch(ovp_ctx* c, const ovp_update_opts* o, const ovp_plane_batch* pb, const PlaneLoopView& v, ForkGuard& fork,
                           PlanePre* pre) {
  const int n = c->n, ld = c->ld, F = c->n_feats, NP = pb->n_planes;
  for (int k = 0; k < NP; ++k)
    if (pb->plane_state_id[k] >= 0 && pb->plane_state_id[k] + 3 > n) return OVP_E_ARG;
  const int n_slam = pre->n_slam = pb->n_slam > 0 ? pb->n_slam : 0;
  if (n_slam > 0 && (!pb->slam_plane || !pb->slam_state_id || !pb->slam_p || !pb->slam_p_fej)) return OVP_E_ARG;
  for (int q = 0; q < n_slam; ++q)
    if (pb->slam_state_id[q] < 0 || pb->slam_state_id[q] + 3 > n || pb->slam_plane[q] < 1 || pb->slam_plane[q] > NP) return OVP_E_ARG;
  int rc = fill_feat_params(c, o);
  if (rc) return rc;
  pre->fp = c->fp;
  pre->fp.skip = nullptr;
  pre->fp.range_lo = 0;  // the plane loop always walks the whole batch
  pre->fp.range_hi = 0x7fffffff;
  const size_t n_extra = v.init ? (size_t)v.init->extra : 0;
  pre->res_bytes = sizeof(double) * (4 * (size_t)NP + n_extra + (size_t)n * NP) + (size_t)F + 64 + 256;  // (+ flags and sequence word)
  rc = plane_buffers(c, NP);
  if (rc) return rc;
  rc = plane2_buffers(c, 0, pre->res_bytes);
  if (rc) return rc;
  hipStream_t s = c->stream;
  pre->t_first = host_now_ms();
  const size_t tstride = pre->tstride = (size_t)(c->n_max + 1) * ld;
  {
    // results, per-plane corrections, used-feature mask (rounded up to whole words: the buffer is f_max + 64 bytes), flags,
    // [0] current T buffer + [1..2] factor bookkeeping (PlaneSolve::cond), half 0 of T (sum of the accepted L0^T A L0): one launch
    // both halves of T: a plane writes its candidate only inside its leading block, the rest of either half must read as zero;
    // the packed factor / inverted diagonal blocks behind the loop start out as the identity for the same reason
    const int ntn = (n + 15) / 16;
    void* zp[8] = {c->pl_res, c->pl_dx, c->pl_used, c->flags, c->pl_cur, c->pl_Tbuf, c->Ltp, c->Dinv};
    const size_t zb[8] = {sizeof(double) * (4 * NP + n_extra), sizeof(double) * (size_t)n * NP, ((size_t)F + 3) & ~(size_t)3, sizeof(int) * 4,
                          3 * sizeof(int), sizeof(double) * (tstride + (size_t)n * ld),
                          v.ordered ? sizeof(double) * 256 * (size_t)(ntn * (ntn + 1) / 2) : 0,
                          v.ordered ? sizeof(double) * 256 * (size_t)ntn : 0};
    const int zpat[8] = {0, 0, 0, 0, 0, 0, 2, 1};
    HIPCHK(ovp_launch_fill_regions(zp, zb, zpat, 8, ntn, s));
  }
  if (c->pl_ktimer) {  // [0 | 1] = the whole loop on the device clock (first launch .. covariance product), then a pair per plane
    HIPCHK(ensure_events(c->pl_ev_loop, 2));
    if (!v.ordered) HIPCHK(hipEventRecord(c->pl_ev_loop[0], s));  // (plane_update_ordered: in front of its permutation)
  }
  // (a cheap look at the batch first: when no plane can qualify - update/UpdaterMSCKF.cpp:316-317, 384-396 - nothing below needs the
  // factor, and a singular prior must not fail a call that has nothing to update)
  {
    const int GF = v.gen ? v.gen->n_feats : 0;
    std::vector<int> cnt((size_t)NP + 1, 0);
    for (int f = 0; f < F; ++f) {
      const int pf = pb->plane_of_feat[f];
      if (pf >= 1 && pf <= NP && c->h_n_meas[f] >= 2) ++cnt[pf];
    }
    for (int q = 0; q < n_slam; ++q) ++cnt[pb->slam_plane[q]];
    for (int g = 0; g < GF; ++g)
      if (v.plane_of_gen[g] >= 1 && v.plane_of_gen[g] <= NP && v.gen->n_meas[g] >= 2) ++cnt[v.plane_of_gen[g]];
    for (int pl = 1; pl <= NP && !pre->any_candidate; ++pl)
      pre->any_candidate = cnt[pl] >= (v.init ? 3 : (pb->plane_state_id[pl - 1] >= 0 ? 1 : 4));
  }
  // L0 = chol(P), dense lower triangular in c->L.  Nothing needs it before the first plane's W = A L0, so it runs on the side
  // stream beside that plane's rows / Gram pair / assembly (round 5; one workgroup - the small kernels of the front end leave it a
  // CU on every XCD) and is joined in front of that product (A/B in round 5: config 3 2.776 -> 2.719 ms).
  if (pre->any_candidate) {
    if (s == c->stream) {
      HIPCHK(hipEventRecord(c->ev_fork, s));
      HIPCHK(hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
      fork.forked = true;
      rc = chol_of_P(c, c->stream2, v.psd);
      if (rc) return rc;
      HIPCHK(hipEventRecord(c->ev_join, c->stream2));
    } else {
      rc = chol_of_P(c, s, v.psd);
      if (rc) return rc;
    }
  }
  return 0;
}

// items 0 .. count-1 bucketed by 1-based plane slot (slot(i) outside 1 .. NP: left out) in one pass, order kept: plane pl (0-based)
// has items[start[pl + 1] .. start[pl + 2])  (a scan of the whole batch per plane was 0.4 ms of host time in front of the first
// launch at 8000 features x 50 planes)
struct PlaneBuckets { std::vector<int> start, items; };
template <class Slot>
static PlaneBuckets bucket_by_plane(int count, int NP, Slot slot) {
  PlaneBuckets b;
  b.start.assign((size_t)NP + 2, 0);
  b.items.resize((size_t)(count > 0 ? count : 1));
  for (int i = 0; i < count; ++i) {
    const int p = slot(i);
    if (p >= 1 && p <= NP) ++b.start[p + 1];
  }
  for (int pl = 1; pl <= NP + 1; ++pl) b.start[pl] += b.start[pl - 1];
  std::vector<int> fill(b.start.begin(), b.start.end());
  for (int i = 0; i < count; ++i) {
    const int p = slot(i);
    if (p >= 1 && p <= NP) b.items[fill[p]++] = i;
  }
  return b;
}

// ---- host-side grouping (update/UpdaterMSCKF.cpp:204-229): no HIP call, nothing of the context written ----
struct PlaneGroups {
  std::vector<PlaneJobH> jobs;
  std::vector<int> featlist;  // batch features of the jobs, by job
  std::vector<int> glist;     // general features of the jobs, by job
  std::vector<int> perms;     // per job: n entries
  int ng_max = 0;
};
// returns a refusal code (the caller bails) or 0
static int plane_group(const ovp_ctx* c, const ovp_update_opts* o, const ovp_plane_batch* pb, const PlaneLoopView& v, int n_slam,
                       PlaneGroups* groups) {
  PlaneGroups& g = *groups;
  const int n = c->n, F = c->n_feats, NP = pb->n_planes, M = c->max_meas;
  const ovp_general_batch* gbp = v.gen;
  const int GF = gbp ? gbp->n_feats : 0, GM = gbp ? gbp->max_meas : 0;
  const int ncal = (o->do_calib_camera_pose ? 6 : 0) + (o->do_calib_camera_intrinsics ? 8 : 0);
  const PlaneBuckets bf = bucket_by_plane(F, NP, [&](int f) { return pb->plane_of_feat[f]; });
  const PlaneBuckets bg = bucket_by_plane(GF, NP, [&](int i) { return gbp->n_meas[i] >= 2 ? v.plane_of_gen[i] : 0; });
  const CalCols cc(c, o);
  for (int pl = 0; pl < NP; ++pl) {
    PlaneJobH j;
    j.pl = pl;
    j.start = (int)g.featlist.size();
    j.nf = 0;
    j.rows_total = 0;
    j.rows_live = 0;
    j.sid = pb->plane_state_id[pl];
    j.in_state = j.sid >= 0;
    unsigned long long seen = 0ull;
    for (int bi = bf.start[pl + 1]; bi < bf.start[pl + 2]; ++bi) {
      const int f = bf.items[bi];
      const int m = c->h_n_meas[f];
      if (m < 2) continue;
      if (m > OVP_MAX_MEAS_DEV) return OVP_E_CAPACITY;  // 2m bearing rows = one wavefront (the constraint row is wave-uniform)
      g.featlist.push_back(f);
      j.nf++;
      j.rows_total += 3 * m - 3;
      j.rows_live += 2 * m - 2;  // the m identical constraint rows are one direction (k_chol2 gate)
      for (int k = 0; k < m; ++k) seen |= 1ull << c->h_clone_idx[(size_t)f * M + k];
    }
    // general features on this plane: same rows per feature, any clone, any camera (its calibration columns are involved)
    j.g_start = (int)g.glist.size();
    j.ng = 0;
    unsigned cams_seen = j.nf > 0 ? 1u : 0u;  // (the batch's features are camera 0's)
    for (int gi = bg.start[pl + 1]; gi < bg.start[pl + 2]; ++gi) {
      const int gf = bg.items[gi], m = gbp->n_meas[gf];
      g.glist.push_back(gf);
      j.ng++;
      j.rows_total += 3 * m - 3;
      j.rows_live += 2 * m - 2;
      for (int k = 0; k < m; ++k) {
        seen |= 1ull << gbp->clone_idx[(size_t)gf * GM + k];
        cams_seen |= 1u << gbp->cam_idx[(size_t)gf * GM + k];
      }
    }
    const int ncal_pl = j.ng > 0 ? ncal * __builtin_popcount(cams_seen) : ncal;
    int ns_pl = 0;  // SLAM landmarks on this (out-of-state) plane: one row and three involved columns each
    if (!j.in_state)
      for (int q = 0; q < n_slam; ++q)
        if (pb->slam_plane[q] == pl + 1) ++ns_pl;
    if (ns_pl > PA_MAXQ) return OVP_E_CAPACITY;
    j.ns_pl = ns_pl;
    const bool too_few = v.init ? j.nf + j.ng < 3  // update/UpdaterPlane.cpp:303
                                : (j.nf + j.ng == 0 || (!j.in_state && j.nf + j.ng + ns_pl < 4));  // update/UpdaterMSCKF.cpp:316-317,384-396
    if (too_few) {
      g.featlist.resize(j.start);
      g.glist.resize(j.g_start);
      continue;
    }
    j.rows_total += ns_pl;
    j.rows_live += ns_pl;
    const int c_ref = 6 * __builtin_popcountll(seen) + ncal_pl + 3 * ns_pl;
    const int rows_c = j.rows_total > c_ref ? c_ref : j.rows_total;  // UpdaterPlane::measurement_compress_inplace
    j.rows_u = j.in_state ? rows_c : rows_c - 3;
    j.n_involved = c_ref + (j.in_state ? 3 : 0);
    if (!j.in_state) j.rows_total -= 3;
    if (!j.in_state) j.rows_live -= 3;
    if (j.rows_u < 1) {
      g.featlist.resize(j.start);
      g.glist.resize(j.g_start);
      continue;
    }
    if (j.ng > g.ng_max) g.ng_max = j.ng;
    // (initialisation: the chi2 of StateHelper::initialize covers the rows that do not involve the plane, with dof = all rows, :471)
    j.dof = v.init ? rows_c : j.rows_u;
    j.thr = v.init ? v.init->chi2 * ovp_chi2_quantile_095(rows_c) : o->chi2_multiplier * ovp_chi2_quantile_095(j.rows_u);
    // order of the involved columns in the normalised Gram: everything that is not a clone first, the clones last (a rank
    // deficiency - gauge freedom, planar scene - then shows up in the trailing pivots, k_chol2 mode 2)
    {
      std::vector<int> perm(n, -1);
      int pos = 0;
      std::vector<char> inv(n, 0);
      // (camera 0's columns: the batch's features are its, and so is every plane without general features as before; a plane whose
      // general features are all another camera's does not involve them - c_ref above counts the same cameras)
      const bool cam0 = j.ng == 0 || (cams_seen & 1u);
      if (o->do_calib_camera_pose && cam0)
        for (int k = 0; k < 6; ++k) inv[c->calib_id + k] = 1;
      if (o->do_calib_camera_intrinsics && cam0)
        for (int k = 0; k < 8; ++k) inv[c->intr_id + k] = 1;
      if (j.ng > 0)  // the cameras of this plane's general features
        for (int cam = 0; cam < c->gen_ncams; ++cam)
          if ((cams_seen >> cam) & 1u)
            for (int k = 0; k < 14; ++k) {
              if (!cc.on(k)) continue;
              const int col = gen_cam_col(cc, v.gen_pos, v.n_state, cam, k);
              if (col < 0 || col >= n) return OVP_E_ARG;
              inv[col] = 1;
            }
      if (j.in_state)
        for (int k = 0; k < 3; ++k) inv[j.sid + k] = 1;
      if (!j.in_state)
        for (int q = 0; q < n_slam; ++q)
          if (pb->slam_plane[q] == pl + 1)
            for (int k = 0; k < 3; ++k) inv[pb->slam_state_id[q] + k] = 1;
      for (int col = 0; col < n; ++col)
        if (inv[col]) perm[col] = pos++;
      for (int ci = 0; ci < (int)c->h_clone_id.size(); ++ci)
        if ((seen >> ci) & 1ull)
          for (int k = 0; k < 6; ++k) {
            const int col = c->h_clone_id[ci] + k;
            if (col >= 0 && col < n && perm[col] < 0) perm[col] = pos++;
          }
      j.n_inv_cols = pos;
      g.perms.insert(g.perms.end(), perm.begin(), perm.end());
    }
    g.jobs.push_back(j);
  }
  return 0;
}

// ---- staging: ints [featlist | sid NP | perms NJ*n | slam_plane | slam_id], doubles [cp | cp_fej | slam_p | slam_p_fej] ----
struct PlaneStage {  // device addresses of the tables inside c->pl_stage
  const int *feat, *sid, *perm, *slam_plane, *slam_id;
  double *cp, *cp_fej, *slam_p, *slam_p_fej;
};
static int plane_stage_upload(ovp_ctx* c, const ovp_plane_batch* pb, const PlaneGroups& g, const PlanePre& pre, PlaneStage* st) {
  const int NP = pb->n_planes, n_slam = pre.n_slam;
  const size_t n_int = g.featlist.size() + (size_t)NP + g.perms.size() + 2 * (size_t)n_slam;
  const size_t int_bytes = ((n_int * sizeof(int) + 15) / 16) * 16;
  const size_t n_dbl = 6 * (size_t)NP + 6 * (size_t)n_slam;
  const size_t stage_bytes = int_bytes + n_dbl * sizeof(double);
  int rc = plane2_buffers(c, stage_bytes, pre.res_bytes);  // (grows the staging block when this frame needs more)
  if (rc) return rc;
  char* h = c->pl_stage.begin(stage_bytes, &rc);
  if (!h) return rc;
  int* hi = (int*)h;
  double* hd = (double*)(h + int_bytes);
  int* di = (int*)c->pl_stage.dev();
  double* dd = (double*)(c->pl_stage.dev() + int_bytes);
  size_t io = 0;
  st->feat = di + io;
  memcpy(hi + io, g.featlist.data(), sizeof(int) * g.featlist.size());
  io += g.featlist.size();
  st->sid = di + io;
  memcpy(hi + io, pb->plane_state_id, sizeof(int) * NP);
  io += NP;
  st->perm = di + io;
  if (!g.perms.empty()) memcpy(hi + io, g.perms.data(), sizeof(int) * g.perms.size());
  io += g.perms.size();
  st->slam_plane = di + io;
  if (n_slam) memcpy(hi + io, pb->slam_plane, sizeof(int) * n_slam);
  io += n_slam;
  st->slam_id = di + io;
  if (n_slam) memcpy(hi + io, pb->slam_state_id, sizeof(int) * n_slam);
  io += n_slam;
  memcpy(hd, pb->cp, sizeof(double) * 3 * NP);
  memcpy(hd + 3 * NP, pb->cp_fej, sizeof(double) * 3 * NP);
  if (n_slam) {
    memcpy(hd + 6 * NP, pb->slam_p, sizeof(double) * 3 * n_slam);
    memcpy(hd + 6 * NP + 3 * n_slam, pb->slam_p_fej, sizeof(double) * 3 * n_slam);
  }
  HIPCHK(c->pl_stage.send(stage_bytes, c->stream, Fence::CallerWaits));
  st->cp = dd;
  st->cp_fej = dd + 3 * NP;
  st->slam_p = dd + 6 * NP;
  st->slam_p_fej = dd + 6 * NP + 3 * n_slam;
  return 0;
}

// ---- general features: the batch and the per-plane lists, the marks and the staged rows ----
struct PlaneGenStage {
  ovp::PlaneGenParams gp0;   // everything but the per-plane fields (plane_gen_params)
  ovp::PlaneGenCols cols;
  unsigned calmask = 0;
};
static int plane_gen_upload(ovp_ctx* c, const ovp_update_opts* o, const PlaneLoopView& v, const PlanePre& pre, const PlaneGroups& g,
                            ForkGuard& fork, PlaneGenStage* gs) {
  const int n = c->n;
  const ovp_general_batch* gbp = v.gen;
  hipStream_t s = c->stream;
  memset(&gs->gp0, 0, sizeof(gs->gp0));
  memset(&gs->cols, 0xff, sizeof(gs->cols));
  const CalCols cc(c, o);
  gs->calmask = cc.mask;
  if (gbp) {
    for (int cam = 0; cam < c->gen_ncams; ++cam)
      for (int k = 0; k < 14; ++k)
        if (cc.on(k)) {
          gs->cols.col[cam][k] = gen_cam_col(cc, v.gen_pos, v.n_state, cam, k);
          if (gs->cols.col[cam][k] < 0 || gs->cols.col[cam][k] >= n) return plane_bail(c, fork, OVP_E_ARG);
        }
  }
  if (!gbp || g.glist.empty()) return 0;
  const int GF = gbp->n_feats, GM = gbp->max_meas;
  const size_t GFM = (size_t)GF * GM;
  StageLayout lay;
  const size_t o_uv = lay.take(sizeof(float) * 2 * GFM), o_ci = lay.take(sizeof(int) * GFM), o_cam = lay.take(sizeof(int) * GFM),
               o_nm = lay.take(sizeof(int) * GF), o_p = lay.take(sizeof(double) * 3 * GF), o_list = lay.take(sizeof(int) * g.glist.size()),
               in_bytes = lay.bytes();
  const size_t mark_stride = (size_t)((n + 4 + 15) & ~15), hp_stride = (size_t)ovp::PG_ROWS * (n + 4);
  // inputs through the pinned arena (nobody else uses it while a plane loop is enqueued; the previous user has waited for its
  // copy), marks and staged rows in a device block of their own: no host synchronisation unless a block has to grow
  const size_t o_hp = StageLayout::al(sizeof(int) * mark_stride * g.ng_max), total = o_hp + sizeof(double) * hp_stride * g.ng_max;
  if (total > c->pl_gen_dev.capacity()) {
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(c->pl_gen_dev.reserve(total, total / 2));
  }
  void *ah = nullptr, *ad = nullptr;
  {
    const int rca = ovp_io_arena(c, in_bytes, &ah, &ad);
    if (rca) return plane_bail(c, fork, rca);
  }
  char* h = (char*)ah;
  memcpy(h + o_uv, gbp->uv, sizeof(float) * 2 * GFM);
  memcpy(h + o_ci, gbp->clone_idx, sizeof(int) * GFM);
  memcpy(h + o_cam, gbp->cam_idx, sizeof(int) * GFM);
  memcpy(h + o_nm, gbp->n_meas, sizeof(int) * GF);
  memcpy(h + o_p, gbp->p_FinG, sizeof(double) * 3 * GF);
  memcpy(h + o_list, g.glist.data(), sizeof(int) * g.glist.size());
  HIPCHK(hipMemcpyAsync(ad, ah, in_bytes, hipMemcpyHostToDevice, s));
  char* d = (char*)ad;
  char* ds = (char*)c->pl_gen_dev;
  ovp::PlaneGenParams& gp0 = gs->gp0;
  gp0.fp = pre.fp;
  gp0.fp.calmask = gs->calmask;
  cc.fill_cameras(gp0);
  gp0.cc = gs->cols;
  gp0.uv = (const float*)(d + o_uv);
  gp0.clone_idx = (const int*)(d + o_ci);
  gp0.cam_idx = (const int*)(d + o_cam);
  gp0.n_meas = (const int*)(d + o_nm);
  gp0.p_FinG = (const double*)(d + o_p);
  gp0.max_meas = GM;
  gp0.list = (const int*)(d + o_list);
  gp0.mark = (int*)ds;
  gp0.mark_stride = (int)mark_stride;
  gp0.hp = (double*)(ds + o_hp);
  gp0.hp_stride = hp_stride;
  return 0;
}

// ---- one plane's enqueue: the parameter blocks of its launches ----
struct PlaneCall {  // what every plane of a call shares
  const ovp_update_opts* o; const ovp_plane_batch* pb; const PlaneLoopView* v; const PlanePre* pre; const PlaneStage* st;
  const PlaneGenStage* gs; int NJ; double white_c, noise_scale;
};
static ovp::PlaneParams plane_feat_params(const ovp_ctx* c, const PlaneCall& k, const PlaneJobH& j) {
  ovp::PlaneParams pp;
  pp.feat_list = k.st->feat + j.start;
  pp.n_local = j.nf;
  pp.plane = j.pl;
  pp.in_state = j.in_state;
  pp.plane_sid = j.sid;
  pp.white_c = k.white_c;
  pp.cp = k.st->cp;
  pp.cp_fej = k.st->cp_fej;
  pp.cst = c->pl_cst;
  return pp;
}
static ovp::PlaneGenParams plane_gen_params(const ovp_ctx* c, const PlaneCall& k, const PlaneJobH& j, int nk, int nsplit, int ntile_pl) {
  ovp::PlaneGenParams g = k.gs->gp0;
  g.list = k.gs->gp0.list + j.g_start;
  g.n_local = j.ng;
  g.plane = j.pl;
  g.in_state = j.in_state;
  g.plane_sid = j.sid;
  g.white_c = k.white_c;
  g.cp = k.st->cp;
  g.cp_fej = k.st->cp_fej;
  g.n = nk;
  g.hp_stride = (size_t)ovp::PG_ROWS * (nk + 4);
  g.part_split = c->part + (size_t)nsplit * ntile_pl * 256;
  g.cst_rec = c->pl_cst + (size_t)j.nf * 10;
  return g;
}
static ovp::PlaneAsm plane_asm_params(const ovp_ctx* c, const PlaneCall& k, const PlaneJobH& j, int jn, int nk, int chunks, int nsplit,
                                      int ntile_pl) {
  const int ld = c->ld;
  ovp::PlaneAsm pa;
  memset(&pa, 0, sizeof(pa));
  pa.gramS = c->gramS;
  pa.n_clones = k.pre->fp.n_clones;
  pa.n_chunks = chunks;
  pa.part = c->part;
  pa.n_split = nsplit + (j.ng > 0 ? 1 : 0);
  pa.ntile = ntile_pl;
  pa.colmap = c->colmap;
  pa.n = nk;
  pa.plane_sid = j.sid;
  pa.in_state = j.in_state;
  pa.cst = c->pl_cst;
  pa.nf = j.nf + (j.ng > 0 ? 1 : 0);
  pa.n_slam = j.in_state ? 0 : k.pre->n_slam;
  pa.plane1 = j.pl + 1;
  pa.slam_plane = k.st->slam_plane;
  pa.slam_id = k.st->slam_id;
  pa.slam_p = k.st->slam_p;
  pa.slam_p_fej = k.st->slam_p_fej;
  pa.cp = k.st->cp + 3 * j.pl;
  pa.cp_fej = k.st->cp_fej + 3 * j.pl;
  pa.white_c = k.white_c;
  pa.do_fej = k.pre->fp.do_fej;
  pa.Ab = c->Ab;
  pa.lda = ld;
  pa.perm = k.st->perm + (size_t)jn * c->n;
  pa.An = c->pl_An;
  pa.ldn = ld;
  pa.bn = c->pl_bn;
  pa.eps = 1e-12;
  pa.scal = c->pl_scal;
  return pa;
}
// both factorizations of a plane: j0 = the update's T_try on the leading block (with the split over two workgroups), j1 = the range part
static void plane_chol_jobs(const ovp_ctx* c, const PlaneCall& k, const PlaneJobH& j, int nk, unsigned seq, ovp::Chol2Job* j0,
                            ovp::Chol2Job* j1) {
  const int ld = c->ld;
  memset(j0, 0, sizeof(*j0));
  memset(j1, 0, sizeof(*j1));
  j0->A = c->pl_Tbuf;
  j0->sel = c->pl_cur;
  j0->sel_xor = 1;
  j0->sel_stride = k.pre->tstride;
  j0->n = nk;
  j0->ld = ld;
  j0->add_identity = 1;
  j0->mode = 1;
  j0->brow = c->pl_crow;
  j0->flag = c->flags;
  j1->A = c->pl_An;
  j1->n = j.n_inv_cols;
  j1->ld = ld;
  j1->add_identity = 0;
  j1->mode = 2;
  j1->brow = c->pl_bn;
  j1->flag = c->flags + 2;
  j1->piv_floor = 1e-5;
  // The update part on two workgroups: tile columns < h and the rest (k_chol2.hip).  Measured (r03, A/B in one call): at 16 tile
  // columns (N = 240) nothing is gained (2.91 against 2.81 ms per config-3 plane loop for h = 5 .. 8: exports + a second gate
  // hand-over cost what the second CU's f64 pipe gives), so one workgroup stays the default there; from 17 tile columns on
  // (N > 255) the tile registers of one workgroup spill and the split wins (config 4, N = 285: 7.91 ms for h = 5 or 6, 8.10 for
  // 7 or 8, 8.69 unsplit).  OVP_C2_SPLIT: 0 = never, h = forced.
  const char* split_s = getenv("OVP_C2_SPLIT");  // (read per call: the tests switch it)
  const int split_env = split_s ? atoi(split_s) : -1;
  const int nb = nk + 1, ntb = (nb + 15) / 16;
  const int nst = (nb % 16 == 1) ? ntb - 1 : ntb;  // a border row alone in its tile row takes no step
  int h = ntb >= 17 ? nst / 3 : 0;  // part B also runs the back half of the chain: 5 - 6 of 18 steps measured best (7.91 ms per
                                    // config-4 plane loop against 8.10 for 7 or 8 and 8.69 unsplit)
  if (split_env >= 0) h = split_env < ntb - 1 ? split_env : 0;
  if (h > 9) h = 9;  // pl_xbuf holds nine exported steps
  j0->split_h = h;
  j0->xbuf = c->pl_xbuf;
  j0->xflag = c->pl_xflag;
  j0->xseq = seq;
}
static ovp::PlaneSolve plane_solve_params(const ovp_ctx* c, const PlaneCall& k, const PlaneJobH& j, int jn, unsigned seq) {
  const int n = c->n;
  ovp::PlaneSolve ps;
  memset(&ps, 0, sizeof(ps));
  ps.scal = c->pl_scal;
  ps.range_done = c->pl_range_done;
  ps.seq = seq;
  ps.xzz = c->pl_xy;
  ps.xy = c->pl_xy + 16;
  ps.xsync = c->pl_xflag + 32;
  ps.thr = j.thr;
  ps.rows_live = j.rows_live;
  ps.rows_u = j.rows_u;
  ps.n_involved = j.n_inv_cols;
  ps.force = k.pb->force_decision ? (int)k.pb->force_decision[j.pl] : -1;
  ps.noise_scale = k.noise_scale;
  ps.tol_strict = 1e-5;
  ps.tol_loose = 1e-5;
  ps.res_out = c->pl_res + 4 * j.pl;
  ps.L0 = c->L;
  ps.ld0 = c->ld;
  ps.n_full = n;
  ps.dx_out = c->pl_dx + (size_t)j.pl * n;
  ps.dx_last = c->pl_dxlast;
  ps.cur = c->pl_cur;
  // The covariance product behind the loop needs the factor of the last ACCEPTED T.  The last few planes leave theirs behind when
  // they are accepted (~8 us of stores each); if one of them stays the last accepted plane, the k_tilechol behind the loop
  // (94 us at N = 240) finds nothing to do.  Which plane that is, is decided on the device.
  const int emit_last = 4;
  ps.cond = c->pl_cur + 1;
  ps.seq_plane = jn + 1;
  ps.emit = (jn >= k.NJ - emit_last) ? 1 : 0;
  ps.Lpack = c->Ltp;
  ps.Dinv = c->Dinv;
  ps.feat_list = k.st->feat + j.start;
  ps.n_feat_local = j.nf;
  ps.feat_used = c->pl_used;
  ps.clone_R = c->clone_R;
  ps.clone_p = c->clone_p;
  ps.clone_id = c->clone_id;
  ps.n_clones = k.pre->fp.n_clones;
  ps.cal = c->cal;
  ps.calib_id = k.o->do_calib_camera_pose ? c->calib_id : -1;
  ps.intr_id = k.o->do_calib_camera_intrinsics ? c->intr_id : -1;
  ps.cp = k.st->cp;
  ps.plane_sid = k.st->sid;
  ps.n_planes = k.pb->n_planes;
  ps.n_slam = k.pre->n_slam;
  ps.slam_id = k.st->slam_id;
  ps.slam_p = k.st->slam_p;
  return ps;
}

// diagnostics: cycle stamps of the last plane's launch - only a library whose k_chol2 was compiled with them writes any
// (tools/build_c2_stamps.sh; the product build leaves them out: their tests cost 1 us per launch).  *out = nullptr: off.
static int plane_stamps_buffer(long long** out) {
  static const bool pl_stamps = getenv("OVP_PL_STAMPS") != nullptr && ovp_chol2_stamps_compiled();
  static long long* d_stamps = nullptr;
  if (pl_stamps && !d_stamps) HIPCHK(hipMalloc((void**)&d_stamps, sizeof(long long) * 2 * 16 * 32));
  *out = pl_stamps ? d_stamps : nullptr;
  return 0;
}
static int plane_stamps_dump(long long* d_stamps, int nk, int split_h, hipStream_t s) {
  long long h[2 * 16 * 32];
  HIPCHK(hipStreamSynchronize(s));
  HIPCHK(hipMemcpy(h, d_stamps, sizeof(h), hipMemcpyDeviceToHost));
  const int ntb = (nk + 1 + 15) / 16;
  const long long* e = h + (ntb + 1) * 16;
  fprintf(stderr, "[plane tail, cycles] factor %lld | gate %lld | back substitution %lld | dx = L0 y %lld | commit %lld\n",
          e[0] - h[0], e[1] - e[0], e[2] - e[1], e[3] - e[2], e[4] - e[3]);
  if (atoi(getenv("OVP_PL_STAMPS")) >= 2) {
    // per step, both parts of a split factorization, relative to part A's first stamp: elimination wave 0 [start | column
    // there | eliminated | signalled], tile wave 0 [start | panel there | next column updated | published | step done]
    const long long t0 = h[0];
    for (int part = 0; part < (split_h > 0 ? 2 : 1); ++part) {
      const long long* hp = h + part * 16 * 32;
      fprintf(stderr, " part %c: prologue stamps %lld %lld %lld\n", part ? 'B' : 'A', hp[13] - t0, hp[14] - t0, hp[15] - t0);
      for (int k = 0; k < ntb; ++k) {
        const long long* q = hp + k * 16;
        if (!q[0] && !q[8]) continue;
        // arrival word of the elimination step: what was missing of {column, panel, trailing} when wave 0 first looked (0 = there)
        const long long aw = q[4] - 500500500;
        const long long am = llround((double)aw / 1e6), ar = aw - am * 1000000, ap = llround((double)ar / 1e3), at = ar - ap * 1000;
        fprintf(stderr, "  k=%2d E %7lld %7lld %7lld %7lld [%3lld %3lld %3lld] | T %7lld %7lld %7lld %7lld %7lld | T7 %7lld %7lld %7lld\n", k,
                q[0] - t0, q[1] - t0, q[2] - t0, q[3] - t0, am, ap, at, q[8] - t0, q[9] - t0, q[10] - t0, q[11] - t0, q[12] - t0,
                q[7] - t0, q[5] - t0, q[6] - t0);
        if (k >= 2 && atoi(getenv("OVP_PL_STAMPS")) >= 3) fprintf(stderr, "        T own tiles final %7lld, column k+1 taken %7lld\n", q[13] - t0, q[14] - t0);
      }
      const long long* m = hp + (ntb + 1) * 16;
      fprintf(stderr, "  tail: factor done %lld, gate %lld, backsolve %lld, dx %lld, commit %lld\n", m[0] - t0, m[1] - t0, m[2] - t0,
              m[3] - t0, m[4] - t0);
    }
  }
  HIPCHK(hipMemset(d_stamps, 0, sizeof(long long) * 2 * 16 * 32));
  return 0;
}

static int plane_enqueue(ovp_ctx* c, const PlaneCall& k, const PlaneJobH& j, int jn, ForkGuard& fork) {
  const int n = c->n, ld = c->ld;
  const ovp::FeatParams& fp = k.pre->fp;
  hipStream_t s = c->stream;
  // leading block this plane's products and factorization run on (plane_update_ordered): every column involved so far
  const int nk = k.v->ordered ? k.v->nl[j.pl] : n;
  // (1) per-feature rows
  const ovp::PlaneParams pp = plane_feat_params(c, k, j);
  ovp::FeatParams fpl = fp;
  fpl.n = nk;
  fpl.P = c->P;
  int chunks = (2 * j.nf + c->rows_per_chunk - 1) / c->rows_per_chunk;
  int nsplit = 1;
  if (j.nf > 0) {
    HIPCHK(ovp_launch_plane_feat(&fpl, &pp, j.nf, s));
    // (2) Gram products
    HIPCHK(ovp_launch_gram_pair(c->rec, fp.n_clones, j.nf, c->rows_per_chunk, chunks, c->gramS, c->G, 3 * j.nf, c->ldg, nk + 4,
                                c->n_split, c->part, &nsplit, s));
  } else {  // a plane with general features only: an empty structured Gram (one chunk of zeros per clone), no G^T G split
    chunks = 1;
    nsplit = 0;
    HIPCHK(hipMemsetAsync(c->gramS, 0, sizeof(double) * (size_t)fp.n_clones * OVP_GRAM_ELEMS, s));
  }
  // (2b) the plane's general features: one more split of the partials and one more moment record (k_plane_feat_gen.hip); a plane
  // without any enqueues nothing here
  const int nt16_pl = (nk + 4 + 15) / 16, ntile_pl = nt16_pl * (nt16_pl + 1) / 2;
  if (j.ng > 0) {
    const ovp::PlaneGenParams g = plane_gen_params(c, k, j, nk, nsplit, ntile_pl);
    HIPCHK(ovp_launch_plane_feat_gen(&g, s));
  }
  // (3) pair on the state columns, normalised Gram, residual energy
  const ovp::PlaneAsm pa = plane_asm_params(c, k, j, jn, nk, chunks, nsplit, ntile_pl);
  HIPCHK(ovp_launch_plane_assemble2(&pa, s));
  if (k.v->init)  // initialisation: the plane rows of the extended pair stay behind for the tail (same partials, same moments)
    HIPCHK(ovp_launch_plane_init_keep(&pa, k.v->init->keep + (size_t)j.pl * 3 * (nk + 4), s));
  // (4) W = A L0 ;  T_try = T_cur + L0^T W ;  c = L0^T b
  HIPCHK(join_chol(fork));  // (first plane: L0 comes from the side stream)
  HIPCHK(ovp_launch_gemm4(0, 0, nk, nk, nk, c->Ab, ld, c->L, ld, c->W1, ld, 0, 0, s));
  HIPCHK(ovp_launch_plane_dT(nk, c->L, ld, c->W1, c->Ab + (size_t)nk * ld, c->pl_Tbuf, k.pre->tstride, c->pl_cur, c->pl_crow, s));
  // (5) both factorizations, gate, solve, commit
  const unsigned seq = ++c->pl_seq;
  ovp::Chol2Job j0, j1;
  plane_chol_jobs(c, k, j, nk, seq, &j0, &j1);
  const ovp::PlaneSolve ps = plane_solve_params(c, k, j, jn, seq);
  if (c->pl_ktimer == 1) {
    HIPCHK(ensure_events(c->pl_ev, 2 * (size_t)(jn + 1)));
    HIPCHK(hipEventRecord(c->pl_ev[2 * jn], s));
  }
  long long* d_stamps = nullptr;
  if (const int r = plane_stamps_buffer(&d_stamps)) return r;
  if (d_stamps) j0.stamps = d_stamps;
  HIPCHK(ovp_launch_chol2(&j0, &j1, &ps, s));
  if (c->pl_ktimer == 1) HIPCHK(hipEventRecord(c->pl_ev[2 * jn + 1], s));
  if (k.v->gen)  // an accepted plane also corrects the tables of ovp_cameras_upload, which the general rows of the planes behind it read
    HIPCHK(ovp_launch_plane_gen_commit(c->pl_res + 4 * j.pl, c->pl_dx + (size_t)j.pl * n, c->gen_cal, c->gen_ncams, &k.gs->cols,
                                       k.gs->calmask, s));
  if (k.v->marginal)
    HIPCHK(ovp_launch_plane_sub_accum(c->pl_res + 4 * j.pl, c->Ab, c->pl_Asum, c->pl_dx + (size_t)j.pl * n,
                                      c->pl_U + (size_t)j.pl * ld, nk, ld, s));
  if (d_stamps && jn == k.NJ - 1) return plane_stamps_dump(d_stamps, nk, j0.split_h, s);
  return 0;
}

// ---- the covariance, once:  P = L0 T^-1 L0^T = V^T V,  V = Lt^-1 L0^T ----
static int plane_cov_product(ovp_ctx* c, const PlaneLoopView& v, size_t tstride, bool* factor_enqueued) {
  const int n = c->n, ld = c->ld;
  hipStream_t s = c->stream;
  // chol of the accepted T (+ I) unless the last accepted plane left its factor behind; the second-generation kernel reads the
  // current half of the double buffer itself (Chol2Job::sel) - no copy into c->T in front of it
  if (n <= ovp_chol2_max_n() + 1) {
    ovp::Chol2Job jt;
    memset(&jt, 0, sizeof(jt));
    jt.A = c->pl_Tbuf;
    jt.sel = c->pl_cur;
    jt.sel_xor = 0;
    jt.sel_stride = tstride;
    jt.n = n;
    jt.ld = ld;
    jt.add_identity = 1;
    jt.mode = 0;
    jt.flag = c->flags;
    jt.Lpack = c->Ltp;
    jt.Dinv_out = c->Dinv;
    jt.skip_cond = c->pl_cur + 1;
    HIPCHK(ovp_launch_chol2(&jt, nullptr, nullptr, s));
  } else {
    HIPCHK(ovp_launch_select_copy(c->T, c->pl_Tbuf, tstride, c->pl_cur, n, ld, 1, s));
    HIPCHK(chol_of_T(c, c->T, n, ld, 1, c->pl_cur + 1, s));
  }
  HIPCHK(ovp_launch_fwdsub(c->Ltp, c->Dinv, c->L, c->Y, n, ld, 0, s));
  HIPCHK(ovp_launch_gemm4c(1, 0, n, n, n, c->Y, ld, c->Y, ld, c->P, ld, 0, 1, c->flags, s));
  // back into the state's own column order (unless a factorization failed: the resident P stays), and the factor of the
  // covariance just formed for the point update behind the loop (P = V^T V: M = V^T, rows in state order) - one launch for both
  const bool keep_factor = getenv("OVP_NO_KEPT_FACTOR") == nullptr;  // (read per call: the tests switch it)
  const bool want_factor = keep_factor && !v.marginal && n <= OVP_TILECHOL_NMAX;
  if (want_factor) HIPCHK(c->Lkeep.alloc((size_t)c->n_max * ld));
  if (v.scatter_dst) {
    HIPCHK(ovp_launch_unpermute_pair(c->P, c->Y, ld, v.scatter_ids, n, v.scatter_dst, want_factor ? c->Lkeep : nullptr, ld,
                                     c->flags, v.boost ? c->boost_vec : nullptr, s));
    c->kept.boost = want_factor && v.boost;  // Lkeep is a factor of P + diag(boost_vec): the point update on it
                                             // takes the amounts off at its end (point_enqueue_tail)
  } else if (want_factor) {
    HIPCHK(ovp_launch_factor_from_V(c->Y, ld, nullptr, n, c->Lkeep, ld, s));
  }
  *factor_enqueued = want_factor;
  return 0;
}

// ---- results: one pinned block, one wait ----
// [chi2, decision, .. per plane | dx per plane | consumed features], and behind `used`, on a 64-byte line of their own, the flags:
// the payload of c->pl_hres, posted on its channel 0
struct PlaneResBlock { double *res, *dx; unsigned char* used; char* flags; };
static PlaneResBlock plane_res_block(const ovp_ctx* c, int NP, int n_extra) {
  PlaneResBlock b;
  b.res = (double*)c->pl_hres.payload();
  b.dx = b.res + 4 * (size_t)NP + n_extra;
  b.used = (unsigned char*)(b.dx + (size_t)c->n * NP);
  b.flags = (char*)b.used + StageLayout::al((size_t)c->n_feats);
  return b;
}
static int plane_publish(ovp_ctx* c, const PlaneResBlock& b, int NP, int n_extra, bool want_dx) {
  const Mailbox& m = c->pl_hres;
  SeqChannel& ch = c->pl_hres.channel(0);
  const unsigned seq = ch.arm();
  hipLaunchKernelGGL(k_publish_plane_results, dim3(1), dim3(1024), 0, c->stream, c->pl_res, 4 * NP + n_extra, c->pl_dx, want_dx ? c->n * NP : 0,
                     c->pl_used, c->n_feats, c->flags, (double*)m.dev(b.res), (double*)m.dev(b.dx), (unsigned char*)m.dev(b.used),
                     (int*)m.dev(b.flags), (volatile unsigned*)ch.word_dev(), seq);
  HIPCHK(hipGetLastError());
  return 0;
}
// host clocks and device timers of the call that has just been waited for
static void plane_account(ovp_ctx* c, double t_entry, double t_first, double t_enq, int NJ) {
  c->host_acc[0] += t_first - t_entry;
  c->host_acc[1] += t_enq - t_entry;
  c->host_acc[2] += host_now_ms() - t_enq;
  c->host_acc[3] += 1.0;
  if (c->pl_ktimer) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, c->pl_ev_loop[0], c->pl_ev_loop[1]) == hipSuccess) c->host_acc[7] += ms;
  }
  if (c->pl_ktimer == 1)
    for (int jn = 0; jn < NJ; ++jn) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, c->pl_ev[2 * jn], c->pl_ev[2 * jn + 1]) == hipSuccess) {
        c->pl_ktime_ms += ms;
        c->pl_klaunches += 1;
      }
    }
}
// The pinned block into the caller's arrays, and what a failed factorization means.  *retry_psd: nothing was committed and chol(P)
// hit a non-positive pivot - the caller runs the same loop once more on the pivot-dropping factor.
static int plane_unpack(ovp_ctx* c, const PlaneLoopView& v, const PlaneGroups& g, const PlaneResBlock& b, int NP, const PlaneOut& out,
                        bool factor_enqueued, bool* retry_psd) {
  const int n = c->n, F = c->n_feats;
  const double* hres = b.res;
  c->pl_used_valid = true;
  c->h_pl_used.assign(b.used, b.used + F);
  if (out.dx_planes) memcpy(out.dx_planes, b.dx, sizeof(double) * (size_t)n * NP);
  if (out.feat_used && F) memcpy(out.feat_used, b.used, (size_t)F);
  if (v.gen && v.gen_used) {  // the general features an accepted plane consumed (the host knows each plane's list)
    memset(v.gen_used, 0, (size_t)v.gen->n_feats);
    for (const PlaneJobH& j : g.jobs)
      if (hres[4 * j.pl + 1] > 0.5)
        for (int k = 0; k < j.ng; ++k) v.gen_used[g.glist[j.g_start + k]] = 1;
  }
  for (const PlaneJobH& j : g.jobs) {
    if (out.plane_ok) out.plane_ok[j.pl] = hres[4 * j.pl + 1] > 0.5 ? 1 : 0;
    if (out.plane_chi2) out.plane_chi2[j.pl] = hres[4 * j.pl];
    if (out.plane_dof) out.plane_dof[j.pl] = j.dof;
  }
  const int bad = c->h_flags[0] | c->h_flags[2];  // (the device words were cleared by the publishing kernel)
  if (bad) {
    // A failed factorization / timed-out hand-over rejects its plane and every later one before anything is committed, and the
    // covariance product behind the loop is cancelled (the resident P is the prior).  Planes accepted BEFORE the failure have
    // committed their corrections to the device tables: those no longer belong to the resident covariance - the caller must
    // upload the state again (OVP_E_STATE until then).  chol(P) itself failing (singular prior) happens in front of every plane.
    bool any_committed = false;
    for (const PlaneJobH& j : g.jobs) any_committed |= hres[4 * j.pl + 1] > 0.5;
    if (any_committed) c->have_state = false;
    if (bad == 1 && !any_committed && !v.psd) {
      // chol(P) hit a non-positive pivot: the prior is only positive SEMI-definite.  Nothing was committed and the resident
      // covariance was not written.
      *retry_psd = true;
      return 0;
    }
  }
  if (bad & 2) return OVP_E_TIMEOUT;
  if (bad) return OVP_E_NOTSPD;
  c->kept.have = factor_enqueued;
  return 0;
}

// ---- the tail of a plane initialisation (k_plane_init2.hip): from the device-resident decisions, no host round trip ----
// solve: numbering, Z, d cp, corrections between the new planes (loop order; results go out with the loop's);  columns: the new
// rows and columns of the resident covariance (needs the covariance behind the last plane in place).  Inside the loop c->n is the
// loop's size and c->pl_dx its stride.
static int plane_init_tail(ovp_ctx* c, const PlaneLoopView& v, int NP, bool solve, bool columns, const int* flags) {
  const PlaneInitView& iv = *v.init;
  ovp::PlaneInitTail t;
  memset(&t, 0, sizeof(t));
  t.res = c->pl_res;
  t.n_planes = NP;
  t.keep = iv.keep;
  t.nk = v.nl[NP - 1];
  t.dx = c->pl_dx;
  t.dx_stride = c->n;
  t.flags = flags;
  t.slot = iv.slot;
  t.extra = c->pl_res + 4 * (size_t)NP;
  t.P = iv.P;
  t.ldp = c->ld;
  t.n_state = iv.n_state;
  t.ids = iv.d_ids;
  if (solve) HIPCHK(ovp_launch_plane_init_solve(&t, c->stream));
  if (columns) HIPCHK(ovp_launch_plane_init_columns(&t, c->stream));
  return 0;
}

// ---- UpdaterMSCKF::update, per-plane loop (second generation) ------------------------------------------------------------
// See k_plane2.hip for the algebra.  Everything of a call is enqueued without a host synchronisation: the per-call tables go
// through one pinned staging block, the results come back through one pinned block the host waits for on a sequence word.
// The caller has checked c, o, pb and the context's state (plane_update_entry).
static int plane_loop(ovp_ctx* c, const ovp_update_opts* o_in, const ovp_plane_batch* pb, const PlaneLoopView& v, const PlaneOut& out) {
  const int n = c->n, F = c->n_feats, NP = pb->n_planes;
  // skip_plane_used is an option of the POINT update that follows; the plane loop itself produces the mask
  ovp_update_opts o_local = *o_in;
  o_local.skip_plane_used = 0;
  const ovp_update_opts* o = &o_local;
  c->pl_used_valid = false;  // (also the retry's: the first attempt's mask no longer counts)
  if (n > ovp_chol2_max_n()) return OVP_E_CAPACITY;  // (plane_update_ordered hands over a sub-state the factorization can take)
  if (out.feat_used) memset(out.feat_used, 0, (size_t)F);
  for (int pl = 0; pl < NP; ++pl) {
    if (out.plane_ok) out.plane_ok[pl] = 0;
    if (out.plane_chi2) out.plane_chi2[pl] = 0.0;
    if (out.plane_dof) out.plane_dof[pl] = 0;
  }
  if (out.dx_planes && NP > 0) memset(out.dx_planes, 0, sizeof(double) * (size_t)n * NP);
  if (NP == 0) {  // a frame without planes: nothing is consumed, and a point update with skip_plane_used may follow
    if (F) HIPCHK(hipMemsetAsync(c->pl_used, 0, (size_t)F, c->stream));
    c->h_pl_used.assign((size_t)F, 0);
    c->pl_used_valid = true;
    return 0;
  }
  hipStream_t s = c->stream;
  ForkGuard fork{s, c->ev_join, c->stream2, false};
  PlanePre pre;
  int rc = plane_prelaunch(c, o, pb, v, fork, &pre);
  if (rc) return rc;
  PlaneGroups g;
  rc = plane_group(c, o, pb, v, pre.n_slam, &g);
  if (rc) return plane_bail(c, fork, rc);
  const int NJ = (int)g.jobs.size();
  if (NJ == 0 && pre.any_candidate) {  // chol(P)'s verdict concerns nobody
    HIPCHK(join_chol(fork));
    HIPCHK(hipMemsetAsync(c->flags, 0, sizeof(int) * 4, s));
  }
  PlaneStage st;
  rc = plane_stage_upload(c, pb, g, pre, &st);
  if (rc) return rc;
  PlaneGenStage gs;
  rc = plane_gen_upload(c, o, v, pre, g, fork, &gs);
  if (rc) return rc;
  // weight of the expected energy of the rounding-decided rows in the gate statistic (k_chol2.hip); OVP_PL_NOISE_SCALE overrides the
  // calibrated constant for the study that produced it (tools/plane_gate_agreement.py --fit)
  double noise_scale = OVP_PLANE_NOISE_KAPPA;
  if (const char* ns_env = getenv("OVP_PL_NOISE_SCALE")) noise_scale = atof(ns_env);  // (read per call)
  const double sigma_c = v.init ? v.init->multi * o->sigma_constraint : o->sigma_constraint;
  const PlaneCall call{o, pb, &v, &pre, &st, &gs, NJ, 1.0 / sigma_c, noise_scale};
  for (int jn = 0; jn < NJ; ++jn) {
    rc = plane_enqueue(c, call, g.jobs[jn], jn, fork);
    if (rc) return rc;
  }
  bool factor_enqueued = false;
  if (NJ > 0) {
    rc = plane_cov_product(c, v, pre.tstride, &factor_enqueued);
    if (rc) return rc;
    if (v.init) {  // the accepted planes become state variables (on a marginal the columns wait for the push-through)
      rc = plane_init_tail(c, v, NP, /*solve=*/true, /*columns=*/!v.marginal, c->flags);
      if (rc) return rc;
    }
  }
  if (c->pl_ktimer) HIPCHK(hipEventRecord(c->pl_ev_loop[1], s));
  const int n_extra = v.init ? v.init->extra : 0;
  const PlaneResBlock blk = plane_res_block(c, NP, n_extra);
  rc = plane_publish(c, blk, NP, n_extra, out.dx_planes != nullptr);
  if (rc) return rc;
  const double t_enq = host_now_ms();
  rc = c->pl_hres.channel(0).wait(s);
  if (rc) return rc;
  c->pl_stage.done();
  c->io.done();  // (plane_gen_upload's tables)
  memcpy(c->h_flags, blk.flags, sizeof(int) * 4);
  plane_account(c, v.t_entry, pre.t_first, t_enq, NJ);
  bool retry_psd = false;
  rc = plane_unpack(c, v, g, blk, NP, out, factor_enqueued, &retry_psd);
  if (!retry_psd) return rc;
  PlaneLoopView v2 = v;  // the same loop once more on the pivot-dropping factor (chol_of_P)
  v2.psd = true;
  if (!v.ordered) v2.t_entry = host_now_ms();
  return plane_loop(c, o, pb, v2, out);
}

// what both entry points share behind their argument checks: v carries the general features, if any
static int plane_update_entry(ovp_ctx* c, const ovp_update_opts* o, const ovp_plane_batch* pb, PlaneLoopView v, const PlaneOut& out) {
  if (!c->have_state || !c->have_cov || !c->have_batch) return OVP_E_STATE;
  if (c->h_n_meas.empty() && c->n_feats > 0) return OVP_E_STATE;  // needs ovp_batch_upload (host copy of the layout)
  v.t_entry = host_now_ms();
  c->kept.have = false;
  c->pl_used_valid = false;
  const int rcu = ensure_pl_used(c);
  if (rcu) return rcu;
  const bool natural_order = getenv("OVP_PL_NATURAL_ORDER") != nullptr;  // A/B: the loop on all n columns in the state's order
  if (pb->n_planes > 0 && (c->n > ovp_chol2_max_n() || !natural_order)) return plane_update_ordered(c, o, pb, v, out);
  return plane_loop(c, o, pb, v, out);
}

extern "C" int ovp_msckf_plane_update(ovp_ctx* c, const ovp_update_opts* o, const ovp_plane_batch* pb, double* dx_planes,
                                      uint8_t* plane_ok, double* plane_chi2, int* plane_dof, uint8_t* feat_used) {
  if (!c || !o || !pb || pb->n_planes < 0) return OVP_E_ARG;
  return plane_update_entry(c, o, pb, PlaneLoopView{}, PlaneOut{dx_planes, plane_ok, plane_chi2, plane_dof, feat_used});
}

// ---- the plane loop with the on-plane features of a general batch behind the batch's (update/UpdaterHelper.cpp:335-344 over every
// camera, :448-512 the point-on-plane rows; update/UpdaterMSCKF.cpp:411-649 the loop) ----
extern "C" int ovp_msckf_plane_update_general(ovp_ctx* c, const ovp_update_opts* o, const ovp_plane_batch* pb, const ovp_general_batch* gb,
                                              const int* plane_of_gen, double* dx_planes, uint8_t* plane_ok, double* plane_chi2,
                                              int* plane_dof, uint8_t* feat_used, uint8_t* gen_used) {
  if (!c || !o || !pb || !gb || pb->n_planes < 0 || gb->n_feats < 0) return OVP_E_ARG;
  const int GF = gb->n_feats, NP = pb->n_planes;
  if (GF > 0 && (!plane_of_gen || !gb->n_meas)) return OVP_E_ARG;
  bool any = false;
  for (int g = 0; g < GF; ++g) {
    if (plane_of_gen[g] < 0 || plane_of_gen[g] > NP) return OVP_E_ARG;
    any |= plane_of_gen[g] > 0;
  }
  if (any) {  // everything that can refuse the general features is looked at before anything is enqueued
    if (!c->have_state || !c->have_cov || c->gen_ncams < 1) return OVP_E_STATE;
    const int rc = check_general_batch(c, gb, true, plane_of_gen);
    if (rc) return rc;
    if (CalCols(c, o).check(c->n, true)) return OVP_E_ARG;  // calibration columns of every camera the options estimate
  }
  if (gen_used && GF > 0) memset(gen_used, 0, (size_t)GF);
  const PlaneOut out{dx_planes, plane_ok, plane_chi2, plane_dof, feat_used};
  PlaneLoopView v;
  if (!any) return plane_update_entry(c, o, pb, v, out);
  std::vector<unsigned char> marks((size_t)GF, 0);  // (the caller's array is written only by a call that succeeds)
  v.gen = gb;
  v.plane_of_gen = plane_of_gen;
  v.gen_used = marks.data();
  const int rc = plane_update_entry(c, o, pb, v, out);
  if (!rc && gen_used) memcpy(gen_used, marks.data(), (size_t)GF);
  return rc;
}

// ---- UpdaterPlane::init_vio_plane core in one device pass, any camera (update/UpdaterPlane.cpp:296-481 over the rows of
// update/UpdaterHelper.cpp:335-344, 448-512) ----
// Initialisation is the loop's out-of-state plane update with a flat prior on the plane (white_c = 1 / (const_init_multi sigma_c),
// StateHelper::initialize's gate), so everything in front of the gate is plane_loop in the column order of plane_update_ordered; the
// accepted planes are appended behind the last plane from the device-resident decisions (k_plane_init2.hip).
extern "C" int ovp_plane_init_general(ovp_ctx* c, const ovp_update_opts* o, const ovp_plane_batch* pb, double const_init_multi,
                                      double const_init_chi2, double* dx_planes, int dx_stride, uint8_t* plane_ok, double* plane_chi2,
                                      int* plane_dof, int* new_ids, double* cp_new, uint8_t* feat_used, const ovp_general_batch* gb,
                                      const int* plane_of_gen, uint8_t* gen_used) {
  if (!c || !o || !pb || pb->n_planes < 0 || (gb && gb->n_feats < 0)) return OVP_E_ARG;
  if (!pb->cp || (dx_planes && dx_stride < 0)) return OVP_E_ARG;
  const int GF = gb ? gb->n_feats : 0, NP = pb->n_planes, F = c->n_feats, n = c->n;
  if (GF > 0 && (!plane_of_gen || !gb->n_meas)) return OVP_E_ARG;
  bool any = false;
  int cand = 0;  // planes with at least three features: the only ones that can append columns
  for (int g = 0; g < GF; ++g) {
    if (plane_of_gen[g] < 0 || plane_of_gen[g] > NP) return OVP_E_ARG;
    any |= plane_of_gen[g] > 0;
  }
  if (!c->have_state || !c->have_cov || !c->have_batch) return OVP_E_STATE;
  if (c->h_n_meas.empty() && F > 0) return OVP_E_STATE;
  if (F > 0 && !pb->plane_of_feat) return OVP_E_ARG;
  // ---- everything that can refuse the call, before anything is enqueued or written ----
  if (any) {
    if (c->gen_ncams < 1) return OVP_E_STATE;
    const int rc = check_general_batch(c, gb, true, plane_of_gen);  // (a track above OVP_GEN_MAX_MEAS: OVP_E_CAPACITY)
    if (rc) return rc;
    if (CalCols(c, o).check(n, true)) return OVP_E_ARG;
  }
  {
    std::vector<int> cnt((size_t)NP + 1, 0);
    for (int f = 0; f < F; ++f) {
      const int pf = pb->plane_of_feat[f];
      if (pf >= 1 && pf <= NP && c->h_n_meas[f] >= 2) ++cnt[pf];
    }
    for (int g = 0; g < GF; ++g)
      if (plane_of_gen[g] >= 1 && gb->n_meas[g] >= 2) ++cnt[plane_of_gen[g]];
    for (int pl = 1; pl <= NP; ++pl) cand += cnt[pl] >= 3;
    if (n + 3 * cand > c->n_max) return OVP_E_CAPACITY;
    ColumnOrder co(n, n);  // the involved columns: one factorization has to hold them (plane_update_ordered places the same)
    co.place_clones_and_calibration(c, o);
    if (any)
      for (int k = 0; k < c->gen_ncams; ++k) {
        if (o->do_calib_camera_pose) co.place(c->gen_calib_id[k], 6);
        if (o->do_calib_camera_intrinsics) co.place(c->gen_intr_id[k], 8);
      }
    if (co.bad_id) return OVP_E_ARG;
    if ((int)co.ids.size() > ovp_chol2_max_n()) return OVP_E_CAPACITY;
  }
  if (feat_used && F) memset(feat_used, 0, (size_t)F);
  if (gen_used && GF) memset(gen_used, 0, (size_t)GF);
  for (int pl = 0; pl < NP; ++pl) {
    if (new_ids) new_ids[pl] = -1;
    if (cp_new) memcpy(cp_new + 3 * pl, pb->cp + 3 * pl, 3 * sizeof(double));
    if (dx_planes) memset(dx_planes + (size_t)pl * dx_stride, 0, sizeof(double) * dx_stride);
    if (plane_ok) plane_ok[pl] = 0;
    if (plane_chi2) plane_chi2[pl] = 0.0;
    if (plane_dof) plane_dof[pl] = 0;
  }
  if (NP == 0 || cand == 0) return 0;  // update/UpdaterPlane.cpp:303: no plane of the call can be initialised
  drop_kept_factor(c);  // (writes the covariance: a kept factor no longer belongs to it)
  c->pl_used_valid = false;
  if (const int rcu = ensure_pl_used(c)) return rcu;
  // per-call device buffers of the tail: the kept plane rows of every plane, the numbering of the accepted ones; its results ride
  // behind the loop's in c->pl_res
  const int nk_max = (n < ovp_chol2_max_n() ? n : ovp_chol2_max_n()) + 4;
  PlaneInitView iv;
  iv.multi = const_init_multi;
  iv.chi2 = const_init_chi2;
  iv.extra = 3 * NP + 3 * NP * NP;
  HIPCHK(c->pl_init_keep.reserve((size_t)NP * 3 * nk_max, (size_t)4 * 3 * nk_max));
  HIPCHK(c->pl_init_slot.reserve(2 * (size_t)NP, 16));
  HIPCHK(c->pl_res.reserve(4 * (size_t)NP + iv.extra, 64));
  iv.keep = c->pl_init_keep;
  iv.slot = c->pl_init_slot;
  // no plane numbered until k_plane_init_solve has run: a loop that enqueues no plane (rows_c - 3 < 1 for all of them) leaves it so,
  // and the column kernels behind a marginal's push-through then find nothing to append
  HIPCHK(hipMemsetAsync(c->pl_init_slot, 0xff, sizeof(int) * 2 * (size_t)NP, c->stream));
  // the loop's batch: every plane outside the state, no first estimate of its own, no landmark rows
  std::vector<int> sid((size_t)NP, -1);
  ovp_plane_batch pbi = *pb;
  pbi.plane_state_id = sid.data();
  pbi.cp_fej = pb->cp;
  pbi.n_slam = 0;
  pbi.slam_plane = pbi.slam_state_id = nullptr;
  pbi.slam_p = pbi.slam_p_fej = nullptr;
  pbi.force_decision = nullptr;
  std::vector<double> dxp((size_t)NP * n, 0.0);
  std::vector<uint8_t> ok((size_t)NP, 0);
  std::vector<unsigned char> marks((size_t)(GF > 0 ? GF : 1), 0);
  PlaneLoopView v;
  v.t_entry = host_now_ms();
  v.init = &iv;
  if (any) {
    v.gen = gb;
    v.plane_of_gen = plane_of_gen;
    v.gen_used = marks.data();
  }
  const int rc = plane_update_ordered(c, o, &pbi, v, PlaneOut{dxp.data(), ok.data(), plane_chi2, plane_dof, feat_used});
  c->kept.have = false;  // (the loop's factor is the n x n block's; the state has grown)
  if (rc) {
    if (feat_used && F) memset(feat_used, 0, (size_t)F);
    for (int pl = 0; pl < NP; ++pl) {
      if (plane_chi2) plane_chi2[pl] = 0.0;
      if (plane_dof) plane_dof[pl] = 0;
    }
    return rc;
  }
  // ---- the accepted planes, numbered as the device numbered them ----
  const double* extra = (const double*)c->pl_hres.payload() + 4 * (size_t)NP;  // [d cp | corrections between the new planes]
  int q = 0;
  std::vector<int> nid((size_t)NP, -1);
  for (int pl = 0; pl < NP; ++pl)
    if (ok[pl]) nid[pl] = n + 3 * q++;
  for (int pl = 0; pl < NP; ++pl) {
    if (plane_ok) plane_ok[pl] = ok[pl];
    if (!ok[pl]) continue;
    if (new_ids) new_ids[pl] = nid[pl];
    if (cp_new)
      for (int k = 0; k < 3; ++k) cp_new[3 * pl + k] = pb->cp[3 * pl + k] + extra[3 * pl + k];
    if (dx_planes) {  // the variables that existed before this plane: the state, then the planes initialised earlier in the call
      double* row = dx_planes + (size_t)pl * dx_stride;
      memcpy(row, dxp.data() + (size_t)pl * n, sizeof(double) * (size_t)(n < dx_stride ? n : dx_stride));
      for (int pj = 0; pj < pl; ++pj)
        if (ok[pj])
          for (int k = 0; k < 3; ++k)
            if (nid[pj] + k < dx_stride) row[nid[pj] + k] = extra[3 * NP + ((size_t)pj * NP + pl) * 3 + k];
    }
  }
  if (gen_used && any) memcpy(gen_used, marks.data(), (size_t)GF);
  c->n = n + 3 * q;
  return 0;
}

// The batch's features alone (UpdaterPlane::init_vio_plane core, camera 0): ovp_plane_init_general without a general batch.
extern "C" int ovp_plane_init(ovp_ctx* c, const ovp_update_opts* o, const ovp_plane_batch* pb, double const_init_multi,
                              double const_init_chi2, double* dx_planes, int dx_stride, uint8_t* plane_ok, double* plane_chi2,
                              int* plane_dof, int* new_ids, double* cp_new, uint8_t* feat_used) {
  return ovp_plane_init_general(c, o, pb, const_init_multi, const_init_chi2, dx_planes, dx_stride, plane_ok, plane_chi2, plane_dof,
                                new_ids, cp_new, feat_used, nullptr, nullptr, nullptr);
}
