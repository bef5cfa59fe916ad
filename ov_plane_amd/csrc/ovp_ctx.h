// Internal header of the C-ABI shim (libovplane_hip.so): the context, the launch prototypes of the kernels' translation units and
// the helpers the entry-point files share.  Not installed; the boundary is include/ovplane_hip.h.
//   ovp_api_ctx.hip    context, covariance residency and bookkeeping (upload / marginal / propagate / clone / marginalize /
//                      initialize), pose tables, feature batch, diagnostics
//   ovp_api_point.hip  point update: K1 -> information pair -> EKF update (ovp_msckf_update and its staged form), ovp_ekf_update;
//                      what a call does is decided by the pure planner of ovp_point_plan.h, the stages enqueue a PointPlan
//   ovp_api_rccl.hip   feature-sharded update over RCCL
//   ovp_api_plane.hip  plane loop (ovp_msckf_plane_update) and plane initialisation (ovp_plane_init_general: the loop as its front,
//                      k_plane_init2.hip as its tail; ovp_plane_init: the same without a general batch)
//   ovp_api_slam.hip   SLAM landmarks (ovp_slam_update, ovp_slam_delayed_init), triangulation
//   ovp_api_general.hip general point features (any camera, long tracks): camera tables, gate + pending pair, triangulation
//   k_plane_detect.hip plane detection from the tracked features: its kernels and its entry points
//   k_delaunay.hip     the Delaunay triangulation of a frame's vertices in one workgroup (ovp_launch_delaunay, k_delaunay.h)
//   k_active_tracks.hip re-triangulation of a frame's active tracks (ovp_active_tracks_*): its kernel and its entry points
//   k_featdb.hip       the feature database (ovp_featdb_*): the track table, its kernels and entry points
//   k_klt.hip          the image front end (ovp_klt_*): equalisation, image pyramid and pyramidal Lucas-Kanade, kernels and entry points
//   k_retire.hip       a frame's retirements in one compaction, its plane merges in sequence in front of it: kernels and entry points
//   k_zupt.hip         the zero-velocity update's gate, rows and apply kernels (entry point: ovp_zupt_update in ovp_api_ctx.hip)
//   k_propagate.hip    the IMU integration, clone-plus-time-offset and publishing kernels of ovp_propagate_and_clone (ovp_api_ctx.hip)
// Results reach the host through ovp_mailbox.h (Mailbox / SeqChannel; the copy-and-post kernel is k_publish.hip); host tables reach
// the device through ovp_staged.h (Staged: pinned block, device block and the fence that says when the host may write again), and
// every event is an OvpEvent from the same header.
#pragma once
#include "ovplane_hip.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <memory>
#include <vector>

#include "ovp_buf.h"
#include "ovp_mailbox.h"
#include "ovp_staged.h"
#include "ovp_kernels.h"
#include "k_chol2.h"
#include "k_plane2.h"
#include "k_slam.h"
#include "k_dinit.h"
#include "k_plane_gen.h"
#include "ovp_lds_sizes.h"

extern "C" int ovp_dbg_tilechol_skip;
extern "C" {
hipError_t ovp_launch_scatter_gram_add(const double* Acc, const double* bcc, int cols, const int* col_ids, double* Ab, int lda, int n,
                                       hipStream_t stream);
hipError_t ovp_launch_scatter_gram(const double* Acc, const double* bcc, int cols, const int* col_ids, double* Ab,
                                   int lda, int n, hipStream_t stream);
hipError_t ovp_launch_gather_marginal(const double* P, int ldp, const int* cols, int m, double* out, hipStream_t stream);
hipError_t ovp_launch_gather_block(const double* P, int ldp, const int* ids, int m, double* out, int ldo, hipStream_t stream);
hipError_t ovp_launch_gather_block_boost(const double* P, int ldp, const int* ids, int m, double* out, int ldo, int from, double rel,
                                         double* boost, hipStream_t stream);
hipError_t ovp_launch_gather_block_unless(const double* P, int ldp, const int* ids, int m, double* out, int ldo, const int* cancel,
                                          hipStream_t stream);
hipError_t ovp_launch_unit_diag(const double* P, int n, int ld, double* C, double* dvec, hipStream_t stream);
hipError_t ovp_launch_unpermute_pair(const double* Pperm, const double* V, int ld, const int* ids, int n, double* Pout, double* Lout,
                                     int ldo, const int* cancel, const double* boost, hipStream_t stream);
hipError_t ovp_launch_factor_from_V(const double* V, int ld, const int* ids, int n, double* out, int ldo, hipStream_t stream);
hipError_t ovp_launch_scale_rows(double* L, int n, int ld, const double* dvec, hipStream_t stream);
hipError_t ovp_launch_gather_cols(const double* P, int ldp, const int* ids, int n, int m, double* G, int ldg, hipStream_t stream);
hipError_t ovp_launch_mat_sub(const double* A, const double* B, double* C, int rows, int cols, int ld, hipStream_t stream);
hipError_t ovp_launch_sub_sym(double* P, const double* D, int n, int ld, hipStream_t stream);
hipError_t ovp_launch_sub_sym_unless(double* P, const double* D, int n, int ld, const int* cancel, hipStream_t stream);
hipError_t ovp_launch_cov_clone(double* P, int ldp, int n_old, int src, int sz, double jitter, hipStream_t stream);
hipError_t ovp_launch_cov_marginalize(const double* src, double* dst, int ld, int n_old, int id, int sz,
                                      hipStream_t stream);
hipError_t ovp_launch_propagate(double* P, int ldp, int n, int start, int phi, const int* oldcol, int nold,
                                const double* Phi, const double* Q, double* CPT, double* PCP, int* negdiag,
                                hipStream_t stream);
hipError_t ovp_launch_propagate_publish(double* P, int ldp, int n, int start, int phi, const int* oldcol, int nold, const double* Phi,
                                        const double* Q, double* CPT, double* PCP, int* negdiag, unsigned* host_dev, unsigned seq,
                                        hipStream_t stream);
hipError_t ovp_launch_augment_dt(double* P, int ldp, int n, int pose, int dt, const double* d, hipStream_t stream);
hipError_t ovp_launch_init_invertible(double* P, int ldp, int n, const int* cols, int ncols, const double* HR, int k,
                                      double* Ma, const double* Hinv, const double* Rk, hipStream_t stream);
hipError_t ovp_launch_tilechol_unless(const double* A, double* L, double* Dinv, double* Lpack, int n, int ld, int* flag,
                                      int add_identity, const int* cond, hipStream_t stream);
hipError_t ovp_launch_tilechol(const double* A, double* L, double* Dinv, double* Lpack, int n, int ld, int* flag, int add_identity,
                               hipStream_t stream);
hipError_t ovp_launch_fwdsub_lead(const double* Ltp, const double* Dinv, const double* Lmat, double* V, int n, int ld, int dense,
                                  int n_lead, hipStream_t stream);
hipError_t ovp_launch_fwdsub(const double* Lt, const double* Dinv, const double* Lmat, double* V, int n, int ld,
                             int dense, hipStream_t stream);
hipError_t ovp_launch_gemm4(int transA, int transB, int M, int N, int K, const double* A, int lda, const double* B,
                            int ldb, double* C, int ldc, int add_identity, int symmetric, hipStream_t stream);
hipError_t ovp_launch_dx_rows_boost(double* P, int n, int ldp, const double* b, double* dx, int* negdiag, unsigned* ticket,
                                    void* res_block, void* host_block, int pub_words, void* seq_host, unsigned seq,
                                    const double* boost, int boost_n, const int* cancel, hipStream_t stream);
hipError_t ovp_launch_dx_rows(const double* P, int n, int ldp, const double* b, double* dx, int* negdiag,
                              unsigned* ticket, void* res_block, void* host_block, int pub_words, void* seq_host,
                              unsigned seq,
                              hipStream_t stream);
hipError_t ovp_launch_reduce_gram(const double* gramS, int n_clones, int n_chunks, double* gramR, hipStream_t stream);
hipError_t ovp_launch_plane_feat(const ovp::FeatParams* p, const ovp::PlaneParams* pp, int n_local, hipStream_t stream);
hipError_t ovp_launch_init_m(const double* P, int ldp, int n, const int* ids, int cols, const double* Ht, int m, double* Mall,
                             hipStream_t stream);
hipError_t ovp_launch_init_core(double* P, int ldp, int n, const int* ids, int cols, const double* Ht, int k, int rup, double* Mall,
                                const double* Hinv, const double* Rk, const double* resid, double r_iso, double thr, double* Linv,
                                double* y, double* res, hipStream_t stream);
hipError_t ovp_launch_init_update(const double* Psrc, double* Pdst, int ldp, int n2, const double* Mall, int m, int k, int rup,
                                  const double* Linv, const double* y, double* res, double* dx, hipStream_t stream);
// the same three behind a device-side predicate (k_init.hip *_sk; skip == nullptr: the plain kernels)
hipError_t ovp_launch_init_m_sk(const double* skip, const double* P, int ldp, int n, const int* ids, int cols, const double* Ht, int m,
                                double* Mall, hipStream_t stream);
hipError_t ovp_launch_init_core_sk(const double* skip, double* P, int ldp, int n, const int* ids, int cols, const double* Ht, int k,
                                   int rup, double* Mall, const double* Hinv, const double* Rk, const double* resid, double r_iso,
                                   double thr, double* Linv, double* y, double* res, hipStream_t stream);
hipError_t ovp_launch_init_update_sk(const double* skip, int res_len, const double* Psrc, double* Pdst, int ldp, int n2,
                                     const double* Mall, int m, int k, int rup, const double* Linv, const double* y, double* res,
                                     double* dx, hipStream_t stream);
hipError_t ovp_launch_gemm4c(int transA, int transB, int M, int N, int K, const double* A, int lda, const double* B, int ldb,
                             double* C, int ldc, int add_identity, int symmetric, const int* cancel, hipStream_t stream);
}


static const int OVP_TILECHOL_NMAX = 288;  // register-resident factorization limit (22 tiles per wave)

#define HIPCHK(x)                               \
  do {                                          \
    hipError_t _e = (x);                        \
    if (_e != hipSuccess) return (int)_e;       \
  } while (0)

static inline int round_up(int v, int m) { return ((v + m - 1) / m) * m; }

// What the second half of an information-form update (point_enqueue_tail, ovp_api_point.hip) runs on.  All zero = the plain tail: the
// Cholesky factor of P in c->L, T = I + L^T A L on all n columns, nothing to take off the diagonal.
struct PointTail {
  const double* factor = nullptr;  // some M with M M^T = P (+ diag(boost)); nullptr: c->L
  int nl = 0;                      // T is the identity outside its leading nl columns (reversed-order factor); 0: all n
  int dense = 0;                   // k_fwdsub's dense mode for `factor`
  const double* boost = nullptr;   // amounts the factorization added to the first boost_n diagonal entries: the last kernel takes them off
  int boost_n = 0;
};
// The half-done point update: the staged C-ABI returns between ovp_msckf_build_gate_gram_async, ovp_ekf_update_from_gram_async and
// ovp_msckf_fetch_results.  Written by those three only; all zero = nothing pending.
struct PointPending {
  PointTail tail;
  bool join_owed = false;  // chol(P) / K2 of the update finish on stream2 (ev_join): the tail waits for them first
  bool pub_armed = false;  // channel 0 of h_res_block is armed and a kernel of the update will post it (k_dx_rows)
  bool k1_timed = false;   // ev_k0 / ev_k1 bracket the update's K1 (dominant-kernel timer)
};
// A factor of the RESIDENT covariance left behind by the plane loop (P = V^T V, Lkeep = V^T in the state's column order): the point
// update that follows needs some M with M M^T = P, not the Cholesky factor, and skips chol(P).  boost: Lkeep is a factor of
// P + diag(boost_vec), the point update on it takes the amounts off at its end.  Written by the plane loop, cleared by everything
// that writes P (drop_kept_factor).
struct KeptFactor {
  bool have = false, boost = false;
};

// ------------------------------------------------------------------------------------------------
struct ovp_ctx {
  int device = 0;
  hipStream_t stream = nullptr, stream2 = nullptr;
  bool own_stream = false;
  OvpEvent ev_fork, ev_join;
  OvpEvent ev_t[6];
  int n_max = 0, c_max = 0, f_max = 0;
  int n = 0, ld = 0;  // current covariance size, leading dimension of every n x n buffer
  // Memory: every buffer the context owns is a DevBuf / PinnedBuf (ovp_buf.h), a Mailbox (ovp_mailbox.h) or a Staged (ovp_staged.h:
  // a host table's pinned and device halves) and goes with the context; a raw pointer below is a view into one of them and says
  // into which.
  DevBuf<double> P, P_tmp;
  // state tables: views into state_block's device half
  double *clone_R = nullptr, *clone_p = nullptr, *clone_R_fej = nullptr, *clone_p_fej = nullptr;
  int* clone_id = nullptr;
  double* cal = nullptr;  // [20] camera extrinsics / intrinsics values
  ovp::ColMap* colmap = nullptr;
  DevBuf<double> chi2_table;
  ovp::FeatParams fp;
  bool have_state = false, have_cov = false, have_batch = false;
  // feature batch: views into batch_block's device half (or into the feature database's batch, ovp_batch_bind_device)
  float* uv = nullptr;
  int *clone_idx = nullptr, *n_meas = nullptr;
  double* p_FinG = nullptr;
  int n_feats = 0, max_meas = 0;
  // work buffers
  DevBuf<double> G, rec, Bscr;
  double* chi2 = nullptr;           // views into res_block: flags, dx, chi2, accept
  unsigned char* accept = nullptr;
  int ldg = 0;
  DevBuf<double> gramS, gramR, part, Dinv, Ltp;
  int n_chunks = 0, rows_per_chunk = 0, n_split = 0;
  DevBuf<double> Ab;  // (n_max+1) x ld
  DevBuf<double> L, W1, T, Lt, Y;
  double* dx = nullptr;
  int* flags = nullptr;  // [0] not spd, [1] neg diag
  DevBuf<double> Hd, Acc, bcc, resd;  // dense-H path
  // ovp_msckf_dense_blocks: the information pair of the accepted dense blocks over the union of their columns, waiting for the
  // point update of the same frame (added to Ab behind K2); empty = none
  std::vector<int> dense_cols;
  std::vector<double> dense_A, dense_b;
  // general features (ovp_api_general.hip): camera tables of ovp_cameras_upload (host copy + device [OVP_MAX_CAMERAS][20] in the
  // layout of `cal`) and the device scratch of ovp_msckf_general_features / ovp_triangulate_general
  int gen_ncams = 0;
  int gen_calib_id[OVP_MAX_CAMERAS] = {-1, -1, -1, -1}, gen_intr_id[OVP_MAX_CAMERAS] = {-1, -1, -1, -1};
  int gen_fisheye[OVP_MAX_CAMERAS] = {0, 0, 0, 0};
  double gen_cal_h[OVP_MAX_CAMERAS * 20] = {};
  DevBuf<double> gen_cal;
  DevBuf<void> gen_buf;
  DevBuf<void> slam_res;           // ovp_slam_update: per-landmark [chi2 | status]
  DevBuf<double> slam_hscr;        // ... blocks that do not fit LDS
  DevBuf<double> dinit_buf;        // ovp_slam_delayed_init: result blocks + shared scratch of the candidate loop
  size_t dinit_pltab_off = 0;      // ovp_slam_delayed_init_planes: the plane table of the last call inside pl_stage (debug read)
  int dinit_nplanes = 0;
  // ovp_slam_update: shape of what the last call left in Hd / resd / smallbuf (debug reads "slam_Ht", "slam_res", "slam_M",
  // "slam_cols", "slam_dims"); sform: the S-form ran, so M_all stands at slam_dbg_M (doubles into smallbuf), [n][m_total];
  // h_in_lds: the gate kept a landmark's block in LDS.  Zero from the entry of a call until its plan and staging have succeeded.
  int slam_dbg_rows = 0, slam_dbg_n = 0, slam_dbg_h_in_lds = 0;
  bool slam_dbg_sform = false;
  size_t slam_dbg_M = 0;
  std::vector<int> slam_dbg_cols;
  int calib_id = -1, intr_id = -1;
  DevBuf<long long> dbg_cycles;
  // plane path
  std::vector<int> h_n_meas, h_clone_idx;  // host copies of the uploaded batch (plane grouping is host logic)
  // plane loop (k_plane2.hip / k_chol2.hip): constraint-row moments, the range part's normalised pair, gate scalars, per-plane results
  DevBuf<double> pl_cst, pl_An, pl_bn, pl_scal;
  DevBuf<double> pl_res, pl_dx;
  DevBuf<double> pl_Tbuf, pl_crow, pl_dxlast;
  DevBuf<int> pl_cur;
  DevBuf<unsigned> pl_range_done;
  unsigned pl_seq = 0;
  int range_lo = -1, range_hi = -1;   // ovp_batch_set_range (-1, -1 = whole batch)
  DevBuf<unsigned char> pl_used;      // [f_max] features consumed by accepted planes (device)
  std::vector<unsigned char> h_pl_used;  // host copy of it behind the last plane loop (ovp_msckf_update_sharded splits the leftovers)
  PinnedBuf<int> h_slot{true};        // [f_max] host-mapped: row block of a feature in the compacted rec / G of a point update (-1: none)
  bool pl_used_valid = false;         // pl_used refers to the uploaded batch
  // plane loop on a sub-state (n above the tile factorization's limit): accumulated pair, u rows, remapped id tables
  Staged io;                                     // ovp_io_arena: pinned host block + device block of the small entry points
  DevBuf<double> pl_xbuf, pl_xy;                 // split plane solve: exported panels, [xzz(2) | y blocks]
  DevBuf<unsigned> pl_xflag;                     // [32 step flags | 2 sync words]
  DevBuf<double> pl_Asum, pl_U;
  DevBuf<double> pl_init_keep;                   // ovp_plane_init_general: [plane][3][nk + 4] plane rows of the extended pairs of the call
  DevBuf<int> pl_init_slot;                      // ... and the numbering of its accepted planes (k_plane_init2.hip)
  Staged pl_sub_tab;                             // [ids | inverse | clone ids | column map] of the loop's column order
  // (what tells the plane loop's routes apart is an argument of the loop, PlaneLoopView in ovp_api_plane.hip, not context state)
  DevBuf<void> pl_gen_dev;                 // device: [marks | projected rows] of one plane's general features of the running loop
  DevBuf<double> Lkeep;
  KeptFactor kept;
  double clone_jitter = 0.0;  // ovp_cov_clone_jitter: relative inflation of a cloned block's diagonal (0 = exact copy, the reference)
  DevBuf<double> boost_vec;  // [n_max] k_gather_block_boost: the plane loop's diagonal boost by STATE column (zero where none)
  DevBuf<double> boost;   // CholJob::boost: the amounts the reversed-order chol(P) added to the diagonal in front of the batch's columns
  // (what tells the point update's routes apart is a PointPlan, ovp_point_plan.h; what its second half needs of it is `point`)
  PointPending point;
  int point_route[8] = {-1, 0, 0, 0, 0, 0, 0, 0};  // the last point update's plan (ovp_debug_read "point_route"); [0] < 0: none yet
  Staged pl_stage;                    // the per-call tables of the plane loop, the point update's sub-state and the SLAM entries
  Mailbox pl_hres;                    // the plane results and the small fetches (ovp_fetch_to_hres): payload from byte 0, channel 0
  // the pose tables and the feature batch (a single copy per upload, an event behind it: the uploads do not wait)
  Staged state_block, batch_block;
  size_t state_bytes = 0;
  size_t so_R = 0, so_Rf = 0, so_p = 0, so_pf = 0, so_cal = 0, so_id = 0, so_cm = 0;
  int pl_ktimer = 0;  // 1 = events around every k_chol2 launch and around the loop, 2 = around the loop only
  std::vector<OvpEvent> pl_ev, pl_ev_loop;
  double pl_ktime_ms = 0.0;
  int pl_klaunches = 0;
  DevBuf<int> idbuf;         // scratch ints (ids)
  DevBuf<double> smallbuf;   // scratch doubles (Phi, Q, CPT, PCP, marginal)
  // sub-state update (n above the tile factorization's limit): involved state columns and six ns x ns scratch matrices
  DevBuf<int> sub_ids;
  int sub_ns = 0;
  std::vector<int> h_clone_id;  // host copy of the clone columns (ovp_state_upload)
  DevBuf<double> sub_buf;
  // pinned host staging: views into h_res_block's payload
  double *h_dx = nullptr, *h_chi2 = nullptr;
  unsigned char* h_accept = nullptr;
  int* h_flags = nullptr;
  DevBuf<void> res_block;                             // [flags | dx | chi2 | accept]
  Mailbox h_res_block;                                // ... its pinned mirror; channel 0: the point update, channel 1: ovp_cov_propagate,
                                                      // channel 2: ovp_zupt_update, whose block [head 8 | dx n_max] starts at zupt_res_off
  size_t zupt_res_off = 0;
  DevBuf<unsigned> ticket;       // block counter of the publishing kernel
  std::vector<int> h_nmeas;                           // host copy of n_meas of the current batch (row count of `info`)
  bool h_nmeas_valid = false;
  size_t res_bytes = 0;
  float last_ms[4] = {0, 0, 0, 0};
  bool timed = false;
  // dominant-kernel timer
  bool ktimer = false;
  OvpEvent ev_k0, ev_k1;
  double ktime_ms = 0.0;
  int klaunches = 0;
  // host-side clock of the two update entry points, accumulated (ovp_host_timing): plane loop [entry -> first launch | entry -> last
  // launch enqueued | wait for the device | calls], point update [enqueue | wait | calls]
  double host_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  std::shared_ptr<void> plane_det;  // ovp_plane_detector_create (k_plane_detect.hip): the detector and its buffers, freed with the context
  std::shared_ptr<void> delaunay_io;  // ovp_delaunay_device (k_plane_detect.hip): its staging and mailbox, made on first use
  std::shared_ptr<void> active_tracks;  // ovp_active_tracks_create (k_active_tracks.hip): the slot table, its staging and mailbox, freed with the context
  std::shared_ptr<void> retire;  // ovp_cov_marginalize_many / ovp_planes_merge_retire (k_retire.hip): their staging, scratch and mailbox, made on first use
  std::shared_ptr<void> zupt;    // ovp_zupt_update (ovp_api_ctx.hip, k_zupt.hip): its staging and device blocks, made on first use
  std::shared_ptr<void> klt;     // ovp_klt_create (k_klt.hip): the two image pyramids, staging, result block and mailbox, freed with the context
  std::shared_ptr<void> featdb;  // ovp_featdb_create (k_featdb.hip): the track table, the gathered batch, staging and mailbox, freed with the context
  std::shared_ptr<void> prop;    // ovp_propagate_and_clone (ovp_api_ctx.hip, k_propagate.hip): its staging, result block and mailbox, made on first use

  ovp_ctx() = default;
  ovp_ctx(const ovp_ctx&) = delete;
  ovp_ctx& operator=(const ovp_ctx&) = delete;
  ~ovp_ctx() {  // the streams; the events and the buffers free themselves behind this
    if (stream2) (void)hipStreamDestroy(stream2);
    if (own_stream && stream) (void)hipStreamDestroy(stream);
  }
};

// The calibration columns an update estimates (ovp_update_opts): bit k of `mask` = column k of a camera's [extrinsics 6 |
// intrinsics 8]; col[] = camera 0's state columns (ovp_state_upload; 0 where not estimated), col_of = those of an uploaded camera.
struct CalCols {
  const ovp_ctx* c;
  unsigned mask;
  int ncal, col[14];
  CalCols(const ovp_ctx* ctx, const ovp_update_opts* o)
      : c(ctx), mask((o->do_calib_camera_pose ? 0x3Fu : 0u) | (o->do_calib_camera_intrinsics ? (0xFFu << 6) : 0u)),
        ncal(__builtin_popcount(mask)) {
    for (int k = 0; k < 14; ++k) col[k] = on(k) ? (k < 6 ? c->calib_id + k : c->intr_id + (k - 6)) : 0;
  }
  bool on(int k) const { return (mask >> k) & 1u; }
  int col_of(int cam, int k) const { return k < 6 ? c->gen_calib_id[cam] + k : c->gen_intr_id[cam] + (k - 6); }
  // every estimated column lies in a state of n columns: camera 0's, or (general) those of every uploaded camera
  int check(int n, bool general) const {
    for (int cam = 0; cam < (general ? c->gen_ncams : 1); ++cam)
      for (int k = 0; k < 14; ++k) {
        const int id = general ? col_of(cam, k) : col[k];
        if (on(k) && (id < 0 || id >= n)) return OVP_E_ARG;
      }
    return 0;
  }
  void fill(ovp::FeatParams& fp) const {
    fp.calmask = mask;
    for (int k = 0; k < 14; ++k) fp.calcol[k] = col[k];
  }
  // the uploaded cameras' tables into a general parameter struct (SlamGenParams, DinitGenParams, GenParams: and where their
  // calibration columns start)
  template <class GP>
  void fill_cameras(GP& gp) const {
    gp.cam_cal = c->gen_cal;
    for (int k = 0; k < OVP_MAX_CAMERAS; ++k) gp.cam_fisheye[k] = c->gen_fisheye[k];
  }
  template <class GP>
  void fill_cameras_and_columns(GP& gp) const {
    fill_cameras(gp);
    for (int k = 0; k < OVP_MAX_CAMERAS; ++k) gp.cam_calib_id[k] = c->gen_calib_id[k], gp.cam_intr_id[k] = c->gen_intr_id[k];
  }
};

// ext FeatureInitializerOptions and the context's clone and calibration tables into the triangulation kernel's arguments; the
// batch (uvn, clone_idx, n_meas, sizes) and the outputs are the caller's.  ovp_triangulate and ovp_featdb_triangulate share it.
static inline void fill_tri_params(ovp::TriParams& tp, const ovp_ctx* c, const ovp_triang_opts* o) {
  tp.clone_R = c->clone_R;
  tp.clone_p = c->clone_p;
  tp.cal = c->cal;
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
}

// Everything that writes the covariance calls this: the factor the plane loop left (Lkeep) and the tail of a staged point update
// that was built but never applied (set by ovp_msckf_build_gate_gram_async) no longer belong to P.
static inline void drop_kept_factor(ovp_ctx* c) {
  if (!c) return;
  c->kept = KeptFactor();
  c->point.tail = PointTail();
  c->dense_cols.clear();  // (a pending dense pair was gated against the covariance that is being replaced)
}

// StateHelper::EKFUpdate takes the information form whatever the size (ovp_ekf_update, ovp_slam_update); read per call: the tests
// run both forms in one process
static inline bool ekf_info_form_only() {
  const char* form_env = getenv("OVP_EKF_INFO_FORM");
  return form_env && form_env[0] == '1';
}

static inline double host_now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}


// ---- shared between the entry-point files ------------------------------------------------------------------------------------
void quat_2_rot(const double q[4], double R[9]);  // JPL quaternion -> row-major rotation (ovp_api_ctx.hip)
extern "C" int ovp_io_arena(ovp_ctx* c, size_t bytes, void** host, void** dev);  // pinned staging arena (ovp_api_ctx.hip)
// ovp_api_point.hip
int fill_feat_params(ovp_ctx* c, const ovp_update_opts* o);
// ovp_api_general.hip: argument checks of a general batch against the context's tables (host only); only != nullptr: features with
// only[f] == 0 are not looked at
// any_length: the batch of ovp_plane_fit_refine - uv is not read and n_meas is bounded by max_meas only
int check_general_batch(const ovp_ctx* c, const ovp_general_batch* b, bool need_p, const int* only = nullptr, bool any_length = false);
int ovp_fetch_to_hres(ovp_ctx* c, const void* dsrc, size_t bytes, hipStream_t s);  // device block -> c->pl_hres, waited for (ovp_api_plane.hip)
int chol_of_P(ovp_ctx* c, hipStream_t s, bool psd = false);  // psd: pivot-dropping factor of a positive semi-definite P (plane path)
hipError_t chol_of_T(ovp_ctx* c, const double* T, int n, int ld, int add_identity, const int* cond, hipStream_t s);
int set_substate(ovp_ctx* c, const std::vector<int>& ids);
int ekf_from_gram(ovp_ctx* c, const PointTail& t);  // chol(P) on the main stream, then the update on the pair in c->Ab
int ekf_sform(ovp_ctx* c);
// ovp_api_plane.hip
int plane2_buffers(ovp_ctx* c, size_t stage_bytes, size_t res_bytes);
