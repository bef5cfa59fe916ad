// Kernel parameter blocks and launch prototypes (internal to libovplane_hip.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define OVP_MAX_MEAS_DEV 32
#define OVP_CHI2_TABLE 1024  // chi2_table[k] for k = 0..OVP_CHI2_TABLE (k=0 unused)
#define OVP_MAX_CLONES 64
#define OVP_GRAM_ELEMS 231   // 21*22/2: packed upper triangle of the per-clone 21x21 Gram
#define OVP_TC_MAX_TILES 18  // tile rows the register-resident Cholesky handles (N <= 288)
#define OVP_FEAT_CHOL_MAX_MEAS 30  // observations per feature the fused feature kernel takes (ovp_feat_chol_supported; the point planner's limit)
#define OVP_BSCR 2112        // doubles of per-feature scratch for B (k_feat.hip LCOLS)
// Plane-level gate (k_chol2.hip): weight of the expected energy of the reference's rounding-decided rows; 1 = the plain
// expectation (rounds 2-5: +0.35 +- 0.06 above the mean of four roundings of the oracle).  Round 6: the weight that zeroes that
// difference on 1000 planes of config 3's shape is 0.9606 (in-state planes alone 0.9614, out-of-state 0.9598, least squares 0.9598);
// on the 350 held-out planes of configs 3 and 4 it leaves +0.01 +- 0.13 (profiles/r06_plane_gate_kappa_fit.json,
// tools/plane_gate_agreement.py --fit; NOTES.md 3b)
#define OVP_PLANE_NOISE_KAPPA 0.96
#define OVP_LDG_CAP 704      // max leading dimension of the projector-row buffer G (LDS staging in the feature kernels)

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a per-DEVICE setting: a process that drives contexts on several GPUs (one
// filter per device) must raise the limit on each of them.  Launchers keep one mask per kernel family; true = this device has not
// been set up yet (the caller sets the attributes, checks the return codes, and calls ovp_lds_attr_done on success).
static inline int ovp_lds_attr_device() {
  int dev = 0;
  return hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64 ? dev : -1;
}
static inline bool ovp_lds_attr_needed(const unsigned long long* mask) {
  const int dev = ovp_lds_attr_device();
  return dev < 0 || !((*mask >> dev) & 1ull);
}
static inline void ovp_lds_attr_done(unsigned long long* mask) {
  const int dev = ovp_lds_attr_device();
  if (dev >= 0) *mask |= 1ull << dev;
}

namespace ovp {

// chol(P) riding in workgroup 0 of the fused feature kernel (k_feat.hip): A = L L^T, Dinv = inverse diagonal blocks,
// Lpack = tile-packed factor (see k_tile.hip)
struct CholJob {
  const double* A;
  double* L;
  double* Dinv;
  double* Lpack;
  int n, ld;
  int* flag;
  int flip;  // dense factor of the index-reversed matrix, rows reversed back (k_tile_body.h): L = Lr with Lr Lr^T = A
  // flip only: the diagonal of the first boost_n state columns (the ones in front of the batch's columns: IMU, dt) is read as
  // (1 + boost_rel) x its value and the added amounts are left in boost[0 .. boost_n).  An update whose information matrix is zero
  // on those columns returns exactly P+ + diag(boost) there (H D = 0  =>  (P + D)+ = P+ + D), so the caller subtracts them again:
  // the result is the exact update, and the exact stochastic clone - IMU pose == newest clone, a zero pivot in exactly these
  // columns of the reversed order - factors without a fallback.
  double* boost;
  int boost_n;
  double boost_rel;
};

struct FeatParams {
  // feature batch (device pointers)
  const float* uv;
  const int* clone_idx;
  const int* n_meas;
  const double* p_FinG;
  int n_feats, max_meas;
  // state tables (device pointers)
  const double* clone_R;      // [C][9] row-major R_GtoI
  const double* clone_p;      // [C][3]
  const double* clone_R_fej;  // [C][9]
  const double* clone_p_fej;  // [C][3]
  const int* clone_id;        // [C]
  int n_clones;
  int do_fej;
  int fisheye;        // 0 = radtan, 1 = equidistant (ext CamEqui) camera model
  const double* cal;  // device: [0..8] R_ItoC row-major, [9..11] p_IinC, [12..19] fx fy cx cy k1 k2 p1 p2 (k1..k4 when fisheye)
  int calcol[14];  // state column of calibration column k: k<6 extrinsics, k>=6 intrinsics
  unsigned calmask;  // bit k set = calibration column k is estimated
  double white_px, chi2_mult;
  const double* chi2_table;
  const double* P;
  int n, ldp;
  // outputs
  double* G;  // [3*n_feats][ldg]: columns 0..n-1 = Q1^T H_x scattered to state columns, column n = Q1^T r
  int ldg;
  double* Bscr;  // [n_feats][OVP_BSCR] scratch: per-feature B = H_x P H_x^T + I (packed lower triangle)
  double* rec;  // [n_clones][n_feats][2][OVP_REC]
  double* chi2;
  unsigned char* accept;
  const unsigned char* skip;  // optional [n_feats]: 1 = feature was consumed by an accepted plane (not part of this update)
  int range_lo, range_hi;     // features outside [range_lo, range_hi) are not part of this update (another rank's shard)
  long long* dbg_cycles;  // optional [n_feats][8] phase stamps (diagnostics)
  // compacted outputs (round 5): slot[f] = row block of feature f in rec / G, or -1 = the feature is not part of this update (consumed
  // by a plane, another rank's share) and writes nothing; rec is then [n_clones][n_out][2][OVP_REC], G [3 n_out][ldg].  NULL: slot = f,
  // n_out = n_feats.  The array may live in host-mapped memory (read once per feature wave, long before it is needed).
  const int* slot;
  int n_out;
};

// arguments of the triangulation kernel (ext FeatureInitializerOptions + the feature batch + the clone tables)
struct TriParams {
  const float* uvn;  // [n_feats][max_meas][2] normalised measurements (Feature::uvs_norm)
  const int* clone_idx;
  const int* n_meas;
  int n_feats, max_meas;
  const double* clone_R;  // [C][9] row-major R_GtoI (current estimates)
  const double* clone_p;  // [C][3]
  const double* cal;      // [0..8] R_ItoC, [9..11] p_IinC
  int refine_features, max_runs;
  double init_lamda, max_lamda, min_dx, min_dcost, lam_mult, min_dist, max_dist, max_baseline, max_cond_number;
  int triangulate_1d;
  double* p_FinG;         // [n_feats][3] out
  unsigned char* ok;      // [n_feats] out
};

// arguments of the general-feature kernels (k_feat_gen.hip): any camera per observation, up to OVP_GEN_MAX_MEAS_DEV observations
#define OVP_GEN_MAX_MEAS_DEV 64
#define OVP_GEN_MAX_CAMS 4
struct GenParams {
  FeatParams fp;              // clone tables, do_fej, white_px, calmask; cal / fisheye / uv / p_FinG are set per observation
  const double* cam_cal;      // [OVP_GEN_MAX_CAMS][20] per camera, the layout of FeatParams::cal
  int cam_fisheye[OVP_GEN_MAX_CAMS];
  int cam_calib_id[OVP_GEN_MAX_CAMS], cam_intr_id[OVP_GEN_MAX_CAMS];
  // the batch (device)
  const float* uv;
  const int* clone_idx;
  const int* cam_idx;
  const int* n_meas;
  const double* p_FinG;
  int n_feats, max_meas;
  // gate
  const double* P;
  int ldp;
  const double* chi2_table;
  double chi2_mult;
  // projected rows of the accepted features: the union of the involved state columns is numbered 0..nu-1 (upos[state column], -1 =
  // not involved); feature f owns q[f] of them, local column loc[f * nu + u] (-1 = not its column), and the block hp + hp_off[f]:
  // Hp [2m x q[f]] column-major, then the projected residual [2m]
  const int* upos;
  const int* loc;
  const int* q;
  const long long* hp_off;
  int nu;
  double* hp;
  double* chi2;          // [n_feats] out
  unsigned char* accept;  // [n_feats] out
};

// per-plane arguments of the plane feature kernel
struct PlaneParams {
  const int* feat_list;  // [n_local] indices into the feature batch
  int n_local;
  int plane;             // 0-based plane slot
  int in_state;          // plane is a state variable (State::_features_PLANE)
  int plane_sid;         // its Type::id(), or -1
  double white_c;        // 1 / sigma_constraint
  const double* cp;      // [n_planes][3] current closest-point estimates
  const double* cp_fej;  // [n_planes][3]
  double* cst;           // [n_local][10] constraint-row moments
};

// per-column description of the state used when assembling the information pair
struct ColMap {
  // kind: 0 = not involved, 1 = clone column, 2 = calibration column
  int kind;
  int idx;  // clone slot, or calibration column k (0..13)
  int off;  // offset inside the clone block (0..5)
  int pad;
};

// ovp_plane_fit_refine (k_planefit.hip): every pointer is device memory.  Features / planes / observation items are counted over the
// whole call: F = feat_start[n_planes], O = sum of n_meas.
struct PlaneFrontJob {
  int n_planes, n_free;         // planes of the call; free planes among them (the RANSAC's grid)
  int n_clones, n_cams, max_meas;
  int refine;                   // 0: poses + RANSAC only
  // pose table
  const double* clone_R;        // [n_clones][9] R_GtoI
  const double* clone_p;        // [n_clones][3] p_IinG
  const double* cam_cal;        // [n_cams][20]: R_ItoC (9), p_IinC (3), intrinsics
  double* poses;                // [n_clones][n_cams][12] out: R_GtoC, p_CinG
  // RANSAC over the free planes (compacted: free plane r owns the points [rs_feat_start[r], rs_feat_start[r+1]))
  const int* rs_feat_start;     // [n_free + 1]
  const double* rs_pts;         // [free features][3]
  const int* rs_sets;           // [n_free][200][5]
  int min_inlier_num;
  double max_cond;
  double* rs_abcd;              // [n_free][4] out
  unsigned char* rs_inlier;     // [free features] out
  unsigned char* rs_ok;         // [n_free] out
  // link
  const int* feat_start;        // [n_planes + 1]
  const int* free_slot;         // [n_planes] index among the free planes, -1 = in-state plane
  const int* n_meas;            // [F]
  const int* clone_idx;         // [F][max_meas]
  const int* cam_idx;           // [F][max_meas]
  const float* uvn;             // [F][max_meas][2]
  const double* p_in;           // [F][3]
  const double* cp_in;          // [n_planes][3]
  const unsigned char* fix_plane;  // [n_planes]
  int* c_feat_start;            // [n_planes + 1] the refinement's lists: compacted features ...
  double* c_p0;                 // [F][3]
  int* c_n_obs;                 // [F]
  int* c_src;                   // [F] input index of a compacted feature
  int* item_start;              // [n_planes + 1] ... and observation items
  int* item_ob;                 // [O]
  int* item_lf;                 // [O]
  int* feat_item0;              // [F]
  double* it_uv;                // [O][2]
  double* it_R;                 // [O][9]
  double* it_p;                 // [O][3]
  double* cp0;                  // [n_planes][3]
  // refinement
  double sigma_px_norm, sigma_c;
  double R_GtoC[9], p_CinG[3];  // current camera
  double* cp_out;               // [n_planes][3]
  double* c_p_out;              // [F][3] compacted index
  unsigned char* c_kept;        // [F] compacted index
  unsigned char* ok;            // [n_planes]
  int* iterations;              // [n_planes]
};

// ovp_zupt_update (k_zupt.hip).  The head of the call's staged block; the readings [n_readings][7] follow on the next 64-byte line.
struct ZuptParams {
  double bg[3], ba[3];
  double Rg[3];          // R_GtoI g (the residual's rotation)
  double S3[9];          // skew(R_jac g) row-major (the Jacobian's rotation: the first estimate with do_fej)
  double d_w, d_a;       // D: 1 / (mult sigma_w^2), 1 / (mult sigma_a^2)
  double q_wb, q_ab;     // Q_bias / T: sigma_wb, sigma_ab
  double thr;            // chi2_multipler * quantile(6 (n - 1))
  int n_readings, imu_id, vel_ok, disparity_passed;
};
// the device blocks of a call, in doubles.  Result (published to the host): [accepted | chi2 | rows | negative diagonal | not spd |
// - - -] and dx [n] behind it.  Work: Lbar (6 x 6 lower, row-major), z, H0 (6 x 9), the diagonal of Q_bias, G = H0^T Lbar^-T (9 x 6).
#define OVP_ZUPT_RES_HEAD 8
#define OVP_ZW_L 0
#define OVP_ZW_Z 36
#define OVP_ZW_H0 42
#define OVP_ZW_Q 96
#define OVP_ZW_G 102
#define OVP_ZW_DOUBLES 160

// ovp_propagate_and_clone (k_propagate.hip).  The head of the call's staged block; the readings [n_readings][7] follow on the next
// 64-byte line.
struct PropParams {
  double q[4], p[3], v[3], bg[3], ba[3];
  double q_fej[4], p_fej[3], v_fej[3];
  double g;                        // gravity magnitude (along +z of the global frame)
  double sw2, sa2, swb2, sab2;     // squared continuous-time densities (NoiseManager::with_squares)
  int n_readings, use_rk4, imu_avg, do_fej;
};
// the device result block of a call, in doubles: [q 4 | p 3 | v 3 | last_w 3 | - 3 | Phi 225 | Q 225 | verdict | intervals]; Phi, Q
// column-major 15 x 15.  dnc_dt of the time-offset term is [last_w ; v] of this block, read where it lies.
#define OVP_PR_Q 0
#define OVP_PR_P 4
#define OVP_PR_V 7
#define OVP_PR_LW 10
#define OVP_PR_PHI 16
#define OVP_PR_QS 241
#define OVP_PR_VERDICT 466
#define OVP_PR_NI 467
#define OVP_PR_DOUBLES 468

}  // namespace ovp

extern "C" {
// k_zupt.hip: gate, rows and apply of one ovp_zupt_update, enqueued on `stream` with nothing waiting in between; the last step
// copies OVP_ZUPT_RES_HEAD (+ n when accepted) doubles of res into host_block and stores seq into *word.  ticket: one zeroed word
// the apply kernel counts its workgroups in and clears again.  ev: nullptr, or four events recorded around the three kernels.
hipError_t ovp_launch_zupt(double* P, int ld, int n, int imu_id, const ovp::ZuptParams* zp, const double* readings, double* work,
                           double* Y, double* res, unsigned* ticket, void* host_block, unsigned* word, unsigned seq, hipEvent_t* ev,
                           hipStream_t stream);
// k_propagate.hip.  ovp_launch_prop_integrate: the IMU window of one ovp_propagate_and_clone into the mean, last_w, Phi and Q of
// `res` (one workgroup, intervals in order).  ovp_launch_prop_clone_dt: the exact copy of the pose block [src, src + 6) appended at
// n (jitter as ovp_launch_cov_clone) and, with dt >= 0, the time-offset term of ovp_launch_augment_dt on the new block with
// dnc_dt = [last_w ; v] read from res.  ovp_launch_prop_finish: res[VERDICT] from *negdiag (cleared), the block into host_block,
// seq into *word.
hipError_t ovp_launch_prop_integrate(const ovp::PropParams* pp, const double* readings, double* res, hipStream_t stream);
// ... ovp_launch_prop_cov15: StateHelper::EKFPropagation on the 15 contiguous columns at imu with Phi, Q of res; CPT: n x 15
// doubles of scratch; the 15 x 15 block comes out symmetric to the bit; *negdiag is set on a negative diagonal element
hipError_t ovp_launch_prop_cov15(double* P, int ld, int n, int imu, const double* res, double* CPT, int* negdiag, hipStream_t stream);
hipError_t ovp_launch_prop_clone_dt(double* P, int ld, int n, int src, int dt, double jitter, const double* res, hipStream_t stream);
hipError_t ovp_launch_prop_finish(double* res, int* negdiag, void* host_block, unsigned* word, unsigned seq, hipStream_t stream);
// k_publish.hip: `bytes` of the device block src -> dst (mapped pinned memory), then seq into *word; src, dst 8-byte aligned;
// clear8 leading 8-byte words of src are zeroed behind the post
hipError_t ovp_launch_publish_block(const void* src, void* dst, size_t bytes, unsigned* word, unsigned seq, int clear8,
                                    hipStream_t stream);
// k_planefit.hip: the device sequence of ovp_plane_fit_refine, enqueued on `stream`; the hypothesis sets of one plane's RANSAC
// (PlaneFitting.cpp:104-141; dst [200][5], -1 = the call fails at that iteration)
hipError_t ovp_launch_planefront(const ovp::PlaneFrontJob* j, hipStream_t stream);
void ovp_planefit_sets(const double* pts, int n, int min_inlier_num, int shuffle_variant, int* dst);
hipError_t ovp_launch_feat_gate(const ovp::FeatParams* p, hipStream_t stream);
int ovp_feat_chol_supported(const ovp::FeatParams* p, int n);
int ovp_feat_chol_side_capacity(void);
hipError_t ovp_launch_feat_chol(const ovp::FeatParams* p, const ovp::CholJob* c, hipStream_t stream);
hipError_t ovp_launch_triangulate(const ovp::TriParams* p, hipStream_t stream);
// general batch: cam_idx [n_feats][max_meas], p->cal = [OVP_GEN_MAX_CAMS][20] camera tables (k_triang.hip)
hipError_t ovp_launch_triangulate_gen(const ovp::TriParams* p, const int* cam_idx, hipStream_t stream);
// k_feat_gen.hip: rows + projection + gate of every feature of a general batch, then the information pair of the accepted ones
// over the union of their columns: A [nu x nu], b [nu]
hipError_t ovp_launch_feat_gen(const ovp::GenParams* g, hipStream_t stream);
hipError_t ovp_launch_gen_pair(const ovp::GenParams* g, double* A, double* b, hipStream_t stream);

// K2a: per-clone structured Gram of the sparse rows. gramS [n_clones][n_chunks][OVP_GRAM_ELEMS]
hipError_t ovp_launch_struct_gram(const double* rec, int n_clones, int n_feats, int rows_per_chunk, int n_chunks,
                                  double* gramS, hipStream_t stream);
// K2b: split-K lower-triangular SYRK of G ([rows][ldg]) with f64 MFMA. part [n_split][nt*(nt+1)/2][256]
hipError_t ovp_launch_gram_pair(const double* rec, int n_clones, int n_feats, int rows_per_chunk, int n_chunks,
                                double* gramS, const double* G, int rows, int ldg, int ncols, int n_split_cap,
                                double* part, int* n_split_used, hipStream_t stream);
hipError_t ovp_launch_syrk(const double* G, int rows, int ldg, int ncols, int n_split, double* part,
                           hipStream_t stream);
// K2c: assemble A|b (Ab [(n+1)][lda], row n = b) from the structured Gram and the SYRK partials
hipError_t ovp_launch_assemble(const double* gramS, int n_clones, int n_chunks, const double* part, int n_split,
                               const ovp::ColMap* colmap, int n, double* Ab, int lda, hipStream_t stream);

// K3 building blocks (all matrices row-major == column-major for symmetric ones; ld explicit)
// blocked Cholesky of the n x n SPD matrix A into lower L (both [n][ld]); flag set to 1 on a non-positive pivot
hipError_t ovp_launch_chol(const double* A, double* L, int n, int ld, int* flag, int add_identity,
                           hipStream_t stream);
// C[M][N] = alpha * op(A) * op(B) + beta_identity * I ; op = N or T; sizes given for the result
hipError_t ovp_launch_gemm(int transA, int transB, int M, int N, int K, const double* A, int lda, const double* B,
                           int ldb, double* C, int ldc, int add_identity, hipStream_t stream);
// Y * Lt^T = L  ->  Y = L * Lt^-T  (row-wise forward substitution), all [n][ld]
hipError_t ovp_launch_trsm_right_lt(const double* L, const double* Lt, double* Y, int n, int ld, hipStream_t stream);
// P = Y Y^T (symmetric), dx = P * b, neg-diag flag
hipError_t ovp_launch_cov_finish(const double* Y, int n, int ld, const double* b, double* P, int ldp, double* dx,
                                 int* negdiag, hipStream_t stream);
}
