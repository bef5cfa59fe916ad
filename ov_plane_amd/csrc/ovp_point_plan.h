// The host decisions of the point update (ovp_api_point.hip) in front of anything that touches the device: which features own rows,
// the sub-state's columns, which feature launch runs, where chol(P) runs, the reversed-order factor with its leading block and diagonal
// boost, K2's geometry and what the second half of the update needs to know about all that.  Pure: no HIP header, no ovp_* call, no
// ovp_ctx - what the plan reads from the context, the options and the environment arrives as a PointEnv.  plan_point_update writes
// its output struct and the caller's slot array, nothing else.
// Stand-alone under ASan / UBSan: tests/point_plan_main.cpp.
#pragma once
#include <algorithm>
#include <vector>

// OVP_OVERLAP_MODE (3 or 4, anything else - 0 where unset - is the default), OVP_POINT_NO_FLIP, OVP_POINT_NO_BOOST
struct PointSwitches {
  int overlap = 0;
  bool no_flip = false, no_boost = false;
};

struct PointEnv {
  int n = 0, F = 0, max_meas = 0;
  const int* clone_id = nullptr;  // [n_clones] first column of every clone
  int n_clones = 0;
  unsigned calmask = 0;  // bit k = column k of camera 0's [extrinsics 6 | intrinsics 8] is estimated
  int calib_id = -1, intr_id = -1;
  const int* dense_cols = nullptr;  // columns of the pending dense pair (ovp_msckf_dense_blocks)
  int n_dense = 0;
  int range_lo = -1, range_hi = -1;           // ovp_batch_set_range (lo < 0: whole batch)
  const unsigned char* used = nullptr;        // [F] host copy of the consumed-feature mask ...
  bool used_valid = false;                    // ... asked for (skip_plane_used) and belonging to this batch
  bool have_factor = false, factor_boosted = false;  // the plane loop left a factor of P / of P + diag(its boost)
  int rows_per_chunk = 1, n_split = 1;               // K2's chunking of the context
  // device-side limits, filled in by the entry
  int tilechol_nmax = 0;      // OVP_TILECHOL_NMAX
  int chol2_max_n = 0;        // ovp_chol2_max_n()
  int fused_max_tiles = 0;    // tile rows / observations per feature the fused feature kernel takes (ovp_feat_chol_supported)
  int fused_max_meas = 0;
  int side_capacity = 0;      // ovp_feat_chol_side_capacity()
  PointSwitches sw;
};

enum PointK1 {          // the feature launch
  K1_FUSED_CHOL = 0,    // eight feature waves per workgroup, chol(P) in workgroup 0
  K1_FUSED_IDLE = 1,    // the same shape, workgroup 0 returns at once
  K1_ONE_WAVE = 2,      // one feature wave per workgroup (the fused kernel cannot take the batch)
};
enum PointCholP {       // where chol(P) runs
  CHOLP_NONE = 0,       // nowhere: the update runs on the factor the plane loop left
  CHOLP_WG0 = 1,        // workgroup 0 of the fused feature launch
  CHOLP_SIDE = 2,       // k_chol2 on the side stream, beside the feature launch
  CHOLP_BEHIND_K1 = 3,  // main stream behind K1, K2 beside it on the side stream
};
enum PointTailForm {
  TAIL_TILE = 0,      // tile kernels on the leading nl columns of T
  TAIL_SUBSTATE = 1,  // n above the tile limit: the update of the sub_ns involved columns
  TAIL_GLOBAL = 2,    // ... more of them than the tile limit: global-memory factorization
};
enum PointBoost { BOOST_NONE = 0, BOOST_CHOL = 1, BOOST_LOOP = 2 };  // whose diagonal amounts the last kernel takes off

struct PointPlan {
  int Fa = 0;             // features that own rows of rec / G
  bool slots = false;     // ... numbered in the caller's slot array (-1: none); false: every feature, in batch order
  std::vector<int> sub_ids;  // n above the tile limit: the columns the batch can touch, sorted, unique
  int sub_ns = 0;            // ... their count when the sub-state update can take them, else 0
  PointK1 k1 = K1_ONE_WAVE;
  PointCholP chol_p = CHOLP_BEHIND_K1;
  bool flip = false;      // chol(P) in reversed index order: T = I + L^T A L is the identity outside its leading nl columns
  int s0 = 0;             // first column the batch touches
  int nl = 0;             // leading block of T (n: all of it)
  int boost_n = 0;        // diagonal entries the factor was boosted on and the last kernel takes the amounts off again:
  PointBoost boost = BOOST_NONE;  // the s0 columns in front of the batch's (CholJob::boost) or all n (the plane loop's boost_vec)
  bool clear_Ab = false;  // no feature owns rows: K2 is a clear of the pair
  int used_chunks = 0, nsplit = 0;  // K2's geometry on Fa features
  bool add_pair = false;  // the pending dense pair joins the batch's
  PointTailForm tail = TAIL_TILE;  // (what the second half will find: it decides by n and the sub-state the entry sets from sub_ids)
  int dense = 0;          // k_fwdsub's dense mode: 0 lower-triangular factor, 1 dense factor, 2 reversed-order factor
  bool join = false;      // the side stream holds work of this update: the second half waits for it
};

// the first column a point-feature batch touches / every column it can touch: clones, camera 0's estimated calibration, the
// pending dense pair's
inline int point_first_col(const PointEnv& e) {
  int s0 = e.n;
  for (int k = 0; k < e.n_clones; ++k) s0 = std::min(s0, e.clone_id[k]);
  if (e.calmask & 0x3Fu) s0 = std::min(s0, e.calib_id);
  if (e.calmask & (0xFFu << 6)) s0 = std::min(s0, e.intr_id);
  for (int k = 0; k < e.n_dense; ++k) s0 = std::min(s0, e.dense_cols[k]);  // (a second camera's columns, say)
  return s0;
}
inline void point_cols(const PointEnv& e, std::vector<int>* ids) {
  ids->clear();
  for (int c = 0; c < e.n_clones; ++c)
    for (int k = 0; k < 6; ++k) ids->push_back(e.clone_id[c] + k);
  if (e.calmask & 0x3Fu)
    for (int k = 0; k < 6; ++k) ids->push_back(e.calib_id + k);
  if (e.calmask & (0xFFu << 6))
    for (int k = 0; k < 8; ++k) ids->push_back(e.intr_id + k);
  ids->insert(ids->end(), e.dense_cols, e.dense_cols + e.n_dense);
  std::sort(ids->begin(), ids->end());
  ids->erase(std::unique(ids->begin(), ids->end()), ids->end());
}

// slot: [F], written only when the plan numbers the features (p->slots)
inline void plan_point_update(const PointEnv& e, int* slot, PointPlan* p) {
  *p = PointPlan();
  const int n = e.n, F = e.F;
  // Features that are not part of this update - consumed by an accepted plane, outside this rank's index range - own no rows of
  // rec / G: the others are numbered in batch order, K1 reads a feature's slot and K2 runs on Fa features (same sums over the same
  // rows in the same order)
  p->Fa = F;
  const bool ranged = e.range_lo >= 0;
  if ((ranged || e.used_valid) && F > 0) {
    const int lo = ranged ? e.range_lo : 0, hi = ranged ? std::min(e.range_hi, F) : F;
    int k = 0;
    for (int f = 0; f < F; ++f) slot[f] = (f >= lo && f < hi && !(e.used_valid && e.used[f])) ? k++ : -1;
    p->Fa = k;
    p->slots = true;
  }
  if (n > e.tilechol_nmax) {
    point_cols(e, &p->sub_ids);
    const int ns = (int)p->sub_ids.size();
    p->sub_ns = ns <= e.tilechol_nmax ? ns : 0;
    p->tail = p->sub_ns > 0 ? TAIL_SUBSTATE : TAIL_GLOBAL;
  }
  // chol(P) does not depend on the measurements and hides behind the features.  Up to side_capacity features (a round of feature
  // workgroups that leaves a CU on every XCD) it is a k_chol2 launch on the side stream (4, the default); above that, or where
  // k_chol2 cannot take n, it rides in workgroup 0 of the fused feature launch (3).  Where the fused kernel cannot take the batch,
  // K1 is the one-wave kernel, chol(P) follows it on the main stream and K2 runs beside it on the side stream.
  // The measurements behind the rules are in NOTES.md: chol(P) must not run BESIDE a one-wave K1 (the CU that hosts its eight waves
  // finishes its feature blocks late, K1 112 -> 157 us) nor as a 160 KB-LDS launch beside an 8-wave-workgroup K1 (the two did not
  // overlap) - the "Scheduling" entry of the round-1/3 notes; a round of 255 feature workgroups leaves the side kernel no CU on the XCD it
  // is sent to and the launches serialise (config 2: 316 against 274 us per update), 247 leave one on every XCD - "## Round 5", hence
  // side_capacity = 247 x 8 = 1976 features.
  const bool fused_ok = n <= e.tilechol_nmax && F > 0 && e.max_meas <= e.fused_max_meas && ((n + 15) >> 4) <= e.fused_max_tiles;
  const bool side_ok = e.sw.overlap != 3 && n <= e.chol2_max_n && F <= e.side_capacity;
  p->nl = n;
  if (!fused_ok) {
    p->k1 = K1_ONE_WAVE;
    p->chol_p = CHOLP_BEHIND_K1;
    p->join = true;
  } else if (e.have_factor) {  // M with M M^T = P (+ the loop's boost): any such M serves the update, no chol(P)
    p->k1 = K1_FUSED_IDLE;
    p->chol_p = CHOLP_NONE;
    p->dense = 1;
    if (e.factor_boosted) p->boost = BOOST_LOOP, p->boost_n = n;
  } else {
    p->k1 = side_ok ? K1_FUSED_IDLE : K1_FUSED_CHOL;
    p->chol_p = side_ok ? CHOLP_SIDE : CHOLP_WG0;
    p->join = side_ok;
    // The batch's information matrix lives on the clones and the estimated calibration.  When everything in front of the first of
    // those columns (the IMU block, dt) is untouched, the factor of P is taken in reversed index order: T is then the identity
    // outside its leading n - s0 columns, and both products, chol(T) and the substitution shrink with it, without a permutation of P
    p->s0 = point_first_col(e);
    if (!e.sw.no_flip && p->s0 >= 8 && p->s0 < n) {
      p->flip = true;
      p->nl = n - p->s0;
      p->dense = 2;
      // the columns in front of the batch's take a relative diagonal boost inside the factorization that the end of the update
      // takes off again: exact, and an exact stochastic clone (IMU pose == newest clone) factors on this path
      if (!e.sw.no_boost && p->s0 <= 64) p->boost = BOOST_CHOL, p->boost_n = p->s0;
    }
  }
  p->clear_Ab = p->Fa <= 0;
  if (!p->clear_Ab) {
    p->used_chunks = (2 * p->Fa + e.rows_per_chunk - 1) / e.rows_per_chunk;
    p->nsplit = std::min(std::max((3 * p->Fa + 511) / 512, 1), e.n_split);
  }
  p->add_pair = e.n_dense > 0;
}
