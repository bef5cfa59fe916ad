// The host arithmetic of the two SLAM entries (ovp_api_slam.hip) in front of anything that touches the device: argument checks,
// column lists, row offsets, per-candidate clone and camera blocks, the attempt numbering of on-plane candidates and every LDS
// capacity decision.  Pure: no HIP header, no ovp_* call but the inline size functions of ovp_lds_sizes.h, no ovp_ctx - what the
// plans read from the context and the options arrives as a SlamEnv.  A plan writes nothing but its output struct; the loops run in
// the entries' documented order, so the first offending landmark / candidate decides the return code.
// Stand-alone under ASan / UBSan: tests/slam_plan_main.cpp.
#pragma once
#include <algorithm>
#include <vector>

#include "ovplane_hip.h"
#include "ovp_lds_sizes.h"

// device-side capacities the plans compare against (ovp_api_slam.hip asserts them against the kernels' headers)
static const int SLAM_PLAN_MAX_MEAS_DEV = 32;                                             // OVP_MAX_MEAS_DEV
static const int SLAM_PLAN_LDG_CAP = 704;                                                 // OVP_LDG_CAP
static const int SLAM_PLAN_IDV_CAP = 208;                                                 // DinitParams::idv
static const int SLAM_PLAN_IDG_CAP = 6 * SLAM_PLAN_MAX_MEAS_DEV + 14 * OVP_MAX_CAMERAS;  // DinitGenParams::idg

// What the plans read from (ctx, opts): the state's size and capacity, the clone columns, the calibration columns an update
// estimates (bit k of calmask = column k of a camera's [extrinsics 6 | intrinsics 8]; calcol = camera 0's, 0 where not estimated)
// and where the uploaded cameras' calibration blocks start.
struct SlamEnv {
  int n = 0, n_max = 0;
  const int* clone_id = nullptr;  // [n_clones] first column of every clone
  int n_clones = 0;
  unsigned calmask = 0;
  int calcol[14] = {};
  int gen_ncams = 0;
  int gen_calib_id[OVP_MAX_CAMERAS] = {-1, -1, -1, -1}, gen_intr_id[OVP_MAX_CAMERAS] = {-1, -1, -1, -1};

  bool on(int k) const { return (calmask >> k) & 1u; }
  int ncal() const { return __builtin_popcount(calmask); }
  int col_of(int cam, int k) const { return k < 6 ? gen_calib_id[cam] + k : gen_intr_id[cam] + (k - 6); }
  // every estimated column lies in a state of n columns: camera 0's, or (general) those of every uploaded camera
  int check(bool general) const {
    for (int cam = 0; cam < (general ? gen_ncams : 1); ++cam)
      for (int k = 0; k < 14; ++k) {
        const int id = general ? col_of(cam, k) : calcol[k];
        if (on(k) && (id < 0 || id >= n)) return OVP_E_ARG;
      }
    return 0;
  }
};

// ---- ovp_slam_update / ovp_slam_update_general ---------------------------------------------------------------------------------
struct SlamUpdatePlan {
  int L = 0, M = 0;
  bool gen = false, any_pre = false;
  std::vector<int> gpos, gids;           // state column -> position in the call's column list (-1: none) and its inverse
  std::vector<int> row0;                 // [L] first stacked row of the landmark
  std::vector<int> pre_off, pre_ids_off; // [L] offsets of a host-built block in pre_H (doubles) / pre_ids
  std::vector<int> cam_mask;             // [L] (general) bit c = camera c observes the landmark; 0: host-built block or no rows
  int m_total = 0, rows_max = 1, cols_max = 1, gcols = 0;
  size_t preH = 0, preI = 0;             // doubles of pre_H / ints of pre_ids the call reads
  bool any_built = false;                // some landmark's rows are built on the device
  bool nothing = false;                  // m_total < 1: nothing to update with (update/UpdaterSLAM.cpp:661-663); the rest is unset
  int h_in_lds = 0;                      // the gate kernel keeps a landmark's block in LDS
  bool sform_fits = false;               // the stack fits the one-workgroup S-form (k_init.hip)
};

// cam_idx == nullptr: camera 0's tables for every observation; otherwise observation a of landmark l by cam_idx[l * max_meas + a].
// The column list is in first-seen order (Hx_order_big of :634-646): per landmark its clone blocks, the estimated calibration
// columns of its cameras in camera order, the landmark, its plane.
inline int plan_slam_update(const SlamEnv& env, const ovp_slam_batch* b, const int* cam_idx, SlamUpdatePlan* p) {
  const int L = b->n_landmarks, n = env.n, M = b->max_meas;
  const bool gen = cam_idx != nullptr;
  if (M < 1 || M > OVP_MAX_MEAS || !b->n_meas || !b->landmark_id) return OVP_E_ARG;
  const bool any_pre = b->pre_rows != nullptr;
  if (any_pre && (!b->pre_cols || !b->pre_H || !b->pre_ids)) return OVP_E_ARG;
  if (env.check(gen)) return OVP_E_ARG;
  const int ncal = env.ncal(), C = env.n_clones;
  *p = SlamUpdatePlan();
  p->L = L, p->M = M, p->gen = gen, p->any_pre = any_pre;
  p->cam_mask.assign(gen ? L : 0, 0);
  p->gpos.assign(n, -1);
  p->row0.resize(L);
  p->pre_off.assign(L, 0);
  p->pre_ids_off.assign(L, 0);
  auto touch = [&](int col) {
    if (p->gpos[col] < 0) {
      p->gpos[col] = (int)p->gids.size();
      p->gids.push_back(col);
    }
  };
  for (int l = 0; l < L; ++l) {
    p->row0[l] = p->m_total;
    int rows, cols;
    if (any_pre && b->pre_rows[l] > 0) {
      rows = b->pre_rows[l];
      cols = b->pre_cols[l];
      if (cols < 1 || cols > n) return OVP_E_ARG;
      p->pre_off[l] = (int)p->preH;
      p->pre_ids_off[l] = (int)p->preI;
      for (int k = 0; k < cols; ++k) {
        const int id = b->pre_ids[p->preI + k];
        if (id < 0 || id >= n) return OVP_E_ARG;
        touch(id);
      }
      p->preH += (size_t)rows * cols + rows;
      p->preI += cols;
    } else {
      if (!b->uv || !b->clone_idx || !b->p_FinG || !b->p_FinG_fej) return OVP_E_ARG;
      const int m = b->n_meas[l];
      if (m < 0 || m > M) return OVP_E_ARG;
      const bool plane = b->plane_state_id && b->plane_state_id[l] >= 0;
      if (plane && (!b->cp || !b->cp_fej || b->plane_state_id[l] + 3 > n)) return OVP_E_ARG;
      if (b->landmark_id[l] < 0 || b->landmark_id[l] + 3 > n) return OVP_E_ARG;
      int camm = 1;  // cameras of the landmark (mono: camera 0)
      if (gen) {
        camm = 0;
        for (int a = 0; a < m; ++a) {
          const int cam = cam_idx[(size_t)l * M + a];
          if (cam < 0 || cam >= env.gen_ncams) return OVP_E_ARG;
          camm |= 1 << cam;
        }
        p->cam_mask[l] = camm;
      }
      rows = plane ? 3 * m : 2 * m;
      cols = 6 * m + ncal * __builtin_popcount(camm) + 3 + (plane ? 3 : 0);
      for (int a = 0; a < m; ++a) {
        const int ci = b->clone_idx[(size_t)l * M + a];
        if (ci < 0 || ci >= C) return OVP_E_ARG;
        for (int k = 0; k < 6; ++k) touch(env.clone_id[ci] + k);
      }
      if (m > 0) {
        if (gen) {
          for (int cam = 0; cam < OVP_MAX_CAMERAS; ++cam)
            if ((camm >> cam) & 1)
              for (int k = 0; k < 14; ++k)
                if (env.on(k)) touch(env.col_of(cam, k));
        } else {
          for (int k = 0; k < 14; ++k)
            if (env.on(k)) touch(env.calcol[k]);
        }
        for (int k = 0; k < 3; ++k) touch(b->landmark_id[l] + k);
        if (plane)
          for (int k = 0; k < 3; ++k) touch(b->plane_state_id[l] + k);
      }
      p->any_built = p->any_built || m > 0;
    }
    p->m_total += rows;
    p->rows_max = std::max(p->rows_max, rows);
    p->cols_max = std::max(p->cols_max, cols);
  }
  p->gcols = (int)p->gids.size();
  if (p->m_total < 1) {
    p->nothing = true;
    return 0;
  }
  if (ovp_slam_gate_lds(p->rows_max, p->cols_max, 0) > OVP_SLAM_GATE_MAX_LDS) return OVP_E_CAPACITY;
  p->h_in_lds = ovp_slam_gate_lds(p->rows_max, p->cols_max, 1) <= OVP_SLAM_GATE_MAX_LDS ? 1 : 0;
  p->sform_fits = ovp_init_fits(0, p->m_total, p->gcols);
  return 0;
}

// ---- ovp_slam_delayed_init / _general / _planes ----------------------------------------------------------------------------------
// One attempt of the loop: candidate, plane slot (0 = none), result block, block of the attempt it may skip behind (-1 = none:
// attempt B of an on-plane candidate names attempt A's), and its geometry: observations, columns and rows of H.
struct DinitAttempt {
  int l, slot, blk, skip_blk, m, cols, rows;
};

struct DinitPlan {
  int L = 0, M = 0, n0 = 0, ncal = 0, n_pl = 0;
  bool gen = false, with_planes = false;
  // every candidate's column list: (mono) clone blocks in observation order, camera 0's estimated calibration; (general) the
  // blocks of its distinct clones in first-seen order, then the estimated calibration columns of each of its cameras in camera
  // order.  ocol / ccol (general): local column of observation a's clone block / of camera k's calibration block (-1: not its)
  std::vector<std::vector<int>> ids, ocol, ccol;
  int cols_max = 1, rows_max = 4;
  std::vector<DinitAttempt> att;      // the attempts in order
  std::vector<int> blk_final, blk_A;  // [L] result block of the attempt that decides / of the first attempt
};

// the state columns of attempt a: the candidate's list and, for an attempt with plane rows, the plane's three columns behind it
inline void dinit_attempt_ids(const DinitPlan& p, const ovp_dinit_planes* pl, int a, int* dst) {
  const DinitAttempt& t = p.att[a];
  const std::vector<int>& ids = p.ids[t.l];
  std::copy(ids.begin(), ids.end(), dst);
  if (t.slot > 0)
    for (int k = 0; k < 3; ++k) dst[ids.size() + k] = pl->plane_state_id[t.slot - 1] + k;
}

// cam_idx == nullptr: camera 0's tables (ovp_slam_delayed_init); pl is read with with_planes only; dx_stride < 0: no dx wanted.
// OVP_E_CAPACITY: a candidate outside the one-workgroup S-form (k_init.hip) or the rows kernel - the caller takes
// StateHelper::initialize candidate by candidate, nothing was touched.
inline int plan_delayed_init(const SlamEnv& env, int L, int M, const float* uv, const int* clone_idx, const int* cam_idx,
                             const int* n_meas, const double* p_FinG, const ovp_dinit_planes* pl, bool with_planes, int dx_stride,
                             DinitPlan* p) {
  const int n0 = env.n;
  const bool gen = cam_idx != nullptr;
  if (M < 2 || (!gen && M > OVP_MAX_MEAS) || !uv || !clone_idx || !n_meas || !p_FinG) return OVP_E_ARG;
  if (dx_stride >= 0 && dx_stride < n0 + 3 * L) return OVP_E_ARG;
  if (n0 + 3 * L > env.n_max) return OVP_E_CAPACITY;
  if (env.check(false) || (gen && env.check(true))) return OVP_E_ARG;
  const int ncal = env.ncal(), C = env.n_clones;
  // the planes of the call: every argument checked before anything is enqueued
  const int n_pl = with_planes && pl ? pl->n_planes : 0;
  if (n_pl < 0) return OVP_E_ARG;
  if (n_pl > 0) {
    if (!pl->plane_state_id || !pl->cp || !pl->plane_of_cand) return OVP_E_ARG;
    for (int q = 0; q < n_pl; ++q) {
      const int id = pl->plane_state_id[q];
      if (id < 0 || id + 3 > n0 || id + 3 > SLAM_PLAN_LDG_CAP) return OVP_E_ARG;  // (outside the covariance / the commit's staged correction)
      const double* a = pl->cp + 3 * q;
      const double* f = (pl->cp_fej ? pl->cp_fej : pl->cp) + 3 * q;
      if (!(a[0] * a[0] + a[1] * a[1] + a[2] * a[2] > 0.0) || !(f[0] * f[0] + f[1] * f[1] + f[2] * f[2] > 0.0)) return OVP_E_ARG;
    }
  }
  auto slot_of = [&](int l) { return n_pl > 0 ? pl->plane_of_cand[l] : 0; };
  if (with_planes && pl && pl->plane_of_cand)
    for (int l = 0; l < L; ++l)
      if (pl->plane_of_cand[l] < 0 || pl->plane_of_cand[l] > n_pl) return OVP_E_ARG;
  *p = DinitPlan();
  p->L = L, p->M = M, p->n0 = n0, p->ncal = ncal, p->n_pl = n_pl, p->gen = gen, p->with_planes = with_planes;
  p->ids.resize(L);
  p->ocol.resize(gen ? L : 0);
  p->ccol.resize(gen ? L : 0);
  for (int l = 0; l < L; ++l) {
    const int m = n_meas[l];
    if (m < 2 || m > M) return OVP_E_ARG;  // (update/UpdaterSLAM.cpp:112-118: the caller drops shorter tracks)
    for (int a = 0; a < m; ++a) {
      const int ci = clone_idx[(size_t)l * M + a];
      if (ci < 0 || ci >= C) return OVP_E_ARG;
      if (gen && (cam_idx[(size_t)l * M + a] < 0 || cam_idx[(size_t)l * M + a] >= env.gen_ncams)) return OVP_E_ARG;
    }
    std::vector<int>& ids = p->ids[l];
    if (!gen) {
      for (int a = 0; a < m; ++a)
        for (int k = 0; k < 6; ++k) ids.push_back(env.clone_id[clone_idx[(size_t)l * M + a]] + k);
      for (int k = 0; k < 14; ++k)
        if (env.on(k)) ids.push_back(env.calcol[k]);
    } else {
      if (m > SLAM_PLAN_MAX_MEAS_DEV) return OVP_E_CAPACITY;  // (the rows kernel stages at most this many observations)
      std::vector<int>& oc = p->ocol[l];
      std::vector<int>& cc = p->ccol[l];
      oc.assign(SLAM_PLAN_MAX_MEAS_DEV, 0);
      cc.assign(OVP_MAX_CAMERAS, -1);
      int camm = 0;
      for (int a = 0; a < m; ++a) {
        const int ci = clone_idx[(size_t)l * M + a];
        int prev = -1;
        for (int a2 = 0; a2 < a && prev < 0; ++a2)
          if (clone_idx[(size_t)l * M + a2] == ci) prev = a2;
        if (prev >= 0) {
          oc[a] = oc[prev];
        } else {
          oc[a] = (int)ids.size();
          for (int k = 0; k < 6; ++k) ids.push_back(env.clone_id[ci] + k);
        }
        camm |= 1 << cam_idx[(size_t)l * M + a];
      }
      for (int cam = 0; cam < OVP_MAX_CAMERAS; ++cam)
        if ((camm >> cam) & 1) {
          cc[cam] = (int)ids.size();
          for (int k = 0; k < 14; ++k)
            if (env.on(k)) ids.push_back(env.col_of(cam, k));
        }
    }
    const int cols = (int)ids.size();
    if (!ovp_init_fits(3, 2 * m - 3, cols) || (gen ? ovp_dinit_gen_rows_lds(m, cols) : ovp_dinit_rows_lds(m, ncal)) > OVP_DINIT_DYN_LDS)
      return OVP_E_CAPACITY;
    p->cols_max = std::max(p->cols_max, cols);
    p->rows_max = std::max(p->rows_max, 2 * m);
    if (slot_of(l) > 0) {  // attempt A: m more rows, the plane's three columns
      const int colsA = cols + 3, rowsA = 3 * m;
      if (!ovp_init_fits(3, rowsA - 3, colsA) || ovp_dinit_pl_rows_lds(rowsA, colsA) > OVP_DINIT_DYN_LDS ||
          rowsA > DINIT_MAX_ROWS_THREADS || colsA > (gen ? SLAM_PLAN_IDG_CAP : SLAM_PLAN_IDV_CAP))
        return OVP_E_CAPACITY;
      p->cols_max = std::max(p->cols_max, colsA);
      p->rows_max = std::max(p->rows_max, rowsA);
    }
  }
  p->blk_final.resize(L);
  p->blk_A.resize(L);
  for (int l = 0; l < L; ++l) {
    const int sl = slot_of(l), m = n_meas[l], cols = (int)p->ids[l].size(), blk = (int)p->att.size();
    p->blk_A[l] = blk;
    if (sl > 0) {  // attempt A with the plane's rows, then attempt B without them, skipped on the device when A stood
      p->att.push_back({l, sl, blk, -1, m, cols + 3, 3 * m});
      p->att.push_back({l, 0, blk + 1, blk, m, cols, 2 * m});
    } else {
      p->att.push_back({l, 0, blk, -1, m, cols, 2 * m});
    }
    p->blk_final[l] = (int)p->att.size() - 1;
  }
  return 0;
}
