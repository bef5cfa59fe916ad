// The planner of the two SLAM entries (csrc/ovp_slam_plan.h) on a SlamEnv filled by hand, every field of the plans against values
// written out here.  Includes no HIP header and links nothing of the device; tests/test_slam_plan_cpu.py builds it with the
// address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ovp_slam_plan.h"

#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                           \
    }                                                         \
  } while (0)

typedef std::vector<int> V;

static V range(int from, int count) {
  V v;
  for (int k = 0; k < count; ++k) v.push_back(from + k);
  return v;
}
static V cat(std::initializer_list<V> parts) {
  V v;
  for (const V& p : parts) v.insert(v.end(), p.begin(), p.end());
  return v;
}

// A state of 100 columns: four clones at 0, 6, 12, 18; camera 0's extrinsics at 24, intrinsics at 30; cameras 1 and 2 at 60 / 66
// and 74 / 80; landmarks and planes from 40.
static const int CLONE_ID[4] = {0, 6, 12, 18};
static SlamEnv make_env(unsigned calmask, int gen_ncams = 0) {
  SlamEnv e;
  e.n = 100;
  e.n_max = 130;
  e.clone_id = CLONE_ID;
  e.n_clones = 4;
  e.calmask = calmask;
  for (int k = 0; k < 14; ++k) e.calcol[k] = e.on(k) ? (k < 6 ? 24 + k : 30 + (k - 6)) : 0;
  e.gen_ncams = gen_ncams;
  const int calib[3] = {24, 60, 74}, intr[3] = {30, 66, 80};
  for (int k = 0; k < gen_ncams; ++k) e.gen_calib_id[k] = calib[k], e.gen_intr_id[k] = intr[k];
  return e;
}
static const unsigned POSE = 0x3Fu, ALL = 0x3FFFu;

// a batch over arrays that live in the struct
struct Batch {
  ovp_slam_batch b{};
  std::vector<float> uv;
  V clone_idx, n_meas, lm_id, plane_sid, pre_rows, pre_cols, pre_ids;
  std::vector<double> p, cp, pre_H;
  Batch(int M, const V& n_meas_, const V& clone_idx_, const V& lm_id_) : clone_idx(clone_idx_), n_meas(n_meas_), lm_id(lm_id_) {
    const int L = (int)n_meas.size();
    CHECK((int)clone_idx.size() == L * M);
    uv.assign((size_t)2 * L * M, 0.f);
    p.assign((size_t)3 * L, 1.0);
    b.n_landmarks = L;
    b.max_meas = M;
    b.uv = uv.data();
    b.clone_idx = clone_idx.data();
    b.n_meas = n_meas.data();
    b.p_FinG = b.p_FinG_fej = p.data();
    b.landmark_id = lm_id.data();
  }
  void planes(const V& sid) {
    plane_sid = sid;
    cp.assign(3 * sid.size(), 1.0);
    b.plane_state_id = plane_sid.data();
    b.cp = b.cp_fej = cp.data();
  }
  void pre(const V& rows, const V& cols, const V& ids) {
    pre_rows = rows, pre_cols = cols, pre_ids = ids;
    size_t doubles = 0;
    for (size_t l = 0; l < rows.size(); ++l) doubles += (size_t)rows[l] * cols[l] + rows[l];
    pre_H.assign(doubles, 0.5);
    b.pre_rows = pre_rows.data();
    b.pre_cols = pre_cols.data();
    b.pre_H = pre_H.data();
    b.pre_ids = pre_ids.data();
  }
};

static void check_inverse(const SlamUpdatePlan& p, int n) {
  CHECK((int)p.gpos.size() == n && p.gcols == (int)p.gids.size());
  int listed = 0;
  for (int col = 0; col < n; ++col)
    if (p.gpos[col] >= 0) {
      CHECK(p.gids[p.gpos[col]] == col);
      ++listed;
    }
  CHECK(listed == p.gcols);
}

static void update_plans() {
  SlamUpdatePlan p;
  {  // two mono landmarks sharing clone 1
    Batch t(2, {2, 2}, {0, 1, 1, 2}, {40, 43});
    CHECK(plan_slam_update(make_env(POSE), &t.b, nullptr, &p) == 0);
    CHECK(p.gids == cat({range(0, 12), range(24, 6), range(40, 3), range(12, 6), range(43, 3)}));
    check_inverse(p, 100);
    CHECK(p.row0 == V({0, 4}) && p.m_total == 8 && p.rows_max == 4 && p.cols_max == 21 && p.gcols == 12 + 6 + 3 + 6 + 3);
    CHECK(p.L == 2 && p.M == 2 && !p.gen && !p.any_pre && p.any_built && !p.nothing && p.cam_mask.empty());
    CHECK(p.pre_off == V({0, 0}) && p.pre_ids_off == V({0, 0}) && p.preH == 0 && p.preI == 0);
    CHECK(p.h_in_lds == 1 && p.sform_fits);
  }
  {  // a landmark on a plane of the state: m more rows, the plane's three columns last
    Batch t(2, {2}, {3, 0}, {40});
    t.planes({50});
    CHECK(plan_slam_update(make_env(POSE), &t.b, nullptr, &p) == 0);
    CHECK(p.m_total == 6 && p.rows_max == 6 && p.cols_max == 24);
    CHECK(p.gids == cat({range(18, 6), range(0, 6), range(24, 6), range(40, 3), range(50, 3)}));
    check_inverse(p, 100);
  }
  {  // two host-built blocks (3 x 4, 2 x 2) between two built landmarks
    Batch t(1, {1, 0, 0, 1}, {0, 0, 0, 1}, {40, 0, 0, 43});
    t.pre({0, 3, 2, 0}, {0, 4, 2, 0}, {46, 47, 48, 2, 49, 47});
    CHECK(plan_slam_update(make_env(POSE), &t.b, nullptr, &p) == 0);
    CHECK(p.any_pre && p.any_built);
    CHECK(p.pre_off == V({0, 0, 15, 0}) && p.pre_ids_off == V({0, 0, 4, 0}) && p.preH == 3 * 4 + 3 + 2 * 2 + 2 && p.preI == 6);
    CHECK(p.row0 == V({0, 2, 5, 7}) && p.m_total == 9 && p.rows_max == 3 && p.cols_max == 15);
    CHECK(p.gids == cat({range(0, 6), range(24, 6), range(40, 3), {46, 47, 48}, {49}, range(6, 6), range(43, 3)}));
    check_inverse(p, 100);
  }
  {  // a general landmark seen by cameras 2 and 0 of three: both cameras' estimated columns, in camera order
    Batch t(2, {2}, {0, 1}, {40});
    const int cam_idx[2] = {2, 0};
    CHECK(plan_slam_update(make_env(ALL, 3), &t.b, cam_idx, &p) == 0);
    CHECK(p.gen && p.cam_mask == V({5}));
    CHECK(p.cols_max == 6 * 2 + 14 * 2 + 3 && p.m_total == 4);
    CHECK(p.gids == cat({range(0, 12), range(24, 14), range(74, 14), range(40, 3)}));
    check_inverse(p, 100);
  }
  {  // a landmark without observations beside one with two: the second one's rows are built
    Batch t(2, {0, 2}, {0, 0, 2, 3}, {40, 43});
    CHECK(plan_slam_update(make_env(POSE), &t.b, nullptr, &p) == 0);
    CHECK(p.any_built && !p.nothing && p.row0 == V({0, 0}) && p.m_total == 4);
    CHECK(p.gids == cat({range(12, 12), range(24, 6), range(43, 3)}));
    const int cam_idx[4] = {0, 0, 1, 0};  // (general: no camera of the empty landmark)
    CHECK(plan_slam_update(make_env(POSE, 2), &t.b, cam_idx, &p) == 0);
    CHECK(p.cam_mask == V({0, 3}) && p.any_built);
  }
  {  // nothing to update with
    Batch t(2, {0, 0}, {0, 0, 0, 0}, {40, 43});
    CHECK(plan_slam_update(make_env(POSE), &t.b, nullptr, &p) == 0);
    CHECK(p.nothing && p.m_total == 0 && !p.any_built && p.gcols == 0);
  }
}

static void update_precedence() {
  SlamUpdatePlan p;
  {  // landmark 0's host-built block names a column outside the state, landmark 1 a clone outside the window: landmark 0 decides
    Batch t(1, {0, 1}, {0, 9}, {0, 43});
    t.pre({2, 0}, {1, 0}, {100});
    CHECK(plan_slam_update(make_env(POSE), &t.b, nullptr, &p) == OVP_E_ARG);
    CHECK(p.gids.empty() && p.m_total == 0);  // (landmark 0 ended the plan: no row counted, no column listed)
  }
  {  // a block beyond the gate kernel's LDS alone is OVP_E_CAPACITY; the bad clone index of the landmark behind it wins
    Batch one(1, {0}, {0}, {0});
    one.pre({140}, {1}, {0});
    CHECK(plan_slam_update(make_env(POSE), &one.b, nullptr, &p) == OVP_E_CAPACITY);
    Batch two(1, {0, 1}, {0, 4}, {0, 43});
    two.pre({140, 0}, {1, 0}, {0});
    CHECK(plan_slam_update(make_env(POSE), &two.b, nullptr, &p) == OVP_E_ARG);
  }
  {  // a camera index equal to the number of uploaded cameras
    Batch t(2, {2}, {0, 1}, {40});
    const int cam_idx[2] = {0, 2};
    CHECK(plan_slam_update(make_env(POSE, 2), &t.b, cam_idx, &p) == OVP_E_ARG);
  }
  {  // an estimated calibration column outside the state
    Batch t(2, {2}, {0, 1}, {40});
    SlamEnv e = make_env(POSE);
    e.calcol[5] = 100;
    CHECK(plan_slam_update(e, &t.b, nullptr, &p) == OVP_E_ARG);
  }
}

// candidates over arrays that live in the struct; clone of observation a = clones[(l * M + a) % clones.size()]
struct Cands {
  int L, M;
  std::vector<float> uv;
  V clone_idx, n_meas;
  std::vector<double> p;
  Cands(int M_, const V& n_meas_, const V& clones) : L((int)n_meas_.size()), M(M_), n_meas(n_meas_) {
    uv.assign((size_t)2 * L * M, 0.f);
    p.assign((size_t)3 * L, 1.0);
    for (int e = 0; e < L * M; ++e) clone_idx.push_back(clones[e % clones.size()]);
  }
  int plan(const SlamEnv& e, DinitPlan* out, const int* cam_idx = nullptr, const ovp_dinit_planes* pl = nullptr, int dx_stride = -1) const {
    return plan_delayed_init(e, L, M, uv.data(), clone_idx.data(), cam_idx, n_meas.data(), p.data(), pl, pl != nullptr, dx_stride, out);
  }
};

static bool same_attempt(const DinitAttempt& a, const DinitAttempt& b) {
  return a.l == b.l && a.slot == b.slot && a.blk == b.blk && a.skip_blk == b.skip_blk && a.m == b.m && a.cols == b.cols && a.rows == b.rows;
}

static void dinit_plans() {
  DinitPlan p;
  {  // a mono candidate: clone blocks in observation order, then camera 0's estimated columns
    Cands t(3, {3}, {2, 0, 1});
    CHECK(t.plan(make_env(POSE), &p) == 0);
    CHECK(p.ids.size() == 1 && p.ids[0] == cat({range(12, 6), range(0, 12), range(24, 6)}) && (int)p.ids[0].size() == 6 * 3 + 6);
    CHECK(p.ocol.empty() && p.ccol.empty() && !p.gen && !p.with_planes && p.n_pl == 0 && p.n0 == 100 && p.ncal == 6);
    CHECK(p.cols_max == 24 && p.rows_max == 6 && p.att.size() == 1 && same_attempt(p.att[0], {0, 0, 0, -1, 3, 24, 6}));
    CHECK(p.blk_A == V({0}) && p.blk_final == V({0}));
  }
  {  // a general candidate: clone 1 seen by both cameras is one block
    Cands t(3, {3}, {1, 1, 3});
    const int cam_idx[3] = {0, 1, 1};
    CHECK(t.plan(make_env(POSE, 2), &p, cam_idx) == 0);
    CHECK(p.gen && p.ids[0] == cat({range(6, 6), range(18, 6), range(24, 6), range(60, 6)}));
    CHECK((int)p.ocol[0].size() == SLAM_PLAN_MAX_MEAS_DEV && p.ocol[0][0] == 0 && p.ocol[0][1] == 0 && p.ocol[0][2] == 6);
    CHECK(p.ccol[0] == V({12, 18, -1, -1}));
    CHECK(same_attempt(p.att[0], {0, 0, 0, -1, 3, 24, 6}));
  }
  {  // three candidates, the middle one on plane 1: four attempts, B skips behind A
    Cands t(2, {2, 2, 2}, {0, 1, 2, 3, 1, 0});
    const int sid[1] = {50}, of_cand[3] = {0, 1, 0};
    const double cp[3] = {1.0, 0.0, 0.0};
    const ovp_dinit_planes pl = {1, sid, cp, nullptr, of_cand, nullptr};
    CHECK(t.plan(make_env(POSE), &p, nullptr, &pl, 109) == 0);
    CHECK(p.with_planes && p.n_pl == 1 && p.att.size() == 4);
    CHECK(p.blk_A == V({0, 1, 3}) && p.blk_final == V({0, 2, 3}));
    CHECK(same_attempt(p.att[0], {0, 0, 0, -1, 2, 18, 4}) && same_attempt(p.att[1], {1, 1, 1, -1, 2, 21, 6}) &&
          same_attempt(p.att[2], {1, 0, 2, 1, 2, 18, 4}) && same_attempt(p.att[3], {2, 0, 3, -1, 2, 18, 4}));
    CHECK(p.cols_max == 21 && p.rows_max == 6);
    V row(p.cols_max, -7);
    dinit_attempt_ids(p, &pl, 1, row.data());
    CHECK(row == cat({range(12, 12), range(24, 6), range(50, 3)}));
    row.assign(p.cols_max, -7);
    dinit_attempt_ids(p, &pl, 2, row.data());
    CHECK(row == cat({range(12, 12), range(24, 6), {-7, -7, -7}}));
  }
}

static void dinit_capacity() {
  DinitPlan p;
  const int sid[1] = {50}, on_plane[1] = {1}, no_plane[1] = {0}, beyond[1] = {2};
  const double cp[3] = {0.0, 2.0, 0.0}, zero[3] = {0.0, 0.0, 0.0};
  const ovp_dinit_planes pl = {1, sid, cp, nullptr, on_plane, nullptr}, pl_free = {1, sid, cp, nullptr, no_plane, nullptr};
  // a camera-0 candidate with all 14 calibration columns: k_init_core's 152 KB binds at 3m - 3 update rows over 6m + 17 columns
  CHECK(Cands(32, {22}, {0, 1, 2, 3}).plan(make_env(ALL), &p, nullptr, &pl) == 0);
  CHECK(p.att.size() == 2 && p.att[0].rows == 66 && p.att[0].cols == 6 * 22 + 17 && p.rows_max == 66);
  CHECK(Cands(32, {23}, {0, 1, 2, 3}).plan(make_env(ALL), &p, nullptr, &pl) == OVP_E_CAPACITY);
  // ... and at 2m - 3 rows over 6m + 14 columns without a plane
  CHECK(Cands(32, {30}, {0, 1, 2, 3}).plan(make_env(ALL), &p, nullptr, &pl_free) == 0);
  CHECK(Cands(32, {30}, {0, 1, 2, 3}).plan(make_env(ALL), &p) == 0);
  CHECK(p.att.size() == 1 && p.att[0].cols == 6 * 30 + 14);
  CHECK(Cands(32, {31}, {0, 1, 2, 3}).plan(make_env(ALL), &p) == OVP_E_CAPACITY);
  CHECK(Cands(32, {31}, {0, 1, 2, 3}).plan(make_env(ALL), &p, nullptr, &pl_free) == OVP_E_CAPACITY);
  // the state would outgrow the context; a dx row shorter than the state behind the call
  const Cands two(2, {2, 2}, {0, 1});
  SlamEnv tight = make_env(POSE);
  tight.n_max = 105;
  CHECK(two.plan(tight, &p) == OVP_E_CAPACITY);
  CHECK(two.plan(make_env(POSE), &p, nullptr, nullptr, 105) == OVP_E_ARG);
  CHECK(two.plan(make_env(POSE), &p, nullptr, nullptr, 106) == 0);
  CHECK(two.plan(tight, &p, nullptr, nullptr, 105) == OVP_E_ARG);  // (the stride is looked at first)
  // the plane table
  const Cands one(2, {2}, {0, 1});
  const int outside[1] = {98};
  const ovp_dinit_planes bad_id = {1, outside, cp, nullptr, on_plane, nullptr}, bad_cp = {1, sid, zero, nullptr, on_plane, nullptr},
                         bad_fej = {1, sid, cp, zero, on_plane, nullptr}, bad_slot = {1, sid, cp, nullptr, beyond, nullptr};
  CHECK(one.plan(make_env(POSE), &p, nullptr, &pl) == 0);
  CHECK(one.plan(make_env(POSE), &p, nullptr, &bad_id) == OVP_E_ARG);
  CHECK(one.plan(make_env(POSE), &p, nullptr, &bad_cp) == OVP_E_ARG);
  CHECK(one.plan(make_env(POSE), &p, nullptr, &bad_fej) == OVP_E_ARG);
  CHECK(one.plan(make_env(POSE), &p, nullptr, &bad_slot) == OVP_E_ARG);
  // a track of one observation, a clone outside the window
  CHECK(Cands(2, {1}, {0, 1}).plan(make_env(POSE), &p) == OVP_E_ARG);
  CHECK(Cands(2, {2}, {0, 4}).plan(make_env(POSE), &p) == OVP_E_ARG);
}

int main() {
  update_plans();
  update_precedence();
  dinit_plans();
  dinit_capacity();
  printf("slam plan ok\n");
  return 0;
}
