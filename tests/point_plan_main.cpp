// The planner of the point update (csrc/ovp_point_plan.h) on a PointEnv filled by hand, every field of the plan against values
// written out here.  Includes no HIP header and links nothing of the device; tests/test_point_plan_cpu.py builds it with the
// address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ovp_point_plan.h"

#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                           \
    }                                                         \
  } while (0)

typedef std::vector<int> V;

static V range(int from, int count, int step = 1) {
  V v;
  for (int k = 0; k < count; ++k) v.push_back(from + k * step);
  return v;
}

// An environment over arrays that live in the struct.  The device-side limits are the product's: tile factorization 288, k_chol2
// 287, the fused feature kernel 18 tile rows and 30 observations, 1976 features beside a side-stream kernel; K2 in chunks of 256
// rows, at most 8 splits.
struct Env {
  PointEnv e;
  V clones, dense;
  std::vector<unsigned char> used;
  Env(int n, int F, const V& clones_, unsigned calmask = 0, int calib_id = -1, int intr_id = -1) : clones(clones_) {
    e.n = n, e.F = F, e.max_meas = 30;
    e.calmask = calmask, e.calib_id = calib_id, e.intr_id = intr_id;
    e.rows_per_chunk = 256, e.n_split = 8;
    e.tilechol_nmax = 288, e.chol2_max_n = 287, e.fused_max_tiles = 18, e.fused_max_meas = 30, e.side_capacity = 1976;
    fix();
  }
  void fix() {
    e.clone_id = clones.data(), e.n_clones = (int)clones.size();
    e.dense_cols = dense.data(), e.n_dense = (int)dense.size();
    e.used = used.data();
  }
  PointPlan plan(V* slot = nullptr) {
    fix();
    V mine((size_t)e.F + 1, -7);  // (one past the end: the planner writes F entries at most)
    PointPlan p;
    plan_point_update(e, mine.data(), &p);
    CHECK(mine[e.F] == -7);
    if (!p.slots)
      for (int f = 0; f < e.F; ++f) CHECK(mine[f] == -7);  // untouched where the plan numbers nothing
    mine.pop_back();
    if (slot) *slot = mine;
    return p;
  }
};

static const unsigned ALL = 0x3FFFu;
// BASELINE config 2's state: 30 clones from column 16, camera extrinsics at 196, intrinsics at 202, n = 210
static Env config2(int F) { return Env(210, F, range(16, 30, 6), ALL, 196, 202); }

// every field of the plan
static void same(const PointPlan& p, const PointPlan& x) {
  CHECK(p.Fa == x.Fa);
  CHECK(p.slots == x.slots);
  CHECK(p.sub_ids == x.sub_ids);
  CHECK(p.sub_ns == x.sub_ns);
  CHECK(p.k1 == x.k1);
  CHECK(p.chol_p == x.chol_p);
  CHECK(p.flip == x.flip);
  CHECK(p.s0 == x.s0);
  CHECK(p.nl == x.nl);
  CHECK(p.boost_n == x.boost_n);
  CHECK(p.boost == x.boost);
  CHECK(p.clear_Ab == x.clear_Ab);
  CHECK(p.used_chunks == x.used_chunks);
  CHECK(p.nsplit == x.nsplit);
  CHECK(p.add_pair == x.add_pair);
  CHECK(p.tail == x.tail);
  CHECK(p.dense == x.dense);
  CHECK(p.join == x.join);
}

// the expected plan, written out: K2's geometry for Fa features of a whole batch, then the route
static PointPlan expect(int Fa, int used_chunks, int nsplit, PointK1 k1, PointCholP chol_p, bool join, bool flip, int s0, int nl, int dense,
                        PointBoost boost, int boost_n) {
  PointPlan x;
  x.Fa = Fa, x.used_chunks = used_chunks, x.nsplit = nsplit, x.clear_Ab = Fa == 0;
  x.k1 = k1, x.chol_p = chol_p, x.join = join;
  x.flip = flip, x.s0 = s0, x.nl = nl, x.dense = dense, x.boost = boost, x.boost_n = boost_n;
  x.tail = TAIL_TILE;
  return x;
}

int main() {
  // config 2 at 2000 features: more than a round beside a side-stream kernel takes, so chol(P) rides in workgroup 0; reversed order
  // with the 16 columns in front of the first clone boosted; K2: 4000 rows in 16 chunks, 12 splits wanted, 8 there
  same(config2(2000).plan(), expect(2000, 16, 8, K1_FUSED_CHOL, CHOLP_WG0, false, true, 16, 194, 2, BOOST_CHOL, 16));
  // the boundary: 1976 features leave a CU on every XCD, 1977 do not
  same(config2(1976).plan(), expect(1976, 16, 8, K1_FUSED_IDLE, CHOLP_SIDE, true, true, 16, 194, 2, BOOST_CHOL, 16));
  same(config2(1977).plan(), expect(1977, 16, 8, K1_FUSED_CHOL, CHOLP_WG0, false, true, 16, 194, 2, BOOST_CHOL, 16));
  // n = 288: one above k_chol2's limit, still a tile factorization - workgroup 0 whatever the batch; s0 = 260: no boost
  same(Env(288, 50, range(260, 4, 6)).plan(), expect(50, 1, 1, K1_FUSED_CHOL, CHOLP_WG0, false, true, 260, 28, 2, BOOST_NONE, 0));
  same(Env(287, 50, range(260, 4, 6)).plan(), expect(50, 1, 1, K1_FUSED_IDLE, CHOLP_SIDE, true, true, 260, 27, 2, BOOST_NONE, 0));
  {  // the plane loop left a factor: no chol(P) anywhere, a dense factor on all n columns, the loop's boost off all n entries or none
    Env v = config2(300);
    v.e.have_factor = true, v.e.factor_boosted = true;
    same(v.plan(), expect(300, 3, 2, K1_FUSED_IDLE, CHOLP_NONE, false, false, 0, 210, 1, BOOST_LOOP, 210));
    v.e.factor_boosted = false;
    same(v.plan(), expect(300, 3, 2, K1_FUSED_IDLE, CHOLP_NONE, false, false, 0, 210, 1, BOOST_NONE, 0));
    v.e.F = 2000;  // (the same above the side capacity: the launch itself picks the round)
    same(v.plan(), expect(2000, 16, 8, K1_FUSED_IDLE, CHOLP_NONE, false, false, 0, 210, 1, BOOST_NONE, 0));
    v.e.have_factor = false, v.e.factor_boosted = true;  // (a boost without a factor means nothing)
    same(v.plan(), expect(2000, 16, 8, K1_FUSED_CHOL, CHOLP_WG0, false, true, 16, 194, 2, BOOST_CHOL, 16));
  }
  // the thresholds of the reversed order: s0 = 7 no flip, 8 flip; 64 boost, 65 flip without boost
  same(Env(40, 100, range(7, 3, 6)).plan(), expect(100, 1, 1, K1_FUSED_IDLE, CHOLP_SIDE, true, false, 7, 40, 0, BOOST_NONE, 0));
  same(Env(40, 100, range(8, 3, 6)).plan(), expect(100, 1, 1, K1_FUSED_IDLE, CHOLP_SIDE, true, true, 8, 32, 2, BOOST_CHOL, 8));
  same(Env(90, 100, range(64, 2, 6)).plan(), expect(100, 1, 1, K1_FUSED_IDLE, CHOLP_SIDE, true, true, 64, 26, 2, BOOST_CHOL, 64));
  same(Env(90, 100, range(65, 2, 6)).plan(), expect(100, 1, 1, K1_FUSED_IDLE, CHOLP_SIDE, true, true, 65, 25, 2, BOOST_NONE, 0));
  {  // calibration columns count only where they are estimated: extrinsics at 2 pull s0 under 8, unestimated they do not
    Env v(60, 100, range(20, 4, 6), 0x3Fu, 2, 50);
    same(v.plan(), expect(100, 1, 1, K1_FUSED_IDLE, CHOLP_SIDE, true, false, 2, 60, 0, BOOST_NONE, 0));
    v.e.calmask = 0xFFu << 6;  // intrinsics only, at 50: behind the clones
    same(v.plan(), expect(100, 1, 1, K1_FUSED_IDLE, CHOLP_SIDE, true, true, 20, 40, 2, BOOST_CHOL, 20));
  }
  {  // a pending dense column in front of the first clone lowers s0, and the pair is added
    Env v = config2(2000);
    v.dense = {200, 10};
    PointPlan x = expect(2000, 16, 8, K1_FUSED_CHOL, CHOLP_WG0, false, true, 10, 200, 2, BOOST_CHOL, 10);
    x.add_pair = true;
    same(v.plan(), x);
  }
  {  // 31 observations: the fused kernel cannot take the batch - one-wave K1, chol(P) behind it, K2 aside, a join owed; in the
     // state's own order on all n columns, and a kept factor is not used
    Env v = config2(2000);
    v.e.max_meas = 31;
    const PointPlan x = expect(2000, 16, 8, K1_ONE_WAVE, CHOLP_BEHIND_K1, true, false, 0, 210, 0, BOOST_NONE, 0);
    same(v.plan(), x);
    v.e.have_factor = true, v.e.factor_boosted = true;
    same(v.plan(), x);
    v.e.max_meas = 30, v.e.F = 0, v.e.have_factor = false;  // an empty batch is the fused kernel's neither
    same(v.plan(), expect(0, 0, 0, K1_ONE_WAVE, CHOLP_BEHIND_K1, true, false, 0, 210, 0, BOOST_NONE, 0));
  }
  {  // n = 300 with 11 clones, calibration and a pending pair: the sub-state list sorted and unique, 82 columns
    Env v(300, 120, range(76, 11, -6), ALL, 82, 88);  // (clones 76, 70, ... 16: the order of the table does not matter)
    v.dense = {150, 20, 95, 150};
    PointPlan x = expect(120, 1, 1, K1_ONE_WAVE, CHOLP_BEHIND_K1, true, false, 0, 300, 0, BOOST_NONE, 0);
    x.sub_ids = range(16, 80);
    x.sub_ids.push_back(150);
    x.sub_ns = 81;
    x.tail = TAIL_SUBSTATE;
    x.add_pair = true;
    same(v.plan(), x);
  }
  {  // n = 400 with 49 clones: 294 involved columns, more than the tile factorization holds - global fallback; 48 clones: 288 fit
    Env v(400, 120, range(0, 49, 6));
    PointPlan x = expect(120, 1, 1, K1_ONE_WAVE, CHOLP_BEHIND_K1, true, false, 0, 400, 0, BOOST_NONE, 0);
    x.sub_ids = range(0, 294);
    x.tail = TAIL_GLOBAL;
    same(v.plan(), x);
    v.clones.pop_back();
    x.sub_ids = range(0, 288);
    x.sub_ns = 288;
    x.tail = TAIL_SUBSTATE;
    same(v.plan(), x);
  }
  {  // index range and consumed-feature mask: slots in batch order, -1 outside
    Env v = config2(10);
    v.used = {0, 0, 0, 1, 0, 0, 1, 0, 0, 1};
    V slot;
    PointPlan x = expect(10, 1, 1, K1_FUSED_IDLE, CHOLP_SIDE, true, true, 16, 194, 2, BOOST_CHOL, 16);
    same(v.plan(&slot), x);  // neither asked for: every feature, nothing numbered
    v.e.used_valid = true;
    x.slots = true, x.Fa = 7;
    same(v.plan(&slot), x);
    CHECK(slot == V({0, 1, 2, -1, 3, 4, -1, 5, 6, -1}));
    v.e.range_lo = 2, v.e.range_hi = 8;
    x.Fa = 4;
    same(v.plan(&slot), x);
    CHECK(slot == V({-1, -1, 0, -1, 1, 2, -1, 3, -1, -1}));
    v.e.used_valid = false;  // (the mask is there but was not asked for)
    x.Fa = 6;
    same(v.plan(&slot), x);
    CHECK(slot == V({-1, -1, 0, 1, 2, 3, 4, 5, -1, -1}));
    v.e.range_lo = 5, v.e.range_hi = 50;  // hi past the batch
    x.Fa = 5;
    same(v.plan(&slot), x);
    CHECK(slot == V({-1, -1, -1, -1, -1, 0, 1, 2, 3, 4}));
    v.e.range_lo = 3, v.e.range_hi = 3;  // an empty share: K2 is a clear of the pair
    x.Fa = 0, x.clear_Ab = true, x.used_chunks = 0, x.nsplit = 0;
    same(v.plan(&slot), x);
    CHECK(slot == V(10, -1));
  }
  {  // K2's geometry: 129 features are 258 rows, two chunks of 256; 171 features want (513 + 511) / 512 = 2 splits; one split there
    same(config2(128).plan(), expect(128, 1, 1, K1_FUSED_IDLE, CHOLP_SIDE, true, true, 16, 194, 2, BOOST_CHOL, 16));
    same(config2(129).plan(), expect(129, 2, 1, K1_FUSED_IDLE, CHOLP_SIDE, true, true, 16, 194, 2, BOOST_CHOL, 16));
    same(config2(171).plan(), expect(171, 2, 2, K1_FUSED_IDLE, CHOLP_SIDE, true, true, 16, 194, 2, BOOST_CHOL, 16));
    Env v = config2(1500);
    v.e.n_split = 1;
    same(v.plan(), expect(1500, 12, 1, K1_FUSED_IDLE, CHOLP_SIDE, true, true, 16, 194, 2, BOOST_CHOL, 16));
  }
  {  // the three switches, and an overlap value outside {3, 4}
    Env v = config2(100);
    const PointPlan dflt = expect(100, 1, 1, K1_FUSED_IDLE, CHOLP_SIDE, true, true, 16, 194, 2, BOOST_CHOL, 16);
    same(v.plan(), dflt);
    v.e.sw.overlap = 3;
    same(v.plan(), expect(100, 1, 1, K1_FUSED_CHOL, CHOLP_WG0, false, true, 16, 194, 2, BOOST_CHOL, 16));
    const int others[] = {4, 0, 1, 2, 5, -1, 33};
    for (int o : others) {
      v.e.sw.overlap = o;
      same(v.plan(), dflt);
    }
    v.e.sw = PointSwitches();
    v.e.sw.no_boost = true;
    same(v.plan(), expect(100, 1, 1, K1_FUSED_IDLE, CHOLP_SIDE, true, true, 16, 194, 2, BOOST_NONE, 0));
    v.e.sw.no_flip = true;  // (no boost without the reversed order, whatever the other switch says)
    same(v.plan(), expect(100, 1, 1, K1_FUSED_IDLE, CHOLP_SIDE, true, false, 16, 210, 0, BOOST_NONE, 0));
    v.e.sw.no_boost = false;
    same(v.plan(), expect(100, 1, 1, K1_FUSED_IDLE, CHOLP_SIDE, true, false, 16, 210, 0, BOOST_NONE, 0));
    v.e.sw.overlap = 3;
    same(v.plan(), expect(100, 1, 1, K1_FUSED_CHOL, CHOLP_WG0, false, false, 16, 210, 0, BOOST_NONE, 0));
  }
  printf("point plan ok\n");
  return 0;
}
