// The planner of the batched plane merge (csrc/host/ov_plane_retire_plan.h) without a device, under the sanitizers
// (tests/test_retire_plan_cpu.py): every field of every plan against values written out by hand from
// state/StateHelper.cpp:654-757.
#include <cstdio>
#include <string>

#include "ov_plane_retire_plan.h"

using ov_plane::RetirePlan;
using ov_plane::plan_plane_retire;
typedef std::map<size_t, int> Planes;
typedef std::map<size_t, size_t> F2P;
typedef std::map<size_t, std::set<size_t>> P2O;

static int failures = 0;

struct Op3 { int rename; size_t id, new_id; };
struct Pair4 { size_t new_id, old_id; int new_col, old_col; };

static void expect(const char *what, const RetirePlan &p, std::vector<Op3> ops, std::vector<Pair4> pairs, std::vector<int> plane_col,
                   std::vector<int> retire_col) {
  bool ok = p.ops.size() == ops.size() && p.pairs.size() == pairs.size() && p.plane_col == plane_col && p.retire_col == retire_col;
  for (size_t i = 0; ok && i < ops.size(); ++i)
    ok = (int)p.ops[i].rename == ops[i].rename && p.ops[i].id == ops[i].id && (!ops[i].rename || p.ops[i].new_id == ops[i].new_id);
  for (size_t i = 0; ok && i < pairs.size(); ++i)
    ok = p.pairs[i].new_id == pairs[i].new_id && p.pairs[i].old_id == pairs[i].old_id && p.pairs[i].new_col == pairs[i].new_col &&
         p.pairs[i].old_col == pairs[i].old_col;
  if (!ok) {
    ++failures;
    printf("FAILED %s: %zu ops, %zu pairs, %zu planes, %zu retired\n", what, p.ops.size(), p.pairs.size(), p.plane_col.size(),
           p.retire_col.size());
  }
}

int main() {
  // a surviving id that is not in the state: plane 3 takes the id 9, no pair; 9 is then observed and stays
  expect("rename", plan_plane_retire(Planes{{2, 48}, {3, 51}}, F2P{{100, 2}, {101, 9}}, P2O{{9, {3}}}), {{1, 3, 9}}, {}, {}, {});
  // one survivor with two olds: two pairs in map order, both olds leave
  expect("two olds", plan_plane_retire(Planes{{1, 48}, {2, 51}, {3, 54}}, F2P{{100, 1}}, P2O{{1, {2, 3}}}), {{0, 2, 0}, {0, 3, 0}},
         {{1, 2, 48, 51}, {1, 3, 48, 54}}, {48, 51, 54}, {51, 54});
  // an old whose survivor is itself is skipped
  expect("self", plan_plane_retire(Planes{{4, 48}}, F2P{{100, 4}}, P2O{{4, {4}}}), {}, {}, {}, {});
  // a plane nobody observes is retired and is in no pair (the set names an id the state does not hold)
  expect("unobserved", plan_plane_retire(Planes{{1, 48}, {2, 51}}, F2P{{100, 1}, {101, 1}}, P2O{{1, {7}}}), {{0, 2, 0}}, {}, {}, {51});
  // an empty plane2oldplane, every plane observed
  expect("no merges", plan_plane_retire(Planes{{1, 48}, {2, 51}}, F2P{{100, 1}, {101, 2}}, P2O{}), {}, {}, {}, {});
  // no planes at all
  expect("no planes", plan_plane_retire(Planes{}, F2P{{100, 1}}, P2O{{1, {2}}}), {}, {}, {}, {});
  // the order of the operations matters: plane 2 is fused into 1 and leaves, THEN plane 5 takes the id 2 (which is free by then)
  expect("erase then rename", plan_plane_retire(Planes{{1, 48}, {2, 51}, {5, 54}}, F2P{{100, 1}, {101, 2}}, P2O{{1, {2}}, {2, {5}}}),
         {{0, 2, 0}, {1, 5, 2}}, {{1, 2, 48, 51}}, {48, 51}, {51});
  // a survivor nobody observes any more leaves behind its merge; an unobserved renamed plane leaves under its new id
  expect("survivor retired", plan_plane_retire(Planes{{1, 48}, {2, 51}, {3, 54}}, F2P{}, P2O{{1, {2}}, {8, {3}}}),
         {{0, 2, 0}, {1, 3, 8}, {0, 1, 0}, {0, 8, 0}}, {{1, 2, 48, 51}}, {48, 51}, {51, 48, 54});
  if (failures) return 1;
  printf("retire plan ok\n");
  return 0;
}
