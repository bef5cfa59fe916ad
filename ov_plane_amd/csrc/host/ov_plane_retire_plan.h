// StateHelper::merge_planes_and_marginalize (state/StateHelper.cpp:654-757) as a plan: its two loops run on the plane ids alone.
// Neither the renames, nor the erasures, nor which planes end up without an observer depend on whether a pair passes its gate, so
// everything the device and the bookkeeping need is known before the device is asked.  Pure: no ovp_* call, no State, standard
// library only (tests/retire_plan_main.cpp compiles it on its own under the sanitizers).
#pragma once
#include <cstddef>
#include <map>
#include <set>
#include <vector>

namespace ov_plane {

struct RetirePlan {
  // what happens to _features_PLANE, in the reference's order: a rename (the surviving id is not a state variable: the old
  // variable takes it, :688-690) or an erasure (the variable under `id` leaves the state, :733-734 and :751-753)
  struct Op {
    bool rename;
    size_t id, new_id;  // new_id: renames only
  };
  struct Pair {
    size_t new_id, old_id;
    int new_col, old_col;  // first columns, in the numbering before the call
  };
  std::vector<Op> ops;
  std::vector<Pair> pairs;         // the merges, in the order the reference meets them
  std::vector<int> plane_col;      // first columns of the distinct planes the pairs name, in order of first appearance
  std::vector<int> retire_col;     // first column of the variable of every erasure, in the order of `ops` (each is 3 wide)
};

// planes: _features_PLANE as id -> first column of its variable
inline RetirePlan plan_plane_retire(const std::map<size_t, int> &planes, const std::map<size_t, size_t> &feat2plane,
                                    const std::map<size_t, std::set<size_t>> &plane2oldplane) {
  RetirePlan plan;
  if (planes.empty()) return plan;  // :658-659
  std::map<size_t, int> m = planes;
  auto name = [&plan](int col) {
    for (int c : plan.plane_col)
      if (c == col) return;
    plan.plane_col.push_back(col);
  };
  auto it = m.begin();
  while (it != m.end()) {
    const size_t planeid = it->first;
    int planeid_new = -1;
    bool in_state = false;
    for (auto const &planeset : plane2oldplane)  // :670-675 (the last set that holds the id decides)
      if (planeset.second.find(planeid) != planeset.second.end()) {
        planeid_new = (int)planeset.first;
        in_state = m.find(planeset.first) != m.end();
      }
    if (planeid_new == -1 || (int)planeid == planeid_new) {  // :678-681
      ++it;
      continue;
    }
    if (!in_state) {  // :688-690
      m.insert({(size_t)planeid_new, it->second});
      plan.ops.push_back({true, planeid, (size_t)planeid_new});
      it = m.erase(it);
      continue;
    }
    const int new_col = m.at((size_t)planeid_new), old_col = it->second;
    plan.pairs.push_back({(size_t)planeid_new, planeid, new_col, old_col});
    name(new_col);
    name(old_col);
    plan.ops.push_back({false, planeid, 0});  // :733-734 whether or not the pair is accepted
    plan.retire_col.push_back(old_col);
    it = m.erase(it);
  }
  std::set<size_t> active;  // :739-741
  for (auto const &fp : feat2plane) active.insert(fp.second);
  for (it = m.begin(); it != m.end();) {  // :745-757
    if (active.find(it->first) == active.end()) {
      plan.ops.push_back({false, it->first, 0});
      plan.retire_col.push_back(it->second);
      it = m.erase(it);
    } else {
      ++it;
    }
  }
  return plan;
}

}  // namespace ov_plane
