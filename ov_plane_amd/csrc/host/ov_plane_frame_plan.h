// The survivor / slot replay of a fused frame (ovp_klt_match_frame): which candidates survive, in which order, and which slot of the
// feature database each survivor's observation goes to - the assignment k_klt_keep_append makes on the device, restated for the
// host, which replays it behind the wait to keep its id -> slot map.  Sequential list logic, host code, pure - no device, no state,
// testable on its own (tests/frame_plan_main.cpp).  The rule is ovp_featdb_append's over the survivors alone: a known id keeps its
// slot, the k-th fresh survivor (in candidate order) takes free_slots[k], where free_slots lists the free slots in the order the
// database hands them out.
// Its one caller is the C library's own host side (ovp_featdb_frame_commit, k_featdb.hip), where the id -> slot map lives; the C++
// mirror gets the result through the database's read-backs and does not include this file.  It stands in host/ beside the other pure
// host headers with a stand-alone test (ov_plane_featdb_select.h) and, like ov_plane_delaunay.h, is included by the library from there.
#pragma once
#include <cstdint>
#include <vector>

namespace ov_plane {

struct FramePlan {
  std::vector<int32_t> kept_index;  // the survivors' candidate indices, ascending
  std::vector<int32_t> slot;        // [kept] the slot each survivor's observation goes to
  int n_fresh_kept = 0;             // free slots taken: free_slots[0 .. n_fresh_kept)
  bool ok = true;                   // false: a fresh survivor found no free slot (the plan stops being usable)
};

// keep [n] (non-zero: survivor), fresh [n] (non-zero: the id is new to the database), slot [n] (of a known id; ignored when fresh)
inline FramePlan frame_plan(int n, const uint8_t* keep, const uint8_t* fresh, const int32_t* slot, const int32_t* free_slots, int n_free) {
  FramePlan p;
  for (int i = 0; i < n; ++i) {
    if (!keep[i]) continue;
    int s = slot ? slot[i] : -1;
    if (fresh && fresh[i]) {
      if (p.n_fresh_kept >= n_free) {
        p.ok = false;
        return p;
      }
      s = free_slots[p.n_fresh_kept++];
    }
    p.kept_index.push_back(i);
    p.slot.push_back(s);
  }
  return p;
}

}  // namespace ov_plane
