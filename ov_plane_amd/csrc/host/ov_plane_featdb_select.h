// The selection of VioManager::do_feature_propagate_update (core/VioManager.cpp:373-506) on the class table the device database
// publishes (ovp_featdb_classify): sequential list logic, host code, pure - no device, no state, testable on its own
// (tests/featdb_host_main.cpp).  One camera and no ArUco tracker: the camera filter of :386-403 is a no-op, curr_aruco_tags is 0.
// The table's ids are ascending (this project's rule where the reference iterates a hash map), and every list keeps that order.
#pragma once
#include <algorithm>
#include <cstdint>
#include <set>
#include <vector>

namespace ov_plane {

struct FeatDbSelection {
  std::vector<int64_t> lost, marg, maxtracks;      // feats_lost, feats_marg, what is left of feats_maxtracks (:504-506 stacks the three)
  std::vector<int64_t> slam_delayed, slam_update;  // feats_slam_DELAYED, feats_slam_UPDATE (:488-501)
  std::vector<int64_t> landmarks_marg;             // landmarks whose should_marg is set (:478-479)
};

// cls: 0 none, 1 lost, 2 marg, 3 maxtrack (OVP_FEATDB_*); landmarks: State::_features_SLAM's ids in the caller's order
inline FeatDbSelection featdb_select(const std::vector<int64_t>& ids, const std::vector<int>& cls, const std::vector<int64_t>& landmarks,
                                     int max_slam_features, bool slam_delay_ok) {
  FeatDbSelection s;
  for (size_t i = 0; i < ids.size(); ++i) {
    if (cls[i] == 1) s.lost.push_back(ids[i]);
    if (cls[i] == 2) s.marg.push_back(ids[i]);
    if (cls[i] == 3) s.maxtracks.push_back(ids[i]);
  }
  std::vector<int64_t> slam;
  // :447-460 the LAST valid_amount of the maxtracks become new SLAM features
  if (max_slam_features > 0 && slam_delay_ok && (int)landmarks.size() < max_slam_features) {
    const int amount = max_slam_features - (int)landmarks.size();
    const int valid = std::min(amount, (int)s.maxtracks.size());
    if (valid > 0) {
      slam.insert(slam.end(), s.maxtracks.end() - valid, s.maxtracks.end());
      s.maxtracks.erase(s.maxtracks.end() - valid, s.maxtracks.end());
    }
  }
  // :466-480 a landmark the database still holds is updated (get_feature does not look at to_delete), one it lost is marginalised
  const std::set<int64_t> live(ids.begin(), ids.end());
  std::set<int64_t> left;
  for (int64_t lm : landmarks) {
    if (live.count(lm)) {
      slam.push_back(lm);
      left.insert(lm);
    } else
      s.landmarks_marg.push_back(lm);
  }
  // :488-501
  for (int64_t f : slam) (left.count(f) ? s.slam_update : s.slam_delayed).push_back(f);
  return s;
}

}  // namespace ov_plane
