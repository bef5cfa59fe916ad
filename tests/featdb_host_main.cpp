// Stand-alone driver of the C++ mirror's pure list logic (ov_plane_featdb_select.h), built with -fsanitize=address,undefined by
// tests/test_featdb_cpu.py and run as its own program.  Input: "n n_landmarks max_slam ok", n lines "id cls", the landmark ids.
// Output: six lines, each a count followed by the ids - lost, marg, maxtracks, slam_delayed, slam_update, landmarks_marg.
#include <cstdio>
#include <fstream>

#include "ov_plane_featdb_select.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  long long n = 0, nl = 0, max_slam = 0, ok = 0;
  if (!(in >> n >> nl >> max_slam >> ok)) return 3;
  std::vector<int64_t> ids(n), lms(nl);
  std::vector<int> cls(n);
  for (long long i = 0; i < n; ++i) {
    long long id;
    if (!(in >> id >> cls[i])) return 3;
    ids[i] = id;
  }
  for (long long i = 0; i < nl; ++i) {
    long long id;
    if (!(in >> id)) return 3;
    lms[i] = id;
  }
  const ov_plane::FeatDbSelection s = ov_plane::featdb_select(ids, cls, lms, (int)max_slam, ok != 0);
  for (const std::vector<int64_t>* v : {&s.lost, &s.marg, &s.maxtracks, &s.slam_delayed, &s.slam_update, &s.landmarks_marg}) {
    std::printf("%zu", v->size());
    for (int64_t x : *v) std::printf(" %lld", (long long)x);
    std::printf("\n");
  }
  return 0;
}
