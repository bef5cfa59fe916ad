// Stand-alone driver of ov_plane::frame_plan (ov_plane_frame_plan.h) for tests/test_klt_frame_cpu.py, built under
// -fsanitize=address,undefined.  Input file: "n n_free", then n lines "keep fresh slot", then the free slots.  Output: one line
// "ok n_fresh_kept", then one line "index slot" per survivor.
#include <cstdio>
#include <vector>

#include "ov_plane_frame_plan.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  int n = 0, n_free = 0;
  if (fscanf(f, "%d %d", &n, &n_free) != 2 || n < 0 || n_free < 0) return 2;
  std::vector<uint8_t> keep(n), fresh(n);
  std::vector<int32_t> slot(n), free_slots(n_free);
  for (int i = 0; i < n; ++i) {
    int k, fr, s;
    if (fscanf(f, "%d %d %d", &k, &fr, &s) != 3) return 2;
    keep[i] = (uint8_t)k, fresh[i] = (uint8_t)fr, slot[i] = s;
  }
  for (int i = 0; i < n_free; ++i)
    if (fscanf(f, "%d", &free_slots[i]) != 1) return 2;
  fclose(f);
  const ov_plane::FramePlan p = ov_plane::frame_plan(n, keep.data(), fresh.data(), slot.data(), free_slots.data(), n_free);
  printf("%d %d\n", p.ok ? 1 : 0, p.n_fresh_kept);
  for (size_t k = 0; k < p.kept_index.size(); ++k) printf("%d %d\n", p.kept_index[k], p.slot[k]);
  return 0;
}
