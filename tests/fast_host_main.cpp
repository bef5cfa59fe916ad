// The host half of ov_plane::TrackPlane::perform_detection_monocular (csrc/host/ov_plane_trackplane.h) without a device: reads
//   cols rows num_features grid_x grid_y min_px_dist currid has_mask
//   [rows x cols mask values when has_mask]
//   n  then n lines: id x y            (the existing points; floats as hexadecimal bit patterns)
//   m  then m lines: xi yi rx ry       (the candidates: integer pixel, refined position as bit patterns)
// from the file given and prints: detected currid k, then k lines "id xbits ybits".  tests/test_fast_cpu.py compares them with
// tests/fast_ref.py.
#include <cstdio>
#include <cstring>

#include "ov_plane_trackplane.h"

static float from_bits(unsigned u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}
static unsigned to_bits(float f) {
  unsigned u;
  memcpy(&u, &f, 4);
  return u;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  int cols, rows, nf, gx, gy, mpd, has_mask;
  unsigned long long currid0;
  if (fscanf(f, "%d %d %d %d %d %d %llu %d", &cols, &rows, &nf, &gx, &gy, &mpd, &currid0, &has_mask) != 8) return 2;
  std::vector<uint8_t> mask;
  if (has_mask) {
    mask.resize((size_t)cols * rows);
    for (auto &v : mask) {
      int q;
      if (fscanf(f, "%d", &q) != 1) return 2;
      v = (uint8_t)q;
    }
  }
  int n;
  if (fscanf(f, "%d", &n) != 1) return 2;
  std::vector<float> pts;
  std::vector<size_t> ids;
  for (int i = 0; i < n; ++i) {
    unsigned long long id;
    unsigned xb, yb;
    if (fscanf(f, "%llu %x %x", &id, &xb, &yb) != 3) return 2;
    ids.push_back((size_t)id), pts.push_back(from_bits(xb)), pts.push_back(from_bits(yb));
  }
  int m;
  if (fscanf(f, "%d", &m) != 1) return 2;
  std::vector<int32_t> cxy;
  std::vector<float> cref;
  for (int i = 0; i < m; ++i) {
    int xi, yi;
    unsigned xb, yb;
    if (fscanf(f, "%d %d %x %x", &xi, &yi, &xb, &yb) != 4) return 2;
    cxy.push_back(xi), cxy.push_back(yi), cref.push_back(from_bits(xb)), cref.push_back(from_bits(yb));
  }
  fclose(f);
  size_t currid = (size_t)currid0;
  bool detected = false;
  const int rc = ov_plane::TrackPlane::detection_monocular(cols, rows, nf, gx, gy, mpd, has_mask ? mask.data() : nullptr, pts, ids, currid, detected,
                                                           [&](std::vector<int32_t> &xy, std::vector<float> &ref) {
                                                             xy = cxy, ref = cref;
                                                             return 0;
                                                           });
  if (rc) return 3;
  printf("%d %llu %zu\n", detected ? 1 : 0, (unsigned long long)currid, ids.size());
  for (size_t i = 0; i < ids.size(); ++i) printf("%llu %08x %08x\n", (unsigned long long)ids[i], to_bits(pts[2 * i]), to_bits(pts[2 * i + 1]));
  return 0;
}
