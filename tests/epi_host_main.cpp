// The host logic of ov_plane::TrackPlane's epipolar frame (matching_frame over matching: feed_monocular :510-567 and
// perform_matching :1299-1357) with the two device calls stubbed by what the input file holds - tests/test_epipolar_cpu.py writes
// it from the restatement.  Input: "w h has_mask", the mask, "n", n lines "id x y" (float bits in hex), "m" (0: the stubs must not
// be called), m lines "x y status mask_rsc un vn".  Output: "reset track_calls k", k lines "id x y un vn".
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>

#include "ov_plane_trackplane.h"

static float bits(const std::string &s) {
  const uint32_t u = (uint32_t)std::stoul(s, nullptr, 16);
  float f;
  memcpy(&f, &u, 4);
  return f;
}
static unsigned hex(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  int w, h, has_mask, n, m;
  in >> w >> h >> has_mask;
  std::vector<uint8_t> mask;
  if (has_mask) {
    mask.resize((size_t)w * h);
    for (auto &v : mask) {
      int x;
      in >> x;
      v = (uint8_t)x;
    }
  }
  in >> n;
  std::vector<size_t> ids(n);
  std::vector<float> pts(2 * (size_t)n);
  std::string a, b;
  for (int i = 0; i < n; ++i) {
    in >> ids[i] >> a >> b;
    pts[2 * i] = bits(a), pts[2 * i + 1] = bits(b);
  }
  in >> m;
  std::vector<float> moved(2 * (size_t)m), un(2 * (size_t)m);
  std::vector<uint8_t> st(m), rsc(m);
  for (int i = 0; i < m; ++i) {
    int s, r;
    std::string c, d;
    in >> a >> b >> s >> r >> c >> d;
    moved[2 * i] = bits(a), moved[2 * i + 1] = bits(b), st[i] = (uint8_t)s, rsc[i] = (uint8_t)r, un[2 * i] = bits(c), un[2 * i + 1] = bits(d);
  }
  int track_calls = 0;
  bool reset = false;
  std::vector<float> uvn, match_pts;
  std::vector<uint8_t> match_mask;
  using ov_plane::TrackPlane;
  const int rc = TrackPlane::matching_frame(
      w, h, has_mask ? mask.data() : nullptr, ids, pts, uvn, match_pts, match_mask, reset,
      [&](const std::vector<float> &p0, std::vector<float> &p1, std::vector<uint8_t> &mo, std::vector<float> &u1) {
        return TrackPlane::matching(
            p0, p1, mo, u1,
            [&](const std::vector<float> &, std::vector<float> &q1, std::vector<uint8_t> &mk) {
              ++track_calls;
              if ((int)q1.size() != 2 * m) return 1;
              q1 = moved, mk = st;
              return 0;
            },
            [&](const std::vector<float> &, const std::vector<float> &, const std::vector<uint8_t> &mk, std::vector<uint8_t> &out,
                std::vector<float> &u) {
              for (size_t i = 0; i < mk.size(); ++i) out[i] = mk[i] && rsc[i];  // :1348
              u = un;
              return 0;
            });
      });
  if (rc) return 3;
  printf("%d %d %zu\n", reset ? 1 : 0, track_calls, ids.size());
  for (size_t i = 0; i < ids.size(); ++i)
    printf("%zu %08x %08x %08x %08x\n", ids[i], hex(pts[2 * i]), hex(pts[2 * i + 1]), hex(uvn[2 * i]), hex(uvn[2 * i + 1]));
  return 0;
}
