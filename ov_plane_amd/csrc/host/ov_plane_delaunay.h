// Delaunay triangulation of a frame's pixel positions, part of the host mirror (plain C++, also compiled into the device library's
// entry points): incremental Bowyer-Watson with a ghost vertex
// standing for the point at infinity, so that the hull comes out exact - a finite enclosing triangle loses hull triangles.  Every
// hull edge u -> v carries a ghost triangle (v, u, GHOST); a point lies "inside the circumcircle" of a ghost triangle (a, b, GHOST)
// when it is strictly left of a -> b, i.e. outside the hull across that edge.  Each insertion looks at every triangle (n <= 1024:
// about two million in-circle tests a frame).  Predicates in f64 on f32 coordinates; points in general position are assumed for
// the RESULT (its triangle set is then unique), not for termination or for the validity of the indices.
#pragma once
#include <algorithm>
#include <array>
#include <map>
#include <utility>
#include <vector>

namespace ovp_delaunay_detail {
static const int GHOST = -1;
struct Tri { int v[3]; };
inline double orient(const float* xy, int a, int b, int c) {
  const double ax = xy[2 * a], ay = xy[2 * a + 1];
  return ((double)xy[2 * b] - ax) * ((double)xy[2 * c + 1] - ay) - ((double)xy[2 * b + 1] - ay) * ((double)xy[2 * c] - ax);
}
inline double incircle(const float* xy, int a, int b, int c, int p) {  // > 0: p inside the circle of the positively oriented a, b, c
  const double px = xy[2 * p], py = xy[2 * p + 1];
  const double ax = xy[2 * a] - px, ay = xy[2 * a + 1] - py, bx = xy[2 * b] - px, by = xy[2 * b + 1] - py, cx = xy[2 * c] - px,
               cy = xy[2 * c + 1] - py;
  const double a2 = ax * ax + ay * ay, b2 = bx * bx + by * by, c2 = cx * cx + cy * cy;
  return ax * (by * c2 - b2 * cy) - ay * (bx * c2 - b2 * cx) + a2 * (bx * cy - by * cx);
}
inline bool in_circle_of(const float* xy, const Tri& t, int p) {
  for (int k = 0; k < 3; ++k)
    if (t.v[k] == GHOST) return orient(xy, t.v[(k + 1) % 3], t.v[(k + 2) % 3], p) > 0.0;
  return incircle(xy, t.v[0], t.v[1], t.v[2], p) > 0.0;
}
}  // namespace ovp_delaunay_detail

// out: the triangles, three indices each, positively oriented ((b - a) x (c - a) > 0 in (x, y)), smallest index first, sorted.
inline void ovp_delaunay_host(int n, const float* xy, std::vector<std::array<int, 3>>& out) {
  using namespace ovp_delaunay_detail;
  out.clear();
  if (n < 3) return;
  // seed: point 0, the first point at another position, the first point off the line through the two
  int k1 = -1, k0 = -1;
  for (int k = 1; k < n && k1 < 0; ++k)
    if (xy[2 * k] != xy[0] || xy[2 * k + 1] != xy[1]) k1 = k;
  for (int k = 1; k1 > 0 && k < n && k0 < 0; ++k)
    if (k != k1 && orient(xy, 0, k1, k) != 0.0) k0 = k;
  if (k0 < 0) return;
  std::vector<Tri> tris;
  {
    int a = 0, b = k1, c = k0;
    if (orient(xy, a, b, c) < 0.0) std::swap(b, c);
    tris.push_back({{a, b, c}});
    tris.push_back({{b, a, GHOST}});
    tris.push_back({{c, b, GHOST}});
    tris.push_back({{a, c, GHOST}});
  }
  std::vector<Tri> keep, bad;
  std::map<std::pair<int, int>, int> edges;
  for (int p = 1; p < n; ++p) {
    if (p == k0 || p == k1) continue;
    keep.clear();
    bad.clear();
    for (const Tri& t : tris) (in_circle_of(xy, t, p) ? bad : keep).push_back(t);
    if (bad.empty()) continue;  // (a duplicate of a vertex: left out)
    edges.clear();
    for (const Tri& t : bad)
      for (int k = 0; k < 3; ++k) edges[{t.v[k], t.v[(k + 1) % 3]}] = 1;
    tris.swap(keep);
    for (const auto& e : edges)  // the cavity's boundary: directed edges whose reverse is not a bad triangle's
      if (!edges.count({e.first.second, e.first.first})) tris.push_back({{e.first.first, e.first.second, p}});
  }
  for (const Tri& t : tris) {
    if (t.v[0] == GHOST || t.v[1] == GHOST || t.v[2] == GHOST) continue;
    if (!(orient(xy, t.v[0], t.v[1], t.v[2]) > 0.0)) continue;  // zero area (a point exactly on a hull edge): no normal to take
    const int m = (int)(std::min_element(t.v, t.v + 3) - t.v);
    out.push_back({t.v[m], t.v[(m + 1) % 3], t.v[(m + 2) % 3]});
  }
  std::sort(out.begin(), out.end());
}
