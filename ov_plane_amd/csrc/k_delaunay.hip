// Delaunay triangulation of a frame's pixel positions on the device: ovp_delaunay_host (host/ov_plane_delaunay.h) restated for ONE
// workgroup - the same incremental Bowyer-Watson with a ghost vertex, the same seeds, insertion order and predicates, the same
// output (real triangles of positive orientation, smallest index first, sorted), bit for bit.
//   coordinates and the triangle table live in LDS; per insertion every thread tests its own table slots (one in-circle test
//   each), the bad ones are compacted by a block prefix sum, the cavity's boundary is found in parallel over the 3 n_bad directed
//   edges of the bad triangles (an edge is on the boundary when its reverse is not among them; an edge that appears twice counts
//   once, as in the host's map), and the new triangles fill the freed slots first and are then appended.
// The table is a SET as far as the algorithm goes - nothing depends on the order of its slots - and every position in it is given
// out by a prefix sum: no atomics, two runs give the same bits.  Every loop is bounded by the point count or the table size; no
// spin-wait, no second workgroup.
// The final sort runs in the kernel: the keys are distinct 30-bit numbers already in LDS, so each one's rank is the count of
// smaller keys (at most 2 x 2046 broadcast reads per thread, one barrier) - the host's part of a publication stays a copy.
// Predicates: the f64 expressions of ovp_delaunay_detail::orient / incircle on the f32 coordinates in the same operation order,
// with contraction off (the x86 host build has no fused multiply-add; a contracted device predicate can take another sign on
// near-degenerate input).
#include <algorithm>

#include "ovp_kernels.h"
#include "ovplane_hip.h"
#include "k_delaunay.h"

namespace {

constexpr int DL_MAXP = OVP_DET_MAX_POINTS;
constexpr int DL_CAP = 2 * DL_MAXP;  // table slots: a consistent triangulation of n points holds at most 2n - 2, ghosts included
constexpr int DL_GHOST = -1, DL_DEAD = -2;
constexpr int DL_WAVES = 16;

__device__ __forceinline__ double dl_orient(float xa, float ya, float xb, float yb, float xc, float yc) {
#pragma clang fp contract(off)
  const double ax = xa, ay = ya;
  return ((double)xb - ax) * ((double)yc - ay) - ((double)yb - ay) * ((double)xc - ax);
}

__device__ __forceinline__ double dl_incircle(float xa, float ya, float xb, float yb, float xc, float yc, float xp, float yp) {
#pragma clang fp contract(off)
  const double px = xp, py = yp;
  const double ax = xa - px, ay = ya - py, bx = xb - px, by = yb - py, cx = xc - px, cy = yc - py;
  const double a2 = ax * ax + ay * ay, b2 = bx * bx + by * by, c2 = cx * cx + cy * cy;
  return ax * (by * c2 - b2 * cy) - ay * (bx * c2 - b2 * cx) + a2 * (bx * cy - by * cx);
}

// exclusive prefix sum of v over the workgroup (thread order) and the total; ws: DL_WAVES ints of LDS that nobody else touches
// until every thread has left the call after this one's barrier
__device__ __forceinline__ int dl_scan(int v, int* ws, int& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(inc, d);
    if (lane >= d) inc += o;
  }
  if (lane == 63) ws[w] = inc;
  __syncthreads();
  int base = 0, sum = 0;
  for (int k = 0; k < nw; ++k) {
    const int s = ws[k];
    base += k < w ? s : 0;
    sum += s;
  }
  total = sum;
  return base + inc - v;
}

// minimum of v over the workgroup (same rule for ws)
__device__ __forceinline__ int dl_min(int v, int* ws) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = min(v, __shfl_xor(v, d));
  if (lane == 0) ws[w] = v;
  __syncthreads();
  int m = ws[0];
  for (int k = 1; k < nw; ++k) m = min(m, ws[k]);
  return m;
}

__device__ __forceinline__ int dl_edge_key(int u, int v) { return ((u + 1) << 11) | (v + 1); }  // u, v in -1 .. 1023

// blockDim.x: a multiple of 64, 64 .. 1024 (so a thread owns at most 32 table slots: the mask below)
__global__ __launch_bounds__(1024) void k_det_delaunay(int n, const float* __restrict__ xy, const int* __restrict__ flag,
                                                       int* __restrict__ hdr, int* __restrict__ tris, int tri_cap) {
  __shared__ float px[DL_MAXP], py[DL_MAXP];
  __shared__ short tv0[DL_CAP], tv1[DL_CAP], tv2[DL_CAP];  // the triangle table (tv0 = DL_DEAD: an empty slot)
  __shared__ short badlist[DL_CAP];                        // slots of the bad triangles = the slots that come free
  __shared__ int ekey[3 * DL_CAP];                         // their directed edges; the sort keys at the end
  __shared__ unsigned char isb[3 * DL_CAP];                // edge is on the cavity's boundary (written and read by its owner)
  __shared__ int ws[7][DL_WAVES];
  const int t = threadIdx.x, B = blockDim.x;

  // ---- vertices: the flagged points, in point order ----
  int nv = 0;
  {
    const int chunk = (n + B - 1) / B, lo = min(t * chunk, n), hi = min(lo + chunk, n);
    int cnt = 0;
    for (int i = lo; i < hi; ++i) cnt += flag ? (flag[i] & 1) : 1;
    int at = dl_scan(cnt, ws[3], nv);
    for (int i = lo; i < hi; ++i)
      if (!flag || (flag[i] & 1)) {
        px[at] = xy[2 * i], py[at] = xy[2 * i + 1];  // (at < nv <= n <= DL_MAXP)
        ++at;
      }
  }
  __syncthreads();
  int n_out = 0, overflow = 0, peak = 0, max_cav = 0;
  // ---- seeds: point 0, the first point at another position, the first point off the line through the two ----
  int k1 = DL_MAXP, k0 = DL_MAXP;
  if (nv >= 3) {
    int m = DL_MAXP;
    const float x0 = px[0], y0 = py[0];
    for (int k = 1 + t; k < nv; k += B)
      if (px[k] != x0 || py[k] != y0) {
        m = k;
        break;
      }
    k1 = dl_min(m, ws[4]);
    if (k1 < nv) {
      m = DL_MAXP;
      const float x1 = px[k1], y1 = py[k1];
      for (int k = 1 + t; k < nv; k += B)
        if (k != k1 && dl_orient(x0, y0, x1, y1, px[k], py[k]) != 0.0) {
          m = k;
          break;
        }
      k0 = dl_min(m, ws[5]);
    }
  }
  if (k0 < nv) {  // (uniform: nv, k1 and k0 are the same in every thread)
    int T = 4;
    if (t == 0) {
      int a = 0, b = k1, c = k0;
      if (dl_orient(px[a], py[a], px[b], py[b], px[c], py[c]) < 0.0) {
        const int s = b;
        b = c, c = s;
      }
      tv0[0] = a, tv1[0] = b, tv2[0] = c;
      tv0[1] = b, tv1[1] = a, tv2[1] = DL_GHOST;
      tv0[2] = c, tv1[2] = b, tv2[2] = DL_GHOST;
      tv0[3] = a, tv1[3] = c, tv2[3] = DL_GHOST;
    }
    __syncthreads();
    peak = T;
    int it = 0;
    for (int p = 1; p < nv; ++p) {
      if (p == k0 || p == k1) continue;
      const float xp = px[p], yp = py[p];
      // -- every thread tests its own slots t, t + B, ... (T <= DL_CAP = 32 * 64: at most 32 of them) --
      unsigned mask = 0;
      int cnt = 0;
      for (int s = t, r = 0; s < T; s += B, ++r) {
        const int a = tv0[s], b = tv1[s], c = tv2[s];
        if (a == DL_DEAD) continue;
        bool bad;
        if (a == DL_GHOST)
          bad = dl_orient(px[b], py[b], px[c], py[c], xp, yp) > 0.0;
        else if (b == DL_GHOST)
          bad = dl_orient(px[c], py[c], px[a], py[a], xp, yp) > 0.0;
        else if (c == DL_GHOST)
          bad = dl_orient(px[a], py[a], px[b], py[b], xp, yp) > 0.0;
        else
          bad = dl_incircle(px[a], py[a], px[b], py[b], px[c], py[c], xp, yp) > 0.0;
        if (bad) mask |= 1u << r, ++cnt;
      }
      // (the wave sums alternate between two buffers: an insertion without a bad triangle has no further barrier)
      int nbad;
      int off = dl_scan(cnt, ws[it & 1], nbad);
      ++it;
      if (nbad == 0) continue;  // a duplicate of a vertex: left out
      // -- the bad slots and their directed edges, compacted (off < nbad <= T <= DL_CAP) --
      for (unsigned mm = mask; mm; mm &= mm - 1) {
        const int s = t + __builtin_ctz(mm) * B;
        const int a = tv0[s], b = tv1[s], c = tv2[s];
        badlist[off] = (short)s;
        ekey[3 * off] = dl_edge_key(a, b), ekey[3 * off + 1] = dl_edge_key(b, c), ekey[3 * off + 2] = dl_edge_key(c, a);
        ++off;
      }
      __syncthreads();
      // -- boundary: the edges whose reverse is not among them, the first of equal ones --
      const int E = 3 * nbad;
      int nb = 0;
      for (int e = t; e < E; e += B) {
        const int k = ekey[e], rk = ((k & 2047) << 11) | (k >> 11);
        bool bnd = true;
        for (int j = 0; j < E; ++j) {
          const int kj = ekey[j];
          if (kj == rk || (kj == k && j < e)) {
            bnd = false;
            break;
          }
        }
        isb[e] = bnd ? 1 : 0;
        nb += bnd ? 1 : 0;
      }
      int nnew;
      int pos = dl_scan(nb, ws[2], nnew);
      const int grow = nnew > nbad ? nnew - nbad : 0;
      if (T + grow > DL_CAP) {  // only after inconsistent predicate signs: stop, nothing is written
        overflow = 1;
        break;
      }
      // -- a new triangle (u, v, p) per boundary edge: into the freed slots first, then behind the table --
      for (int e = t; e < E; e += B)
        if (isb[e]) {
          const int slot = pos < nbad ? (int)badlist[pos] : T + (pos - nbad);  // (< T + grow <= DL_CAP)
          const int k = ekey[e];
          tv0[slot] = (short)((k >> 11) - 1), tv1[slot] = (short)((k & 2047) - 1), tv2[slot] = (short)p;
          ++pos;
        }
      for (int j = nnew + t; j < nbad; j += B) tv0[badlist[j]] = DL_DEAD;  // fewer new ones than freed slots: the rest stay empty
      T += grow;
      peak = max(peak, T);
      max_cav = max(max_cav, nbad);
      __syncthreads();
    }
    // ---- output: real triangles of positive orientation, smallest index first, sorted ----
    if (!overflow) {
      unsigned mask = 0;
      int cnt = 0;
      for (int s = t, r = 0; s < T; s += B, ++r) {
        const int a = tv0[s], b = tv1[s], c = tv2[s];
        if (a < 0 || b < 0 || c < 0) continue;
        if (dl_orient(px[a], py[a], px[b], py[b], px[c], py[c]) > 0.0) mask |= 1u << r, ++cnt;
      }
      int m;
      int at = dl_scan(cnt, ws[6], m);
      for (unsigned mm = mask; mm; mm &= mm - 1) {
        const int s = t + __builtin_ctz(mm) * B;
        const int a = tv0[s], b = tv1[s], c = tv2[s];
        int key;
        if (a < b && a < c)
          key = (a << 20) | (b << 10) | c;
        else if (b < c)  // (the host's min_element: the first of equal ones - indices of one triangle differ)
          key = (b << 20) | (c << 10) | a;
        else
          key = (c << 20) | (a << 10) | b;
        ekey[at++] = key;  // (at < m <= T <= DL_CAP)
      }
      __syncthreads();
      if (m > tri_cap)
        overflow = 1;
      else {
        for (int i = t; i < m; i += B) {
          const int k = ekey[i];
          int rank = 0;
          for (int j = 0; j < m; ++j) {
            const int kj = ekey[j];
            rank += (kj < k || (kj == k && j < i)) ? 1 : 0;
          }
          tris[3 * rank] = k >> 20, tris[3 * rank + 1] = (k >> 10) & 1023, tris[3 * rank + 2] = k & 1023;  // (rank < m <= tri_cap)
        }
        n_out = m;
      }
    }
  }
  if (t == 0) {
    hdr[0] = overflow ? 0 : n_out, hdr[1] = overflow, hdr[2] = nv, hdr[3] = peak, hdr[4] = max_cav;
    for (int k = 5; k < OVP_DL_HDR; ++k) hdr[k] = 0;
  }
}

}  // namespace

extern "C" hipError_t ovp_launch_delaunay(int n, const float* xy, const int* flag, int* hdr, int* tris, int tri_cap, hipStream_t stream) {
  if (n < 0 || n > DL_MAXP || tri_cap < 0) return hipErrorInvalidValue;
  // two table slots per point, one slot per thread where that fits: fewer waves make the barriers of a small frame cheaper
  const int B = std::min(1024, std::max(64, (2 * n + 63) / 64 * 64));
  hipLaunchKernelGGL(k_det_delaunay, dim3(1), dim3(B), 0, stream, n, xy, flag, hdr, tris, tri_cap);
  return hipGetLastError();
}
