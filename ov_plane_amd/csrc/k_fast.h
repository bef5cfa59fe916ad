// Feature detection of the image front end: Grider_FAST::perform_griding as TrackPlane::perform_detection_monocular calls it
// (track_plane/TrackPlane.cpp:1262) - cv::FAST with non-maximum suppression per grid cell, the K strongest of a cell, then
// cv::cornerSubPix on the whole image.  Grider_FAST (ov_core) and OpenCV are not in the reference tree: the stage is RECALLED from
// its published form and UNPINNED; tests/fast_ref.py is the restatement these kernels are held to and names every convention.
//   k_fast_score_nms  a workgroup per 64 x 16 tile: the tile and a 4-pixel ring in LDS, the FAST-9/16 score of the tile and a
//                     1-pixel ring in LDS, suppression against the 8 neighbours; writes both maps.  A pixel is tested when it lies
//                     at least 3 from every edge of ITS cell, so the 8 neighbours of a tested pixel are pixels of the same cell and
//                     the untested ones score 0: suppression on the image-wide map never consults another cell.
//   k_fast_select     a workgroup per cell: K rounds of a maximum over the key (score << 32 | ~raster index) - score descending,
//                     ties in raster order (our rule).  A lane keeps its own best key below the last winner and only the winner's
//                     lane scans again.  No atomics: the order is the key's.
//   k_fast_subpix     one wave per slot: the 11 x 11 window at two pixels per lane, patch values and gradients in float without
//                     contraction, the five sums in double through a fixed xor butterfly - two runs give the same bits.
// Address safety: k_fast_score_nms and k_fast_subpix clamp every image coordinate into the level; k_fast_select reads the cells,
// which lie inside the image by construction (ct_cols size_x <= cols, ct_rows size_y <= rows).
#pragma once
#include <cfloat>

namespace {

constexpr int FAST_TW = 64, FAST_TH = 16, FAST_RING = 4, FAST_MAX_K = 256, FAST_MAX_CELLS = 4096;
constexpr int FAST_SUB_HALF = 5, FAST_SUB_WIN = 11, FAST_SUB_ITERS = 20;

struct FastGrid {
  int cols, rows, size_x, size_y, ct_cols, ct_rows, K;
};

// tested by cv::FAST on the cell as an image of its own: at least 3 from every edge of the cell; the strips right of and below the
// cells belong to none
__device__ __forceinline__ bool fast_tested(int x, int y, const FastGrid& g) {
  if (x < 0 || y < 0 || x >= g.ct_cols * g.size_x || y >= g.ct_rows * g.size_y) return false;
  const int lx = x % g.size_x, ly = y % g.size_y;
  return lx >= 3 && lx < g.size_x - 3 && ly >= 3 && ly < g.size_y - 3;
}

// the largest threshold the pixel is still a corner at, 0 for a non-corner: with m the largest, over the 16 arcs of 9, of
// max(min_k (v - p_k), min_k (p_k - v)), the pixel is a corner iff m > thr, and scores m - 1
__device__ __forceinline__ int fast_score(const unsigned char* t, int pitch, int thr) {
  constexpr int DX[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
  constexpr int DY[16] = {-3, -3, -2, -1, 0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3};
  const int v = t[0];
  int d[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) d[k] = (int)t[DY[k] * pitch + DX[k]] - v;
  int m = -256;
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    int lo = d[s], hi = d[s];
#pragma unroll
    for (int k = 1; k < 9; ++k) lo = min(lo, d[(s + k) & 15]), hi = max(hi, d[(s + k) & 15]);
    m = max(m, max(lo, -hi));
  }
  return m > thr ? m - 1 : 0;
}

__global__ __launch_bounds__(256) void k_fast_score_nms(const unsigned char* __restrict__ img, FastGrid g, int thr,
                                                        unsigned char* __restrict__ score, unsigned char* __restrict__ nms) {
  constexpr int IW = FAST_TW + 2 * FAST_RING, IH = FAST_TH + 2 * FAST_RING, SW = FAST_TW + 2, SH = FAST_TH + 2;
  __shared__ unsigned char tile[IH * IW];
  __shared__ unsigned char sc[SH * SW];
  const int bx = blockIdx.x * FAST_TW, by = blockIdx.y * FAST_TH, t = threadIdx.x;
  for (int i = t; i < IW * IH; i += 256) {
    const int ly = i / IW, lx = i - ly * IW;
    const int x = min(max(bx + lx - FAST_RING, 0), g.cols - 1), y = min(max(by + ly - FAST_RING, 0), g.rows - 1);
    tile[i] = img[(size_t)y * g.cols + x];
  }
  __syncthreads();
  for (int i = t; i < SW * SH; i += 256) {
    const int ly = i / SW, lx = i - ly * SW;
    const int x = bx + lx - 1, y = by + ly - 1;
    sc[i] = fast_tested(x, y, g) ? (unsigned char)fast_score(tile + (ly + FAST_RING - 1) * IW + lx + FAST_RING - 1, IW, thr) : 0;
  }
  __syncthreads();
  for (int i = t; i < FAST_TW * FAST_TH; i += 256) {
    const int ly = i / FAST_TW, lx = i - ly * FAST_TW;
    const int x = bx + lx, y = by + ly;
    if (x >= g.cols || y >= g.rows) continue;
    const unsigned char* c = sc + (ly + 1) * SW + lx + 1;
    const int s = c[0];
    const int nb = max(max(max(c[-SW - 1], c[-SW]), max(c[-SW + 1], c[-1])), max(max(c[1], c[SW - 1]), max(c[SW], c[SW + 1])));
    score[(size_t)y * g.cols + x] = (unsigned char)s;
    nms[(size_t)y * g.cols + x] = s > nb ? (unsigned char)s : 0;  // strictly greater than all 8
  }
}

__global__ __launch_bounds__(256) void k_fast_select(const unsigned char* __restrict__ nms, FastGrid g, int* __restrict__ out_xy,
                                                     int* __restrict__ out_resp) {
  __shared__ unsigned long long red[4];
  const int r = blockIdx.x, t = threadIdx.x;
  const int x0 = (r % g.ct_cols) * g.size_x, y0 = (r / g.ct_cols) * g.size_y;
  const unsigned npx = (unsigned)g.size_x * (unsigned)g.size_y;
  auto best_below = [&](unsigned long long bound) {
    unsigned long long b = 0ull;
    for (unsigned i = t; i < npx; i += 256u) {
      const unsigned ly = i / (unsigned)g.size_x, lx = i - ly * (unsigned)g.size_x;
      const unsigned s = nms[(size_t)(y0 + ly) * g.cols + x0 + lx];
      if (!s) continue;
      const unsigned long long key = ((unsigned long long)s << 32) | (0xFFFFFFFFu - i);  // score first, then the earlier pixel
      if (key < bound && key > b) b = key;
    }
    return b;
  };
  unsigned long long mine = best_below(~0ull);
  for (int j = 0; j < g.K; ++j) {
    unsigned long long w = mine;
    for (int m = 32; m >= 1; m >>= 1) {
      const unsigned long long o = __shfl_xor(w, m, 64);
      w = o > w ? o : w;
    }
    if ((t & 63) == 0) red[t >> 6] = w;
    __syncthreads();
    w = red[0];
    for (int k = 1; k < 4; ++k) w = red[k] > w ? red[k] : w;
    __syncthreads();
    if (t == 0) {
      const size_t slot = (size_t)r * g.K + j;
      if (w) {
        const unsigned i = 0xFFFFFFFFu - (unsigned)(w & 0xFFFFFFFFull);
        out_xy[2 * slot] = x0 + (int)(i % (unsigned)g.size_x), out_xy[2 * slot + 1] = y0 + (int)(i / (unsigned)g.size_x);
        out_resp[slot] = (int)(w >> 32);
      } else {
        for (int q = j; q < g.K; ++q) out_xy[2 * ((size_t)r * g.K + q)] = 0, out_xy[2 * ((size_t)r * g.K + q) + 1] = 0, out_resp[(size_t)r * g.K + q] = 0;
      }
    }
    if (!w) break;  // (block-uniform: every lane holds the same w)
    if (mine == w) mine = best_below(w);
  }
}

struct FastSubpixArgs {
  const unsigned char* img;
  int cols, rows, n;
  const int *xy, *resp;  // [2n], [n]: a slot with response 0 is empty
  const float* start;    // NULL: the refinement starts at xy; else [2n] starting positions of the caller's (ovp_klt_debug "refine")
  float* out;            // [2n]
  float w[FAST_SUB_WIN];  // exp(-x^2), x = (j - 5) / 5, rounded to float on the host
};

__device__ __forceinline__ double fast_wave_sum(double v) {  // xor butterfly: a fixed order, the same bits in every lane
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

__global__ __launch_bounds__(256) void k_fast_subpix(FastSubpixArgs a) {
  const int lane = threadIdx.x & 63, pt = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pt >= a.n) return;  // (wave-uniform; the kernel has no barrier)
  if (a.resp[pt] == 0) {
    if (lane == 0) a.out[2 * pt] = 0.f, a.out[2 * pt + 1] = 0.f;
    return;
  }
  const float sx = a.start ? a.start[2 * pt] : (float)a.xy[2 * pt], sy = a.start ? a.start[2 * pt + 1] : (float)a.xy[2 * pt + 1];
  int wi[2], wj[2];
  double wm[2];
  for (int q = 0; q < 2; ++q) {
    const int k = lane + 64 * q;
    wi[q] = k / FAST_SUB_WIN, wj[q] = k - wi[q] * FAST_SUB_WIN;
    wm[q] = k < FAST_SUB_WIN * FAST_SUB_WIN ? (double)__fmul_rn(a.w[wi[q] % FAST_SUB_WIN], a.w[wj[q]]) : 0.0;
  }
  float cx = sx, cy = sy;
  int it = 0;
  double err = 0.0;
  do {
    // getRectSubPix: the 13 x 13 patch's origin, bilinear weights; replicated border (every coordinate clamped into the image)
    const float ox = cx - (float)(FAST_SUB_HALF + 1), oy = cy - (float)(FAST_SUB_HALF + 1);
    const float fx = floorf(ox), fy = floorf(oy);
    const float ca = ox - fx, cb = oy - fy;
    const int ix = (int)fminf(fmaxf(fx, -1073741824.f), 1073741824.f), iy = (int)fminf(fmaxf(fy, -1073741824.f), 1073741824.f);
    const float w00 = __fmul_rn(1.0f - ca, 1.0f - cb), w01 = __fmul_rn(ca, 1.0f - cb), w10 = __fmul_rn(1.0f - ca, cb), w11 = __fmul_rn(ca, cb);
    auto P = [&](int r, int c) {  // patch[r][c], float, evaluated left to right without contraction
      const int xa = min(max(ix + c, 0), a.cols - 1), xb = min(max(ix + c + 1, 0), a.cols - 1);
      const unsigned char *r0 = a.img + (size_t)min(max(iy + r, 0), a.rows - 1) * a.cols, *r1 = a.img + (size_t)min(max(iy + r + 1, 0), a.rows - 1) * a.cols;
      float v = __fmul_rn(w00, (float)r0[xa]);
      v = __fadd_rn(v, __fmul_rn(w01, (float)r0[xb]));
      v = __fadd_rn(v, __fmul_rn(w10, (float)r1[xa]));
      return __fadd_rn(v, __fmul_rn(w11, (float)r1[xb]));
    };
    double sa = 0.0, sb = 0.0, sc = 0.0, s1 = 0.0, s2 = 0.0;
    for (int q = 0; q < 2; ++q) {
      if (lane + 64 * q >= FAST_SUB_WIN * FAST_SUB_WIN) continue;
      const int i = wi[q], j = wj[q];
      const double gx = (double)__fsub_rn(P(i + 1, j + 2), P(i + 1, j)), gy = (double)__fsub_rn(P(i + 2, j + 1), P(i, j + 1));
      const double gxx = gx * gx * wm[q], gxy = gx * gy * wm[q], gyy = gy * gy * wm[q];
      const double px = (double)(j - FAST_SUB_HALF), py = (double)(i - FAST_SUB_HALF);
      sa += gxx, sb += gxy, sc += gyy;
      s1 += gxx * px + gxy * py, s2 += gxy * px + gyy * py;
    }
    sa = fast_wave_sum(sa), sb = fast_wave_sum(sb), sc = fast_wave_sum(sc), s1 = fast_wave_sum(s1), s2 = fast_wave_sum(s2);
    const double det = sa * sc - sb * sb;
    if (fabs(det) <= DBL_EPSILON * DBL_EPSILON) break;
    const double scale = 1.0 / det;
    const float nx = (float)((double)cx + sc * scale * s1 - sb * scale * s2), ny = (float)((double)cy - sb * scale * s1 + sa * scale * s2);
    err = ((double)nx - (double)cx) * ((double)nx - (double)cx) + ((double)ny - (double)cy) * ((double)ny - (double)cy);
    cx = nx, cy = ny;
    if (!(cx >= 0.f && cx < (float)a.cols && cy >= 0.f && cy < (float)a.rows)) break;  // left the image (or not a number)
  } while (++it < FAST_SUB_ITERS && err > 1e-6);
  // more than the half window from the start in x or y: the start
  if (!(fabsf(cx - sx) <= (float)FAST_SUB_HALF && fabsf(cy - sy) <= (float)FAST_SUB_HALF)) cx = sx, cy = sy;
  if (lane == 0) a.out[2 * pt] = cx, a.out[2 * pt + 1] = cy;
}

}  // namespace
