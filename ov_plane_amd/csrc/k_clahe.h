// Contrast-limited adaptive equalisation of the image front end: TrackPlane::feed_new_camera with histogram_method CLAHE
// (track_plane/TrackPlane.cpp:66-70: cv::createCLAHE(10.0, Size(8, 8))->apply).  OpenCV is not in the reference tree: the stage is
// RECALLED from the published clahe.cpp and UNPINNED; tests/clahe_ref.py is the restatement these kernels are held to and names
// every convention.  Included by k_klt.hip behind klt_reflect, which both kernels' image addresses go through.
//   k_clahe_lut    a workgroup of 256 threads per tile: the tile's 256-bin histogram in LDS (LDS atomics: integer, so the order does
//                  not matter), its pixels read from the raw image through the reflect-101 index map - the extended image is never
//                  made; thread t then owns bin t: the excess over the clip limit summed over the workgroup (xor butterfly, four
//                  partial sums in LDS), the batch and the strided residual added, an inclusive prefix sum (shuffle scan per wave,
//                  the waves' totals through LDS) and the bin's LUT byte written to the tiles x 256 table.
//   k_clahe_apply  a thread per pixel: two tile indices and weights per axis, four LUT reads, the bilinear blend in float without
//                  contraction (plain operators under `#pragma clang fp contract(off)`, in clahe.cpp's order), rounded half to even.
// Address safety: k_clahe_lut maps every coordinate through klt_reflect into the image; k_clahe_apply reads and writes pixel
// i < cols rows alone, and its tile indices are clamped into [0, tiles) before the table is read.
#pragma once

namespace {

constexpr int CLAHE_MAX_TILES = 16, CLAHE_BINS = 256;

struct ClaheGeom {
  int cols, rows;                        // the image the equalisation reads
  int tiles_x, tiles_y, tile_w, tile_h;  // tile size = extended size / tiles
  int clip;                              // bins above it are cut to it; 0: no clipping
  float lut_scale, inv_tw, inv_th;       // 255 / tile area, 1 / tile_w, 1 / tile_h: float divisions on the host
};

// clahe.cpp's geometry.  The image is extended (reflect-101, right and bottom) when EITHER axis is not divisible, and then on BOTH:
// a divisible axis grows by a whole `tiles`.  clip = max((int)(clip_limit * area / 256), 1) for clip_limit > 0, in double; a
// value of the area or above clips nothing and is held at the area (no bin exceeds it), which keeps the conversion in range.
inline void clahe_geom(int cols, int rows, int tiles_x, int tiles_y, double clip_limit, ClaheGeom* g) {
  int ew = cols, eh = rows;
  if (cols % tiles_x != 0 || rows % tiles_y != 0) ew += tiles_x - cols % tiles_x, eh += tiles_y - rows % tiles_y;
  g->cols = cols, g->rows = rows, g->tiles_x = tiles_x, g->tiles_y = tiles_y;
  g->tile_w = ew / tiles_x, g->tile_h = eh / tiles_y;
  const int area = g->tile_w * g->tile_h;  // (at most (16384 + 16)^2 < 2^31)
  g->clip = 0;
  if (clip_limit > 0.0) {
    const double v = clip_limit * (double)area / (double)CLAHE_BINS;
    g->clip = v >= (double)area ? area : (int)v < 1 ? 1 : (int)v;
  }
  g->lut_scale = 255.0f / (float)area, g->inv_tw = 1.0f / (float)g->tile_w, g->inv_th = 1.0f / (float)g->tile_h;
}

__global__ __launch_bounds__(256) void k_clahe_lut(const unsigned char* __restrict__ img, ClaheGeom g, unsigned char* __restrict__ lut) {
  __shared__ unsigned hist[CLAHE_BINS];
  __shared__ int excess[4], total[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int tile = blockIdx.x, ty = tile / g.tiles_x, tx = tile - ty * g.tiles_x;
  hist[t] = 0u;
  __syncthreads();
  const int x0 = tx * g.tile_w, y0 = ty * g.tile_h, npx = g.tile_w * g.tile_h;
  for (int i = t; i < npx; i += 256) {
    const int ly = i / g.tile_w, lx = i - ly * g.tile_w;
    atomicAdd(&hist[img[(size_t)klt_reflect(y0 + ly, g.rows) * g.cols + klt_reflect(x0 + lx, g.cols)]], 1u);
  }
  __syncthreads();
  int v = (int)hist[t];  // thread t owns bin t from here on
  if (g.clip > 0) {      // (block-uniform)
    int ex = max(v - g.clip, 0);
    v = min(v, g.clip);
    for (int m = 32; m >= 1; m >>= 1) ex += __shfl_xor(ex, m, 64);
    if (lane == 0) excess[wave] = ex;
    __syncthreads();
    ex = excess[0] + excess[1] + excess[2] + excess[3];
    const int batch = ex / CLAHE_BINS, residual = ex - batch * CLAHE_BINS;
    v += batch;
    if (residual) {  // bins 0, step, 2 step, .. get one more each while the residual lasts
      const int step = max(CLAHE_BINS / residual, 1);
      if (t % step == 0 && t / step < residual) ++v;
    }
  }
  int s = v;  // inclusive prefix sum over the 256 bins
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(s, d, 64);
    if (lane >= d) s += o;
  }
  if (lane == 63) total[wave] = s;
  __syncthreads();
  for (int k = 0; k < wave; ++k) s += total[k];
  lut[(size_t)tile * CLAHE_BINS + t] = (unsigned char)fminf(255.0f, rintf((float)s * g.lut_scale));  // (one product: nothing to fuse)
}

__global__ __launch_bounds__(256) void k_clahe_apply(const unsigned char* __restrict__ src, ClaheGeom g, const unsigned char* __restrict__ lut,
                                                     unsigned char* __restrict__ dst) {
  // plain operators under contract(off): every product and sum rounds once, as the float32 restatement's do.  (__fmul_rn and
  // __fadd_rn would not do it: the header defines them as plain operators of its own, which the compiler fuses into v_fma_f32.)
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= g.cols * g.rows) return;
  const int y = i / g.cols, x = i - y * g.cols;
  // the weight is taken from the unclamped index, the clamp comes after it
  const float txf = (float)x * g.inv_tw - 0.5f, tyf = (float)y * g.inv_th - 0.5f;
  const float fx = floorf(txf), fy = floorf(tyf);
  const float xa = txf - fx, ya = tyf - fy;
  const float xa1 = 1.0f - xa, ya1 = 1.0f - ya;
  // (fx lies in [-1, tiles - 1]: x < cols <= tiles tile_w; the second bound of each index is for the address alone)
  const int tx1 = min(max((int)fx, 0), g.tiles_x - 1), tx2 = max(min((int)fx + 1, g.tiles_x - 1), 0);
  const int ty1 = min(max((int)fy, 0), g.tiles_y - 1), ty2 = max(min((int)fy + 1, g.tiles_y - 1), 0);
  const int v = src[i];
  const unsigned char *p1 = lut + (size_t)ty1 * g.tiles_x * CLAHE_BINS + v, *p2 = lut + (size_t)ty2 * g.tiles_x * CLAHE_BINS + v;
  const float a = (float)p1[tx1 * CLAHE_BINS], b = (float)p1[tx2 * CLAHE_BINS], c = (float)p2[tx1 * CLAHE_BINS], d = (float)p2[tx2 * CLAHE_BINS];
  const float top = a * xa1 + b * xa, bot = c * xa1 + d * xa;
  const float res = top * ya1 + bot * ya;
  dst[i] = (unsigned char)fminf(255.0f, fmaxf(0.0f, rintf(res)));
}

}  // namespace
