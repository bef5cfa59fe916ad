// The image front end of a camera frame: TrackPlane::feed_new_camera (track_plane/TrackPlane.cpp:40-92: cv::equalizeHist and
// cv::buildOpticalFlowPyramid), the cv::calcOpticalFlowPyrLK call of perform_matching (:1299-1357) - kernels and entry points
// (ovp_klt_*).  OpenCV is not in the reference tree: the algorithm is restated from its published form (Bouguet's pyramidal
// Lucas-Kanade with OpenCV's externally visible conventions) and is UNPINNED; tests/klt_ref.py is the restatement the device is
// held to, and names every recalled convention in one place.
//   k_klt_hist      256-bin histogram of the uploaded image: integer atomics in LDS per workgroup, then global - order-independent
//   k_klt_equalize  the LUT of cv::equalizeHist from that histogram (every workgroup builds its own copy), applied
//   k_klt_pyrdown   one level of cv::pyrDown on 8-bit data: [1 4 6 4 1] x [1 4 6 4 1], reflect-101, (sum + 128) >> 8, to the size the
//                   launch names: (w + 1) / 2 for a pyramid level, w / 2 for the intake's halving (downsample_cameras)
//   k_clahe_lut, k_clahe_apply   histogram_method CLAHE (k_clahe.h), through ovp_klt_feed_image_opts
//   k_klt_track     one wave per point, coarse to fine: a lane owns ceil(w^2 / 64) window pixels, the previous image's patch and its
//                   two Scharr gradient patches stay in registers over a level's iterations, the current image is read with four
//                   plain loads per pixel and iteration (every level of a 752 x 480 pyramid fits in L2), the five sums go through
//                   a fixed xor butterfly.  No LDS, no barrier, no atomics: two runs give the same bits.
// Address safety: every image address of every kernel goes through klt_reflect, which maps ANY int into [0, n) - whatever the
// point, the guess or the level size, no read leaves a level's allocation.
#include "ovp_ctx.h"

#include <cmath>

#include "k_fast.h"  // detection: k_fast_score_nms, k_fast_select, k_fast_subpix (ovp_klt_detect below)
#include "k_epipolar.h"  // the epipolar check: the launches of k_epipolar.hip (ovp_klt_epipolar below)
#include "k_klt_frame.h"  // the fused hand-over: k_klt_keep_append and the database's side of it (ovp_klt_match_frame below)

namespace {

constexpr int KLT_MAX_LEVELS = 8, KLT_MAX_POINTS = 4096, KLT_MIN_WIN = 3, KLT_MAX_WIN = 21;  // 21^2 = 441 pixels: 7 per lane
constexpr int KLT_MAX_ITERS = 30;                   // term_crit (:1328)
constexpr float KLT_STOP_EPS = 0.01f, KLT_OSC_EPS = 0.01f, KLT_MIN_EIG = 1e-4f, KLT_GATE_SCALE = 1.0f / 1024.0f;
constexpr float KLT_FLT_EPSILON = 1.1920929e-07f;

// BORDER_REFLECT_101 of any int into [0, n)
__host__ __device__ __forceinline__ int klt_reflect(int i, int n) {
  if (n == 1) return 0;
  const int p = 2 * (n - 1);
  i %= p;
  if (i < 0) i += p;
  return i >= n ? p - i : i;
}

__global__ __launch_bounds__(256) void k_klt_hist(const unsigned char* __restrict__ img, int n, unsigned* __restrict__ hist) {
  __shared__ unsigned h[256];
  h[threadIdx.x] = 0u;
  __syncthreads();
  const int n16 = n >> 4;
  const uint4* v = reinterpret_cast<const uint4*>(img);  // (the block is 256-byte aligned)
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n16; i += gridDim.x * 256) {
    const uint4 q = v[i];
    const unsigned wds[4] = {q.x, q.y, q.z, q.w};
    for (int k = 0; k < 4; ++k)
      for (int b = 0; b < 4; ++b) atomicAdd(&h[(wds[k] >> (8 * b)) & 255u], 1u);
  }
  if (blockIdx.x == 0)
    for (int i = 16 * n16 + threadIdx.x; i < n; i += 256) atomicAdd(&h[img[i]], 1u);
  __syncthreads();
  if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}

__global__ __launch_bounds__(256) void k_klt_equalize(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, int n,
                                                      const unsigned* __restrict__ hist) {
  __shared__ unsigned h[256];
  __shared__ unsigned char lut[256];
  const int t = threadIdx.x;
  h[t] = hist[t];
  __syncthreads();
  int first = 0;
  while (first < 255 && h[first] == 0u) ++first;
  const unsigned rest = (unsigned)n - h[first];
  if (rest == 0u) {
    lut[t] = (unsigned char)t;  // a constant image maps to itself
  } else {
    unsigned s = 0u;
    for (int i = first + 1; i <= t; ++i) s += h[i];
    const float scale = __fdiv_rn(255.0f, (float)rest);
    lut[t] = (unsigned char)fminf(255.0f, rintf(__fmul_rn((float)s, scale)));  // (0 up to and including the first bin)
  }
  __syncthreads();
  const int n16 = n >> 4;
  const uint4* v = reinterpret_cast<const uint4*>(src);
  uint4* o = reinterpret_cast<uint4*>(dst);
  for (int i = blockIdx.x * 256 + t; i < n16; i += gridDim.x * 256) {
    const uint4 q = v[i];
    unsigned wds[4] = {q.x, q.y, q.z, q.w};
    for (int k = 0; k < 4; ++k) {
      unsigned r = 0u;
      for (int b = 0; b < 4; ++b) r |= (unsigned)lut[(wds[k] >> (8 * b)) & 255u] << (8 * b);
      wds[k] = r;
    }
    o[i] = make_uint4(wds[0], wds[1], wds[2], wds[3]);
  }
  if (blockIdx.x == 0)
    for (int i = 16 * n16 + t; i < n; i += 256) dst[i] = lut[src[i]];
}

__global__ __launch_bounds__(256) void k_klt_pyrdown(const unsigned char* __restrict__ src, int w, int h, unsigned char* __restrict__ dst,
                                                     int wo, int ho) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= wo * ho) return;
  const int y = i / wo, x = i - y * wo;
  int xs[5];
  for (int k = 0; k < 5; ++k) xs[k] = klt_reflect(2 * x + k - 2, w);
  int sum = 0;
  for (int k = 0; k < 5; ++k) {
    const unsigned char* row = src + (size_t)klt_reflect(2 * y + k - 2, h) * w;
    const int r = row[xs[0]] + 4 * row[xs[1]] + 6 * row[xs[2]] + 4 * row[xs[3]] + row[xs[4]];
    sum += (k == 0 || k == 4 ? 1 : (k == 2 ? 6 : 4)) * r;
  }
  dst[i] = (unsigned char)((sum + 128) >> 8);
}

struct KltTrackArgs {
  const unsigned char *prev[KLT_MAX_LEVELS], *cur[KLT_MAX_LEVELS];
  int w[KLT_MAX_LEVELS], h[KLT_MAX_LEVELS];
  int n_levels, n, win;
  const float *pts, *guess;  // [2n] each
  float* out;                // [2n]
  unsigned char *status, *iters;  // [n], [n * KLT_MAX_LEVELS] iterations run per level
};

__device__ __forceinline__ float klt_wave_sum(float v) {  // xor butterfly: a fixed order, the same bits in every lane
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// the window rule on a corner, on floats (which is the rule on its floor); false for a non-finite corner
__device__ __forceinline__ bool klt_inside(float x, float y, int win, int cols, int rows) {
  return x >= (float)-win && x < (float)cols && y >= (float)-win && y < (float)rows;
}

template <int NPL>
__global__ __launch_bounds__(256) void k_klt_track(KltTrackArgs a) {
  const int lane = threadIdx.x & 63, pt = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pt >= a.n) return;  // (wave-uniform; the kernel has no barrier)
  const float px = a.pts[2 * pt], py = a.pts[2 * pt + 1], g0x = a.guess[2 * pt], g0y = a.guess[2 * pt + 1];
  const int win = a.win, top = a.n_levels - 1;
  if (!(isfinite(px) && isfinite(py) && isfinite(g0x) && isfinite(g0y))) {  // refused on the host; status 0 before any image load
    if (lane == 0) {
      a.out[2 * pt] = g0x, a.out[2 * pt + 1] = g0y, a.status[pt] = 0;
      for (int l = 0; l < KLT_MAX_LEVELS; ++l) a.iters[pt * KLT_MAX_LEVELS + l] = 0;
    }
    return;
  }
  int pr[NPL], pc[NPL];
  bool valid[NPL];
  for (int j = 0; j < NPL; ++j) {
    const int k = lane + 64 * j;
    valid[j] = k < win * win;
    pr[j] = k / win, pc[j] = k - pr[j] * win;
  }
  const float half = (float)(win - 1) * 0.5f;
  float gx = g0x * (1.0f / (float)(1 << top)), gy = g0y * (1.0f / (float)(1 << top));
  bool st = true;
  for (int lvl = top; lvl >= 0; --lvl) {
    if (lvl != top) gx *= 2.0f, gy *= 2.0f;
    int it = 0;
    do {
      const int cols = a.w[lvl], rows = a.h[lvl];
      const unsigned char *I = a.prev[lvl], *J = a.cur[lvl];
      const float s = 1.0f / (float)(1 << lvl);
      const float pwx = px * s - half, pwy = py * s - half;
      if (!klt_inside(pwx, pwy, win, cols, rows)) {
        if (lvl == 0) st = false;
        break;
      }
      const float fx = floorf(pwx), fy = floorf(pwy);
      const int ipx = (int)fx, ipy = (int)fy;  // (in [-win, size): the rule above)
      const float ca = pwx - fx, cb = pwy - fy;
      const float w00 = (1.0f - ca) * (1.0f - cb), w01 = ca * (1.0f - cb), w10 = (1.0f - ca) * cb, w11 = ca * cb;
      float Iw[NPL], Ix[NPL], Iy[NPL];
      float sxx = 0.f, sxy = 0.f, syy = 0.f;
      for (int j = 0; j < NPL; ++j) {
        Iw[j] = Ix[j] = Iy[j] = 0.f;
        if (!valid[j]) continue;
        const int X = ipx + pc[j], Y = ipy + pr[j];
        float v[4][4];
        int xs[4];
        for (int q = 0; q < 4; ++q) xs[q] = klt_reflect(X - 1 + q, cols);
        for (int r = 0; r < 4; ++r) {
          const unsigned char* row = I + (size_t)klt_reflect(Y - 1 + r, rows) * cols;
          for (int q = 0; q < 4; ++q) v[r][q] = (float)row[xs[q]];
        }
        Iw[j] = w00 * v[1][1] + w01 * v[1][2] + w10 * v[2][1] + w11 * v[2][2];
        // Scharr (3, 10, 3) x (-1, 0, 1) / 32 at the four pixels of the bilinear cell; a gradient pixel outside the level is zero
        float dxv[2][2], dyv[2][2];
        for (int dy = 0; dy < 2; ++dy)
          for (int dx = 0; dx < 2; ++dx) {
            const bool in = X + dx >= 0 && X + dx < cols && Y + dy >= 0 && Y + dy < rows;
            const float ddx = 3.f * (v[dy][dx + 2] - v[dy][dx]) + 10.f * (v[dy + 1][dx + 2] - v[dy + 1][dx]) + 3.f * (v[dy + 2][dx + 2] - v[dy + 2][dx]);
            const float ddy = 3.f * (v[dy + 2][dx] - v[dy][dx]) + 10.f * (v[dy + 2][dx + 1] - v[dy][dx + 1]) + 3.f * (v[dy + 2][dx + 2] - v[dy][dx + 2]);
            dxv[dy][dx] = in ? ddx * (1.0f / 32.0f) : 0.f;
            dyv[dy][dx] = in ? ddy * (1.0f / 32.0f) : 0.f;
          }
        Ix[j] = w00 * dxv[0][0] + w01 * dxv[0][1] + w10 * dxv[1][0] + w11 * dxv[1][1];
        Iy[j] = w00 * dyv[0][0] + w01 * dyv[0][1] + w10 * dyv[1][0] + w11 * dyv[1][1];
        sxx += Ix[j] * Ix[j], sxy += Ix[j] * Iy[j], syy += Iy[j] * Iy[j];
      }
      const float A11 = klt_wave_sum(sxx) * KLT_GATE_SCALE, A12 = klt_wave_sum(sxy) * KLT_GATE_SCALE, A22 = klt_wave_sum(syy) * KLT_GATE_SCALE;
      const float D = A11 * A22 - A12 * A12;
      const float min_eig = (A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) / (float)(2 * win * win);
      if (min_eig < KLT_MIN_EIG || D < KLT_FLT_EPSILON) {  // the texture gate
        if (lvl == 0) st = false;
        break;
      }
      float vx = gx - half, vy = gy - half, pdx = 0.f, pdy = 0.f;
      for (int j = 0; j < KLT_MAX_ITERS; ++j) {
        if (!klt_inside(vx, vy, win, cols, rows)) {
          if (lvl == 0) st = false;
          break;
        }
        ++it;
        const float qx = floorf(vx), qy = floorf(vy);
        const int iqx = (int)qx, iqy = (int)qy;
        const float ja = vx - qx, jb = vy - qy;
        const float u00 = (1.0f - ja) * (1.0f - jb), u01 = ja * (1.0f - jb), u10 = (1.0f - ja) * jb, u11 = ja * jb;
        float b1 = 0.f, b2 = 0.f;
        for (int k = 0; k < NPL; ++k) {
          if (!valid[k]) continue;
          const int x0 = klt_reflect(iqx + pc[k], cols), x1 = klt_reflect(iqx + pc[k] + 1, cols);
          const unsigned char *r0 = J + (size_t)klt_reflect(iqy + pr[k], rows) * cols, *r1 = J + (size_t)klt_reflect(iqy + pr[k] + 1, rows) * cols;
          const float jv = u00 * (float)r0[x0] + u01 * (float)r0[x1] + u10 * (float)r1[x0] + u11 * (float)r1[x1];
          const float diff = jv - Iw[k];
          b1 += diff * Ix[k], b2 += diff * Iy[k];
        }
        b1 = klt_wave_sum(b1) * KLT_GATE_SCALE, b2 = klt_wave_sum(b2) * KLT_GATE_SCALE;
        const float dx = (A12 * b2 - A22 * b1) / D, dy = (A12 * b1 - A11 * b2) / D;
        vx += dx, vy += dy;
        if (dx * dx + dy * dy <= KLT_STOP_EPS * KLT_STOP_EPS) break;
        if (j > 0 && fabsf(dx + pdx) < KLT_OSC_EPS && fabsf(dy + pdy) < KLT_OSC_EPS) {
          vx -= dx * 0.5f, vy -= dy * 0.5f;
          break;
        }
        pdx = dx, pdy = dy;
      }
      gx = vx + half, gy = vy + half;
    } while (0);
    if (lane == 0) a.iters[pt * KLT_MAX_LEVELS + lvl] = (unsigned char)it;
  }
  if (lane == 0) {
    a.out[2 * pt] = gx, a.out[2 * pt + 1] = gy, a.status[pt] = st ? 1 : 0;
    for (int l = a.n_levels; l < KLT_MAX_LEVELS; ++l) a.iters[pt * KLT_MAX_LEVELS + l] = 0;
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
struct Klt {
  int width = 0, height = 0, n_levels = 0, win = 0, max_points = 0;
  int lw[KLT_MAX_LEVELS] = {}, lh[KLT_MAX_LEVELS] = {};
  size_t loff[KLT_MAX_LEVELS] = {};  // a level's offset in a half (256-byte aligned)
  size_t half_bytes = 0;
  DevBuf<unsigned char> pyr[2], raw;  // the two halves, swapped by index; the uploaded image in front of the equalisation
  DevBuf<unsigned> hist;
  DevBuf<unsigned char> clahe_lut;  // ovp_klt_feed_image_opts: the tiles' LUTs [tiles_y tiles_x][256] of the last CLAHE feed
  int lut_tiles = 0;                // tiles of that feed (0: none yet)
  DevBuf<unsigned char> full;       // the full-size image in front of the halving; made by the first call that halves
  PinnedBuf<unsigned char> hfull;   // its staging, rows packed
  DevBuf<unsigned char> halved;     // ovp_klt_halve: its result, and the block it is read back through
  PinnedBuf<unsigned char> hhalved;
  DevBuf<unsigned char> score, nms;  // ovp_klt_detect: the level-0 score map and the same after suppression
  bool det_done = false;
  DevBuf<int> epi_samples, epi_nmodels, epi_counts;  // ovp_klt_epipolar: what its kernels leave for ovp_klt_debug
  DevBuf<double> epi_models;
  std::vector<int32_t> epi_table;
  int epi_H = 0;  // max_iters of the last ovp_klt_epipolar that ran its kernels (0: none)
  PinnedBuf<unsigned char> himg;  // the upload's staging, rows packed
  UploadFence up;                 // ... the fence of himg and hfull alike (their copies go where the call says: no Staged)
  Staged stage;                   // a track's or an epipolar check's tables
  DevBuf<void> dres;
  Mailbox hres;
  size_t res_cap = 0;
  int cur = 0, fed = 0;  // index of the current half; images fed since create / reset
  // timed mode (EV_IN0: in front of the halving, EV_LUT: between k_clahe_lut and k_clahe_apply)
  enum { EV_EQ0, EV_EQ1, EV_PYR1, EV_TRK0, EV_TRK1, EV_DET, EV_EPI = EV_DET + 4, EV_IN0 = EV_EPI + 5, EV_LUT, EV_FRM0, EV_FRM1, EV_COUNT };
  OvpEvent ev[EV_COUNT];
  bool timed = false;
  // equalise, pyramid launches together, k_klt_track, k_fast_score_nms, k_fast_select, k_fast_subpix, the four k_epi_* kernels, then
  // the intake's halving, k_clahe_lut and k_clahe_apply, and behind them k_klt_keep_append
  float ms[14] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int last_n = 0;
  // ovp_klt_match_frame: the survivors the last call published (offsets into the mailbox's payload), good while the mailbox's
  // sequence number is still that call's
  int frm_kept = -1;
  unsigned frm_seq = 0;
  bool frm_uvn = false;
  size_t frm_uv_off = 0, frm_uvn_off = 0;
};

Klt* klt_of(ovp_ctx* c) { return c ? (Klt*)c->klt.get() : nullptr; }

}  // namespace

#include "k_clahe.h"  // histogram_method CLAHE: k_clahe_lut, k_clahe_apply (behind klt_reflect, which they use)

extern "C" int ovp_klt_create(ovp_ctx* c, int width, int height, int n_levels, int win, int max_points) {
  if (!c) return OVP_E_ARG;
  if (width < 2 || height < 2 || width > 16384 || height > 16384 || n_levels < 1 || n_levels > KLT_MAX_LEVELS) return OVP_E_ARG;
  if (win < KLT_MIN_WIN || win > KLT_MAX_WIN || !(win & 1) || max_points < 1 || max_points > KLT_MAX_POINTS) return OVP_E_ARG;
  auto d = std::make_shared<Klt>();
  d->width = width, d->height = height, d->n_levels = n_levels, d->win = win, d->max_points = max_points;
  size_t off = 0;
  for (int l = 0, w = width, h = height; l < n_levels; ++l, w = (w + 1) / 2, h = (h + 1) / 2) {
    if (w < 2 || h < 2) return OVP_E_ARG;  // a level smaller than 2 x 2
    d->lw[l] = w, d->lh[l] = h, d->loff[l] = off;
    off += ((size_t)w * h + 255) & ~(size_t)255;
  }
  d->half_bytes = off;
  HIPCHK(hipSetDevice(c->device));
  if (c->klt) HIPCHK(hipStreamSynchronize(c->stream));  // (a second create replaces the first - once it has succeeded: a failure below leaves the first in place)
  for (auto& p : d->pyr) HIPCHK(p.alloc(off));
  HIPCHK(d->raw.alloc(((size_t)width * height + 255) & ~(size_t)255));
  HIPCHK(d->hist.alloc(256));
  HIPCHK(d->clahe_lut.alloc((size_t)CLAHE_MAX_TILES * CLAHE_MAX_TILES * CLAHE_BINS));
  HIPCHK(d->score.alloc((size_t)width * height));
  HIPCHK(d->nms.alloc((size_t)width * height));
  HIPCHK(d->himg.alloc((size_t)width * height));
  // a track's points and guesses, or an epipolar check's two point sets, status and table
  HIPCHK(d->stage.alloc(64 * 4 + (sizeof(float) * 4 + 1 + sizeof(int)) * (size_t)max_points + sizeof(int)));
  // a track's results, a detection's, or an epipolar check's (mask, two coordinate sets, info)
  d->res_cap = 64 * 4 + sizeof(EpiInfoDev) + std::max(sizeof(float) * 2 + 1 + KLT_MAX_LEVELS, sizeof(int) * 3 + sizeof(float) * 2) * (size_t)max_points;
  HIPCHK(d->epi_samples.alloc((size_t)EPI_MAX_ITERS * 7));
  HIPCHK(d->epi_nmodels.alloc(EPI_MAX_ITERS));
  HIPCHK(d->epi_counts.alloc((size_t)EPI_MAX_ITERS * 3));
  HIPCHK(d->epi_models.alloc((size_t)EPI_MAX_ITERS * 27));
  HIPCHK(d->dres.alloc(d->res_cap));
  HIPCHK(d->hres.alloc(d->res_cap));
  for (OvpEvent& e : d->ev) HIPCHK(e.create());
  c->klt = d;
  return 0;
}

extern "C" int ovp_klt_destroy(ovp_ctx* c) {
  if (!c) return OVP_E_ARG;
  if (!c->klt) return OVP_E_STATE;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->klt.reset();
  return 0;
}

extern "C" int ovp_klt_reset(ovp_ctx* c) {
  Klt* d = klt_of(c);
  if (!d) return c ? OVP_E_STATE : OVP_E_ARG;
  d->fed = 0;  // (a half is overwritten when an image takes it)
  d->det_done = false;
  d->lut_tiles = 0;
  return 0;
}

// the full-size image and its staging: made by the first call that halves, for the largest source a feed can hand over,
// (2 w + 1) x (2 h + 1), or for ovp_klt_halve's own source when that is larger.  Growing waits for the stream, which may still read
// the old block.
static int klt_full_buffers(ovp_ctx* c, Klt* d, size_t count) {
  count = std::max(count, (size_t)(2 * d->width + 1) * (2 * d->height + 1));
  if (count <= d->full.capacity()) return 0;
  HIPCHK(hipStreamSynchronize(c->stream));
  d->up.done();
  HIPCHK(d->hfull.reserve(count, 0));
  HIPCHK(d->full.reserve(count, 0));  // (second: the capacity asked above is this one's)
  return 0;
}

// the source of a call that halves: (sw / 2, sh / 2) is the tracker's size
static bool klt_halves_to(const Klt* d, int sw, int sh) { return sw >= 2 && sh >= 2 && sw / 2 == d->width && sh / 2 == d->height; }

// cv::pyrDown to an explicit size (the pyramid's (w + 1) / 2, or the intake's w / 2)
static int klt_pyrdown(const unsigned char* src, int w, int h, unsigned char* dst, int wo, int ho, hipStream_t stream) {
  const int m = wo * ho;
  hipLaunchKernelGGL(k_klt_pyrdown, dim3((m + 255) / 256), dim3(256), 0, stream, src, w, h, dst, wo, ho);
  HIPCHK(hipGetLastError());
  return 0;
}

// One image into the current half: upload (of the full-size image with `halve`), halving, equalisation, pyramid - every argument
// checked by the caller.  sw x sh: the size of the image handed over.
static int klt_feed(ovp_ctx* c, Klt* d, const uint8_t* img, int stride, int method, const ClaheGeom* clahe, bool halve, int sw, int sh) {
  HIPCHK(hipSetDevice(c->device));
  if (halve) {
    const int rf = klt_full_buffers(c, d, 0);
    if (rf) return rf;
  }
  HIPCHK(d->up.wait());
  const int w = d->width, h = d->height, n = w * h;
  unsigned char* stage = halve ? d->hfull.get() : d->himg.get();
  for (int y = 0; y < sh; ++y) memcpy(stage + (size_t)y * sw, img + (size_t)y * stride, sw);
  const int nxt = d->cur ^ 1;  // the former current half becomes "previous" by index: nothing is copied
  unsigned char* lv0 = d->pyr[nxt].get();
  const bool eq = method != OVP_KLT_HIST_NONE;
  unsigned char* in = eq ? d->raw.get() : lv0;  // what the equalisation reads, or level 0 itself
  HIPCHK(hipMemcpyAsync(halve ? d->full.get() : in, stage, (size_t)sw * sh, hipMemcpyHostToDevice, c->stream));
  HIPCHK(d->up.sent(c->stream, Fence::Event));
  if (halve) {  // core/VioManager.cpp:279-289 cv::pyrDown to (cols / 2, rows / 2)
    if (d->timed) HIPCHK(hipEventRecord(d->ev[Klt::EV_IN0], c->stream));
    const int rp = klt_pyrdown(d->full.get(), sw, sh, in, w, h, c->stream);
    if (rp) return rp;
  }
  if (d->timed) HIPCHK(hipEventRecord(d->ev[Klt::EV_EQ0], c->stream));
  if (method == OVP_KLT_HIST_HISTOGRAM) {
    HIPCHK(hipMemsetAsync(d->hist.get(), 0, 256 * sizeof(unsigned), c->stream));
    const int blocks = std::max(1, std::min(256, (n / 16 + 255) / 256));
    hipLaunchKernelGGL(k_klt_hist, dim3(blocks), dim3(256), 0, c->stream, (const unsigned char*)d->raw.get(), n, d->hist.get());
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_klt_equalize, dim3(blocks), dim3(256), 0, c->stream, (const unsigned char*)d->raw.get(), lv0, n,
                       (const unsigned*)d->hist.get());
    HIPCHK(hipGetLastError());
  } else if (method == OVP_KLT_HIST_CLAHE) {  // track_plane/TrackPlane.cpp:66-70
    hipLaunchKernelGGL(k_clahe_lut, dim3(clahe->tiles_x * clahe->tiles_y), dim3(256), 0, c->stream, (const unsigned char*)d->raw.get(), *clahe,
                       d->clahe_lut.get());
    HIPCHK(hipGetLastError());
    if (d->timed) HIPCHK(hipEventRecord(d->ev[Klt::EV_LUT], c->stream));
    hipLaunchKernelGGL(k_clahe_apply, dim3((n + 255) / 256), dim3(256), 0, c->stream, (const unsigned char*)d->raw.get(), *clahe,
                       (const unsigned char*)d->clahe_lut.get(), lv0);
    HIPCHK(hipGetLastError());
    d->lut_tiles = clahe->tiles_x * clahe->tiles_y;
  }
  if (d->timed) HIPCHK(hipEventRecord(d->ev[Klt::EV_EQ1], c->stream));
  for (int l = 1; l < d->n_levels; ++l) {
    const int rp = klt_pyrdown(lv0 + d->loff[l - 1], d->lw[l - 1], d->lh[l - 1], lv0 + d->loff[l], d->lw[l], d->lh[l], c->stream);
    if (rp) return rp;
  }
  d->cur = nxt;
  if (d->fed < 2) ++d->fed;
  if (d->timed) {
    HIPCHK(hipEventRecord(d->ev[Klt::EV_PYR1], c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipEventElapsedTime(&d->ms[0], d->ev[Klt::EV_EQ0], d->ev[Klt::EV_EQ1]));
    HIPCHK(hipEventElapsedTime(&d->ms[1], d->ev[Klt::EV_EQ1], d->ev[Klt::EV_PYR1]));
    d->ms[10] = d->ms[11] = d->ms[12] = 0.f;
    if (halve) HIPCHK(hipEventElapsedTime(&d->ms[10], d->ev[Klt::EV_IN0], d->ev[Klt::EV_EQ0]));
    if (method == OVP_KLT_HIST_CLAHE) {
      HIPCHK(hipEventElapsedTime(&d->ms[11], d->ev[Klt::EV_EQ0], d->ev[Klt::EV_LUT]));
      HIPCHK(hipEventElapsedTime(&d->ms[12], d->ev[Klt::EV_LUT], d->ev[Klt::EV_EQ1]));
    }
  }
  return 0;
}

extern "C" int ovp_klt_feed_image(ovp_ctx* c, const uint8_t* img, int stride, int hist_method) {
  Klt* d = klt_of(c);
  if (!d) return c ? OVP_E_STATE : OVP_E_ARG;
  if (!img || stride < d->width) return OVP_E_ARG;
  // CLAHE takes parameters this entry has no place for: ovp_klt_feed_image_opts
  if (hist_method != OVP_KLT_HIST_NONE && hist_method != OVP_KLT_HIST_HISTOGRAM) return OVP_E_ARG;
  return klt_feed(c, d, img, stride, hist_method, nullptr, false, d->width, d->height);
}

extern "C" void ovp_klt_intake_defaults(ovp_klt_intake* o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->hist_method = OVP_KLT_HIST_HISTOGRAM;                       // TrackBase's default
  o->clahe_clip = 10.0, o->clahe_tiles_x = o->clahe_tiles_y = 8;  // track_plane/TrackPlane.cpp:67-68
}

extern "C" int ovp_klt_feed_image_opts(ovp_ctx* c, const uint8_t* img, int stride, const ovp_klt_intake* o) {
  Klt* d = klt_of(c);
  if (!d) return c ? OVP_E_STATE : OVP_E_ARG;
  // ---- every check before anything is touched or enqueued ----
  if (!img || !o) return OVP_E_ARG;
  if (o->hist_method != OVP_KLT_HIST_NONE && o->hist_method != OVP_KLT_HIST_HISTOGRAM && o->hist_method != OVP_KLT_HIST_CLAHE) return OVP_E_ARG;
  if (o->downsample != 0 && o->downsample != 1) return OVP_E_ARG;
  if (o->clahe_tiles_x < 1 || o->clahe_tiles_x > CLAHE_MAX_TILES || o->clahe_tiles_y < 1 || o->clahe_tiles_y > CLAHE_MAX_TILES) return OVP_E_ARG;
  if (!std::isfinite(o->clahe_clip) || o->clahe_clip < 0.0) return OVP_E_ARG;
  if (o->src_width < 1 || o->src_height < 1 || stride < o->src_width) return OVP_E_ARG;
  if (o->downsample ? !klt_halves_to(d, o->src_width, o->src_height) : (o->src_width != d->width || o->src_height != d->height)) return OVP_E_ARG;
  // ---- from here on the call goes through ----
  ClaheGeom g;
  clahe_geom(d->width, d->height, o->clahe_tiles_x, o->clahe_tiles_y, o->clahe_clip, &g);
  return klt_feed(c, d, img, stride, o->hist_method, &g, o->downsample != 0, o->src_width, o->src_height);
}

extern "C" int ovp_klt_halve(ovp_ctx* c, const uint8_t* src, int stride, int src_width, int src_height, uint8_t* dst) {
  Klt* d = klt_of(c);
  if (!d) return c ? OVP_E_STATE : OVP_E_ARG;
  if (!src || !dst || stride < src_width || src_width / 2 < 1 || src_height / 2 < 1 || src_width > 32768 || src_height > 32768) return OVP_E_ARG;
  HIPCHK(hipSetDevice(c->device));
  const int w = src_width / 2, h = src_height / 2;
  const int rf = klt_full_buffers(c, d, (size_t)src_width * src_height);
  if (rf) return rf;
  if ((size_t)w * h > d->halved.capacity()) {
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(d->halved.reserve((size_t)w * h, 0));
    HIPCHK(d->hhalved.reserve((size_t)w * h, 0));
  }
  HIPCHK(d->up.wait());  // (a feed's upload may still read the staging block)
  for (int y = 0; y < src_height; ++y) memcpy(d->hfull.get() + (size_t)y * src_width, src + (size_t)y * stride, src_width);
  // `full` is free in stream order: a feed enqueued before has halved it by then, and this call returns when its own copies are done
  HIPCHK(hipMemcpyAsync(d->full.get(), d->hfull.get(), (size_t)src_width * src_height, hipMemcpyHostToDevice, c->stream));
  HIPCHK(d->up.sent(c->stream, Fence::CallerWaits));
  const int rp = klt_pyrdown(d->full.get(), src_width, src_height, d->halved.get(), w, h, c->stream);
  if (rp) return rp;
  HIPCHK(hipMemcpyAsync(d->hhalved.get(), d->halved.get(), (size_t)w * h, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  d->up.done();
  memcpy(dst, d->hhalved.get(), (size_t)w * h);
  return 0;
}

extern "C" int ovp_klt_track(ovp_ctx* c, int n, const float* pts_prev, const float* guess, float* pts_out, uint8_t* status) {
  Klt* d = klt_of(c);
  if (!d) return c ? OVP_E_STATE : OVP_E_ARG;
  // ---- every check before anything is touched or enqueued ----
  if (n < 0) return OVP_E_ARG;
  if (d->fed < 2) return OVP_E_STATE;
  if (n > d->max_points) return OVP_E_CAPACITY;
  if (n == 0) return 0;
  if (!pts_prev || !pts_out || !status) return OVP_E_ARG;
  for (int i = 0; i < 2 * n; ++i)
    if (!std::isfinite(pts_prev[i]) || (guess && !std::isfinite(guess[i]))) return OVP_E_ARG;
  StageLayout L;
  const size_t o_pts = L.take(sizeof(float) * 2 * n), o_guess = L.take(sizeof(float) * 2 * n);
  StageLayout R;
  const size_t r_out = R.take(sizeof(float) * 2 * n), r_st = R.take(n), r_it = R.take((size_t)n * KLT_MAX_LEVELS);
  if (L.bytes() > d->stage.capacity() || R.bytes() > d->res_cap) return OVP_E_CAPACITY;  // (cannot happen below max_points)
  // ---- from here on the call goes through ----
  HIPCHK(hipSetDevice(c->device));
  int rc = 0;
  char* h = d->stage.begin(L.bytes(), &rc);
  if (!h) return rc;
  memcpy(h + o_pts, pts_prev, sizeof(float) * 2 * n);
  memcpy(h + o_guess, guess ? guess : pts_prev, sizeof(float) * 2 * n);  // :1329 the reference passes pts1 = pts0
  const char* dv = d->stage.dev();
  char* dr = (char*)d->dres.get();
  HIPCHK(d->stage.send(L.bytes(), c->stream, Fence::CallerWaits));
  KltTrackArgs a;
  const unsigned char *pc = d->pyr[d->cur].get(), *pp = d->pyr[d->cur ^ 1].get();
  for (int l = 0; l < KLT_MAX_LEVELS; ++l) {
    const int q = l < d->n_levels ? l : 0;
    a.prev[l] = pp + d->loff[q], a.cur[l] = pc + d->loff[q], a.w[l] = d->lw[q], a.h[l] = d->lh[q];
  }
  a.n_levels = d->n_levels, a.n = n, a.win = d->win;
  a.pts = (const float*)(dv + o_pts), a.guess = (const float*)(dv + o_guess);
  a.out = (float*)(dr + r_out), a.status = (unsigned char*)(dr + r_st), a.iters = (unsigned char*)(dr + r_it);
  if (d->timed) HIPCHK(hipEventRecord(d->ev[Klt::EV_TRK0], c->stream));
  const dim3 grid((n + 3) / 4), block(256);
  const int npl = (d->win * d->win + 63) / 64;
  if (npl <= 1) hipLaunchKernelGGL(k_klt_track<1>, grid, block, 0, c->stream, a);
  else if (npl <= 2) hipLaunchKernelGGL(k_klt_track<2>, grid, block, 0, c->stream, a);
  else if (npl <= 4) hipLaunchKernelGGL(k_klt_track<4>, grid, block, 0, c->stream, a);
  else hipLaunchKernelGGL(k_klt_track<7>, grid, block, 0, c->stream, a);
  HIPCHK(hipGetLastError());
  if (d->timed) HIPCHK(hipEventRecord(d->ev[Klt::EV_TRK1], c->stream));
  SeqChannel& ch = d->hres.channel(0);
  const unsigned seq = ch.arm();
  HIPCHK(ovp_launch_publish_block(dr, d->hres.dev(d->hres.payload()), R.bytes(), ch.word_dev(), seq, 0, c->stream));
  const int rw = ch.wait(c->stream);
  if (rw) return rw;
  d->stage.done();
  if (d->timed) {
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipEventElapsedTime(&d->ms[2], d->ev[Klt::EV_TRK0], d->ev[Klt::EV_TRK1]));
  }
  const char* hr = (const char*)d->hres.payload();
  memcpy(pts_out, hr + r_out, sizeof(float) * 2 * n);
  memcpy(status, hr + r_st, n);
  d->last_n = n;
  return 0;
}

// the cells of Grider_FAST::perform_griding (recalled): false when a cell would be empty
static bool fast_grid(int cols, int rows, int num_features, int grid_x, int grid_y, FastGrid* g) {
  if (num_features < grid_x * (long long)grid_y) {
    const double ratio = (double)grid_x / (double)grid_y;
    grid_y = (int)std::ceil(std::sqrt(num_features / ratio));
    grid_x = (int)std::ceil(grid_y * ratio);
  }
  if (grid_x < 1 || grid_y < 1 || grid_x > cols || grid_y > rows) return false;
  g->cols = cols, g->rows = rows;
  const long long k = (long long)(num_features / (double)((long long)grid_x * grid_y)) + 1;
  g->K = (int)std::min<long long>(k, FAST_MAX_K + 1);  // (anything above the limit is refused: no overflow on the way there)
  g->size_x = cols / grid_x, g->size_y = rows / grid_y;
  g->ct_cols = cols / g->size_x, g->ct_rows = rows / g->size_y;
  return true;
}

// cornerSubPix's window weights per axis: exp(-x^2), x = (j - 5) / 5 in float
static void fast_subpix_weights(float* w) {
  for (int j = 0; j < FAST_SUB_WIN; ++j) {
    const float x = (float)(j - FAST_SUB_HALF) / (float)FAST_SUB_HALF;
    w[j] = (float)std::exp(-(double)(x * x));  // one rounding to float: the same bits from every libm
  }
}

extern "C" int ovp_klt_detect(ovp_ctx* c, int half, int num_features, int grid_x, int grid_y, int threshold, int* n_out, int32_t* xy_int,
                              int32_t* response, float* xy_refined, int32_t* cell, int cap) {
  Klt* d = klt_of(c);
  if (!d) return c ? OVP_E_STATE : OVP_E_ARG;
  // ---- every check before anything is touched or enqueued ----
  if (half != 0 && half != 1) return OVP_E_ARG;
  if (d->fed < 1 + half) return OVP_E_STATE;
  if (threshold < 0 || threshold > 255 || num_features < 1 || grid_x < 1 || grid_y < 1 || cap < 0) return OVP_E_ARG;
  if (grid_x > d->width || grid_y > d->height) return OVP_E_ARG;
  if (!n_out || !xy_int || !response || !xy_refined || !cell) return OVP_E_ARG;
  FastGrid g;
  if (!fast_grid(d->width, d->height, num_features, grid_x, grid_y, &g)) return OVP_E_ARG;
  const long long cells = (long long)g.ct_cols * g.ct_rows;
  if (cells > FAST_MAX_CELLS || g.K > FAST_MAX_K) return OVP_E_CAPACITY;
  const long long slots = cells * g.K;
  if (slots > cap || slots > d->max_points) return OVP_E_CAPACITY;
  const int n = (int)slots;
  StageLayout R;
  const size_t r_xy = R.take(sizeof(int) * 2 * n), r_resp = R.take(sizeof(int) * n), r_ref = R.take(sizeof(float) * 2 * n);
  if (R.bytes() > d->res_cap) return OVP_E_CAPACITY;  // (cannot happen below max_points)
  // ---- from here on the call goes through ----
  HIPCHK(hipSetDevice(c->device));
  const unsigned char* img = d->pyr[half ? d->cur ^ 1 : d->cur].get();  // level 0 of that half
  char* dr = (char*)d->dres.get();
  if (d->timed) HIPCHK(hipEventRecord(d->ev[Klt::EV_DET + 0], c->stream));
  hipLaunchKernelGGL(k_fast_score_nms, dim3((d->width + FAST_TW - 1) / FAST_TW, (d->height + FAST_TH - 1) / FAST_TH), dim3(256), 0, c->stream,
                     img, g, threshold, d->score.get(), d->nms.get());
  HIPCHK(hipGetLastError());
  if (d->timed) HIPCHK(hipEventRecord(d->ev[Klt::EV_DET + 1], c->stream));
  hipLaunchKernelGGL(k_fast_select, dim3((unsigned)cells), dim3(256), 0, c->stream, (const unsigned char*)d->nms.get(), g, (int*)(dr + r_xy),
                     (int*)(dr + r_resp));
  HIPCHK(hipGetLastError());
  if (d->timed) HIPCHK(hipEventRecord(d->ev[Klt::EV_DET + 2], c->stream));
  FastSubpixArgs a;
  a.img = img, a.cols = d->width, a.rows = d->height, a.n = n;
  a.xy = (const int*)(dr + r_xy), a.resp = (const int*)(dr + r_resp), a.out = (float*)(dr + r_ref), a.start = nullptr;
  fast_subpix_weights(a.w);
  hipLaunchKernelGGL(k_fast_subpix, dim3((n + 3) / 4), dim3(256), 0, c->stream, a);
  HIPCHK(hipGetLastError());
  if (d->timed) HIPCHK(hipEventRecord(d->ev[Klt::EV_DET + 3], c->stream));
  SeqChannel& ch = d->hres.channel(0);
  const unsigned seq = ch.arm();
  HIPCHK(ovp_launch_publish_block(dr, d->hres.dev(d->hres.payload()), R.bytes(), ch.word_dev(), seq, 0, c->stream));
  const int rw = ch.wait(c->stream);
  if (rw) return rw;
  if (d->timed) {
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int k = 0; k < 3; ++k) HIPCHK(hipEventElapsedTime(&d->ms[3 + k], d->ev[Klt::EV_DET + k], d->ev[Klt::EV_DET + k + 1]));
  }
  // the slots in output order (cell ascending, then selection order), the empty ones gone
  const char* hr = (const char*)d->hres.payload();
  const int32_t *sxy = (const int32_t*)(hr + r_xy), *sresp = (const int32_t*)(hr + r_resp);
  const float* sref = (const float*)(hr + r_ref);
  int m = 0;
  for (int s = 0; s < n; ++s) {
    if (sresp[s] == 0) continue;
    xy_int[2 * m] = sxy[2 * s], xy_int[2 * m + 1] = sxy[2 * s + 1], response[m] = sresp[s];
    xy_refined[2 * m] = sref[2 * s], xy_refined[2 * m + 1] = sref[2 * s + 1], cell[m] = s / g.K;
    ++m;
  }
  *n_out = m;
  d->last_n = 0;  // (the mailbox no longer holds a track's iterations)
  d->det_done = true;
  return 0;
}

extern "C" void ovp_epipolar_defaults(ovp_epipolar_opts* o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->mode = OVP_EPI_MODE_NORMALISED, o->max_iters = 1000;
  o->intrinsics[0] = o->intrinsics[1] = 1.0;
  o->threshold = 2.0 / 458.654, o->confidence = 0.999, o->seed = 0u;
}

extern "C" int ovp_klt_epipolar(ovp_ctx* c, const ovp_epipolar_opts* o, int n, const float* pts0, const float* pts1, const uint8_t* status,
                                uint8_t* mask_out, float* uvn0, float* uvn1, ovp_epipolar_info* info) {
  static_assert(sizeof(EpiInfoDev) == sizeof(ovp_epipolar_info), "the device writes ovp_epipolar_info in place");
  Klt* d = klt_of(c);
  if (!d) return c ? OVP_E_STATE : OVP_E_ARG;
  // ---- every check before anything is touched or enqueued ----
  if (!o || n < 0) return OVP_E_ARG;
  if (o->mode != OVP_EPI_MODE_NORMALISED && o->mode != OVP_EPI_MODE_RADTAN && o->mode != OVP_EPI_MODE_EQUIDISTANT) return OVP_E_ARG;
  if (!(o->threshold > 0.0) || !std::isfinite(o->threshold) || !(o->confidence > 0.0 && o->confidence < 1.0)) return OVP_E_ARG;
  if (o->max_iters < 1 || o->max_iters > OVP_EPI_MAX_ITERS) return OVP_E_ARG;
  for (double v : o->intrinsics)
    if (!std::isfinite(v)) return OVP_E_ARG;
  if (o->mode != OVP_EPI_MODE_NORMALISED && (o->intrinsics[0] == 0.0 || o->intrinsics[1] == 0.0)) return OVP_E_ARG;
  if (n > d->max_points) return OVP_E_CAPACITY;
  if (n == 0) return 0;
  if (!pts0 || !pts1) return OVP_E_ARG;
  for (int i = 0; i < 2 * n; ++i)
    if (!std::isfinite(pts0[i]) || !std::isfinite(pts1[i])) return OVP_E_ARG;
  const bool few = n < OVP_EPI_MIN_POINTS;
  StageLayout L;
  const size_t o_p0 = L.take(sizeof(float) * 2 * n), o_p1 = L.take(sizeof(float) * 2 * n), o_st = L.take(n), o_tab = L.take(sizeof(int) * (n + 1));
  StageLayout R;
  const size_t r_mask = R.take(n), r_u0 = R.take(sizeof(float) * 2 * n), r_u1 = R.take(sizeof(float) * 2 * n), r_info = R.take(sizeof(EpiInfoDev));
  if (L.bytes() > d->stage.capacity() || R.bytes() > d->res_cap) return OVP_E_CAPACITY;  // (cannot happen below max_points)
  // ---- from here on the call goes through ----
  HIPCHK(hipSetDevice(c->device));
  int rc = 0;
  char* h = d->stage.begin(L.bytes(), &rc);
  if (!h) return rc;
  memcpy(h + o_p0, pts0, sizeof(float) * 2 * n);
  memcpy(h + o_p1, pts1, sizeof(float) * 2 * n);
  for (int i = 0; i < n; ++i) h[o_st + i] = status ? (status[i] != 0) : 1;
  std::vector<int32_t> table(n + 1, 0);
  if (!few) ovp_epi_table(n, o->confidence, o->max_iters, table.data());
  memcpy(h + o_tab, table.data(), sizeof(int) * (n + 1));
  const char* dv = d->stage.dev();
  char* dr = (char*)d->dres.get();
  HIPCHK(d->stage.send(L.bytes(), c->stream, Fence::CallerWaits));
  EpiLaunch a;
  a.n = n, a.max_iters = o->max_iters, a.mode = o->mode, a.seed = o->seed;
  for (int k = 0; k < 8; ++k) a.intr[k] = o->intrinsics[k];
  a.thr2 = (float)(o->threshold * o->threshold);
  a.pts0 = (const float*)(dv + o_p0), a.pts1 = (const float*)(dv + o_p1), a.status = (const unsigned char*)(dv + o_st);
  a.table = (const int*)(dv + o_tab);
  a.samples = d->epi_samples.get(), a.n_models = d->epi_nmodels.get(), a.models = d->epi_models.get(), a.counts = d->epi_counts.get();
  a.mask = (unsigned char*)(dr + r_mask), a.uvn0 = (float*)(dr + r_u0), a.uvn1 = (float*)(dr + r_u1), a.info = (EpiInfoDev*)(dr + r_info);
  hipEvent_t ev_epi[5];
  for (int k = 0; k < 5; ++k) ev_epi[k] = d->ev[Klt::EV_EPI + k];
  a.ev = d->timed ? ev_epi : nullptr;
  const int rl = ovp_epi_enqueue(a, c->stream);  // (a set below OVP_EPI_MIN_POINTS: the undistortion, a zero mask and too_few)
  if (rl) return rl;
  SeqChannel& ch = d->hres.channel(0);
  const unsigned seq = ch.arm();
  HIPCHK(ovp_launch_publish_block(dr, d->hres.dev(d->hres.payload()), R.bytes(), ch.word_dev(), seq, 0, c->stream));
  const int rw = ch.wait(c->stream);
  if (rw) return rw;
  d->stage.done();
  if (d->timed && !few) {
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int k = 0; k < 4; ++k) HIPCHK(hipEventElapsedTime(&d->ms[6 + k], d->ev[Klt::EV_EPI + k], d->ev[Klt::EV_EPI + k + 1]));
  }
  const char* hr = (const char*)d->hres.payload();
  if (mask_out) memcpy(mask_out, hr + r_mask, n);
  if (uvn0) memcpy(uvn0, hr + r_u0, sizeof(float) * 2 * n);
  if (uvn1) memcpy(uvn1, hr + r_u1, sizeof(float) * 2 * n);
  if (info) memcpy(info, hr + r_info, sizeof(*info));
  d->last_n = 0;  // (the mailbox no longer holds a track's iterations)
  if (!few) d->epi_H = o->max_iters, d->epi_table.swap(table);  // (what the debug reads belong to: one and the same run)
  return 0;
}

// what ovp_klt_epipolar refuses in its options.  A second statement of that entry's own checks (the lines behind its "every check"
// comment), because the entry itself stays as it is: a rule added there is added here, and
// tests/test_klt_frame_gpu.py::test_option_refusals_equal_the_epipolar_entrys holds the two to the same verdict option by option.
static bool klt_epi_opts_ok(const ovp_epipolar_opts* o) {
  if (o->mode != OVP_EPI_MODE_NORMALISED && o->mode != OVP_EPI_MODE_RADTAN && o->mode != OVP_EPI_MODE_EQUIDISTANT) return false;
  if (!(o->threshold > 0.0) || !std::isfinite(o->threshold) || !(o->confidence > 0.0 && o->confidence < 1.0)) return false;
  if (o->max_iters < 1 || o->max_iters > OVP_EPI_MAX_ITERS) return false;
  for (double v : o->intrinsics)
    if (!std::isfinite(v)) return false;
  return o->mode == OVP_EPI_MODE_NORMALISED || (o->intrinsics[0] != 0.0 && o->intrinsics[1] != 0.0);
}

extern "C" int ovp_klt_match_frame(ovp_ctx* c, const ovp_klt_frame_in* in, ovp_klt_frame_out* out) {
  Klt* d = klt_of(c);
  if (!c || !in || !out) return OVP_E_ARG;
  if (!d) return OVP_E_STATE;
  // ---- every check before anything is touched or enqueued ----
  const int n = in->n;
  const bool check = in->check != 0, to_db = in->to_database != 0;
  if (n < 0) return OVP_E_ARG;
  if (d->fed < 2 || (to_db && !c->featdb)) return OVP_E_STATE;
  if (n > d->max_points) return OVP_E_CAPACITY;
  if (!in->epi && (check || to_db)) return OVP_E_ARG;
  if (in->epi && !klt_epi_opts_ok(in->epi)) return OVP_E_ARG;
  if (in->mask && in->mask_stride < d->width) return OVP_E_ARG;
  if (to_db && !(in->timestamp == in->timestamp)) return OVP_E_ARG;
  if (n == 0) {
    out->n_kept = 0;
    return 0;
  }
  if (!in->pts_prev || !in->ids) return OVP_E_ARG;
  for (int i = 0; i < 2 * n; ++i)
    if (!std::isfinite(in->pts_prev[i])) return OVP_E_ARG;
  {
    std::vector<int64_t> sorted(in->ids, in->ids + n);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return OVP_E_ARG;  // the ids of a frame are distinct
  }
  if (check && n < OVP_EPI_MIN_POINTS) {  // :1319-1323 all zeros, no KLT; nothing is kept and nothing appended
    out->n_kept = 0;
    if (out->keep) memset(out->keep, 0, n);
    if (out->mask_epi) memset(out->mask_epi, 0, n);
    memset(&out->info, 0, sizeof(out->info));
    out->info.winner_h = out->info.winner_model = -1, out->info.too_few = 1;
    return 0;
  }
  std::vector<int32_t> slot, free_list;
  std::vector<unsigned char> fresh;
  int n_fresh = 0;
  FdbTable table = {};
  if (to_db) {
    slot.resize(n), free_list.resize(n), fresh.resize(n);
    const int rp = ovp_featdb_frame_plan(c, in->timestamp, n, in->ids, slot.data(), fresh.data(), free_list.data(), &n_fresh, &table);
    if (rp) return rp;
  }
  const size_t mask_bytes = in->mask ? (size_t)d->width * d->height : 0;
  StageLayout L;
  const size_t o_pts = L.take(sizeof(float) * 2 * n), o_id = L.take(sizeof(long long) * n), o_slot = L.take(sizeof(int) * n),
               o_fresh = L.take(n), o_free = L.take(sizeof(int) * n), o_tab = L.take(sizeof(int) * (n + 1)), o_mask = L.take(mask_bytes);
  StageLayout R;
  const size_t r_out = R.take(sizeof(float) * 2 * n), r_st = R.take(n), r_mepi = R.take(n), r_uvn = R.take(sizeof(float) * 2 * n),
               r_keep = R.take(n), r_idx = R.take(sizeof(int) * n), r_kuv = R.take(sizeof(float) * 2 * n),
               r_kuvn = R.take(sizeof(float) * 2 * n), r_nk = R.take(sizeof(int)), r_info = R.take(sizeof(EpiInfoDev)),
               r_u0 = R.take(sizeof(float) * 2 * n), r_it = R.take((size_t)n * KLT_MAX_LEVELS);
  // ---- from here on the call goes through ----
  HIPCHK(hipSetDevice(c->device));
  // the first fused call (or the first with a mask) grows the staging - the mask's device buffer is its tail - and the result block
  // to a frame's size at max_points, and waits for the stream once
  {
    StageLayout LM, RM;
    const size_t m = (size_t)d->max_points;
    LM.take(8 * m), LM.take(8 * m), LM.take(4 * m), LM.take(m), LM.take(4 * m), LM.take(4 * (m + 1)), LM.take(mask_bytes);
    RM.take(8 * m), RM.take(m), RM.take(m), RM.take(8 * m), RM.take(m), RM.take(4 * m), RM.take(8 * m), RM.take(8 * m), RM.take(4),
        RM.take(sizeof(EpiInfoDev)), RM.take(8 * m), RM.take(m * KLT_MAX_LEVELS);
    HIPCHK(d->stage.reserve(LM.bytes(), 0, c->stream));
    if (RM.bytes() > d->res_cap) {
      HIPCHK(hipStreamSynchronize(c->stream));
      HIPCHK(d->dres.reserve(RM.bytes(), 0));
      HIPCHK(d->hres.reserve(RM.bytes(), 0));
      d->res_cap = RM.bytes(), d->last_n = 0;
    }
  }
  int rc = 0;
  char* h = d->stage.begin(L.bytes(), &rc);
  if (!h) return rc;
  memcpy(h + o_pts, in->pts_prev, sizeof(float) * 2 * n);
  memcpy(h + o_id, in->ids, sizeof(long long) * n);
  if (to_db) {
    memcpy(h + o_slot, slot.data(), sizeof(int) * n);
    memcpy(h + o_fresh, fresh.data(), n);
    memcpy(h + o_free, free_list.data(), sizeof(int) * n_fresh);
  }
  std::vector<int32_t> table_it(n + 1, 0);
  if (check) {
    ovp_epi_table(n, in->epi->confidence, in->epi->max_iters, table_it.data());
    memcpy(h + o_tab, table_it.data(), sizeof(int) * (n + 1));
  }
  for (int y = 0; in->mask && y < d->height; ++y) memcpy(h + o_mask + (size_t)y * d->width, in->mask + (size_t)y * in->mask_stride, d->width);
  const char* dv = d->stage.dev();
  char* dr = (char*)d->dres.get();
  HIPCHK(d->stage.send(L.bytes(), c->stream, Fence::CallerWaits));
  // :1326-1330 k_klt_track, its output stays on the device
  KltTrackArgs a;
  const unsigned char *pc = d->pyr[d->cur].get(), *pp = d->pyr[d->cur ^ 1].get();
  for (int l = 0; l < KLT_MAX_LEVELS; ++l) {
    const int q = l < d->n_levels ? l : 0;
    a.prev[l] = pp + d->loff[q], a.cur[l] = pc + d->loff[q], a.w[l] = d->lw[q], a.h[l] = d->lh[q];
  }
  a.n_levels = d->n_levels, a.n = n, a.win = d->win;
  a.pts = a.guess = (const float*)(dv + o_pts);  // :1329 the reference passes pts1 = pts0
  a.out = (float*)(dr + r_out), a.status = (unsigned char*)(dr + r_st), a.iters = (unsigned char*)(dr + r_it);
  if (d->timed) HIPCHK(hipEventRecord(d->ev[Klt::EV_TRK0], c->stream));
  const dim3 grid((n + 3) / 4), block(256);
  const int npl = (d->win * d->win + 63) / 64;
  if (npl <= 1) hipLaunchKernelGGL(k_klt_track<1>, grid, block, 0, c->stream, a);
  else if (npl <= 2) hipLaunchKernelGGL(k_klt_track<2>, grid, block, 0, c->stream, a);
  else if (npl <= 4) hipLaunchKernelGGL(k_klt_track<4>, grid, block, 0, c->stream, a);
  else hipLaunchKernelGGL(k_klt_track<7>, grid, block, 0, c->stream, a);
  HIPCHK(hipGetLastError());
  if (d->timed) HIPCHK(hipEventRecord(d->ev[Klt::EV_TRK1], c->stream));
  // :1331-1350 the epipolar kernels on the device-resident points and status; without the check the undistortion alone
  if (in->epi) {
    const ovp_epipolar_opts* o = in->epi;
    EpiLaunch e;
    e.n = n, e.max_iters = o->max_iters, e.mode = o->mode, e.seed = o->seed;
    for (int k = 0; k < 8; ++k) e.intr[k] = o->intrinsics[k];
    e.thr2 = (float)(o->threshold * o->threshold);
    e.pts0 = (const float*)(dv + o_pts), e.pts1 = (const float*)(dr + r_out), e.status = (const unsigned char*)(dr + r_st);
    e.table = (const int*)(dv + o_tab);
    e.samples = d->epi_samples.get(), e.n_models = d->epi_nmodels.get(), e.models = d->epi_models.get(), e.counts = d->epi_counts.get();
    e.mask = (unsigned char*)(dr + r_mepi), e.uvn0 = (float*)(dr + r_u0), e.uvn1 = (float*)(dr + r_uvn), e.info = (EpiInfoDev*)(dr + r_info);
    hipEvent_t ev_epi[5];
    for (int k = 0; k < 5; ++k) ev_epi[k] = d->ev[Klt::EV_EPI + k];
    e.ev = d->timed && check ? ev_epi : nullptr;
    if (d->timed && !check) HIPCHK(hipEventRecord(ev_epi[0], c->stream));
    const int rl = check ? ovp_epi_enqueue(e, c->stream) : ovp_epi_enqueue_undistort(e, c->stream);
    if (rl) return rl;
    if (d->timed && !check) HIPCHK(hipEventRecord(ev_epi[1], c->stream));
  }
  // :536-557 the keep rule, the survivors and database->update_feature
  KltFrameArgs f = {};
  f.n = n, f.cols = d->width, f.rows = d->height, f.to_db = to_db ? 1 : 0;
  f.pts = (const float2*)(dr + r_out), f.mask_epi = (const unsigned char*)(dr + (check ? r_mepi : r_st));
  f.uvn = in->epi ? (const float2*)(dr + r_uvn) : nullptr;
  f.mask = in->mask ? (const unsigned char*)(dv + o_mask) : nullptr;
  f.slot = (const int*)(dv + o_slot), f.fresh = (const unsigned char*)(dv + o_fresh), f.ids = (const long long*)(dv + o_id);
  f.free_slots = (const int*)(dv + o_free), f.stamp = in->timestamp, f.t = table;
  f.keep = (unsigned char*)(dr + r_keep), f.kept_index = (int*)(dr + r_idx), f.kept_uv = (float2*)(dr + r_kuv);
  f.kept_uvn = (float2*)(dr + r_kuvn), f.n_kept = (int*)(dr + r_nk);
  if (d->timed) HIPCHK(hipEventRecord(d->ev[Klt::EV_FRM0], c->stream));
  const int rf = ovp_klt_frame_enqueue(f, c->stream);
  if (rf) return rf;
  if (d->timed) HIPCHK(hipEventRecord(d->ev[Klt::EV_FRM1], c->stream));
  SeqChannel& ch = d->hres.channel(0);
  const unsigned seq = ch.arm();
  HIPCHK(ovp_launch_publish_block(dr, d->hres.dev(d->hres.payload()), r_u0, ch.word_dev(), seq, 0, c->stream));  // (up to the info block)
  const int rw = ch.wait(c->stream);
  if (rw) return rw;
  d->stage.done();
  if (d->timed) {
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipEventElapsedTime(&d->ms[2], d->ev[Klt::EV_TRK0], d->ev[Klt::EV_TRK1]));
    // the epipolar slots are this call's: the four kernels with the check, the undistortion alone without it, zeros for what did not run
    for (int k = 0; k < 4; ++k) d->ms[6 + k] = 0.0f;
    for (int k = 0; in->epi && k < (check ? 4 : 1); ++k)
      HIPCHK(hipEventElapsedTime(&d->ms[6 + k], d->ev[Klt::EV_EPI + k], d->ev[Klt::EV_EPI + k + 1]));
    HIPCHK(hipEventElapsedTime(&d->ms[13], d->ev[Klt::EV_FRM0], d->ev[Klt::EV_FRM1]));
  }
  const char* hr = (const char*)d->hres.payload();
  const unsigned char* keep = (const unsigned char*)(hr + r_keep);
  const int n_kept = *(const int*)(hr + r_nk);
  // the database's map and shadow follow the device: the same assignment, replayed over the published keep vector
  if (to_db) ovp_featdb_frame_commit(c, in->timestamp, n, in->ids, keep);
  out->n_kept = n_kept;
  if (out->keep) memcpy(out->keep, keep, n);
  if (out->pts_out) memcpy(out->pts_out, hr + r_out, sizeof(float) * 2 * n);
  if (out->status) memcpy(out->status, hr + r_st, n);
  if (out->mask_epi) memcpy(out->mask_epi, hr + (check ? r_mepi : r_st), n);
  if (out->uvn && in->epi) memcpy(out->uvn, hr + r_uvn, sizeof(float) * 2 * n);
  if (out->kept_index) memcpy(out->kept_index, hr + r_idx, sizeof(int) * (size_t)n_kept);
  memset(&out->info, 0, sizeof(out->info));
  out->info.winner_h = out->info.winner_model = -1;
  if (check) memcpy(&out->info, hr + r_info, sizeof(out->info));
  d->last_n = 0;  // (the mailbox no longer holds a track's iterations)
  d->frm_kept = n_kept, d->frm_seq = seq, d->frm_uvn = in->epi != nullptr, d->frm_uv_off = r_kuv, d->frm_uvn_off = r_kuvn;
  if (check) d->epi_H = in->epi->max_iters, d->epi_table.swap(table_it);
  return 0;
}

extern "C" long ovp_klt_debug(ovp_ctx* c, const char* what, int level, void* out, long cap) {
  Klt* d = klt_of(c);
  if (!d) return c ? OVP_E_STATE : OVP_E_ARG;
  if (!what || !out || cap < 0) return OVP_E_ARG;
  if (!strncmp(what, "epi_", 4)) {
    if (!d->epi_H) return OVP_E_STATE;
    const size_t H = (size_t)d->epi_H;
    if (!strcmp(what, "epi_table")) {
      const size_t bytes = sizeof(int32_t) * d->epi_table.size();
      if ((size_t)cap < bytes) return OVP_E_ARG;
      memcpy(out, d->epi_table.data(), bytes);
      return (long)bytes;
    }
    const void* src[2] = {nullptr, nullptr};
    size_t bytes[2] = {0, 0};
    if (!strcmp(what, "epi_samples")) src[0] = d->epi_samples.get(), bytes[0] = sizeof(int) * 7 * H;
    else if (!strcmp(what, "epi_counts")) src[0] = d->epi_counts.get(), bytes[0] = sizeof(int) * 3 * H;
    else if (!strcmp(what, "epi_models"))
      src[0] = d->epi_nmodels.get(), bytes[0] = sizeof(int) * H, src[1] = d->epi_models.get(), bytes[1] = sizeof(double) * 27 * H;
    else return OVP_E_ARG;
    const size_t off1 = (bytes[0] + 7) & ~(size_t)7;
    const size_t total = bytes[1] ? off1 + bytes[1] : bytes[0];
    if ((size_t)cap < total) return OVP_E_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(out, src[0], bytes[0], hipMemcpyDeviceToHost));
    if (bytes[1]) HIPCHK(hipMemcpy((char*)out + off1, src[1], bytes[1], hipMemcpyDeviceToHost));
    return (long)total;
  }
  if (!strcmp(what, "timer")) {
    d->timed = level != 0;
    return 0;
  }
  if (!strcmp(what, "time")) {
    if (cap < (long)(3 * sizeof(float))) return OVP_E_ARG;  // [3] of the tracker alone, [6] with the detector's kernels, .. [14]
    const size_t bytes = std::min((size_t)cap / sizeof(float), sizeof(d->ms) / sizeof(float)) * sizeof(float);
    memcpy(out, d->ms, bytes);
    return (long)bytes;
  }
  if (!strcmp(what, "frame_uv") || !strcmp(what, "frame_uvn")) {  // the compacted survivors of the last ovp_klt_match_frame
    const bool un = what[8] == 'n';
    if (d->frm_kept < 0 || d->hres.channel(0).armed() != d->frm_seq || (un && !d->frm_uvn)) return OVP_E_STATE;
    const size_t bytes = sizeof(float) * 2 * (size_t)d->frm_kept;
    if ((size_t)cap < bytes) return OVP_E_ARG;
    if (bytes) memcpy(out, (const char*)d->hres.payload() + (un ? d->frm_uvn_off : d->frm_uv_off), bytes);
    return (long)bytes;
  }
  if (!strcmp(what, "refine")) {  // k_fast_subpix on `level` points of the caller's: out holds float [2n] starts, then float [2n]
    const int n = level;
    if (n < 1 || n > d->max_points || (size_t)cap < sizeof(float) * 2 * (size_t)n) return OVP_E_ARG;
    if (d->fed < 1) return OVP_E_STATE;
    StageLayout R;
    const size_t r_xy = R.take(sizeof(int) * 2 * n), r_resp = R.take(sizeof(int) * n), r_ref = R.take(sizeof(float) * 2 * n);
    if (R.bytes() > d->res_cap) return OVP_E_CAPACITY;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    char* dr = (char*)d->dres.get();
    for (int i = 0; i < 2 * n; ++i)
      if (!std::isfinite(((const float*)out)[i])) return OVP_E_ARG;
    HIPCHK(hipMemcpy(dr + r_xy, out, sizeof(float) * 2 * n, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(dr + r_resp, 1, sizeof(int) * n));  // (every slot is taken)
    FastSubpixArgs a;
    a.img = d->pyr[d->cur].get(), a.cols = d->width, a.rows = d->height, a.n = n;
    a.xy = nullptr, a.start = (const float*)(dr + r_xy), a.resp = (const int*)(dr + r_resp), a.out = (float*)(dr + r_ref);
    fast_subpix_weights(a.w);
    hipLaunchKernelGGL(k_fast_subpix, dim3((n + 3) / 4), dim3(256), 0, c->stream, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(out, dr + r_ref, sizeof(float) * 2 * n, hipMemcpyDeviceToHost));
    return (long)(sizeof(float) * 2 * n);
  }
  if (!strcmp(what, "score") || !strcmp(what, "nms")) {  // of the last ovp_klt_detect, level 0
    if (!d->det_done) return OVP_E_STATE;
    const size_t bytes = (size_t)d->width * d->height;
    if ((size_t)cap < bytes) return OVP_E_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(out, what[0] == 's' ? d->score.get() : d->nms.get(), bytes, hipMemcpyDeviceToHost));
    return (long)bytes;
  }
  if (!strcmp(what, "clahe_lut")) {  // of the last CLAHE feed: [tiles_y tiles_x][256]
    if (!d->lut_tiles) return OVP_E_STATE;
    const size_t bytes = (size_t)d->lut_tiles * CLAHE_BINS;
    if ((size_t)cap < bytes) return OVP_E_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(out, d->clahe_lut.get(), bytes, hipMemcpyDeviceToHost));
    return (long)bytes;
  }
  if (!strcmp(what, "iters")) {  // of the last ovp_klt_track: [n][8] iterations per level (the mailbox still holds them)
    const size_t off = StageLayout::al(sizeof(float) * 2 * d->last_n) + StageLayout::al(d->last_n), bytes = (size_t)d->last_n * KLT_MAX_LEVELS;
    if ((size_t)cap < bytes) return OVP_E_ARG;
    if (bytes) memcpy(out, (const char*)d->hres.payload() + off, bytes);
    return (long)bytes;
  }
  if (!strcmp(what, "dims")) {
    if (level < 0 || level >= d->n_levels || cap < (long)(2 * sizeof(int))) return OVP_E_ARG;
    const int wh[2] = {d->lw[level], d->lh[level]};
    memcpy(out, wh, sizeof(wh));
    return (long)sizeof(wh);
  }
  int half;
  if (!strcmp(what, "cur")) half = d->cur;
  else if (!strcmp(what, "prev")) half = d->cur ^ 1;
  else if (!strcmp(what, "equalized")) half = d->cur, level = 0;  // the equalised image is level 0 of the current half
  else return OVP_E_ARG;
  if (level < 0 || level >= d->n_levels) return OVP_E_ARG;
  if (d->fed < (half == d->cur ? 1 : 2)) return OVP_E_STATE;
  const size_t bytes = (size_t)d->lw[level] * d->lh[level];
  if ((size_t)cap < bytes) return OVP_E_ARG;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpy(out, d->pyr[half].get() + d->loff[level], bytes, hipMemcpyDeviceToHost));
  return (long)bytes;
}
