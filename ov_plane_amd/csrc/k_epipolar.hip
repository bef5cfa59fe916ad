// The epipolar check of TrackPlane::perform_matching (track_plane/TrackPlane.cpp:1331-1350) on the device: undistort_cv of both
// point sets and cv::findFundamentalMat(FM_RANSAC).  OpenCV and ov_core are not in the reference tree: the stage is RECALLED from
// its published form and UNPINNED; tests/epi_ref.py is the restatement it is held to and says which conventions are recalled and
// which are our own (the generator, the tries per hypothesis, the elimination with complete pivoting).
//   k_epi_undistort  a thread per point and image: cv::undistortPoints (5 fixed-point iterations) or cv::fisheye::undistortPoints
//                    (Newton on theta, at most 10 steps, 1e-8), f64, rounded to f32 as undistort_cv's cv::Point2f is
//   k_epi_models     a lane per hypothesis: the draws, checkSubset, the 7 x 9 system, its null space by Gauss-Jordan elimination
//                    with complete pivoting, the cubic in closed form, the scaling.  The matrix, the set's points and the column
//                    permutation are lane-private in LDS at a stride of 64 elements: lane l's element e is word e * 64 + l, so a
//                    wave's access to one element - whichever element each lane picked - never meets a bank twice within a half.
//   k_epi_count      a wave per (hypothesis, model): lanes stride over the points, ballot and popcount per 64
//   k_epi_select     one wave: lane 0 replays RANSACPointSetRegistrator::run over the counts with the host's table, then the wave
//                    recomputes the winner's mask, ANDs the status (:1348) and writes the info block
// All of it is f64 with contraction off: the samples, the elimination and every decision up to the cubic's libm calls (acos, cos,
// cbrt, sqrt) are the restatement's bits.  Every index into a point array is a draw in [0, n) or a loop index below n.
#include "k_epipolar.h"

#include <cfloat>
#include <cmath>

#include "ovplane_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr double EPI_PI = 3.141592653589793;

__global__ __launch_bounds__(256) void k_epi_undistort(EpiLaunch a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * a.n) return;
  const int img = i >= a.n, p = img ? i - a.n : i;
  const float* src = img ? a.pts1 : a.pts0;
  float* dst = img ? a.uvn1 : a.uvn0;
  const float u = src[2 * p], v = src[2 * p + 1];
  if (a.mode == 0) {
    dst[2 * p] = u, dst[2 * p + 1] = v;
    return;
  }
  const double fx = a.intr[0], fy = a.intr[1], cx = a.intr[2], cy = a.intr[3], k1 = a.intr[4], k2 = a.intr[5], k3 = a.intr[6], k4 = a.intr[7];
  const double x0 = ((double)u - cx) / fx, y0 = ((double)v - cy) / fy;
  double x = x0, y = y0;
  if (a.mode == 1) {
    const double p1 = k3, p2 = k4;
    for (int it = 0; it < 5; ++it) {
      const double r2 = x * x + y * y;
      const double icdist = 1.0 / (1.0 + (k2 * r2 + k1) * r2);
      const double dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x);
      const double dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y;
      x = (x0 - dx) * icdist, y = (y0 - dy) * icdist;
    }
  } else {
    double th_d = sqrt(x0 * x0 + y0 * y0);
    th_d = fmin(fmax(th_d, -0.5 * EPI_PI), 0.5 * EPI_PI);
    double scale = 1.0;
    if (th_d > 1e-8) {
      double th = th_d;
      for (int it = 0; it < 10; ++it) {
        const double t2 = th * th, t4 = t2 * t2, t6 = t2 * t2 * t2, t8 = t2 * t2 * t2 * t2;
        const double fix = (th * (1.0 + k1 * t2 + k2 * t4 + k3 * t6 + k4 * t8) - th_d) /
                           (1.0 + 3.0 * k1 * t2 + 5.0 * k2 * t4 + 7.0 * k3 * t6 + 9.0 * k4 * t8);
        th = th - fix;
        if (fabs(fix) < 1e-8) break;
      }
      scale = tan(th) / th_d;
    }
    x = x0 * scale, y = y0 * scale;
  }
  dst[2 * p] = (float)x, dst[2 * p + 1] = (float)y;
}

__device__ __forceinline__ unsigned epi_draw(unsigned seed, unsigned h, unsigned t, unsigned n) {
  unsigned x = seed + 0x9E3779B9u * (h + 1u) + 0x85EBCA6Bu * (t + 1u);
  x ^= x >> 16, x *= 0x85EBCA6Bu, x ^= x >> 13, x *= 0xC2B2AE35u, x ^= x >> 16;
  return (unsigned)(((unsigned long long)x * n) >> 32);
}

// haveCollinearPoints: the last of the seven against every pair of the others; px / py lane-private at stride 64
__device__ __forceinline__ bool epi_collinear(const double* px, const double* py) {
  const double xi = px[6 * 64], yi = py[6 * 64];
  for (int j = 0; j < 6; ++j) {
    const double dx1 = px[j * 64] - xi, dy1 = py[j * 64] - yi;
    for (int k = 0; k < j; ++k) {
      const double dx2 = px[k * 64] - xi, dy2 = py[k * 64] - yi;
      if (fabs(dx2 * dy1 - dy2 * dx1) <= (double)FLT_EPSILON * (fabs(dx1) + fabs(dy1) + fabs(dx2) + fabs(dy2))) return true;
    }
  }
  return false;
}

__device__ __forceinline__ double epi_det3(const double* m) {
  return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

// det of a with row i taken from b
__device__ __forceinline__ double epi_det3_mix(const double* a, const double* b, int i) {
  double m[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) m[k] = (k / 3 == i) ? b[k] : a[k];
  return epi_det3(m);
}

// cv::solveCubic (recalled): c0 x^3 + c1 x^2 + c2 x + c3 = 0 -> number of real roots, in its order
__device__ int epi_solve_cubic(double a0, double a1, double a2, double a3, double& r0, double& r1, double& r2) {
  if (a0 == 0.0) {
    if (a1 == 0.0) {
      if (a2 == 0.0) return 0;
      r0 = -a3 / a2;
      return 1;
    }
    double d = a2 * a2 - 4.0 * a1 * a3;
    if (d < 0.0) return 0;
    d = sqrt(d);
    const double q1 = (-a2 + d) * 0.5, q2 = (a2 + d) * -0.5;
    if (fabs(q1) > fabs(q2)) r0 = q1 / a1, r1 = a3 / q1;
    else r0 = q2 / a1, r1 = a3 / q2;
    return d > 0.0 ? 2 : 1;
  }
  const double b1 = a1 / a0, b2 = a2 / a0, b3 = a3 / a0;
  const double Q = (b1 * b1 - 3.0 * b2) / 9.0;
  const double R = (2.0 * b1 * b1 * b1 - 9.0 * b1 * b2 + 27.0 * b3) / 54.0;
  const double Q3 = Q * Q * Q, d = Q3 - R * R, t2 = b1 / 3.0;
  if (d > 0.0) {
    const double theta = acos(R / sqrt(Q3));
    const double t0 = -2.0 * sqrt(Q), t1 = theta / 3.0, pi23 = 2.0 * EPI_PI / 3.0;
    r0 = t0 * cos(t1) - t2, r1 = t0 * cos(t1 + pi23) - t2, r2 = t0 * cos(t1 + pi23 + pi23) - t2;
    return 3;
  }
  if (d == 0.0) {
    const double e = cbrt(fabs(R));
    if (R >= 0.0) r0 = -2.0 * e - t2, r1 = e - t2;
    else r0 = 2.0 * e - t2, r1 = -e - t2;
    return 2;
  }
  double e = cbrt(sqrt(-d) + fabs(R));
  if (R > 0.0) e = -e;
  r0 = (e + Q / e) - t2;
  return 1;
}

constexpr int EPI_LDS_A = 63 * 64, EPI_LDS_P = 28 * 64;  // doubles: the matrix; the set's points (later the two null vectors)

__global__ __launch_bounds__(64) void k_epi_models(EpiLaunch a) {
  __shared__ double sA[EPI_LDS_A];
  __shared__ double sP[EPI_LDS_P];
  __shared__ int sI[7 * 64];
  __shared__ int sPerm[9 * 64];
  const int lane = threadIdx.x, h = blockIdx.x * 64 + lane;
  if (h >= a.max_iters) return;  // (no barrier below: every lane works on its own words)
  double* A = sA + lane;         // A[(i * 9 + j) * 64]
  double* P = sP + lane;         // x0 [0..6], y0 [7..13], x1 [14..20], y1 [21..27], each * 64
  int* I = sI + lane;
  int* perm = sPerm + lane;
  const unsigned n = (unsigned)a.n;
  // ---- the draws and checkSubset ----
  int t = 0, tries = 0, cnt = 0;
  bool have = false;
  while (tries < EPI_MAX_SUBSET_TRIES && t < EPI_MAX_DRAWS) {
    const int i = (int)epi_draw(a.seed, (unsigned)h, (unsigned)t, n);
    ++t;
    bool dup = false;
    for (int k = 0; k < cnt; ++k) dup |= I[k * 64] == i;
    if (dup) continue;
    I[cnt * 64] = i;
    P[cnt * 64] = (double)a.uvn0[2 * i], P[(7 + cnt) * 64] = (double)a.uvn0[2 * i + 1];
    P[(14 + cnt) * 64] = (double)a.uvn1[2 * i], P[(21 + cnt) * 64] = (double)a.uvn1[2 * i + 1];
    if (++cnt < 7) continue;
    if (epi_collinear(P, P + 7 * 64) || epi_collinear(P + 14 * 64, P + 21 * 64)) {
      ++tries, cnt = 0;
      continue;
    }
    have = true;
    break;
  }
  for (int k = 0; k < 7; ++k) a.samples[h * 7 + k] = have ? I[k * 64] : -1;
  double* Fout = a.models + (size_t)h * 27;
  for (int k = 0; k < 27; ++k) Fout[k] = 0.0;
  int nm = 0;
  bool alive = have;
  if (alive) {
    // ---- the 7 x 9 system, m1^T F m0 = 0 ----
    for (int i = 0; i < 7; ++i) {
      const double x0 = P[i * 64], y0 = P[(7 + i) * 64], x1 = P[(14 + i) * 64], y1 = P[(21 + i) * 64];
      double* r = A + i * 9 * 64;
      r[0] = x1 * x0, r[64] = x1 * y0, r[2 * 64] = x1, r[3 * 64] = y1 * x0, r[4 * 64] = y1 * y0, r[5 * 64] = y1, r[6 * 64] = x0, r[7 * 64] = y0,
      r[8 * 64] = 1.0;
    }
    for (int j = 0; j < 9; ++j) perm[j * 64] = j;
    // ---- Gauss-Jordan with complete pivoting: the first largest |a| of the remaining block in row-major order ----
    for (int k = 0; k < 7 && alive; ++k) {
      int pr = k, pc = k;
      double big = -1.0;
      for (int i = k; i < 7; ++i)
        for (int j = k; j < 9; ++j) {
          const double v = fabs(A[(i * 9 + j) * 64]);
          if (v > big) big = v, pr = i, pc = j;
        }
      if (pr != k)
        for (int j = 0; j < 9; ++j) {
          const double s = A[(k * 9 + j) * 64];
          A[(k * 9 + j) * 64] = A[(pr * 9 + j) * 64], A[(pr * 9 + j) * 64] = s;
        }
      if (pc != k) {
        for (int i = 0; i < 7; ++i) {
          const double s = A[(i * 9 + k) * 64];
          A[(i * 9 + k) * 64] = A[(i * 9 + pc) * 64], A[(i * 9 + pc) * 64] = s;
        }
        const int s = perm[k * 64];
        perm[k * 64] = perm[pc * 64], perm[pc * 64] = s;
      }
      const double piv = A[(k * 9 + k) * 64];
      if (!(isfinite(piv) && piv != 0.0)) {
        alive = false;
        break;
      }
      for (int j = k; j < 9; ++j) A[(k * 9 + j) * 64] = A[(k * 9 + j) * 64] / piv;
      for (int i = 0; i < 7; ++i) {
        if (i == k) continue;
        const double f = A[(i * 9 + k) * 64];
        for (int j = k; j < 9; ++j) A[(i * 9 + j) * 64] = A[(i * 9 + j) * 64] - f * A[(k * 9 + j) * 64];
      }
    }
  }
  if (alive) {
    // ---- the two null vectors, back in the columns' own order (the set's points are no longer needed: P holds them) ----
    for (int c = 0; c < 2; ++c) {
      for (int j = 0; j < 7; ++j) P[(c * 9 + perm[j * 64]) * 64] = -A[(j * 9 + 7 + c) * 64];
      P[(c * 9 + perm[(7 + c) * 64]) * 64] = 1.0;
      P[(c * 9 + perm[(8 - c) * 64]) * 64] = 0.0;
    }
    double Ad[9], B[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) B[k] = P[(9 + k) * 64], Ad[k] = P[k * 64] - B[k];
    const double c0 = epi_det3(Ad), c3 = epi_det3(B);
    const double c1 = (epi_det3_mix(Ad, B, 0) + epi_det3_mix(Ad, B, 1)) + epi_det3_mix(Ad, B, 2);
    const double c2 = (epi_det3_mix(B, Ad, 0) + epi_det3_mix(B, Ad, 1)) + epi_det3_mix(B, Ad, 2);
    if (isfinite(c0) && isfinite(c1) && isfinite(c2) && isfinite(c3)) {
      double r0 = 0.0, r1 = 0.0, r2 = 0.0;
      const int nr = epi_solve_cubic(c0, c1, c2, c3, r0, r1, r2);
      for (int q = 0; q < nr; ++q) {
        double lam = q == 0 ? r0 : (q == 1 ? r1 : r2), mu = 1.0;
        const double s = Ad[8] * lam + B[8];
        const bool tiny = !(fabs(s) > DBL_EPSILON);  // run7Point: F33 = 1 when it is not tiny
        if (!tiny) mu = mu / s, lam = lam * mu;
        double F[9];
        bool fin = true;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          F[k] = Ad[k] * lam + B[k] * mu;
          if (k < 8) fin = fin && isfinite(F[k]);
        }
        F[8] = tiny ? 0.0 : 1.0;
        if (!fin) continue;  // (our own rule: a root whose matrix is not finite is dropped)
#pragma unroll
        for (int k = 0; k < 9; ++k) Fout[nm * 9 + k] = F[k];
        ++nm;
      }
    }
  }
  a.n_models[h] = nm;
}

// computeError for a fundamental matrix on point i: is the larger squared distance, as a float, at most thr2?
__device__ __forceinline__ bool epi_inlier(const double* F, const float* u0, const float* u1, int i, float thr2) {
  const double x0 = (double)u0[2 * i], y0 = (double)u0[2 * i + 1], x1 = (double)u1[2 * i], y1 = (double)u1[2 * i + 1];
  double a = F[0] * x0 + F[1] * y0 + F[2], b = F[3] * x0 + F[4] * y0 + F[5], c = F[6] * x0 + F[7] * y0 + F[8];
  const double s2 = 1.0 / (a * a + b * b), d2 = x1 * a + y1 * b + c;
  a = F[0] * x1 + F[3] * y1 + F[6], b = F[1] * x1 + F[4] * y1 + F[7], c = F[2] * x1 + F[5] * y1 + F[8];
  const double s1 = 1.0 / (a * a + b * b), d1 = x0 * a + y0 * b + c;
  const double e1 = d1 * d1 * s1, e2 = d2 * d2 * s2;
  return (float)e1 <= thr2 && (float)e2 <= thr2;  // the rounding is monotonic: max first or last is the same; a NaN is no inlier
}

__global__ __launch_bounds__(256) void k_epi_count(EpiLaunch a) {
  const int lane = threadIdx.x & 63, hm = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (hm >= a.max_iters * 3) return;  // (wave-uniform)
  const int h = hm / 3, m = hm - 3 * h;
  int total = 0;
  if (m < a.n_models[h]) {
    double F[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) F[k] = a.models[(size_t)h * 27 + m * 9 + k];
    for (int base = 0; base < a.n; base += 64) {
      const int i = base + lane;
      const bool in = i < a.n && epi_inlier(F, a.uvn0, a.uvn1, i, a.thr2);
      total += __popcll(__ballot(in));
    }
  }
  if (lane == 0) a.counts[hm] = total;
}

__global__ __launch_bounds__(64) void k_epi_select(EpiLaunch a) {
  __shared__ int s_best[2];
  const int lane = threadIdx.x;
  if (lane == 0) {
    int niters = a.max_iters, bh = -1, bm = -1, best = 0, h = 0, with_model = 0;
    for (; h < niters; ++h)
      for (int m = 0; m < a.n_models[h]; ++m) {
        const int c = a.counts[h * 3 + m];
        if (c > (best > 6 ? best : 6)) {
          best = c, bh = h, bm = m;
          const int t = a.table[c];  // (c <= n: the table holds n + 1 entries)
          if (t < niters) niters = t;
        }
      }
    for (int k = 0; k < a.max_iters; ++k) with_model += a.n_models[k] > 0;
    EpiInfoDev* o = a.info;
    for (int k = 0; k < 9; ++k) o->F[k] = bh >= 0 ? a.models[(size_t)bh * 27 + bm * 9 + k] : 0.0;
    o->best_count = best, o->winner_h = bh, o->winner_model = bm, o->niters = niters, o->n_with_model = with_model;
    o->too_few = 0, o->no_model = bh < 0, o->stop = h;
    s_best[0] = bh, s_best[1] = bm;
  }
  __syncthreads();
  const int bh = s_best[0], bm = s_best[1];
  double F[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) F[k] = bh >= 0 ? a.models[(size_t)bh * 27 + bm * 9 + k] : 0.0;
  for (int i = lane; i < a.n; i += 64)
    a.mask[i] = (bh >= 0 && a.status[i] && epi_inlier(F, a.uvn0, a.uvn1, i, a.thr2)) ? 1 : 0;  // :1348
}

// :1319-1323 fewer than ten points: all zeros, no RANSAC
__global__ __launch_bounds__(64) void k_epi_too_few(EpiLaunch a) {
  const int lane = threadIdx.x;
  for (int i = lane; i < a.n; i += 64) a.mask[i] = 0;
  if (lane == 0) {
    EpiInfoDev* o = a.info;
    for (int k = 0; k < 9; ++k) o->F[k] = 0.0;
    o->best_count = 0, o->winner_h = -1, o->winner_model = -1, o->niters = 0, o->n_with_model = 0, o->too_few = 1, o->no_model = 0, o->stop = 0;
  }
}

}  // namespace

int ovp_epi_enqueue(const EpiLaunch& a, hipStream_t stream) {
  if (a.n < 1 || a.max_iters < 1 || a.max_iters > EPI_MAX_ITERS) return OVP_E_ARG;
  hipError_t e;
  if (a.n < EPI_MIN_POINTS) {
    hipLaunchKernelGGL(k_epi_undistort, dim3((2 * a.n + 255) / 256), dim3(256), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_epi_too_few, dim3(1), dim3(64), 0, stream, a);
    return (int)hipGetLastError();
  }
#define EPI_STEP(k)                                                                  \
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;                          \
  if (a.ev && (e = hipEventRecord(a.ev[k], stream)) != hipSuccess) return (int)e;
  if (a.ev && (e = hipEventRecord(a.ev[0], stream)) != hipSuccess) return (int)e;
  hipLaunchKernelGGL(k_epi_undistort, dim3((2 * a.n + 255) / 256), dim3(256), 0, stream, a);
  EPI_STEP(1)
  hipLaunchKernelGGL(k_epi_models, dim3((a.max_iters + 63) / 64), dim3(64), 0, stream, a);
  EPI_STEP(2)
  hipLaunchKernelGGL(k_epi_count, dim3((a.max_iters * 3 + 3) / 4), dim3(256), 0, stream, a);
  EPI_STEP(3)
  hipLaunchKernelGGL(k_epi_select, dim3(1), dim3(64), 0, stream, a);
  EPI_STEP(4)
#undef EPI_STEP
  return 0;
}

int ovp_epi_enqueue_undistort(const EpiLaunch& a, hipStream_t stream) {
  if (a.n < 1) return OVP_E_ARG;
  hipLaunchKernelGGL(k_epi_undistort, dim3((2 * a.n + 255) / 256), dim3(256), 0, stream, a);
  return (int)hipGetLastError();
}

static int epi_update_num_iters(double p, double ep, int model_points, int max_iters) {  // RANSACUpdateNumIters (recalled)
  p = std::min(std::max(p, 0.0), 1.0), ep = std::min(std::max(ep, 0.0), 1.0);
  double num = std::max(1.0 - p, DBL_MIN), denom = 1.0 - std::pow(1.0 - ep, model_points);
  if (denom < DBL_MIN) return 0;
  num = std::log(num), denom = std::log(denom);
  return denom >= 0 || -num >= max_iters * (-denom) ? max_iters : (int)std::lrint(num / denom);
}

void ovp_epi_table(int n, double confidence, int max_iters, int32_t* table) {
  for (int c = 0; c <= n; ++c) table[c] = epi_update_num_iters(confidence, (double)(n - c) / (double)n, 7, max_iters);
}
