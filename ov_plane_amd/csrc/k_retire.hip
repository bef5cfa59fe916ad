// A frame's bookkeeping step on the resident covariance: StateHelper::marginalize for several variables at once
// (state/StateHelper.cpp:276-344) and StateHelper::merge_planes_and_marginalize (state/StateHelper.cpp:654-757) from the first
// fused pair to the last retired plane.  Kernels and entry points of ovp_cov_marginalize_many / ovp_planes_merge_retire:
//   k_cov_compact         P -> P_tmp without the rows / columns of a sorted list of ranges, one launch whatever their number.  A
//                         workgroup scans the removed widths once in LDS, turns them into the map output index -> source index (one
//                         bisection of the scanned prefix per index, once per workgroup, none per element), and then only copies:
//                         16 rows x 256 columns per workgroup, a thread walks one column, reads and writes run along the rows of P.  Columns n_out .. ld of the destination are not written, as k_cov_marginalize
//                         (k_ekf.hip) leaves them.
//   k_plane_merge_gate    one workgroup per merged pair: M = (P[:, new] - P[:, old]) / sigma (n x 3), S = H P H^T + I (3 x 3), its
//                         Cholesky factor, chi2, the angle of the two normals and the decision (:698-723); on acceptance
//                         W = M L^-T, dx = W (L^-1 res) and cp += dx for every plane of the call's table (closest points are Vec(3)).
//   k_plane_merge_apply   P -= W W^T by tiles, both triangles (StateHelper::EKFUpdate, :121-202, for the three rows of the pair); a
//                         rejected pair's launch returns at its decision word, as the _sk kernels of k_init_body.h do.
// Removing rows and columns changes no other entry of P, so the pairs run on the un-compacted matrix, in the reference's order,
// each on the P and the closest points its predecessor left, and ONE compaction behind the last pair retires everything.  The
// result block goes to the host through the object's own Mailbox (ovp_mailbox.h, k_publish.hip).  Plain f64 VALU, every sum in a
// fixed order, no atomics: two runs give the same bits.
#include "ovp_ctx.h"

namespace {

constexpr int RC_ROWS = 16;            // rows of P a workgroup of k_cov_compact copies
constexpr int RT_MAX_PAIRS = 64;       // pairs of one ovp_planes_merge_retire
constexpr int RT_MAX_PLANES = 2 * RT_MAX_PAIRS;
constexpr size_t RT_LDS_CAP = 60 * 1024;

// rg: the removed ranges (x = first column, y = width), sorted by column and disjoint (checked on the host)
__global__ __launch_bounds__(256) void k_cov_compact(const double* __restrict__ src, double* __restrict__ dst, int ld, int n_out,
                                                     const int2* __restrict__ rg, int nr) {
  extern __shared__ int rc_sm[];
  int* a = rc_sm;           // [nr + 1] a[r]: width removed in front of the kept segment r (an inclusive scan, ping-pong with b)
  int* b = a + nr + 1;
  int* smap = b + nr + 1;   // [n_out] source index of an output index
  const int t = threadIdx.x;
  for (int r = t; r <= nr; r += 256) a[r] = r ? rg[r - 1].y : 0;
  __syncthreads();
  for (int off = 1; off <= nr; off <<= 1) {
    for (int r = t; r <= nr; r += 256) b[r] = a[r] + (r >= off ? a[r - off] : 0);
    __syncthreads();
    int* q = a;
    a = b;
    b = q;
  }
  // a[r] = width removed up to and including range r - 1: kept segment r (the source columns between range r - 1 and range r) moves
  // down by a[r] and starts at output index seg0(r) = (r ? rg[r - 1].x + rg[r - 1].y : 0) - a[r].  Every thread takes output
  // indices and finds their segment by bisection of that increasing sequence (<= 10 steps), so the fill is shared by the workgroup
  // whatever the number of ranges.
  for (int o = t; o < n_out; o += 256) {
    int lo = 0, hi = nr;  // the last segment whose first output index is <= o
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (rg[mid - 1].x + rg[mid - 1].y - a[mid] <= o) lo = mid;
      else hi = mid - 1;
    }
    smap[o] = o + a[lo];
  }
  __syncthreads();
  const int c = blockIdx.x * 256 + t;
  if (c >= n_out) return;
  const int cs = smap[c], r0 = blockIdx.y * RC_ROWS;
#pragma unroll 4
  for (int k = 0; k < RC_ROWS; ++k) {
    const int r = r0 + k;
    if (r < n_out) dst[(size_t)r * ld + c] = src[(size_t)smap[r] * ld + cs];
  }
}

// One call's tables on the device.  res: per pair [accepted | chi2 | angle (deg) | negative diagonal | dx n], `stride` doubles apart.
struct MergeJob {
  double* P;
  int ld, n, np, n_planes, stride;
  const int* pair;       // [4][np] first column of the survivor, of the old plane, their rows of the plane table
  const int* plane_col;  // [n_planes]
  double* cp;            // [n_planes][3] closest points as the pairs so far left them
  double white_c, chi2_thr, deg_max;
  double *W, *res;       // [n][3] scratch of the running pair; the result block
};

__global__ __launch_bounds__(256) void k_plane_merge_gate(MergeJob j, int k) {
  extern __shared__ double mg_sm[];
  double* Ms = mg_sm;          // [n][3]
  double* dxs = Ms + 3 * j.n;  // [n]
  __shared__ double Li[9], y[3];
  __shared__ int ok;
  const int t = threadIdx.x, n = j.n;
  const int cn = j.pair[k], co = j.pair[j.np + k], sn = j.pair[2 * j.np + k], so = j.pair[3 * j.np + k];
  double* r = j.res + (size_t)k * j.stride;
  for (int i = t; i < n; i += 256) {
    const double* pr = j.P + (size_t)i * j.ld;
#pragma unroll
    for (int a = 0; a < 3; ++a) Ms[3 * i + a] = j.white_c * (pr[cn + a] - pr[co + a]);
  }
  __syncthreads();
  if (t == 0) {
    // :696-702 the normals and their angle
    double c1[3], c0[3], nn = 0.0, no = 0.0, dot = 0.0;
    for (int a = 0; a < 3; ++a) {
      c1[a] = j.cp[3 * sn + a];
      c0[a] = j.cp[3 * so + a];
      nn += c1[a] * c1[a];
      no += c0[a] * c0[a];
    }
    nn = sqrt(nn);
    no = sqrt(no);
    for (int a = 0; a < 3; ++a) dot += (c1[a] / nn) * (c0[a] / no);
    const double angle = (180.0 / 3.14159265358979323846) * acos(dot);
    // :707-718 S = H P H^T + I from the pair's rows of M (lower triangle), S = L L^T, y = L^-1 res, chi2 = |y|^2
    double S[9], L[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) S[3 * a + b] = j.white_c * (Ms[3 * (cn + a) + b] - Ms[3 * (co + a) + b]) + (a == b ? 1.0 : 0.0);
    bool spd = true;
    for (int q = 0; q < 3; ++q) {
      double d = S[3 * q + q];
      for (int p = 0; p < q; ++p) d -= L[3 * q + p] * L[3 * q + p];
      if (!(d > 0.0)) spd = false, d = 1.0;
      L[3 * q + q] = sqrt(d);
      for (int i = q + 1; i < 3; ++i) {
        double s = S[3 * i + q];
        for (int p = 0; p < q; ++p) s -= L[3 * i + p] * L[3 * q + p];
        L[3 * i + q] = s / L[3 * q + q];
      }
    }
    double chi2 = 0.0;
    for (int i = 0; i < 3; ++i) {
      double s = j.white_c * (0.0 - (c1[i] - c0[i]));
      for (int p = 0; p < i; ++p) s -= L[3 * i + p] * y[p];
      y[i] = s / L[3 * i + i];
      chi2 += y[i] * y[i];
    }
    // L^-1 (lower), column by column
    for (int c = 0; c < 3; ++c)
      for (int i = 0; i < 3; ++i) {
        double s = i == c ? 1.0 : 0.0;
        for (int p = c; p < i; ++p) s -= L[3 * i + p] * Li[3 * p + c];
        Li[3 * i + c] = i < c ? 0.0 : s / L[3 * i + i];
      }
    ok = (spd && chi2 < j.chi2_thr && angle < j.deg_max) ? 1 : 0;  // :723
    r[0] = ok ? 1.0 : 0.0;
    r[1] = chi2;
    r[2] = angle;
    r[3] = 0.0;
  }
  __syncthreads();
  const bool acc = ok != 0;
  for (int i = t; i < n; i += 256) {
    double dx = 0.0;
    if (acc) {
      const double m0 = Ms[3 * i], m1 = Ms[3 * i + 1], m2 = Ms[3 * i + 2];
      const double w0 = m0 * Li[0];
      const double w1 = fma(m1, Li[4], m0 * Li[3]);
      const double w2 = fma(m2, Li[8], fma(m1, Li[7], m0 * Li[6]));
      j.W[3 * i] = w0;
      j.W[3 * i + 1] = w1;
      j.W[3 * i + 2] = w2;
      dx = fma(w2, y[2], fma(w1, y[1], w0 * y[0]));
    }
    r[4 + i] = dx;
    dxs[i] = dx;
  }
  __syncthreads();
  // the planes' values behind the correction, for the pairs to come (Vec::update adds)
  if (acc && t < j.n_planes) {
    const int c = j.plane_col[t];
#pragma unroll
    for (int a = 0; a < 3; ++a) j.cp[3 * t + a] += dxs[c + a];
  }
}

// tiles of 4 rows x 64 columns; r: the pair's result block ([0] decision, [3] negative diagonal)
__global__ __launch_bounds__(256) void k_plane_merge_apply(double* __restrict__ P, int ld, int n, const double* __restrict__ W,
                                                           double* __restrict__ r) {
  if (r[0] == 0.0) return;
  const int t = threadIdx.x;
  const int i = blockIdx.y * 4 + (t >> 6), c = blockIdx.x * 64 + (t & 63);
  if (i >= n || c >= n) return;
  const double* wi = W + 3 * i;
  const double* wc = W + 3 * c;
  const double s = fma(wi[2], wc[2], fma(wi[1], wc[1], wi[0] * wc[0]));
  const double v = P[(size_t)i * ld + c] - s;
  P[(size_t)i * ld + c] = v;
  if (i == c && v < 0.0) r[3] = 1.0;
}

// The entries' own buffers, made on first use and freed with the context.
struct Retire {
  Staged stage;          // the call's tables (a call that reports nothing does not wait: Fence::Event)
  DevBuf<double> dres, W;
  Mailbox hres;          // the merge results: payload from byte 0, channel 0
  size_t res_doubles = 0;
  int stride = 0;
};

int retire_of(ovp_ctx* c, Retire** out) {
  if (!c->retire) {
    auto d = std::make_shared<Retire>();
    d->stride = round_up(4 + c->n_max, 8);
    d->res_doubles = (size_t)RT_MAX_PAIRS * d->stride;
    HIPCHK(d->stage.alloc(64 * 8 + sizeof(int2) * (size_t)c->n_max + sizeof(int) * (4 * (size_t)RT_MAX_PAIRS + RT_MAX_PLANES) +
                          sizeof(double) * 3 * RT_MAX_PLANES));
    HIPCHK(d->dres.alloc(d->res_doubles));
    HIPCHK(d->W.alloc(3 * (size_t)c->n_max + 8));
    HIPCHK(d->hres.alloc(sizeof(double) * d->res_doubles));
    c->retire = d;
  }
  *out = (Retire*)c->retire.get();
  return 0;
}

// The ranges sorted by column; OVP_E_ARG for one outside [0, n), a width below 1 or two that overlap.  *gone: the columns they hold.
int sorted_ranges(int n, int nr, const int* ids, const int* sizes, std::vector<int2>& out, int* gone) {
  out.resize(nr);
  for (int r = 0; r < nr; ++r) {
    if (sizes[r] < 1 || ids[r] < 0 || ids[r] > n - sizes[r]) return OVP_E_ARG;
    out[r] = make_int2(ids[r], sizes[r]);
  }
  std::sort(out.begin(), out.end(), [](const int2& p, const int2& q) { return p.x < q.x; });
  int w = 0;
  for (int r = 0; r < nr; ++r) {
    if (r && out[r - 1].x + out[r - 1].y > out[r].x) return OVP_E_ARG;
    w += out[r].y;
  }
  *gone = w;
  return 0;
}

size_t compact_lds(int nr, int n_out) { return sizeof(int) * (2 * ((size_t)nr + 1) + (size_t)n_out); }

hipError_t launch_compact(const double* src, double* dst, int ld, int n_out, const int2* rg, int nr, hipStream_t s) {
  if (n_out < 1) return hipSuccess;
  hipLaunchKernelGGL(k_cov_compact, dim3((n_out + 255) / 256, (n_out + RC_ROWS - 1) / RC_ROWS), dim3(256), compact_lds(nr, n_out), s, src,
                     dst, ld, n_out, rg, nr);
  return hipGetLastError();
}

}  // namespace

extern "C" int ovp_cov_marginalize_many(ovp_ctx* c, int n_ranges, const int* ids, const int* sizes) {
  if (!c || n_ranges < 0 || (n_ranges > 0 && (!ids || !sizes))) return OVP_E_ARG;
  if (!c->have_cov) return OVP_E_STATE;
  if (n_ranges == 0) return 0;
  std::vector<int2> rg;
  int gone = 0;
  if (const int rc = sorted_ranges(c->n, n_ranges, ids, sizes, rg, &gone)) return rc;
  const int n_out = c->n - gone;
  if (compact_lds(n_ranges, n_out) > RT_LDS_CAP) return OVP_E_CAPACITY;
  // ---- from here on the call goes through ----
  drop_kept_factor(c);  // (writes the covariance: a kept factor no longer belongs to it; a refused or empty call keeps it)
  HIPCHK(hipSetDevice(c->device));
  Retire* d = nullptr;
  if (const int rc = retire_of(c, &d)) return rc;
  int rc = 0;
  char* h = d->stage.begin(sizeof(int2) * n_ranges, &rc);
  if (!h) return rc;
  memcpy(h, rg.data(), sizeof(int2) * n_ranges);
  HIPCHK(d->stage.send(sizeof(int2) * n_ranges, c->stream, Fence::Event));
  HIPCHK(launch_compact(c->P, c->P_tmp, c->ld, n_out, (const int2*)d->stage.dev(), n_ranges, c->stream));
  c->P.swap(c->P_tmp);
  c->n = n_out;
  return 0;
}

extern "C" int ovp_planes_merge_retire(ovp_ctx* c, const ovp_plane_merge_in* in, uint8_t* accepted, double* chi2, double* angle_deg,
                                       double* dx, int dx_stride) {
  if (!c || !in || in->n_pairs < 0 || in->n_planes < 0 || in->n_retire < 0) return OVP_E_ARG;
  if (!c->have_cov) return OVP_E_STATE;
  const int n = c->n, np = in->n_pairs, npl = in->n_planes, nr = in->n_retire;
  // ---- every check before anything is touched or enqueued ----
  if (np > RT_MAX_PAIRS || npl > RT_MAX_PLANES) return OVP_E_CAPACITY;
  if (np > 0 && (!in->new_col || !in->old_col || !in->plane_col || !in->cp || !accepted || !chi2 || !angle_deg || !dx || dx_stride < n))
    return OVP_E_ARG;
  if (npl > 0 && (!in->plane_col || !in->cp)) return OVP_E_ARG;
  if (nr > 0 && (!in->retire_ids || !in->retire_sizes)) return OVP_E_ARG;
  if (np > 0 && !(in->sigma_plane_merge > 0.0)) return OVP_E_ARG;
  std::vector<int2> rg;
  int gone = 0;
  if (nr > 0)
    if (const int rc = sorted_ranges(n, nr, in->retire_ids, in->retire_sizes, rg, &gone)) return rc;
  for (int p = 0; p < npl; ++p) {
    if (in->plane_col[p] < 0 || in->plane_col[p] > n - 3) return OVP_E_ARG;
    for (int q = 0; q < p; ++q)
      if (in->plane_col[q] == in->plane_col[p]) return OVP_E_ARG;
  }
  std::vector<int> pair(4 * (size_t)np);
  for (int k = 0; k < np; ++k) {
    const int cn = in->new_col[k], co = in->old_col[k];
    if (cn < 0 || cn > n - 3 || co < 0 || co > n - 3 || abs(cn - co) < 3) return OVP_E_ARG;
    int sn = -1, so = -1;
    for (int p = 0; p < npl; ++p) {
      if (in->plane_col[p] == cn) sn = p;
      if (in->plane_col[p] == co) so = p;
    }
    if (sn < 0 || so < 0) return OVP_E_ARG;
    bool leaves = false;  // the old plane's three columns are inside one retired range
    for (const int2& g : rg) leaves = leaves || (g.x <= co && co + 3 <= g.x + g.y);
    if (!leaves) return OVP_E_ARG;
    for (int q = 0; q < k; ++q)  // a plane that was fused away takes part in no later pair
      if (in->old_col[q] == cn || in->old_col[q] == co) return OVP_E_ARG;
    pair[k] = cn, pair[np + k] = co, pair[2 * (size_t)np + k] = sn, pair[3 * (size_t)np + k] = so;
  }
  if (np == 0 && nr == 0) return 0;
  const int n_out = n - gone;
  if (compact_lds(nr, n_out) > RT_LDS_CAP || sizeof(double) * 4 * (size_t)n > RT_LDS_CAP) return OVP_E_CAPACITY;
  // ---- from here on the call goes through ----
  drop_kept_factor(c);  // (writes the covariance: a kept factor no longer belongs to it; a refused or empty call keeps it)
  HIPCHK(hipSetDevice(c->device));
  Retire* d = nullptr;
  if (const int rc = retire_of(c, &d)) return rc;
  StageLayout lay;
  const size_t o_rg = lay.take(sizeof(int2) * nr), o_pair = lay.take(sizeof(int) * 4 * np), o_col = lay.take(sizeof(int) * npl),
               o_cp = lay.take(sizeof(double) * 3 * npl);
  int rc = 0;
  char* h = d->stage.begin(lay.bytes(), &rc);  // (above the capacity: cannot happen below the limits above)
  if (!h) return rc;
  char* dv = d->stage.dev();
  hipStream_t s = c->stream;
  if (nr > 0) memcpy(h + o_rg, rg.data(), sizeof(int2) * nr);
  if (np > 0) memcpy(h + o_pair, pair.data(), sizeof(int) * 4 * np);
  if (npl > 0) {
    memcpy(h + o_col, in->plane_col, sizeof(int) * npl);
    memcpy(h + o_cp, in->cp, sizeof(double) * 3 * npl);
  }
  // (nothing to report: the compaction alone does not wait, as ovp_cov_marginalize_many leaves it)
  HIPCHK(d->stage.send(lay.bytes(), s, np == 0 ? Fence::Event : Fence::CallerWaits));
  MergeJob j;
  j.P = c->P, j.ld = c->ld, j.n = n, j.np = np, j.n_planes = npl, j.stride = d->stride;
  j.pair = (const int*)(dv + o_pair), j.plane_col = (const int*)(dv + o_col), j.cp = (double*)(dv + o_cp);
  j.white_c = np > 0 ? 1.0 / in->sigma_plane_merge : 0.0;
  j.chi2_thr = in->plane_merge_chi2 * ovp_chi2_quantile_095(3);
  j.deg_max = in->plane_merge_deg_max;
  j.W = d->W, j.res = d->dres;
  for (int k = 0; k < np; ++k) {
    hipLaunchKernelGGL(k_plane_merge_gate, dim3(1), dim3(256), sizeof(double) * 4 * (size_t)n, s, j, k);
    hipLaunchKernelGGL(k_plane_merge_apply, dim3((n + 63) / 64, (n + 3) / 4), dim3(256), 0, s, j.P, j.ld, n, j.W,
                       j.res + (size_t)k * j.stride);
  }
  HIPCHK(hipGetLastError());
  if (nr > 0) HIPCHK(launch_compact(c->P, c->P_tmp, c->ld, n_out, (const int2*)(dv + o_rg), nr, s));
  // everything is enqueued: the compacted matrix is the covariance from here on, whatever the wait below returns (the merges
  // have rewritten the other buffer in place, so there is no way back to the state before the call)
  if (nr > 0) {
    c->P.swap(c->P_tmp);
    c->n = n_out;
  }
  if (np > 0) {
    SeqChannel& ch = d->hres.channel(0);
    const unsigned seq = ch.arm();
    HIPCHK(ovp_launch_publish_block(d->dres.get(), d->hres.dev(d->hres.payload()), sizeof(double) * (size_t)np * d->stride, ch.word_dev(),
                                    seq, 0, s));
    const int rw = ch.wait(s);
    if (rw) return rw;
    d->stage.done();
  }
  bool neg = false;
  const double* hr = (const double*)d->hres.payload();
  for (int k = 0; k < np; ++k) {
    const double* r = hr + (size_t)k * d->stride;
    accepted[k] = r[0] != 0.0 ? 1 : 0;
    chi2[k] = r[1];
    angle_deg[k] = r[2];
    neg = neg || r[3] != 0.0;
    memcpy(dx + (size_t)k * dx_stride, r + 4, sizeof(double) * n);
  }
  return neg ? OVP_E_NEGDIAG : 0;
}
