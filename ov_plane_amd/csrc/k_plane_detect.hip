// Plane detection from a frame's tracked features: TrackPlane::perform_plane_detection_monocular (track_plane/TrackPlane.cpp:
// 580-1121) restated.  The data-parallel pieces are the kernels below; the greedy merge and the pruning are sequential by
// definition and stay on the host, in the entry points at the end of this file.  The Delaunay triangulation runs on the host
// (host/ov_plane_delaunay.h) or, with ovp_plane_detector_set_device_delaunay, on the device behind k_det_triangulate
// (k_det_delaunay, k_delaunay.hip: the same algorithm, the same triangles).
//   k_det_triangulate     one thread per tracked point: accumulate the linear triangulation system, solve and gate it (:632-681)
//   k_det_tri_normals     one thread per triangle: side test, unit normal, sign towards the camera (:733-776)
//   k_det_vertex_norms    one thread per vertex: its triangles' normals into its history, in triangle order, and avg_norm (:778-806,
//                         :1123-1171)
//   k_det_match           one thread per directed neighbour edge: the validity tests and the three predicates (:850-886)
//   k_det_spatial_filter  one workgroup per plane: k nearest squared f32 distances by brute force, z-test (:1003-1058)
// The result block of each stage goes to the host through the detector's Mailbox (ovp_mailbox.h, k_publish.hip).
// No atomics, every order fixed: two runs give the same bits.
#include "ovp_ctx.h"
#include "host/ov_plane_delaunay.h"
#include "k_delaunay.h"
#include "k_tri3.h"

#include <map>
#include <set>

namespace {

struct DetState {  // per feature slot
  double *A, *b, *p;  // [S*6] upper triangle of the system matrix (00 01 02 11 12 22), [S*3] its right side, [S*3] p_FinG
  int *count, *valid;  // observations, p_FinG holds an estimate
  double *ring, *avg;  // [S*OVP_DET_MAX_NORMS*3] the last normals, oldest first; [S*3] avg_norm of them
  int* ring_n;
};

constexpr double kRad2Deg = 180.0 / 3.14159265358979323846;

__global__ __launch_bounds__(256) void k_det_triangulate(DetState st, int n, const int* __restrict__ slot,
                                                         const unsigned char* __restrict__ fresh, const double* __restrict__ uvn,
                                                         const double* __restrict__ pose, int min_obs, double max_cond,
                                                         double min_dist, double max_dist, double* __restrict__ out_p,
                                                         int* __restrict__ out_flag) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int s = slot[i];
  double R[9], pc[3];
  for (int k = 0; k < 9; ++k) R[k] = pose[k];
  for (int k = 0; k < 3; ++k) pc[k] = pose[9 + k];
  double A[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0};
  int cnt = 0, valid = 0;
  if (!fresh[i]) {
    for (int k = 0; k < 6; ++k) A[k] = st.A[s * 6 + k];
    for (int k = 0; k < 3; ++k) b[k] = st.b[s * 3 + k];
    cnt = st.count[s];
    valid = st.valid[s];
  } else {
    st.ring_n[s] = 0;
    for (int k = 0; k < 3; ++k) st.avg[s * 3 + k] = 0.0;
  }
  // bearing in G, A_i = skew(b)^T skew(b), b_i = A_i p_CiinG
  const double x = uvn[2 * i], y = uvn[2 * i + 1];
  double bx = R[0] * x + R[3] * y + R[6], by = R[1] * x + R[4] * y + R[7], bz = R[2] * x + R[5] * y + R[8];
  const double bn = sqrt(bx * bx + by * by + bz * bz);
  bx /= bn, by /= bn, bz /= bn;
  const double Ai[6] = {bz * bz + by * by, -bx * by, -bx * bz, bz * bz + bx * bx, -by * bz, by * by + bx * bx};
  for (int k = 0; k < 6; ++k) A[k] += Ai[k];
  b[0] += Ai[0] * pc[0] + Ai[1] * pc[1] + Ai[2] * pc[2];
  b[1] += Ai[1] * pc[0] + Ai[3] * pc[1] + Ai[4] * pc[2];
  b[2] += Ai[2] * pc[0] + Ai[4] * pc[1] + Ai[5] * pc[2];
  cnt += 1;
  for (int k = 0; k < 6; ++k) st.A[s * 6 + k] = A[k];
  for (int k = 0; k < 3; ++k) st.b[s * 3 + k] = b[k];
  st.count[s] = cnt;
  int accepted = 0;
  double p[3] = {0, 0, 0};
  if (valid)
    for (int k = 0; k < 3; ++k) p[k] = st.p[s * 3 + k];
  if (cnt >= min_obs) {
    // A x = b by row-pivoted elimination, the condition number from the eigenvalues of the symmetric A (k_tri3.h)
    double q[3];
    ovp_tri3_solve(A, b, q);
    const double cond = ovp_tri3_cond(A);
    const double d0 = q[0] - pc[0], d1 = q[1] - pc[1], d2 = q[2] - pc[2];
    const double cx = R[0] * d0 + R[1] * d1 + R[2] * d2, cy = R[3] * d0 + R[4] * d1 + R[5] * d2, cz = R[6] * d0 + R[7] * d1 + R[8] * d2;
    const double nrm = sqrt(cx * cx + cy * cy + cz * cz);
    if (fabs(cond) <= max_cond && cz >= min_dist && cz <= max_dist && !isnan(nrm)) {
      accepted = 1;
      valid = 1;
      for (int k = 0; k < 3; ++k) p[k] = q[k], st.p[s * 3 + k] = q[k];
    }
  }
  st.valid[s] = valid;
  for (int k = 0; k < 3; ++k) out_p[3 * i + k] = p[k];
  out_flag[i] = valid | (accepted << 1) | (cnt << 8);
}

__global__ __launch_bounds__(256) void k_det_tri_normals(int nt, const int* __restrict__ tris, const int* __restrict__ vslot,
                                                         const float* __restrict__ vpx, const double* __restrict__ P,
                                                         const double* __restrict__ pose, double max_side,
                                                         double* __restrict__ tri_n, unsigned char* __restrict__ tri_ok) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= nt) return;
  const int v0 = tris[3 * t], v1 = tris[3 * t + 1], v2 = tris[3 * t + 2];
  // cv::norm of a Point2f difference: the difference in f32, the length in f64
  const float x0 = vpx[2 * v0], y0 = vpx[2 * v0 + 1], x1 = vpx[2 * v1], y1 = vpx[2 * v1 + 1], x2 = vpx[2 * v2], y2 = vpx[2 * v2 + 1];
  const double ax = (double)(x0 - x1), ay = (double)(y0 - y1), bx = (double)(x1 - x2), by = (double)(y1 - y2), cx = (double)(x2 - x0),
               cy = (double)(y2 - y0);
  const double l01 = sqrt(ax * ax + ay * ay), l12 = sqrt(bx * bx + by * by), l20 = sqrt(cx * cx + cy * cy);
  double nx = 0.0, ny = 0.0, nz = 0.0;
  const bool ok = !(l01 > max_side || l12 > max_side || l20 > max_side);
  if (ok) {
    const double* p1 = P + 3 * vslot[v0];
    const double* p2 = P + 3 * vslot[v1];
    const double* p3 = P + 3 * vslot[v2];
    double d1x = p2[0] - p1[0], d1y = p2[1] - p1[1], d1z = p2[2] - p1[2];
    const double n1 = sqrt(d1x * d1x + d1y * d1y + d1z * d1z);
    d1x /= n1, d1y /= n1, d1z /= n1;
    double d2x = p3[0] - p1[0], d2y = p3[1] - p1[1], d2z = p3[2] - p1[2];
    const double n2 = sqrt(d2x * d2x + d2y * d2y + d2z * d2z);
    d2x /= n2, d2y /= n2, d2z /= n2;
    nx = d1y * d2z - d1z * d2y, ny = d1z * d2x - d1x * d2z, nz = d1x * d2y - d1y * d2x;
    const double nn = sqrt(nx * nx + ny * ny + nz * nz);
    nx /= nn, ny /= nn, nz /= nn;
    // seen from the camera the plane lies at a positive distance
    const double fx = p1[0] - pose[9], fy = p1[1] - pose[10], fz = p1[2] - pose[11];
    double dot = 0.0;
    for (int r = 0; r < 3; ++r) {
      const double fc = pose[3 * r] * fx + pose[3 * r + 1] * fy + pose[3 * r + 2] * fz;
      const double nc = pose[3 * r] * nx + pose[3 * r + 1] * ny + pose[3 * r + 2] * nz;
      dot += nc * fc;
    }
    if (dot < 0.0) nx *= -1.0, ny *= -1.0, nz *= -1.0;
  }
  tri_n[3 * t] = nx, tri_n[3 * t + 1] = ny, tri_n[3 * t + 2] = nz;
  tri_ok[t] = ok ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_det_vertex_norms(int nv, const int* __restrict__ vslot, const int* __restrict__ vt_ptr,
                                                          const int* __restrict__ vt_idx, const double* __restrict__ tri_n,
                                                          const unsigned char* __restrict__ tri_ok, DetState st, int max_count,
                                                          double avg_max, double avg_var) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= nv) return;
  const int s = vslot[v];
  double* ring = st.ring + (size_t)s * OVP_DET_MAX_NORMS * 3;
  int cnt = st.ring_n[s];
  for (int e = vt_ptr[v]; e < vt_ptr[v + 1]; ++e) {
    const int t = vt_idx[e];
    if (!tri_ok[t]) continue;
    if (cnt == max_count) {  // the oldest goes
      for (int k = 0; k < 3 * (max_count - 1); ++k) ring[k] = ring[k + 3];
      cnt -= 1;
    }
    for (int k = 0; k < 3; ++k) ring[3 * cnt + k] = tri_n[3 * t + k];
    cnt += 1;
  }
  st.ring_n[s] = cnt;
  // avg_norm
  int count = 0;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int k = 0; k < cnt; ++k) {
    const double x = ring[3 * k], y = ring[3 * k + 1], z = ring[3 * k + 2];
    if (sqrt(x * x + y * y + z * z) <= 0.0) continue;
    sx += x, sy += y, sz += z;
    count++;
  }
  const double sn = sqrt(sx * sx + sy * sy + sz * sz);
  sx /= sn, sy /= sn, sz /= sn;
  bool zero = cnt == 0 || count < 2;
  if (!zero) {
    double max_deg = 0.0, var_deg = 0.0;
    for (int k = 0; k < cnt; ++k) {
      const double x = ring[3 * k], y = ring[3 * k + 1], z = ring[3 * k + 2];
      if (sqrt(x * x + y * y + z * z) <= 0.0) continue;
      const double d = kRad2Deg * acos(x * sx + y * sy + z * sz);
      var_deg += d * d;
      max_deg = (max_deg < d) ? d : max_deg;  // std::max: a NaN leaves it
    }
    var_deg /= (double)(count - 1);
    zero = sqrt(var_deg) > avg_var || max_deg > avg_max;
  }
  st.avg[3 * s] = zero ? 0.0 : sx, st.avg[3 * s + 1] = zero ? 0.0 : sy, st.avg[3 * s + 2] = zero ? 0.0 : sz;
}

__global__ __launch_bounds__(256) void k_det_match(int ne, const int* __restrict__ e_src, const int* __restrict__ e_dst,
                                                   const int* __restrict__ vslot, const float* __restrict__ vpx, DetState st,
                                                   int min_norms, double max_px, double max_deg, double max_z,
                                                   unsigned char* __restrict__ match) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= ne) return;
  const int v = e_src[e], w = e_dst[e], s = vslot[v], s2 = vslot[w];
  const double nx = st.avg[3 * s], ny = st.avg[3 * s + 1], nz = st.avg[3 * s + 2];
  const double mx = st.avg[3 * s2], my = st.avg[3 * s2 + 1], mz = st.avg[3 * s2 + 2];
  bool ok = st.ring_n[s] >= min_norms && !(sqrt(nx * nx + ny * ny + nz * nz) <= 0.0);
  ok = ok && st.ring_n[s2] >= min_norms && !(sqrt(mx * mx + my * my + mz * mz) <= 0.0);
  const double dx = (double)(vpx[2 * v] - vpx[2 * w]), dy = (double)(vpx[2 * v + 1] - vpx[2 * w + 1]);
  ok = ok && !(sqrt(dx * dx + dy * dy) > max_px);
  const double* p = st.p + 3 * s;
  const double* p2 = st.p + 3 * s2;
  const double d = p[0] * nx + p[1] * ny + p[2] * nz;
  const double plane_dist = (p2[0] * nx + p2[1] * ny + p2[2] * nz) - d;
  const double angle = kRad2Deg * acos(nx * mx + ny * my + nz * mz);
  ok = ok && !isnan(angle) && angle < max_deg && fabs(plane_dist) < max_z;
  match[e] = ok ? 1 : 0;
}

// KD_TREE::calc_dist: squared, in f32, each product and sum rounded on its own
__device__ __forceinline__ float det_dist2(float ax, float ay, float az, float bx, float by, float bz) {
#pragma clang fp contract(off)
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
  const float xy = xx + yy;
  return xy + zz;
}

__global__ __launch_bounds__(256) void k_det_spatial_filter(const int* __restrict__ pl_ptr, const int* __restrict__ pl_slot,
                                                            const double* __restrict__ P, int kn, double z_thresh,
                                                            double* __restrict__ out_d, unsigned char* __restrict__ out_flag) {
  __shared__ float pts[OVP_DET_MAX_POINTS * 3];
  __shared__ double dv[OVP_DET_MAX_POINTS];
  __shared__ double red[256];
  const int t = threadIdx.x, lo = pl_ptr[blockIdx.x], n = pl_ptr[blockIdx.x + 1] - lo;  // kn < n <= OVP_DET_MAX_POINTS (host)
  for (int i = t; i < n; i += 256) {
    const double* p = P + 3 * pl_slot[lo + i];
    pts[3 * i] = (float)p[0], pts[3 * i + 1] = (float)p[1], pts[3 * i + 2] = (float)p[2];
  }
  __syncthreads();
  double part = 0.0;
  for (int i = t; i < n; i += 256) {
    float best[OVP_DET_MAX_FILTER_K];
#pragma unroll
    for (int q = 0; q < OVP_DET_MAX_FILTER_K; ++q) best[q] = INFINITY;
    const float ax = pts[3 * i], ay = pts[3 * i + 1], az = pts[3 * i + 2];
    for (int j = 0; j < n; ++j) {
      if (j == i) continue;
      float d = det_dist2(ax, ay, az, pts[3 * j], pts[3 * j + 1], pts[3 * j + 2]);
#pragma unroll
      for (int q = 0; q < OVP_DET_MAX_FILTER_K; ++q)  // sorted insertion into the kn smallest
        if (q < kn && d < best[q]) {
          const float tmp = best[q];
          best[q] = d;
          d = tmp;
        }
    }
    double sum = 0.0;
#pragma unroll
    for (int q = 0; q < OVP_DET_MAX_FILTER_K; ++q)
      if (q < kn) sum += (double)best[q];
    const double m = sum / (double)kn;
    dv[i] = m;
    part += m;
  }
  // mean and sample deviation: per-thread partial sums in index order, then a fixed tree
  red[t] = part;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) red[t] += red[t + w];
    __syncthreads();
  }
  const double mean = red[0] / (double)n;
  __syncthreads();
  part = 0.0;
  for (int i = t; i < n; i += 256) part += (dv[i] - mean) * (dv[i] - mean);
  red[t] = part;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) red[t] += red[t + w];
    __syncthreads();
  }
  const double sd = sqrt(red[0] / ((double)n - 1.0));
  for (int i = t; i < n; i += 256) {
    out_d[lo + i] = dv[i];
    out_flag[lo + i] = (fabs(dv[i] - mean) / sd > z_thresh) ? 1 : 0;
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
constexpr int S = OVP_DET_MAX_POINTS;          // feature slots: a feature not in the frame gives its slot back, so a frame's points fit
constexpr int MAX_TRIS = 2 * S, MAX_EDGES = 6 * MAX_TRIS;

struct Detector {
  ovp_trackplane_opts o;
  DevBuf<double> A, b, p, ring, avg;
  DevBuf<int> count, valid, ring_n;
  Staged stage;  // the tables of a stage
  Mailbox hres;  // the results of a stage: payload from byte 0, channel 0
  DevBuf<void> dres;
  size_t res_cap = 0;
  OvpEvent ev[8];
  float ms[4] = {0, 0, 0, 0};
  float ms_delaunay[2] = {0, 0};  // k_det_delaunay of the last timed frame / of the last timed ovp_delaunay_device
  bool timed = false;  // ovp_plane_detector_debug "timer": events around the kernels, read behind a stream synchronisation
  // host state of TrackPlane
  std::map<int64_t, int> slot_of;
  std::set<int> free_slots;
  std::map<int64_t, int64_t> feat2plane;
  std::map<int64_t, std::set<int64_t>> plane2old;
  int64_t currplaneid = 0;
  // the frame between its two calls
  bool have_frame = false;
  std::vector<int64_t> v_id;  // vertices: the frame's points that have an estimate, in point order
  std::vector<int> v_slot;
  std::vector<float> v_px;
  double pose[12];
  std::vector<double> filt_dbg;
  // ovp_plane_detector_set_device_delaunay: the frame's triangles as the first call's kernel left them
  bool dev_delaunay = false, dev_tris_ok = false;
  std::vector<int> dev_tris;
  int dev_hdr[OVP_DL_HDR] = {};
  int tri_source = 0;  // of the last ovp_plane_detect_planes: 0 the caller's, 1 ovp_delaunay_host, 2 the device's
  DetState st() const { return DetState{A.get(), b.get(), p.get(), count.get(), valid.get(), ring.get(), avg.get(), ring_n.get()}; }
  void forget() {
    slot_of.clear();
    free_slots.clear();
    for (int s = 0; s < S; ++s) free_slots.insert(s);
    feat2plane.clear();
    plane2old.clear();
    currplaneid = 0;
    have_frame = false;
    dev_tris_ok = false;
    v_id.clear(), v_slot.clear(), v_px.clear(), filt_dbg.clear();
  }
};

// ovp_delaunay_device: staging, result block and mailbox of its own (a context without a detector has none), made on first use
struct DelaunayIo {
  Staged stage;
  DevBuf<void> dres;
  Mailbox hres;
  OvpEvent ev[2];
};

Detector* det_of(ovp_ctx* c) { return c ? (Detector*)c->plane_det.get() : nullptr; }

// device result block -> pinned, waited for: the stage's tables have been read by then
int publish_and_wait(ovp_ctx* c, Detector* d, size_t bytes) {
  SeqChannel& ch = d->hres.channel(0);
  const unsigned seq = ch.arm();
  HIPCHK(ovp_launch_publish_block(d->dres.get(), d->hres.dev(d->hres.payload()), bytes, ch.word_dev(), seq, 0, c->stream));
  const int rw = ch.wait(c->stream);
  if (!rw) d->stage.done();
  return rw;
}

}  // namespace

extern "C" void ovp_trackplane_defaults(ovp_trackplane_opts* o) {
  if (!o) return;
  o->max_tri_side_px = 200, o->max_norm_count = 5, o->max_norm_avg_max = 25.0, o->max_norm_avg_var = 25.0, o->max_norm_deg = 25.0;
  o->max_dist_between_z = 0.10, o->max_pairwise_px = 100, o->min_norms = 3, o->check_old_feats = 1, o->filter_num_feat = 4;
  o->filter_z_thresh = 1.2, o->feat_init_min_obs = 4, o->min_dist = 0.10, o->max_dist = 60, o->max_cond_number = 8000;
}

extern "C" int ovp_plane_detector_create(ovp_ctx* c, const ovp_trackplane_opts* opts) {
  if (!c || !opts) return OVP_E_ARG;
  if (opts->max_norm_count < 1 || opts->max_norm_count > OVP_DET_MAX_NORMS || opts->filter_num_feat < 2 ||
      opts->filter_num_feat > OVP_DET_MAX_FILTER_K || opts->feat_init_min_obs < 1)
    return OVP_E_ARG;
  HIPCHK(hipSetDevice(c->device));
  auto d = std::make_shared<Detector>();
  d->o = *opts;
  HIPCHK(d->A.alloc((size_t)S * 6));
  HIPCHK(d->b.alloc((size_t)S * 3));
  HIPCHK(d->p.alloc((size_t)S * 3));
  HIPCHK(d->ring.alloc((size_t)S * OVP_DET_MAX_NORMS * 3));
  HIPCHK(d->avg.alloc((size_t)S * 3));
  HIPCHK(d->count.alloc(S));
  HIPCHK(d->valid.alloc(S));
  HIPCHK(d->ring_n.alloc(S));
  // the largest of the three staged tables / result blocks (second call: triangles, two CSR lists, edge ends)
  // (and the first call's with the device triangulation: the pixel positions in, the header and the triangles out)
  HIPCHK(d->stage.alloc(64 * 16 + sizeof(int) * ((size_t)S * 4 + 3 * MAX_TRIS * 2 + 2 * MAX_EDGES + 2 * (S + 1)) +
                        sizeof(double) * (2 * S + 12) + sizeof(float) * 2 * S));
  d->res_cap = 64 * 8 + sizeof(double) * 3 * MAX_TRIS + MAX_TRIS + MAX_EDGES + sizeof(double) * 3 * S + sizeof(int) * S +
               sizeof(int) * (OVP_DL_HDR + 3 * MAX_TRIS);
  HIPCHK(d->dres.alloc(d->res_cap));
  HIPCHK(d->hres.alloc(d->res_cap));
  for (OvpEvent& e : d->ev) HIPCHK(e.create());
  HIPCHK(hipMemsetAsync(d->valid.get(), 0, sizeof(int) * S, c->stream));
  HIPCHK(hipMemsetAsync(d->ring_n.get(), 0, sizeof(int) * S, c->stream));
  HIPCHK(hipMemsetAsync(d->avg.get(), 0, sizeof(double) * 3 * S, c->stream));
  HIPCHK(hipMemsetAsync(d->p.get(), 0, sizeof(double) * 3 * S, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  d->forget();
  c->plane_det = d;
  return 0;
}

extern "C" int ovp_plane_detector_destroy(ovp_ctx* c) {
  if (!c) return OVP_E_ARG;
  if (!c->plane_det) return OVP_E_STATE;
  HIPCHK(hipStreamSynchronize(c->stream));
  c->plane_det.reset();
  return 0;
}

extern "C" int ovp_plane_detector_reset(ovp_ctx* c) {
  Detector* d = det_of(c);
  if (!d) return c ? OVP_E_STATE : OVP_E_ARG;
  d->forget();  // (a slot's device state is cleared when a feature takes it)
  return 0;
}

extern "C" int ovp_plane_detect_triangulate(ovp_ctx* c, int n, const int64_t* ids, const float* uv, const double* uv_norm,
                                            const double* R_GtoC, const double* p_CinG, uint8_t* has_est, double* p_FinG) {
  Detector* d = det_of(c);
  if (!d) return c ? OVP_E_STATE : OVP_E_ARG;
  if (n < 0) return OVP_E_ARG;
  if (n > OVP_DET_MAX_POINTS) return OVP_E_CAPACITY;
  if (n == 0) {  // (TrackPlane.cpp:600-601: nothing happens, and there is no frame for ovp_plane_detect_planes)
    d->have_frame = false;
    return 0;
  }
  if (!ids || !uv || !uv_norm || !R_GtoC || !p_CinG) return OVP_E_ARG;
  const std::set<int64_t> now(ids, ids + n);
  if ((int)now.size() != n) return OVP_E_ARG;  // two points of one feature would share a slot
  HIPCHK(hipSetDevice(c->device));
  d->have_frame = false;
  d->dev_tris_ok = false;
  // remove_feats: a feature not seen in this frame gives its slot back
  {
    for (auto it = d->slot_of.begin(); it != d->slot_of.end();)
      if (!now.count(it->first)) {
        d->free_slots.insert(it->second);
        it = d->slot_of.erase(it);
      } else
        ++it;
  }
  StageLayout L;
  const size_t o_slot = L.take(sizeof(int) * n), o_fresh = L.take(n), o_uvn = L.take(sizeof(double) * 2 * n), o_pose = L.take(sizeof(double) * 12);
  StageLayout Rl;
  const size_t r_p = Rl.take(sizeof(double) * 3 * n), r_flag = Rl.take(sizeof(int) * n);
  // device triangulation: the pixel positions behind the rest, the header and the triangles behind the flags - same block, same wait
  const bool dl = d->dev_delaunay;
  const int dl_cap = 2 * n;
  const size_t o_uv = dl ? L.take(sizeof(float) * 2 * n) : 0, r_dhdr = dl ? Rl.take(sizeof(int) * OVP_DL_HDR) : 0,
               r_dtri = dl ? Rl.take(sizeof(int) * 3 * dl_cap) : 0;
  if (Rl.bytes() > d->res_cap) return OVP_E_CAPACITY;
  int rc = 0;
  char* h = d->stage.begin(L.bytes(), &rc);
  if (!h) return rc;
  int* h_slot = (int*)(h + o_slot);
  for (int i = 0; i < n; ++i) {
    auto it = d->slot_of.find(ids[i]);
    if (it == d->slot_of.end()) {
      const int s = *d->free_slots.begin();  // (never empty: at most n <= S slots are held by this frame's features)
      d->free_slots.erase(d->free_slots.begin());
      it = d->slot_of.emplace(ids[i], s).first;
      h[o_fresh + i] = 1;
    } else
      h[o_fresh + i] = 0;
    h_slot[i] = it->second;
  }
  memcpy(h + o_uvn, uv_norm, sizeof(double) * 2 * n);
  memcpy(h + o_pose, R_GtoC, sizeof(double) * 9);
  memcpy(h + o_pose + sizeof(double) * 9, p_CinG, sizeof(double) * 3);
  memcpy(d->pose, h + o_pose, sizeof(double) * 12);
  if (dl) memcpy(h + o_uv, uv, sizeof(float) * 2 * n);
  const char* dv = d->stage.dev();
  char* dr = (char*)d->dres.get();
  HIPCHK(d->stage.send(L.bytes(), c->stream, Fence::CallerWaits));
  if (d->timed) HIPCHK(hipEventRecord(d->ev[0], c->stream));
  hipLaunchKernelGGL(k_det_triangulate, dim3((n + 255) / 256), dim3(256), 0, c->stream, d->st(), n, (const int*)(dv + o_slot),
                     (const unsigned char*)(dv + o_fresh), (const double*)(dv + o_uvn), (const double*)(dv + o_pose),
                     d->o.feat_init_min_obs, d->o.max_cond_number, d->o.min_dist, d->o.max_dist, (double*)(dr + r_p), (int*)(dr + r_flag));
  HIPCHK(hipGetLastError());
  if (d->timed) HIPCHK(hipEventRecord(d->ev[1], c->stream));
  if (dl) {  // the vertices are the points whose flag bit 0 the kernel above has just set, in point order
    HIPCHK(ovp_launch_delaunay(n, (const float*)(dv + o_uv), (const int*)(dr + r_flag), (int*)(dr + r_dhdr), (int*)(dr + r_dtri), dl_cap,
                               c->stream));
    if (d->timed) HIPCHK(hipEventRecord(d->ev[7], c->stream));
  }
  const int rw = publish_and_wait(c, d, Rl.bytes());
  if (rw) return rw;
  d->ms[0] = d->ms[1] = d->ms[2] = d->ms[3] = 0.f;
  d->ms_delaunay[0] = 0.f;
  if (d->timed) {
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipEventElapsedTime(&d->ms[0], d->ev[0], d->ev[1]));
    if (dl) HIPCHK(hipEventElapsedTime(&d->ms_delaunay[0], d->ev[1], d->ev[7]));
  }
  const char* hr = (const char*)d->hres.payload();
  const double* rp = (const double*)(hr + r_p);
  const int* rf = (const int*)(hr + r_flag);
  d->v_id.clear(), d->v_slot.clear(), d->v_px.clear();
  for (int i = 0; i < n; ++i) {
    const bool est = rf[i] & 1;
    if (has_est) has_est[i] = (uint8_t)(rf[i] & 3);
    if (p_FinG)
      for (int k = 0; k < 3; ++k) p_FinG[3 * i + k] = rp[3 * i + k];
    if (est) {
      d->v_id.push_back(ids[i]);
      d->v_slot.push_back(h_slot[i]);
      d->v_px.push_back(uv[2 * i]);
      d->v_px.push_back(uv[2 * i + 1]);
    }
  }
  if (dl) {  // (an overflow - inconsistent predicate signs - leaves the frame to ovp_delaunay_host)
    const int* hd = (const int*)(hr + r_dhdr);
    memcpy(d->dev_hdr, hd, sizeof(d->dev_hdr));
    const int nt = hd[0];
    d->dev_tris_ok = !hd[1] && hd[2] == (int)d->v_id.size() && nt >= 0 && nt <= dl_cap;
    if (d->dev_tris_ok) d->dev_tris.assign((const int*)(hr + r_dtri), (const int*)(hr + r_dtri) + 3 * (size_t)nt);
  }
  d->have_frame = true;
  return 0;
}

extern "C" int ovp_delaunay(int n, const float* xy, int32_t* tris, int cap, int* n_tris) {
  if (n < 0 || (n > 0 && !xy) || !n_tris || cap < 0 || (cap > 0 && !tris)) return OVP_E_ARG;
  std::vector<std::array<int, 3>> out;
  ovp_delaunay_host(n, xy, out);
  *n_tris = (int)out.size();
  if ((int)out.size() > cap) return OVP_E_CAPACITY;
  for (size_t t = 0; t < out.size(); ++t)
    for (int k = 0; k < 3; ++k) tris[3 * t + k] = out[t][k];
  return 0;
}

extern "C" int ovp_plane_detector_set_device_delaunay(ovp_ctx* c, int on) {
  Detector* d = det_of(c);
  if (!d) return c ? OVP_E_STATE : OVP_E_ARG;
  d->dev_delaunay = on != 0;
  d->dev_tris_ok = false;  // (a frame between its two calls keeps the route it was staged for: the host's)
  return 0;
}

// ovp_delaunay on the device: one upload, one launch, one publication.  No fallback: an overflow of the kernel's table is
// OVP_E_CAPACITY, so a caller can tell this result from the host's.
extern "C" int ovp_delaunay_device(ovp_ctx* c, int n, const float* xy, int32_t* tris, int cap, int* n_tris) {
  if (!c || n < 0 || (n > 0 && !xy) || !n_tris || cap < 0 || (cap > 0 && !tris)) return OVP_E_ARG;
  if (n > OVP_DET_MAX_POINTS) return OVP_E_CAPACITY;
  *n_tris = 0;
  if (n < 3) return 0;
  HIPCHK(hipSetDevice(c->device));
  if (!c->delaunay_io) {
    auto io = std::make_shared<DelaunayIo>();
    const size_t res = sizeof(int) * (OVP_DL_HDR + 3 * (size_t)MAX_TRIS);
    HIPCHK(io->stage.alloc(sizeof(float) * 2 * S));
    HIPCHK(io->dres.alloc(res));
    HIPCHK(io->hres.alloc(res));
    for (OvpEvent& e : io->ev) HIPCHK(e.create());
    c->delaunay_io = io;
  }
  DelaunayIo* io = (DelaunayIo*)c->delaunay_io.get();
  Detector* d = det_of(c);
  const bool timed = d && d->timed;
  const int dl_cap = 2 * n;
  int* dhdr = (int*)io->dres.get();
  int rc = 0;
  char* h = io->stage.begin(sizeof(float) * 2 * n, &rc);
  if (!h) return rc;
  memcpy(h, xy, sizeof(float) * 2 * n);
  HIPCHK(io->stage.send(sizeof(float) * 2 * n, c->stream, Fence::CallerWaits));
  if (timed) HIPCHK(hipEventRecord(io->ev[0], c->stream));
  HIPCHK(ovp_launch_delaunay(n, (const float*)io->stage.dev(), nullptr, dhdr, dhdr + OVP_DL_HDR, dl_cap, c->stream));
  if (timed) HIPCHK(hipEventRecord(io->ev[1], c->stream));
  SeqChannel& ch = io->hres.channel(0);
  const unsigned seq = ch.arm();
  HIPCHK(ovp_launch_publish_block(dhdr, io->hres.dev(io->hres.payload()), sizeof(int) * (OVP_DL_HDR + 3 * (size_t)dl_cap), ch.word_dev(), seq,
                                  0, c->stream));
  const int rw = ch.wait(c->stream);
  if (rw) return rw;
  io->stage.done();
  if (timed) {
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipEventElapsedTime(&d->ms_delaunay[1], io->ev[0], io->ev[1]));
  }
  const int* hd = (const int*)io->hres.payload();
  if (hd[1] || hd[0] < 0 || hd[0] > dl_cap) return OVP_E_CAPACITY;
  *n_tris = hd[0];
  if (hd[0] > cap) return OVP_E_CAPACITY;
  memcpy(tris, hd + OVP_DL_HDR, sizeof(int32_t) * 3 * (size_t)hd[0]);
  return 0;
}

extern "C" int ovp_plane_detect_planes(ovp_ctx* c, int n_tris, const int32_t* tris_in) {
  Detector* d = det_of(c);
  if (!d) return c ? OVP_E_STATE : OVP_E_ARG;
  if (!d->have_frame) return OVP_E_STATE;
  const int nv = (int)d->v_id.size();
  std::vector<int> tris;
  if (tris_in) {
    if (n_tris < 0) return OVP_E_ARG;
    if (n_tris > MAX_TRIS) return OVP_E_CAPACITY;
    tris.assign(tris_in, tris_in + 3 * (size_t)n_tris);
    d->tri_source = 0;
  } else if (d->dev_delaunay && d->dev_tris_ok) {
    tris = d->dev_tris;
    d->tri_source = 2;
  } else {
    std::vector<std::array<int, 3>> out;
    ovp_delaunay_host(nv, d->v_px.data(), out);
    for (const auto& t : out) tris.insert(tris.end(), t.begin(), t.end());
    d->tri_source = 1;
  }
  const int nt = (int)tris.size() / 3;
  if (nt > MAX_TRIS) return OVP_E_CAPACITY;
  for (int t = 0; t < nt; ++t) {  // every index is checked before anything is enqueued
    const int a = tris[3 * t], b = tris[3 * t + 1], e = tris[3 * t + 2];
    if (a < 0 || b < 0 || e < 0 || a >= nv || b >= nv || e >= nv || a == b || b == e || a == e) return OVP_E_ARG;
  }
  if (3 * (size_t)nt * 2 > (size_t)MAX_EDGES) return OVP_E_CAPACITY;  // (directed neighbour edges: at most six per triangle)
  HIPCHK(hipSetDevice(c->device));
  const ovp_trackplane_opts& o = d->o;
  int rc = 0;
  char* h = nullptr;  // (the staging block, taken anew for each of the call's two uploads)
  const char* dv = d->stage.dev();
  char* dr = (char*)d->dres.get();
  const char* hr = (const char*)d->hres.payload();
  std::vector<std::vector<int>> nb(nv);  // feat_to_close_feat: neighbours, ascending feature id
  std::vector<unsigned char> match;
  std::vector<int> e_ptr(nv + 1, 0);
  if (nt > 0) {
    std::vector<std::vector<int>> vt(nv);
    std::vector<std::set<std::pair<int64_t, int>>> nbs(nv);
    for (int t = 0; t < nt; ++t)
      for (int k = 0; k < 3; ++k) {
        const int v = tris[3 * t + k];
        vt[v].push_back(t);
        for (int j = 1; j < 3; ++j) {
          const int w = tris[3 * t + (k + j) % 3];
          nbs[v].insert({d->v_id[w], w});
        }
      }
    int ne = 0;
    for (int v = 0; v < nv; ++v) {
      for (const auto& pr : nbs[v]) nb[v].push_back(pr.second);
      e_ptr[v] = ne;
      ne += (int)nb[v].size();
    }
    e_ptr[nv] = ne;
    if (ne > MAX_EDGES) return OVP_E_CAPACITY;  // (cannot happen: nt <= MAX_TRIS)
    StageLayout L;
    const size_t o_vslot = L.take(sizeof(int) * nv), o_vpx = L.take(sizeof(float) * 2 * nv), o_tris = L.take(sizeof(int) * 3 * nt),
                 o_vtp = L.take(sizeof(int) * (nv + 1)), o_vti = L.take(sizeof(int) * 3 * nt), o_es = L.take(sizeof(int) * ne),
                 o_ed = L.take(sizeof(int) * ne), o_pose = L.take(sizeof(double) * 12);
    StageLayout Rl;
    const size_t r_match = Rl.take(ne), r_trin = Rl.take(sizeof(double) * 3 * nt), r_triok = Rl.take(nt);
    if (Rl.bytes() > d->res_cap) return OVP_E_CAPACITY;
    if (!(h = d->stage.begin(L.bytes(), &rc))) return rc;
    d->have_frame = false;  // from here on the frame is consumed: the normal histories change
    memcpy(h + o_vslot, d->v_slot.data(), sizeof(int) * nv);
    memcpy(h + o_vpx, d->v_px.data(), sizeof(float) * 2 * nv);
    memcpy(h + o_tris, tris.data(), sizeof(int) * 3 * nt);
    int* vtp = (int*)(h + o_vtp);
    int* vti = (int*)(h + o_vti);
    int* es = (int*)(h + o_es);
    int* ed = (int*)(h + o_ed);
    int at = 0;
    for (int v = 0; v < nv; ++v) {
      vtp[v] = at;
      for (int t : vt[v]) vti[at++] = t;
      for (size_t k = 0; k < nb[v].size(); ++k) es[e_ptr[v] + k] = v, ed[e_ptr[v] + k] = nb[v][k];
    }
    vtp[nv] = at;
    memcpy(h + o_pose, d->pose, sizeof(double) * 12);
    HIPCHK(d->stage.send(L.bytes(), c->stream, Fence::CallerWaits));
    if (d->timed) HIPCHK(hipEventRecord(d->ev[2], c->stream));
    hipLaunchKernelGGL(k_det_tri_normals, dim3((nt + 255) / 256), dim3(256), 0, c->stream, nt, (const int*)(dv + o_tris),
                       (const int*)(dv + o_vslot), (const float*)(dv + o_vpx), (const double*)d->p.get(), (const double*)(dv + o_pose),
                       (double)o.max_tri_side_px, (double*)(dr + r_trin), (unsigned char*)(dr + r_triok));
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_det_vertex_norms, dim3((nv + 255) / 256), dim3(256), 0, c->stream, nv, (const int*)(dv + o_vslot),
                       (const int*)(dv + o_vtp), (const int*)(dv + o_vti), (const double*)(dr + r_trin),
                       (const unsigned char*)(dr + r_triok), d->st(), o.max_norm_count, o.max_norm_avg_max, o.max_norm_avg_var);
    HIPCHK(hipGetLastError());
    if (d->timed) HIPCHK(hipEventRecord(d->ev[3], c->stream));
    hipLaunchKernelGGL(k_det_match, dim3((ne + 255) / 256), dim3(256), 0, c->stream, ne, (const int*)(dv + o_es), (const int*)(dv + o_ed),
                       (const int*)(dv + o_vslot), (const float*)(dv + o_vpx), d->st(), o.min_norms, (double)o.max_pairwise_px,
                       o.max_norm_deg, o.max_dist_between_z, (unsigned char*)(dr + r_match));
    HIPCHK(hipGetLastError());
    if (d->timed) HIPCHK(hipEventRecord(d->ev[4], c->stream));
    const int rw = publish_and_wait(c, d, ne);  // (the match bytes lead the block)
    if (rw) return rw;
    if (d->timed) {
      HIPCHK(hipStreamSynchronize(c->stream));
      HIPCHK(hipEventElapsedTime(&d->ms[1], d->ev[2], d->ev[3]));
      HIPCHK(hipEventElapsedTime(&d->ms[2], d->ev[3], d->ev[4]));
    }
    match.assign((const unsigned char*)hr + r_match, (const unsigned char*)hr + r_match + ne);

    // ---- greedy merge, ascending feature id (TrackPlane.cpp:817-979) ----
    std::vector<int> order(nv);
    for (int v = 0; v < nv; ++v) order[v] = v;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return d->v_id[a] < d->v_id[b]; });
    auto& f2p = d->feat2plane;
    auto update_plane_ids = [&](int64_t min_planeid, int64_t oldplaneid) {
      if (min_planeid == oldplaneid) return;
      for (auto& pr : f2p)
        if (pr.second == oldplaneid) pr.second = min_planeid;
      d->plane2old[min_planeid].insert(oldplaneid);
      auto it = d->plane2old.find(oldplaneid);
      if (it != d->plane2old.end()) {
        const std::set<int64_t> olds = it->second;
        for (int64_t t : olds) d->plane2old[min_planeid].insert(t);
        d->plane2old.erase(oldplaneid);
      }
    };
    std::set<int> done_verts;
    for (int v : order) {
      const int64_t featid = d->v_id[v];
      if (!o.check_old_feats && f2p.count(featid)) continue;
      std::vector<int64_t> matches;
      for (size_t k = 0; k < nb[v].size(); ++k)
        if (match[e_ptr[v] + k] && !done_verts.count(nb[v][k])) matches.push_back(d->v_id[nb[v][k]]);
      if (matches.empty()) continue;
      int64_t min_planeid = -1;
      if (f2p.count(featid)) min_planeid = f2p.at(featid);
      for (int64_t m : matches) {
        auto it = f2p.find(m);
        if (it == f2p.end()) continue;
        min_planeid = min_planeid == -1 ? it->second : std::min(min_planeid, it->second);
      }
      if (min_planeid != -1) {
        for (int64_t m : matches)
          if (f2p.count(m)) update_plane_ids(min_planeid, f2p.at(m));
        if (f2p.count(featid)) update_plane_ids(min_planeid, f2p.at(featid));
        for (int64_t m : matches) f2p[m] = min_planeid;
        f2p[featid] = min_planeid;
        done_verts.insert(v);
      } else {
        const int64_t fresh_id = ++d->currplaneid;
        for (int64_t m : matches) f2p[m] = fresh_id;
        f2p[featid] = fresh_id;
      }
    }
  }

  d->have_frame = false;
  // ---- spatial filter (TrackPlane.cpp:989-1058): planes of more than filter_num_feat active features ----
  std::map<int64_t, int> vert_of;
  for (int v = 0; v < nv; ++v) vert_of[d->v_id[v]] = v;
  d->filt_dbg.clear();
  {
    std::map<int64_t, std::vector<int64_t>> plane_to_feat;
    for (const auto& pr : d->feat2plane)
      if (vert_of.count(pr.first)) plane_to_feat[pr.second].push_back(pr.first);
    std::vector<int> pl_ptr(1, 0), pl_slot;
    std::vector<int64_t> pl_feat, pl_id;
    for (const auto& pr : plane_to_feat) {
      if ((int)pr.second.size() <= o.filter_num_feat) continue;
      for (int64_t f : pr.second) pl_feat.push_back(f), pl_id.push_back(pr.first), pl_slot.push_back(d->v_slot[vert_of.at(f)]);
      pl_ptr.push_back((int)pl_slot.size());
    }
    const int np = (int)pl_ptr.size() - 1, m = (int)pl_slot.size();  // m <= nv <= OVP_DET_MAX_POINTS: so is every plane
    if (np > 0) {
      StageLayout L;
      const size_t o_ptr = L.take(sizeof(int) * (np + 1)), o_sl = L.take(sizeof(int) * m);
      StageLayout Rl;
      const size_t r_d = Rl.take(sizeof(double) * m), r_f = Rl.take(m);
      if (Rl.bytes() > d->res_cap) return OVP_E_CAPACITY;
      if (!(h = d->stage.begin(L.bytes(), &rc))) return rc;
      memcpy(h + o_ptr, pl_ptr.data(), sizeof(int) * (np + 1));
      memcpy(h + o_sl, pl_slot.data(), sizeof(int) * m);
      HIPCHK(d->stage.send(L.bytes(), c->stream, Fence::CallerWaits));
      if (d->timed) HIPCHK(hipEventRecord(d->ev[5], c->stream));
      hipLaunchKernelGGL(k_det_spatial_filter, dim3(np), dim3(256), 0, c->stream, (const int*)(dv + o_ptr), (const int*)(dv + o_sl),
                         (const double*)d->p.get(), o.filter_num_feat, o.filter_z_thresh, (double*)(dr + r_d), (unsigned char*)(dr + r_f));
      HIPCHK(hipGetLastError());
      if (d->timed) HIPCHK(hipEventRecord(d->ev[6], c->stream));
      const int rw = publish_and_wait(c, d, Rl.bytes());
      if (rw) return rw;
      if (d->timed) {
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipEventElapsedTime(&d->ms[3], d->ev[5], d->ev[6]));
      }
      const double* rd = (const double*)(hr + r_d);
      const unsigned char* rf = (const unsigned char*)(hr + r_f);
      for (int i = 0; i < m; ++i) {
        if (rf[i]) d->feat2plane.erase(pl_feat[i]);
        const double row[4] = {(double)pl_feat[i], (double)pl_id[i], rd[i], (double)rf[i]};
        d->filt_dbg.insert(d->filt_dbg.end(), row, row + 4);
      }
    }
  }

  // ---- keep the planes of more than three active features, and their merge history (TrackPlane.cpp:1064-1095) ----
  {
    std::map<int64_t, int> plane2featct;
    for (int v = 0; v < nv; ++v) {
      auto it = d->feat2plane.find(d->v_id[v]);
      if (it != d->feat2plane.end()) plane2featct[it->second]++;
    }
    std::map<int64_t, int64_t> f2p_tmp;
    std::map<int64_t, std::set<int64_t>> p2o_tmp;
    for (int v = 0; v < nv; ++v) {
      auto it = d->feat2plane.find(d->v_id[v]);
      if (it != d->feat2plane.end() && plane2featct.at(it->second) > 3) f2p_tmp.insert({it->first, it->second});
    }
    for (const auto& pr : f2p_tmp) {
      auto it = d->plane2old.find(pr.second);
      if (it != d->plane2old.end()) p2o_tmp.insert({pr.second, it->second});
    }
    d->feat2plane.swap(f2p_tmp);
    d->plane2old.swap(p2o_tmp);
  }
  return 0;
}

extern "C" int ovp_plane_spatial_filter(ovp_ctx* c, int n_planes, const int* feat_start, const double* p_FinG, int filter_num_feat,
                                        double filter_z_thresh, double* mean_dist, uint8_t* flagged) {
  Detector* d = det_of(c);
  if (!d) return c ? OVP_E_STATE : OVP_E_ARG;
  if (n_planes < 0 || !feat_start || filter_num_feat < 2 || filter_num_feat > OVP_DET_MAX_FILTER_K) return OVP_E_ARG;
  const int m = n_planes ? feat_start[n_planes] : 0;
  if (m < 0 || (m > 0 && (!p_FinG || !mean_dist || !flagged)) || feat_start[0] != 0) return OVP_E_ARG;
  std::vector<int> ptr(1, 0), src;  // the planes the filter looks at, compacted
  for (int k = 0; k < n_planes; ++k) {
    const int n = feat_start[k + 1] - feat_start[k];
    if (n < 0) return OVP_E_ARG;
    if (n > OVP_DET_MAX_POINTS) return OVP_E_CAPACITY;
    if (n <= filter_num_feat) continue;
    for (int i = 0; i < n; ++i) src.push_back(feat_start[k] + i);
    ptr.push_back((int)src.size());
  }
  const int np = (int)ptr.size() - 1, mm = (int)src.size();
  StageLayout L;
  const size_t o_ptr = L.take(sizeof(int) * (np + 1)), o_sl = L.take(sizeof(int) * mm), o_p = L.take(sizeof(double) * 3 * mm);
  StageLayout Rl;
  const size_t r_d = Rl.take(sizeof(double) * mm), r_f = Rl.take(mm);
  if (L.bytes() > d->stage.capacity() || Rl.bytes() > d->res_cap) return OVP_E_CAPACITY;
  for (int i = 0; i < m; ++i) mean_dist[i] = 0.0, flagged[i] = 0;
  if (np == 0) return 0;
  HIPCHK(hipSetDevice(c->device));
  int rc = 0;
  char* h = d->stage.begin(L.bytes(), &rc);
  if (!h) return rc;
  const char* dv = d->stage.dev();
  char* dr = (char*)d->dres.get();
  memcpy(h + o_ptr, ptr.data(), sizeof(int) * (np + 1));
  for (int i = 0; i < mm; ++i) {
    ((int*)(h + o_sl))[i] = i;
    memcpy(h + o_p + sizeof(double) * 3 * i, p_FinG + 3 * (size_t)src[i], sizeof(double) * 3);
  }
  HIPCHK(d->stage.send(L.bytes(), c->stream, Fence::CallerWaits));
  if (d->timed) HIPCHK(hipEventRecord(d->ev[5], c->stream));
  hipLaunchKernelGGL(k_det_spatial_filter, dim3(np), dim3(256), 0, c->stream, (const int*)(dv + o_ptr), (const int*)(dv + o_sl),
                     (const double*)(dv + o_p), filter_num_feat, filter_z_thresh, (double*)(dr + r_d), (unsigned char*)(dr + r_f));
  HIPCHK(hipGetLastError());
  if (d->timed) HIPCHK(hipEventRecord(d->ev[6], c->stream));
  const int rw = publish_and_wait(c, d, Rl.bytes());
  if (rw) return rw;
  if (d->timed) {
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipEventElapsedTime(&d->ms[3], d->ev[5], d->ev[6]));
  }
  const char* hr = (const char*)d->hres.payload();
  for (int i = 0; i < mm; ++i) mean_dist[src[i]] = ((const double*)(hr + r_d))[i], flagged[src[i]] = ((const unsigned char*)(hr + r_f))[i];
  return 0;
}

extern "C" int ovp_plane_detector_map(ovp_ctx* c, int64_t* ids, int64_t* planes, int cap, int* n) {
  Detector* d = det_of(c);
  if (!d) return c ? OVP_E_STATE : OVP_E_ARG;
  if (!n || cap < 0 || (cap > 0 && (!ids || !planes))) return OVP_E_ARG;
  *n = (int)d->feat2plane.size();
  int i = 0;
  for (const auto& pr : d->feat2plane) {
    if (i >= cap) break;
    ids[i] = pr.first, planes[i] = pr.second;
    ++i;
  }
  return 0;
}

extern "C" int ovp_plane_detector_merges(ovp_ctx* c, int64_t* pairs, int cap, int* n) {
  Detector* d = det_of(c);
  if (!d) return c ? OVP_E_STATE : OVP_E_ARG;
  if (!n || cap < 0 || (cap > 0 && !pairs)) return OVP_E_ARG;
  int i = 0;
  for (const auto& pr : d->plane2old)
    for (int64_t old : pr.second) {
      if (i < cap) pairs[2 * i] = pr.first, pairs[2 * i + 1] = old;
      ++i;
    }
  *n = i;
  return 0;
}

extern "C" long ovp_plane_detector_debug(ovp_ctx* c, const char* what, int64_t id, double* out, long cap) {
  Detector* d = det_of(c);
  if (!d) return c ? OVP_E_STATE : OVP_E_ARG;
  if (!what || !out || cap < 0) return OVP_E_ARG;
  if (!strcmp(what, "filter")) {
    const long k = std::min<long>(cap, (long)d->filt_dbg.size());
    memcpy(out, d->filt_dbg.data(), sizeof(double) * k);
    return k;
  }
  if (!strcmp(what, "timer")) {
    d->timed = id != 0;
    return 0;
  }
  if (!strcmp(what, "time")) {
    if (cap < 4) return OVP_E_ARG;
    for (int k = 0; k < 4; ++k) out[k] = d->ms[k];
    return 4;
  }
  if (!strcmp(what, "time_delaunay")) {
    if (cap < 2) return OVP_E_ARG;
    out[0] = d->ms_delaunay[0], out[1] = d->ms_delaunay[1];
    return 2;
  }
  if (!strcmp(what, "tris")) {
    if (cap < 6) return OVP_E_ARG;
    out[0] = d->tri_source, out[1] = d->dev_delaunay ? 1 : 0;
    for (int k = 0; k < 4; ++k) out[2 + k] = d->dev_hdr[k + 1];
    return 6;
  }
  if (strcmp(what, "feat")) return OVP_E_ARG;
  auto it = d->slot_of.find(id);
  if (it == d->slot_of.end()) return OVP_E_ARG;
  if (cap < 9 + 3 * OVP_DET_MAX_NORMS) return OVP_E_ARG;
  const int s = it->second;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  int cnt = 0, valid = 0, rn = 0;
  HIPCHK(hipMemcpy(&cnt, d->count.get() + s, sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(&valid, d->valid.get() + s, sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(&rn, d->ring_n.get() + s, sizeof(int), hipMemcpyDeviceToHost));
  if (rn < 0 || rn > OVP_DET_MAX_NORMS) return OVP_E_STATE;
  out[0] = cnt, out[1] = valid, out[5] = rn;
  HIPCHK(hipMemcpy(out + 2, d->p.get() + 3 * s, sizeof(double) * 3, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(out + 6, d->avg.get() + 3 * s, sizeof(double) * 3, hipMemcpyDeviceToHost));
  if (rn > 0) HIPCHK(hipMemcpy(out + 9, d->ring.get() + (size_t)s * OVP_DET_MAX_NORMS * 3, sizeof(double) * 3 * rn, hipMemcpyDeviceToHost));
  return 9 + 3 * rn;
}
