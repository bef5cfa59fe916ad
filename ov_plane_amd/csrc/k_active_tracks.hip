// Re-triangulation of a frame's active tracks: VioManager::retriangulate_active_tracks (core/VioManagerHelper.cpp:220-418)
// restated - every point tracked into the frame becomes a position in G and, when camera 0 sees it, a (u, v, depth) triple.
// The per-feature history (active_feat_linsys_A / _b / _count) is a device table of feature slots, the feature id -> slot map
// lives on the host.  One compute launch per frame:
//   k_active_tracks   threads [0, nf): one per distinct tracked feature, walking its <= 4 observations in the caller's order -
//                     the frame's system, the 3 x 3 solve and the gates after each of them (:268-326), the projection into camera 0
//                     (:372-410); threads [nf, nf + nl): one per SLAM landmark - its position (:342-357) and the same projection.
// A landmark's position does not depend on any tracked point and a tracked point's projection only on its own position, so the
// two halves of the reference's function need no second launch.  The result block goes to the host through the object's own
// Mailbox (ovp_mailbox.h, k_publish.hip).  No atomics, every order fixed: two runs give the same bits.
// Not built: display_active (:229-234) and the distort_d branch at :387-391, which cannot be reached - the `continue` at :376
// has already left the iteration for every feature without a camera-0 pixel.
#include "ovp_ctx.h"
#include "k_tri3.h"

#include <array>
#include <map>

namespace {

struct AtFrame {
  double *A, *b;  // the slot table: [S*6] upper triangle (00 01 02 11 12 22), [S*3]
  int* count;     // [S]
  int nf, nl;
  const int *f_slot, *f_obs, *f_px;  // [nf] slot (-1: the id is a SLAM landmark), [nf*4] observations in order (-1: none), [nf] camera-0 observation or -1
  const unsigned char* f_fresh;      // [nf] the feature was not in the table the previous frame left
  const int* o_cam;                  // per observation: camera, normalised coordinates, raw pixel
  const double* o_uvn;
  const float* o_uv;
  const double *poses, *cam0;  // [OVP_MAX_CAMERAS][R_GtoC 9 | p_CinG 3]; [R_ItoC 9 | p_IinC 3 | R_GtoI 9 | p_IinG 3] of camera 0 / the newest clone
  const double *l_xyz, *l_anchor;  // [nl*3]; [nl][R_GtoI 9 | p_IinG 3 | R_ItoC 9 | p_IinC 3] of the anchor (read for relative ones)
  const unsigned char* l_rel;
  const int* l_px;  // [nl] camera-0 observation of the landmark's id or -1
  double min_dist, max_dist, max_cond;
  int width, height;
  double *out_p, *out_uvd;  // [(nf + nl)*3] each
  unsigned char* out_flag;  // [nf + nl] bit 0: has a position, bit 1: has a uvd
};

// :381-409 a position into camera 0 of the newest clone; uvd = (raw pixel, depth) unless the depth or the pixel is out of range
__device__ __forceinline__ bool at_project(const double* __restrict__ c0, const double p[3], float u_raw, float v_raw, int w, int h,
                                           double uvd[3]) {
  const double d0 = p[0] - c0[21], d1 = p[1] - c0[22], d2 = p[2] - c0[23];
  double pi[3], pc[3];
  for (int r = 0; r < 3; ++r) pi[r] = c0[12 + 3 * r] * d0 + c0[12 + 3 * r + 1] * d1 + c0[12 + 3 * r + 2] * d2;
  for (int r = 0; r < 3; ++r) pc[r] = c0[3 * r] * pi[0] + c0[3 * r + 1] * pi[1] + c0[3 * r + 2] * pi[2] + c0[9 + r];
  const double depth = pc[2], u = (double)u_raw, v = (double)v_raw;
  if (depth < 0.1) return false;                                       // :394 (a NaN depth passes, as in the reference)
  if (u < 0 || (int)u >= w || v < 0 || (int)v >= h) return false;      // :401
  uvd[0] = u, uvd[1] = v, uvd[2] = depth;
  return true;
}

__global__ __launch_bounds__(256) void k_active_tracks(AtFrame f) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= f.nf + f.nl) return;
  double p[3] = {0, 0, 0}, uvd[3] = {0, 0, 0};
  int has = 0, px = -1;
  if (i < f.nf) {
    const int s = f.f_slot[i];
    px = f.f_px[i];
    // :277-280 a SLAM landmark's pixel counts for camera 0, but it adds no row to any system (and the host has dropped its slot)
    if (s >= 0) {
      const bool fresh = f.f_fresh[i] != 0;
      double Ao[6] = {0, 0, 0, 0, 0, 0}, bo[3] = {0, 0, 0}, An[6] = {0, 0, 0, 0, 0, 0}, bn[3] = {0, 0, 0};
      int co = 0, cn = 0;
      if (!fresh) {
        for (int k = 0; k < 6; ++k) Ao[k] = f.A[s * 6 + k];
        for (int k = 0; k < 3; ++k) bo[k] = f.b[s * 3 + k];
        co = f.count[s];
      }
      for (int k = 0; k < OVP_MAX_CAMERAS; ++k) {
        const int o = f.f_obs[4 * i + k];
        if (o < 0) break;
        const double* R = f.poses + 12 * f.o_cam[o];
        const double* pc = R + 9;
        // :283-292 bearing in G, A_i = skew(b)^T skew(b), b_i = A_i p_CiinG
        const double x = f.o_uvn[2 * o], y = f.o_uvn[2 * o + 1];
        double bx = R[0] * x + R[3] * y + R[6], by = R[1] * x + R[4] * y + R[7], bz = R[2] * x + R[5] * y + R[8];
        const double nb = sqrt(bx * bx + by * by + bz * bz);
        bx /= nb, by /= nb, bz /= nb;
        const double Ai[6] = {bz * bz + by * by, -bx * by, -bx * bz, bz * bz + bx * bx, -by * bz, by * by + bx * bx};
        const double bi[3] = {Ai[0] * pc[0] + Ai[1] * pc[1] + Ai[2] * pc[2], Ai[1] * pc[0] + Ai[3] * pc[1] + Ai[4] * pc[2],
                              Ai[2] * pc[0] + Ai[4] * pc[1] + Ai[5] * pc[2]};
        if (!fresh) {
          // :297-301 the frame's system is OLD + A_i and the count OLD + 1, old being what the previous frame left: a second camera's
          // observation in the same frame replaces the first one's term, it does not join it
          for (int q = 0; q < 6; ++q) An[q] = Ai[q] + Ao[q];
          for (int q = 0; q < 3; ++q) bn[q] = bi[q] + bo[q];
          cn = 1 + co;
        } else if (k == 0) {
          // :293-296 a feature the previous frame did not leave is inserted - and std::map::insert does not replace: of such a
          // feature's observations in this frame the FIRST one's term stays
          for (int q = 0; q < 6; ++q) An[q] = Ai[q];
          for (int q = 0; q < 3; ++q) bn[q] = bi[q];
          cn = 1;
        }
        // :304 the solve runs above three observations - a literal of the reference, not feat_init_min_obs - after every
        // observation, in the observing camera; the last solve that passes the gates leaves its position (:323)
        if (cn > 3) {
          double q[3];
          ovp_tri3_solve(An, bn, q);
          const double cond = ovp_tri3_cond(An);
          const double d0 = q[0] - pc[0], d1 = q[1] - pc[1], d2 = q[2] - pc[2];
          const double cx = R[0] * d0 + R[1] * d1 + R[2] * d2, cy = R[3] * d0 + R[4] * d1 + R[5] * d2,
                       cz = R[6] * d0 + R[7] * d1 + R[8] * d2;
          const double nrm = sqrt(cx * cx + cy * cy + cz * cz);
          // :321-322 condition number, distance along the observing camera's axis, finite norm
          if (fabs(cond) <= f.max_cond && cz >= f.min_dist && cz <= f.max_dist && !isnan(nrm)) {
            has = 1;
            for (int r = 0; r < 3; ++r) p[r] = q[r];
          }
        }
      }
      // :331-334 only the features observed in this frame are in the next frame's table (the host has given the other slots back)
      for (int k = 0; k < 6; ++k) f.A[s * 6 + k] = An[k];
      for (int k = 0; k < 3; ++k) f.b[s * 3 + k] = bn[k];
      f.count[s] = cn;
    }
  } else {
    const int j = i - f.nf;
    px = f.l_px[j];
    // :343-356 the state's estimate; a relative representation goes through its anchor clone and anchor camera into G
    for (int r = 0; r < 3; ++r) p[r] = f.l_xyz[3 * j + r];
    if (f.l_rel[j]) {
      const double* a = f.l_anchor + 24 * j;
      const double d0 = p[0] - a[21], d1 = p[1] - a[22], d2 = p[2] - a[23];
      double t[3];
      for (int r = 0; r < 3; ++r) t[r] = a[12 + r] * d0 + a[12 + 3 + r] * d1 + a[12 + 6 + r] * d2;  // R_ItoC^T (xyz - p_IinC)
      for (int r = 0; r < 3; ++r) p[r] = a[r] * t[0] + a[3 + r] * t[1] + a[6 + r] * t[2] + a[9 + r];  // R_GtoI^T (.) + p_IinG
    }
    has = 1;
  }
  // :372-410 every position whose feature camera 0 sees in this frame
  int vis = 0;
  if (has && px >= 0 && at_project(f.cam0, p, f.o_uv[2 * px], f.o_uv[2 * px + 1], f.width, f.height, uvd)) vis = 1;
  for (int r = 0; r < 3; ++r) f.out_p[3 * i + r] = p[r], f.out_uvd[3 * i + r] = uvd[r];
  f.out_flag[i] = (unsigned char)(has | (vis << 1));
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
constexpr int S = OVP_MAX_CAMERAS * OVP_AT_MAX_POINTS;  // feature slots: a frame's distinct features fit, the others have given theirs back
constexpr int MAX_OBS = OVP_MAX_CAMERAS * OVP_AT_MAX_POINTS, MAX_OUT = S + OVP_AT_MAX_LANDMARKS;

struct ActiveTracks {
  DevBuf<double> A, b;
  DevBuf<int> count;
  Staged stage;  // the frame's tables
  DevBuf<void> dres;
  Mailbox hres;  // the frame's results: payload from byte 0, channel 0
  size_t res_cap = 0;
  OvpEvent ev[2];
  float ms = 0.f;
  bool timed = false;  // ovp_active_tracks_debug "timer": events around the kernel, read behind a stream synchronisation
  std::map<int64_t, int> slot_of;
  std::vector<int> free_slots;  // a stack, so which slot a feature takes is a function of the call sequence alone
  void forget() {
    slot_of.clear();
    free_slots.clear();
    for (int s = S - 1; s >= 0; --s) free_slots.push_back(s);
  }
};

ActiveTracks* at_of(ovp_ctx* c) { return c ? (ActiveTracks*)c->active_tracks.get() : nullptr; }

}  // namespace

extern "C" int ovp_active_tracks_create(ovp_ctx* c) {
  if (!c) return OVP_E_ARG;
  HIPCHK(hipSetDevice(c->device));
  auto d = std::make_shared<ActiveTracks>();
  HIPCHK(d->A.alloc((size_t)S * 6));
  HIPCHK(d->b.alloc((size_t)S * 3));
  HIPCHK(d->count.alloc(S));
  HIPCHK(d->stage.alloc(64 * 16 + sizeof(int) * ((size_t)S * 6 + MAX_OBS + OVP_AT_MAX_LANDMARKS) + S + OVP_AT_MAX_LANDMARKS +
                        sizeof(double) * (2 * (size_t)MAX_OBS + 12 * OVP_MAX_CAMERAS + 24 + 27 * (size_t)OVP_AT_MAX_LANDMARKS) +
                        sizeof(float) * 2 * (size_t)MAX_OBS));
  d->res_cap = 64 * 4 + sizeof(double) * 6 * (size_t)MAX_OUT + MAX_OUT;
  HIPCHK(d->dres.alloc(d->res_cap));
  HIPCHK(d->hres.alloc(d->res_cap));
  for (OvpEvent& e : d->ev) HIPCHK(e.create());
  d->forget();
  c->active_tracks = d;
  return 0;
}

extern "C" int ovp_active_tracks_destroy(ovp_ctx* c) {
  if (!c) return OVP_E_ARG;
  if (!c->active_tracks) return OVP_E_STATE;
  HIPCHK(hipStreamSynchronize(c->stream));
  c->active_tracks.reset();
  return 0;
}

extern "C" int ovp_active_tracks_reset(ovp_ctx* c) {
  ActiveTracks* d = at_of(c);
  if (!d) return c ? OVP_E_STATE : OVP_E_ARG;
  d->forget();  // (a slot's device state is overwritten when a feature takes it)
  return 0;
}

extern "C" int ovp_active_tracks_update(ovp_ctx* c, const ovp_active_tracks_in* in, ovp_active_tracks_out* out) {
  ActiveTracks* d = at_of(c);
  if (!d) return c ? OVP_E_STATE : OVP_E_ARG;
  if (!in || !out) return OVP_E_ARG;
  const int n = in->n_obs, nl = in->n_slam;
  // ---- every check before anything is touched or enqueued ----
  if (n < 0 || nl < 0 || in->n_cams < 1 || in->n_cams > OVP_MAX_CAMERAS || out->cap < 0) return OVP_E_ARG;
  if (n > 0 && (!in->cam_idx || !in->feat_id || !in->uv || !in->uv_norm)) return OVP_E_ARG;
  if (!in->R_GtoC || !in->p_CinG) return OVP_E_ARG;
  if (nl > 0 && (!in->slam_id || !in->slam_xyz || !in->slam_relative)) return OVP_E_ARG;
  if (nl > OVP_AT_MAX_LANDMARKS) return OVP_E_CAPACITY;
  std::map<int64_t, int> lm_of;  // landmark id -> input index
  for (int j = 0; j < nl; ++j) {
    if (!lm_of.emplace(in->slam_id[j], j).second) return OVP_E_ARG;
    if (in->slam_relative[j] && (!in->slam_anchor_R_GtoI || !in->slam_anchor_p_IinG || !in->slam_anchor_R_ItoC || !in->slam_anchor_p_IinC))
      return OVP_E_ARG;
  }
  // the distinct features in order of first appearance, each with its observations in the caller's order
  std::map<int64_t, int> feat_of;
  std::vector<int64_t> f_id;
  std::vector<std::array<int, 4>> f_obs;
  std::vector<unsigned> f_cams;  // cameras that have seen it, as a mask
  std::vector<int> f_px;
  int per_cam[OVP_MAX_CAMERAS] = {0, 0, 0, 0};
  for (int o = 0; o < n; ++o) {
    const int cam = in->cam_idx[o];
    if (cam < 0 || cam >= in->n_cams) return OVP_E_ARG;
    if (++per_cam[cam] > OVP_AT_MAX_POINTS) return OVP_E_CAPACITY;
    auto it = feat_of.find(in->feat_id[o]);
    if (it == feat_of.end()) {
      it = feat_of.emplace(in->feat_id[o], (int)f_id.size()).first;
      f_id.push_back(in->feat_id[o]);
      f_obs.push_back({-1, -1, -1, -1});
      f_cams.push_back(0u);
      f_px.push_back(-1);
    }
    const int i = it->second;
    if (f_cams[i] & (1u << cam)) return OVP_E_ARG;  // one observation per feature and camera (get_last_ids of one camera are distinct)
    int k = 0;
    while (f_obs[i][k] >= 0) ++k;
    f_obs[i][k] = o;
    f_cams[i] |= 1u << cam;
    if (cam == 0) f_px[i] = o;  // :273-275 feat_uvs_in_cam0
  }
  const int nf = (int)f_id.size(), m = nf + nl;
  out->n_feats = nf, out->n = m;
  if (m > out->cap) return OVP_E_CAPACITY;
  if (m > 0 && (!out->ids || !out->flags || !out->p_FinG || !out->uvd)) return OVP_E_ARG;
  StageLayout L;
  const size_t o_fslot = L.take(sizeof(int) * nf), o_fobs = L.take(sizeof(int) * 4 * nf), o_fpx = L.take(sizeof(int) * nf),
               o_ffresh = L.take(nf), o_ocam = L.take(sizeof(int) * n), o_ouvn = L.take(sizeof(double) * 2 * n),
               o_ouv = L.take(sizeof(float) * 2 * n), o_poses = L.take(sizeof(double) * 12 * OVP_MAX_CAMERAS),
               o_cam0 = L.take(sizeof(double) * 24), o_lxyz = L.take(sizeof(double) * 3 * nl), o_lanc = L.take(sizeof(double) * 24 * nl),
               o_lrel = L.take(nl), o_lpx = L.take(sizeof(int) * nl);
  StageLayout Rl;
  const size_t r_p = Rl.take(sizeof(double) * 3 * m), r_uvd = Rl.take(sizeof(double) * 3 * m), r_flag = Rl.take(m);
  if (L.bytes() > d->stage.capacity() || Rl.bytes() > d->res_cap) return OVP_E_CAPACITY;  // (cannot happen below the limits above)
  // ---- from here on the call goes through ----
  HIPCHK(hipSetDevice(c->device));
  // :331-334 a feature not observed in this frame, or one that has become a landmark (:277-280), gives its slot back
  for (auto it = d->slot_of.begin(); it != d->slot_of.end();)
    if (!feat_of.count(it->first) || lm_of.count(it->first)) {
      d->free_slots.push_back(it->second);
      it = d->slot_of.erase(it);
    } else
      ++it;
  if (m == 0) return 0;  // :338 nothing tracked and no landmark: the maps are empty
  int rc = 0;
  char* h = d->stage.begin(L.bytes(), &rc);
  if (!h) return rc;
  int* h_slot = (int*)(h + o_fslot);
  for (int i = 0; i < nf; ++i) {
    h[o_ffresh + i] = 0;
    if (lm_of.count(f_id[i])) {
      h_slot[i] = -1;
    } else {
      auto it = d->slot_of.find(f_id[i]);
      if (it == d->slot_of.end()) {
        const int s = d->free_slots.back();  // (never empty: at most nf <= S slots are held by this frame's features)
        d->free_slots.pop_back();
        it = d->slot_of.emplace(f_id[i], s).first;
        h[o_ffresh + i] = 1;
      }
      h_slot[i] = it->second;
    }
    memcpy(h + o_fobs + sizeof(int) * 4 * i, f_obs[i].data(), sizeof(int) * 4);
    ((int*)(h + o_fpx))[i] = f_px[i];
  }
  if (n > 0) {
    memcpy(h + o_ocam, in->cam_idx, sizeof(int) * n);
    memcpy(h + o_ouvn, in->uv_norm, sizeof(double) * 2 * n);
    memcpy(h + o_ouv, in->uv, sizeof(float) * 2 * n);
  }
  double* hp = (double*)(h + o_poses);
  for (int k = 0; k < OVP_MAX_CAMERAS; ++k)
    for (int q = 0; q < 12; ++q)
      hp[12 * k + q] = k < in->n_cams ? (q < 9 ? in->R_GtoC[9 * k + q] : in->p_CinG[3 * k + q - 9]) : 0.0;
  double* h0 = (double*)(h + o_cam0);
  memcpy(h0, in->R_ItoC0, sizeof(double) * 9);
  memcpy(h0 + 9, in->p_IinC0, sizeof(double) * 3);
  memcpy(h0 + 12, in->R_GtoI, sizeof(double) * 9);
  memcpy(h0 + 21, in->p_IinG, sizeof(double) * 3);
  for (int j = 0; j < nl; ++j) {
    memcpy(h + o_lxyz + sizeof(double) * 3 * j, in->slam_xyz + 3 * j, sizeof(double) * 3);
    double* a = (double*)(h + o_lanc) + 24 * j;
    const bool rel = in->slam_relative[j] != 0;
    h[o_lrel + j] = rel ? 1 : 0;
    if (rel) {
      memcpy(a, in->slam_anchor_R_GtoI + 9 * j, sizeof(double) * 9);
      memcpy(a + 9, in->slam_anchor_p_IinG + 3 * j, sizeof(double) * 3);
      memcpy(a + 12, in->slam_anchor_R_ItoC + 9 * j, sizeof(double) * 9);
      memcpy(a + 21, in->slam_anchor_p_IinC + 3 * j, sizeof(double) * 3);
    } else
      memset(a, 0, sizeof(double) * 24);
    auto it = feat_of.find(in->slam_id[j]);
    ((int*)(h + o_lpx))[j] = it == feat_of.end() ? -1 : f_px[it->second];
  }
  const char* dv = d->stage.dev();
  char* dr = (char*)d->dres.get();
  HIPCHK(d->stage.send(L.bytes(), c->stream, Fence::CallerWaits));
  AtFrame f;
  f.A = d->A.get(), f.b = d->b.get(), f.count = d->count.get();
  f.nf = nf, f.nl = nl;
  f.f_slot = (const int*)(dv + o_fslot), f.f_obs = (const int*)(dv + o_fobs), f.f_px = (const int*)(dv + o_fpx);
  f.f_fresh = (const unsigned char*)(dv + o_ffresh);
  f.o_cam = (const int*)(dv + o_ocam), f.o_uvn = (const double*)(dv + o_ouvn), f.o_uv = (const float*)(dv + o_ouv);
  f.poses = (const double*)(dv + o_poses), f.cam0 = (const double*)(dv + o_cam0);
  f.l_xyz = (const double*)(dv + o_lxyz), f.l_anchor = (const double*)(dv + o_lanc);
  f.l_rel = (const unsigned char*)(dv + o_lrel), f.l_px = (const int*)(dv + o_lpx);
  f.min_dist = in->min_dist, f.max_dist = in->max_dist, f.max_cond = in->max_cond_number;
  f.width = in->width, f.height = in->height;
  f.out_p = (double*)(dr + r_p), f.out_uvd = (double*)(dr + r_uvd), f.out_flag = (unsigned char*)(dr + r_flag);
  if (d->timed) HIPCHK(hipEventRecord(d->ev[0], c->stream));
  hipLaunchKernelGGL(k_active_tracks, dim3((m + 255) / 256), dim3(256), 0, c->stream, f);
  HIPCHK(hipGetLastError());
  if (d->timed) HIPCHK(hipEventRecord(d->ev[1], c->stream));
  SeqChannel& ch = d->hres.channel(0);
  const unsigned seq = ch.arm();
  HIPCHK(ovp_launch_publish_block(d->dres.get(), d->hres.dev(d->hres.payload()), Rl.bytes(), ch.word_dev(), seq, 0, c->stream));
  const int rw = ch.wait(c->stream);
  if (rw) return rw;
  d->stage.done();
  d->ms = 0.f;
  if (d->timed) {
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipEventElapsedTime(&d->ms, d->ev[0], d->ev[1]));
  }
  const char* hr = (const char*)d->hres.payload();
  for (int i = 0; i < m; ++i) out->ids[i] = i < nf ? f_id[i] : in->slam_id[i - nf];
  memcpy(out->p_FinG, hr + r_p, sizeof(double) * 3 * m);
  memcpy(out->uvd, hr + r_uvd, sizeof(double) * 3 * m);
  memcpy(out->flags, hr + r_flag, m);
  return 0;
}

extern "C" long ovp_active_tracks_debug(ovp_ctx* c, const char* what, int64_t id, double* out, long cap) {
  ActiveTracks* d = at_of(c);
  if (!d) return c ? OVP_E_STATE : OVP_E_ARG;
  if (!what || !out || cap < 0) return OVP_E_ARG;
  if (!strcmp(what, "timer")) {
    d->timed = id != 0;
    return 0;
  }
  if (!strcmp(what, "time")) {
    if (cap < 1) return OVP_E_ARG;
    out[0] = d->ms;
    return 1;
  }
  if (!strcmp(what, "size")) {
    if (cap < 1) return OVP_E_ARG;
    out[0] = (double)d->slot_of.size();
    return 1;
  }
  if (strcmp(what, "feat")) return OVP_E_ARG;
  auto it = d->slot_of.find(id);
  if (it == d->slot_of.end()) return 0;  // not in the table: the frame did not see it, or it is a landmark
  if (cap < 10) return OVP_E_ARG;
  const int s = it->second;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  int cnt = 0;
  HIPCHK(hipMemcpy(&cnt, d->count.get() + s, sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(out + 1, d->A.get() + 6 * s, sizeof(double) * 6, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(out + 7, d->b.get() + 3 * s, sizeof(double) * 3, hipMemcpyDeviceToHost));
  out[0] = cnt;
  return 10;
}
