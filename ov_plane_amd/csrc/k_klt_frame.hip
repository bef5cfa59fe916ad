// The back half of TrackPlane::feed_monocular (track_plane/TrackPlane.cpp:536-557) on the device, behind k_klt_track and the
// epipolar kernels in the same enqueue (ovp_klt_match_frame, k_klt.hip): the keep rule, the compaction of the survivors and
// database->update_feature for each of them.
//   k_klt_keep_append  ONE workgroup of 1024 threads walks the n <= 4096 points in chunks of 1024, a thread per point.  Two
//                      order-preserving exclusive prefix sums - over keep, and over keep && fresh - each a ballot and popcount within a
//                      wave, the 16 wave totals through LDS, a running carry across chunks.  A survivor writes its index, uv and
//                      uv_norm at its rank and, with to_db, its observation into the database's table (fdb_append_one, the body
//                      k_featdb_append runs); the k-th fresh survivor takes free_slots[k].  Latency-bound: a single small workgroup,
//                      like k_featdb_classify - the point is that nothing crosses the bus between the stages.
// Integer decisions and copies only, no atomics, every order fixed: two runs give the same bytes.
// Address safety: the image mask is read only after the bounds test has passed on floats, so (int) y * cols + (int) x lies inside
// the mask; kept_* are written at a rank below n; a slot comes from the host's plan (a known id's slot, or one of the free slots the
// host counted the fresh candidates against), and fdb_append_one refuses a full slot.
#include "k_klt_frame.h"

#include "ovplane_hip.h"

namespace {

constexpr int FRM_THREADS = 1024, FRM_WAVES = FRM_THREADS / 64;

__global__ __launch_bounds__(FRM_THREADS) void k_klt_keep_append(KltFrameArgs a) {
  __shared__ int s_tot[2][FRM_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  int carry_keep = 0, carry_fresh = 0;
  for (int base = 0; base < a.n; base += FRM_THREADS) {
    const int i = base + tid;
    bool keep = false, fresh = false;
    float2 p = make_float2(0.f, 0.f);
    if (i < a.n) {
      p = a.pts[i];
      // :538-546 in float: no conversion overflows, and a NaN fails trunc(x) < cols
      keep = a.mask_epi[i] != 0 && !(p.x < 0.f) && !(p.y < 0.f) && truncf(p.x) < (float)a.cols && truncf(p.y) < (float)a.rows;
      if (keep && a.mask) keep = a.mask[(size_t)(int)p.y * a.cols + (int)p.x] <= 127;
      fresh = keep && a.to_db && a.fresh[i];
      a.keep[i] = keep ? 1 : 0;
    }
    const unsigned long long bk = __ballot(keep), bf = __ballot(fresh);
    if (lane == 0) s_tot[0][wave] = __popcll(bk), s_tot[1][wave] = __popcll(bf);
    __syncthreads();
    int before_keep = 0, before_fresh = 0, all_keep = 0, all_fresh = 0;
#pragma unroll
    for (int w = 0; w < FRM_WAVES; ++w) {
      const int ck = s_tot[0][w], cf = s_tot[1][w];
      if (w < wave) before_keep += ck, before_fresh += cf;
      all_keep += ck, all_fresh += cf;
    }
    if (keep) {
      const int at = carry_keep + before_keep + __popcll(bk & below);
      const float2 q = a.uvn ? a.uvn[i] : make_float2(0.f, 0.f);
      a.kept_index[at] = i;
      a.kept_uv[at] = p;
      if (a.uvn) a.kept_uvn[at] = q;
      if (a.to_db) {  // :553-557 database->update_feature
        const int s = fresh ? a.free_slots[carry_fresh + before_fresh + __popcll(bf & below)] : a.slot[i];
        fdb_append_one(a.t, s, fresh, a.ids[i], a.stamp, p, q);
      }
    }
    carry_keep += all_keep, carry_fresh += all_fresh;
    __syncthreads();  // (the next chunk writes s_tot again)
  }
  if (tid == 0) *a.n_kept = carry_keep;
}

}  // namespace

int ovp_klt_frame_enqueue(const KltFrameArgs& a, hipStream_t stream) {
  if (a.n < 1 || a.n > OVP_KLT_MAX_POINTS) return OVP_E_ARG;
  hipLaunchKernelGGL(k_klt_keep_append, dim3(1), dim3(FRM_THREADS), 0, stream, a);
  return (int)hipGetLastError();
}
