// The feature database on the device: ext ov_core::FeatureDatabase (update_feature, features_not_containing_newer,
// features_containing, get_feature, cleanup, cleanup_measurements) and the cleaning of update/UpdaterMSCKF.cpp:74-100, as
// VioManager::do_feature_propagate_update calls them (core/VioManager.cpp:373-506, :855-869).  ov_core is not in the reference tree:
// the methods are RECALLED from their published form and UNPINNED; tests/featdb_ref.py is the restatement they are held to.
// One camera (camera 0), as ovp_state_tables is: the camera filter of :386-403 is a no-op.
// The table: S slots of up to M observations (time stamp f64, uv f32 x 2, uv_norm f32 x 2), per slot a count, a to_delete flag and
// the feature id.  The id -> slot map, the counts and the time stamps are shadowed on the host (every argument check is made there,
// before anything is touched); the slots themselves never leave the device.
//   k_featdb_append    one thread per observation of a frame, placed at count[slot]
//   k_featdb_mark      to_delete of the named slots
//   k_featdb_classify  one workgroup, a thread per live slot: class, raw and cleaned count, the totals; modifies nothing
//   k_featdb_gather    one wave per feature: the cleaned observations, in stored order, into the ovp_feature_batch layout
//   k_featdb_cleanup   one thread per live slot: cleanup() and cleanup_measurements(t)
// No atomics, every order fixed: two runs give the same bytes.  Results reach the host through the object's own Mailbox.
#include "ovp_ctx.h"

#include <map>

#include "host/ov_plane_frame_plan.h"  // the survivor / slot replay of a fused frame (ovp_featdb_frame_commit below)
#include "k_klt_frame.h"  // FdbTable, fdb_append_one (shared with k_klt_keep_append), the database's side of ovp_klt_match_frame

namespace {

__global__ __launch_bounds__(256) void k_featdb_append(FdbTable t, int n, double stamp, const int* __restrict__ slot,
                                                       const unsigned char* __restrict__ fresh, const long long* __restrict__ ids,
                                                       const float2* __restrict__ uv, const float2* __restrict__ uvn) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  fdb_append_one(t, slot[i], fresh[i] != 0, ids[i], stamp, uv[i], uvn[i]);
}

__global__ __launch_bounds__(256) void k_featdb_mark(FdbTable t, int n, const int* __restrict__ slot) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) t.del[slot[i]] = 1;
}

// index of x among the ascending times [0, n), by exact equality of doubles; -1 when absent
__device__ __forceinline__ int fdb_find(const double* times, int n, double x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (times[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && times[lo] == x ? lo : -1;
}

struct FdbClassify {
  int n, n_clones, max_clone_size, want_marg;
  double t_now, marg_time;
  const int* slot;       // [n] the live slots in ascending feature id
  const double* clones;  // [n_clones] ascending
  long long* out_id;     // the published table
  int *out_cls, *out_count, *out_cleaned;
  unsigned char* out_flags;
  int* out_totals;  // [4] lost, marg, maxtrack, to_delete
};

__global__ __launch_bounds__(1024) void k_featdb_classify(FdbTable t, FdbClassify a) {
  __shared__ double s_clone[OVP_MAX_MEAS];
  __shared__ int s_tot[4][16];
  const int tid = threadIdx.x;
  if (tid < a.n_clones) s_clone[tid] = a.clones[tid];
  __syncthreads();
  int tot[4] = {0, 0, 0, 0};
  for (int i = tid; i < a.n; i += 1024) {
    const int s = a.slot[i], cnt = t.count[s], del = t.del[s] != 0;
    const double* ts = t.ts + (size_t)s * t.M;
    // features_not_containing_newer(t_now, false, true): no last time stamp >= t_now; to_delete is skipped
    const bool newer = cnt > 0 && ts[cnt - 1] >= a.t_now;
    bool holds = false;  // features_containing(marg_time, false, true)
    int cleaned = 0;     // clean_old_measurements(clonetimes): a time stamp that is no clone's goes
    for (int k = 0; k < cnt; ++k) {
      holds |= ts[k] == a.marg_time;
      cleaned += fdb_find(s_clone, a.n_clones, ts[k]) >= 0;
    }
    const bool marg = a.want_marg && !del && holds, lost = !del && !newer;
    // :405-415 lost and marg is marg; :418-436 marg with more than max_clone_size measurements is a maxtrack
    const int cls = marg ? (cnt > a.max_clone_size ? OVP_FEATDB_MAXTRACK : OVP_FEATDB_MARG) : lost ? OVP_FEATDB_LOST : OVP_FEATDB_NONE;
    a.out_id[i] = t.id[s];
    a.out_cls[i] = cls;
    a.out_count[i] = cnt;
    a.out_cleaned[i] = cleaned;
    a.out_flags[i] = (unsigned char)((cleaned < 2 ? 1 : 0) | (del ? 2 : 0));  // update/UpdaterMSCKF.cpp:94 ct_meas < 2
    tot[0] += cls == OVP_FEATDB_LOST, tot[1] += cls == OVP_FEATDB_MARG, tot[2] += cls == OVP_FEATDB_MAXTRACK, tot[3] += del;
  }
  // the totals: a wave's sum by shuffles, the 16 waves' by thread 0 - integers, any order gives the same
  for (int q = 0; q < 4; ++q) {
    int v = tot[q];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((tid & 63) == 0) s_tot[q][tid >> 6] = v;
  }
  __syncthreads();
  if (tid < 4) {
    int v = 0;
    for (int w = 0; w < 16; ++w) v += s_tot[tid][w];
    a.out_totals[tid] = v;
  }
}

struct FdbGather {
  int n, n_clones;
  const int *slot, *old_index;  // [n]; old_index == nullptr: the linearisation points are zero
  const double* clones;
  const double* p_old;  // the points of the batch gathered before
  float2 *uv, *uvn;     // [n][M]
  int *clone_idx, *n_meas;
  double* p;
};

// One wave per feature, a lane per stored observation (M <= 32 < 64): the survivors keep their order through a prefix count over
// the wave's ballot.
__global__ __launch_bounds__(256) void k_featdb_gather(FdbTable t, FdbGather g) {
  const int f = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (f >= g.n) return;
  const int s = g.slot[f], cnt = t.count[s], M = t.M;
  int ci = -1;
  float2 a = make_float2(0.f, 0.f), b = make_float2(0.f, 0.f);
  if (lane < cnt) {
    ci = fdb_find(g.clones, g.n_clones, t.ts[(size_t)s * M + lane]);
    a = t.uv[(size_t)s * M + lane], b = t.uvn[(size_t)s * M + lane];
  }
  const unsigned long long keep = __ballot(ci >= 0);
  const int at = __popcll(keep & ((1ull << lane) - 1ull)), kept = __popcll(keep);
  if (ci >= 0) {
    g.uv[(size_t)f * M + at] = a, g.uvn[(size_t)f * M + at] = b;
    g.clone_idx[(size_t)f * M + at] = ci;
  }
  if (lane >= kept && lane < M) {  // the padding of the row
    g.uv[(size_t)f * M + lane] = make_float2(0.f, 0.f), g.uvn[(size_t)f * M + lane] = make_float2(0.f, 0.f);
    g.clone_idx[(size_t)f * M + lane] = -1;
  }
  if (lane == 0) g.n_meas[f] = kept;
  if (lane < 3) g.p[3 * (size_t)f + lane] = g.old_index ? g.p_old[3 * (size_t)g.old_index[f] + lane] : 0.0;
}

// cleanup(): a slot whose to_delete is set is freed; cleanup_measurements(before): every observation with a time stamp < before
// goes, the others close up in stored order, and a slot left empty is freed.  before = NaN: no measurement is looked at.
__global__ __launch_bounds__(256) void k_featdb_cleanup(FdbTable t, int n, const int* __restrict__ slot, int do_cleanup, double before,
                                                        int* __restrict__ out_count, int* __restrict__ out_freed) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int s = slot[i], M = t.M;
  int cnt = t.count[s], freed = 0;
  if (do_cleanup && t.del[s]) freed = 1;
  if (!freed && before == before) {
    int w = 0;
    for (int k = 0; k < cnt; ++k) {
      const double x = t.ts[(size_t)s * M + k];
      if (x < before) continue;
      if (w != k) {
        t.ts[(size_t)s * M + w] = x;
        t.uv[(size_t)s * M + w] = t.uv[(size_t)s * M + k];
        t.uvn[(size_t)s * M + w] = t.uvn[(size_t)s * M + k];
      }
      ++w;
    }
    cnt = w;
    if (cnt == 0) freed = 1;
  }
  if (freed) cnt = 0, t.del[s] = 0;
  t.count[s] = cnt;
  out_count[i] = cnt;
  out_freed[i] = freed;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
struct FeatDb {
  int S = 0, M = 0;
  DevBuf<double> ts;
  DevBuf<float2> uv, uvn;
  DevBuf<int> count, del;
  DevBuf<long long> id;
  // the gathered batch: the ovp_feature_batch the context is bound to, its uv_norm, two sets of points (a rebuild from the
  // survivors reads the one and writes the other) and the triangulation's ok
  DevBuf<float2> g_uv, g_uvn;
  DevBuf<int> g_ci, g_nm;
  DevBuf<double> g_p[2];
  int cur = 0, g_n = -1;  // the set the batch's p_FinG is; features gathered (-1: nothing gathered yet)
  Staged stage;  // no entry waits for its tables' copy alone: Fence::Event at every site
  DevBuf<void> dres;
  Mailbox hres;
  size_t res_cap = 0;
  OvpEvent ev[2];
  bool timed = false;
  float ms = 0.f;
  // the host's shadow: id -> slot (ascending id is the order of every list), per slot the time stamps of its observations
  std::map<int64_t, int> slot_of;
  std::vector<int> free_slots;  // a stack: which slot a feature takes is a function of the call sequence alone
  std::vector<std::vector<double>> stamps;
  // the cleaned counts the last ovp_featdb_classify published, by slot, good while the table and the clone times are the same:
  // ovp_featdb_gather's argument check reads them instead of searching every time stamp again
  unsigned long long version = 0, cls_version = ~0ull;
  std::vector<double> cls_times;
  std::vector<int> cls_cleaned;
  std::vector<long long> last_cleanup;  // [id, new count, freed] per slot that was live at the last ovp_featdb_cleanup (tests)
  void forget() {
    slot_of.clear();
    free_slots.clear();
    for (int s = S - 1; s >= 0; --s) free_slots.push_back(s);
    stamps.assign(S, {});
    last_cleanup.clear();
    ++version;
    g_n = -1;
  }
  FdbTable table() const { return FdbTable{ts.get(), uv.get(), uvn.get(), count.get(), del.get(), id.get(), M}; }
  void release(int s) {
    free_slots.push_back(s);
    stamps[s].clear();
  }
};

FeatDb* db_of(ovp_ctx* c) { return c ? (FeatDb*)c->featdb.get() : nullptr; }

int publish_wait(ovp_ctx* c, FeatDb* d, size_t bytes) {
  SeqChannel& ch = d->hres.channel(0);
  const unsigned seq = ch.arm();
  HIPCHK(ovp_launch_publish_block(d->dres.get(), d->hres.dev(d->hres.payload()), bytes, ch.word_dev(), seq, 0, c->stream));
  const int rw = ch.wait(c->stream);
  if (rw) return rw;
  d->ms = 0.f;
  if (d->timed) {
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipEventElapsedTime(&d->ms, d->ev[0], d->ev[1]));
  }
  return 0;
}
int cleaned_count(const std::vector<double>& st, const double* clones, int n_clones) {
  int k = 0;
  for (double x : st) k += std::binary_search(clones, clones + n_clones, x) ? 1 : 0;
  return k;
}
bool ascending(const double* t, int n) {
  for (int k = 0; k < n; ++k)
    if (!(t[k] == t[k]) || (k > 0 && !(t[k - 1] < t[k]))) return false;
  return true;
}

}  // namespace

extern "C" int ovp_featdb_create(ovp_ctx* c, int max_slots, int max_meas) {
  if (!c || max_slots < 1 || max_slots > OVP_FEATDB_MAX_SLOTS || max_meas < 1 || max_meas > OVP_MAX_MEAS) return OVP_E_ARG;
  if (c->featdb) return OVP_E_STATE;  // one database per context: destroy the first
  HIPCHK(hipSetDevice(c->device));
  auto d = std::make_shared<FeatDb>();
  d->S = max_slots, d->M = max_meas;
  const size_t S = (size_t)max_slots, SM = S * (size_t)max_meas;
  HIPCHK(d->ts.alloc(SM));
  HIPCHK(d->uv.alloc(SM));
  HIPCHK(d->uvn.alloc(SM));
  HIPCHK(d->count.alloc(S));
  HIPCHK(d->del.alloc(S));
  HIPCHK(d->id.alloc(S));
  HIPCHK(d->g_uv.alloc(SM));
  HIPCHK(d->g_uvn.alloc(SM));
  HIPCHK(d->g_ci.alloc(SM));
  HIPCHK(d->g_nm.alloc(S));
  HIPCHK(d->g_p[0].alloc(3 * S));
  HIPCHK(d->g_p[1].alloc(3 * S));
  HIPCHK(hipMemsetAsync(d->count.get(), 0, sizeof(int) * S, c->stream));
  HIPCHK(hipMemsetAsync(d->del.get(), 0, sizeof(int) * S, c->stream));
  // staging: the largest of [slot | fresh | id | uv | uv_norm] of a frame and [slot | old index | clone times] of a gather;
  // results: the largest of the class table, the cleanup table and [points | ok]
  HIPCHK(d->stage.alloc(64 * 8 + S * (sizeof(int) + 1 + sizeof(long long) + 2 * sizeof(float2)) + sizeof(double) * OVP_MAX_MEAS));
  d->res_cap = 64 * 8 + S * (sizeof(long long) + 3 * sizeof(int) + 1 + 3 * sizeof(double)) + sizeof(int) * 4;
  HIPCHK(d->dres.alloc(d->res_cap));
  HIPCHK(d->hres.alloc(d->res_cap));
  for (OvpEvent& e : d->ev) HIPCHK(e.create());
  d->forget();
  c->featdb = d;
  return 0;
}

extern "C" int ovp_featdb_destroy(ovp_ctx* c) {
  if (!c) return OVP_E_ARG;
  FeatDb* d = db_of(c);
  if (!d) return OVP_E_STATE;
  HIPCHK(hipStreamSynchronize(c->stream));
  // a batch bound to the database's buffers goes with them
  if (c->have_batch && c->fp.uv == (const float*)d->g_uv.get()) c->have_batch = false;
  c->featdb.reset();
  return 0;
}

extern "C" int ovp_featdb_reset(ovp_ctx* c) {
  FeatDb* d = db_of(c);
  if (!d) return c ? OVP_E_STATE : OVP_E_ARG;
  d->forget();  // (a slot's device state is overwritten when a feature takes it)
  if (c->have_batch && c->fp.uv == (const float*)d->g_uv.get()) c->have_batch = false;  // the gathered batch is forgotten too
  return 0;
}

extern "C" int ovp_featdb_append(ovp_ctx* c, double timestamp, int n, const int64_t* ids, const float* uv, const float* uv_norm) {
  FeatDb* d = db_of(c);
  if (!d) return c ? OVP_E_STATE : OVP_E_ARG;
  if (n < 0 || !(timestamp == timestamp) || (n > 0 && (!ids || !uv || !uv_norm))) return OVP_E_ARG;
  if (n == 0) return 0;
  // ---- every check before anything is touched ----
  {
    std::vector<int64_t> sorted(ids, ids + n);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return OVP_E_ARG;  // the ids of a frame are distinct
  }
  size_t fresh = 0;
  for (int i = 0; i < n; ++i) {
    auto it = d->slot_of.find(ids[i]);
    if (it == d->slot_of.end()) ++fresh;
    else if ((int)d->stamps[it->second].size() >= d->M) return OVP_E_CAPACITY;
  }
  if (fresh > d->free_slots.size()) return OVP_E_CAPACITY;
  StageLayout L;
  const size_t o_slot = L.take(sizeof(int) * n), o_fresh = L.take(n), o_id = L.take(sizeof(long long) * n),
               o_uv = L.take(sizeof(float2) * n), o_uvn = L.take(sizeof(float2) * n);
  if (L.bytes() > d->stage.capacity()) return OVP_E_CAPACITY;  // (n <= S after the checks above: cannot happen)
  // ---- from here on the call goes through ----
  HIPCHK(hipSetDevice(c->device));
  int rs = 0;
  char* h = d->stage.begin(L.bytes(), &rs);
  if (!h) return rs;
  for (int i = 0; i < n; ++i) {
    auto it = d->slot_of.find(ids[i]);
    h[o_fresh + i] = it == d->slot_of.end();
    if (it == d->slot_of.end()) {
      it = d->slot_of.emplace(ids[i], d->free_slots.back()).first;
      d->free_slots.pop_back();
    }
    ((int*)(h + o_slot))[i] = it->second;
    d->stamps[it->second].push_back(timestamp);
  }
  ++d->version;
  memcpy(h + o_id, ids, sizeof(long long) * n);
  memcpy(h + o_uv, uv, sizeof(float2) * n);
  memcpy(h + o_uvn, uv_norm, sizeof(float2) * n);
  HIPCHK(d->stage.send(L.bytes(), c->stream, Fence::Event));
  const char* dv = d->stage.dev();
  if (d->timed) HIPCHK(hipEventRecord(d->ev[0], c->stream));
  hipLaunchKernelGGL(k_featdb_append, dim3((n + 255) / 256), dim3(256), 0, c->stream, d->table(), n, timestamp, (const int*)(dv + o_slot),
                     (const unsigned char*)(dv + o_fresh), (const long long*)(dv + o_id), (const float2*)(dv + o_uv),
                     (const float2*)(dv + o_uvn));
  HIPCHK(hipGetLastError());
  if (d->timed) {
    HIPCHK(hipEventRecord(d->ev[1], c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipEventElapsedTime(&d->ms, d->ev[0], d->ev[1]));
  }
  return 0;
}

// ---- the database's side of ovp_klt_match_frame (k_klt.hip): the plan in front of the enqueue, the shadow's replay behind the wait ----
int ovp_featdb_frame_plan(ovp_ctx* c, double stamp, int n, const int64_t* ids, int32_t* slot, unsigned char* fresh, int32_t* free_slots,
                          int* n_fresh, FdbTable* table) {
  FeatDb* d = db_of(c);
  if (!d) return OVP_E_STATE;
  if (!(stamp == stamp)) return OVP_E_ARG;
  int nf = 0;
  for (int i = 0; i < n; ++i) {
    auto it = d->slot_of.find(ids[i]);
    fresh[i] = it == d->slot_of.end();
    slot[i] = fresh[i] ? -1 : it->second;
    if (fresh[i]) ++nf;
    else if ((int)d->stamps[it->second].size() >= d->M) return OVP_E_CAPACITY;
  }
  if ((size_t)nf > d->free_slots.size()) return OVP_E_CAPACITY;
  for (int k = 0; k < nf; ++k) free_slots[k] = d->free_slots[d->free_slots.size() - 1 - (size_t)k];  // the stack, from its top
  *n_fresh = nf;
  *table = d->table();
  return 0;
}

void ovp_featdb_frame_commit(ovp_ctx* c, double stamp, int n, const int64_t* ids, const unsigned char* keep) {
  FeatDb* d = db_of(c);
  if (!d) return;
  std::vector<int32_t> slot(n), free_list(d->free_slots.rbegin(), d->free_slots.rend());
  std::vector<unsigned char> fresh(n);
  for (int i = 0; i < n; ++i) {
    auto it = d->slot_of.find(ids[i]);
    fresh[i] = it == d->slot_of.end();
    slot[i] = fresh[i] ? -1 : it->second;
  }
  const ov_plane::FramePlan p = ov_plane::frame_plan(n, keep, fresh.data(), slot.data(), free_list.data(), (int)free_list.size());
  for (size_t k = 0; k < p.kept_index.size(); ++k) {
    const int i = p.kept_index[k];
    if (fresh[i]) d->slot_of.emplace(ids[i], p.slot[k]);
    d->stamps[p.slot[k]].push_back(stamp);
  }
  d->free_slots.resize(d->free_slots.size() - (size_t)p.n_fresh_kept);
  if (!p.kept_index.empty()) ++d->version;  // (ovp_featdb_append of no points changes nothing either)
}

extern "C" int ovp_featdb_mark_deleted(ovp_ctx* c, int n, const int64_t* ids) {
  FeatDb* d = db_of(c);
  if (!d) return c ? OVP_E_STATE : OVP_E_ARG;
  if (n < 0 || (n > 0 && !ids)) return OVP_E_ARG;
  if (n > d->S) return OVP_E_CAPACITY;
  for (int i = 0; i < n; ++i)
    if (!d->slot_of.count(ids[i])) return OVP_E_ARG;
  if (n == 0) return 0;
  HIPCHK(hipSetDevice(c->device));
  int rs = 0;
  int* h = (int*)d->stage.begin(sizeof(int) * n, &rs);
  if (!h) return rs;
  for (int i = 0; i < n; ++i) h[i] = d->slot_of[ids[i]];
  HIPCHK(d->stage.send(sizeof(int) * n, c->stream, Fence::Event));
  hipLaunchKernelGGL(k_featdb_mark, dim3((n + 255) / 256), dim3(256), 0, c->stream, d->table(), n, (const int*)d->stage.dev());
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" void ovp_featdb_classify_defaults(ovp_featdb_classify_in* o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->max_clone_size = 11;  // StateOptions::max_clone_size
  o->want_marg = 1;
}

extern "C" int ovp_featdb_classify(ovp_ctx* c, const ovp_featdb_classify_in* in, ovp_featdb_classify_out* out) {
  FeatDb* d = db_of(c);
  if (!d) return c ? OVP_E_STATE : OVP_E_ARG;
  if (!in || !out || in->n_clones < 0 || in->n_clones > OVP_MAX_MEAS || (in->n_clones > 0 && !in->clone_times) || out->cap < 0)
    return OVP_E_ARG;
  if (!ascending(in->clone_times, in->n_clones) || !(in->t_now == in->t_now)) return OVP_E_ARG;
  const int n = (int)d->slot_of.size();
  out->n = n;
  if (n > out->cap) return OVP_E_CAPACITY;
  if (n > 0 && (!out->ids || !out->cls || !out->count || !out->cleaned || !out->flags)) return OVP_E_ARG;
  memset(out->totals, 0, sizeof(out->totals));
  if (n == 0) return 0;
  StageLayout L, R;
  const size_t o_slot = L.take(sizeof(int) * n), o_cl = L.take(sizeof(double) * OVP_MAX_MEAS);
  const size_t r_id = R.take(sizeof(long long) * n), r_cls = R.take(sizeof(int) * n), r_cnt = R.take(sizeof(int) * n),
               r_cln = R.take(sizeof(int) * n), r_fl = R.take(n), r_tot = R.take(sizeof(int) * 4);
  if (L.bytes() > d->stage.capacity() || R.bytes() > d->res_cap) return OVP_E_CAPACITY;
  HIPCHK(hipSetDevice(c->device));
  int rs = 0;
  char* h = d->stage.begin(L.bytes(), &rs);
  if (!h) return rs;
  int k = 0;
  for (const auto& e : d->slot_of) ((int*)(h + o_slot))[k++] = e.second;
  if (in->n_clones) memcpy(h + o_cl, in->clone_times, sizeof(double) * in->n_clones);
  HIPCHK(d->stage.send(L.bytes(), c->stream, Fence::Event));
  const char* dv = d->stage.dev();
  char* dr = (char*)d->dres.get();
  FdbClassify a;
  a.n = n, a.n_clones = in->n_clones, a.max_clone_size = in->max_clone_size, a.want_marg = in->want_marg != 0;
  a.t_now = in->t_now, a.marg_time = in->marg_time;
  a.slot = (const int*)(dv + o_slot), a.clones = (const double*)(dv + o_cl);
  a.out_id = (long long*)(dr + r_id), a.out_cls = (int*)(dr + r_cls), a.out_count = (int*)(dr + r_cnt);
  a.out_cleaned = (int*)(dr + r_cln), a.out_flags = (unsigned char*)(dr + r_fl), a.out_totals = (int*)(dr + r_tot);
  if (d->timed) HIPCHK(hipEventRecord(d->ev[0], c->stream));
  hipLaunchKernelGGL(k_featdb_classify, dim3(1), dim3(1024), 0, c->stream, d->table(), a);
  HIPCHK(hipGetLastError());
  if (d->timed) HIPCHK(hipEventRecord(d->ev[1], c->stream));
  const int rp = publish_wait(c, d, R.bytes());
  if (rp) return rp;
  const char* hr = (const char*)d->hres.payload();
  memcpy(out->ids, hr + r_id, sizeof(long long) * n);
  memcpy(out->cls, hr + r_cls, sizeof(int) * n);
  memcpy(out->count, hr + r_cnt, sizeof(int) * n);
  memcpy(out->cleaned, hr + r_cln, sizeof(int) * n);
  memcpy(out->flags, hr + r_fl, n);
  memcpy(out->totals, hr + r_tot, sizeof(int) * 4);
  d->cls_cleaned.assign(d->S, 0);
  k = 0;
  for (const auto& e : d->slot_of) d->cls_cleaned[e.second] = out->cleaned[k++];
  d->cls_times.assign(in->clone_times, in->clone_times + in->n_clones);
  d->cls_version = d->version;
  return 0;
}

extern "C" int ovp_featdb_gather(ovp_ctx* c, int n, const int64_t* ids, const int* old_index, const double* clone_times, int n_clones) {
  FeatDb* d = db_of(c);
  if (!d) return c ? OVP_E_STATE : OVP_E_ARG;
  if (n < 0 || n_clones < 0 || n_clones > OVP_MAX_MEAS || (n > 0 && !ids) || (n_clones > 0 && !clone_times)) return OVP_E_ARG;
  if (!ascending(clone_times, n_clones)) return OVP_E_ARG;
  if (n > d->S || n > c->f_max) return OVP_E_CAPACITY;
  if (old_index && d->g_n < 0) return OVP_E_STATE;  // no batch to carry points over from
  const bool cached = d->cls_version == d->version && (int)d->cls_times.size() == n_clones &&
                      (n_clones == 0 || !memcmp(d->cls_times.data(), clone_times, sizeof(double) * n_clones));
  for (int i = 0; i < n; ++i) {
    auto it = d->slot_of.find(ids[i]);
    if (it == d->slot_of.end()) return OVP_E_ARG;
    const int k = cached ? d->cls_cleaned[it->second] : cleaned_count(d->stamps[it->second], clone_times, n_clones);
    if (k == 0 || k > d->M) return OVP_E_ARG;  // nothing to stack; beyond the batch's pitch
    if (old_index && (old_index[i] < 0 || old_index[i] >= d->g_n)) return OVP_E_ARG;
  }
  StageLayout L;
  const size_t o_slot = L.take(sizeof(int) * n), o_old = L.take(sizeof(int) * n), o_cl = L.take(sizeof(double) * OVP_MAX_MEAS);
  if (L.bytes() > d->stage.capacity()) return OVP_E_CAPACITY;
  const int nxt = old_index ? 1 - d->cur : d->cur;
  // the context's batch is the database's buffers from here on, exactly as ovp_batch_bind_device binds a caller's - bound before
  // anything is enqueued, so that a refusal of the bind leaves the database as it was
  ovp_feature_batch b;
  b.n_feats = n, b.max_meas = d->M;
  b.uv = (const float*)d->g_uv.get(), b.clone_idx = d->g_ci.get(), b.n_meas = d->g_nm.get(), b.p_FinG = d->g_p[nxt].get();
  const int rb = ovp_batch_bind_device(c, &b);
  if (rb) return rb;
  HIPCHK(hipSetDevice(c->device));
  if (n > 0) {
    int rs = 0;
    char* h = d->stage.begin(L.bytes(), &rs);
    if (!h) return rs;
    for (int i = 0; i < n; ++i) ((int*)(h + o_slot))[i] = d->slot_of[ids[i]];
    if (old_index) memcpy(h + o_old, old_index, sizeof(int) * n);
    if (n_clones) memcpy(h + o_cl, clone_times, sizeof(double) * n_clones);
    HIPCHK(d->stage.send(L.bytes(), c->stream, Fence::Event));
    const char* dv = d->stage.dev();
    FdbGather g;
    g.n = n, g.n_clones = n_clones;
    g.slot = (const int*)(dv + o_slot), g.old_index = old_index ? (const int*)(dv + o_old) : nullptr;
    g.clones = (const double*)(dv + o_cl);
    g.p_old = d->g_p[d->cur].get();
    g.uv = d->g_uv.get(), g.uvn = d->g_uvn.get(), g.clone_idx = d->g_ci.get(), g.n_meas = d->g_nm.get(), g.p = d->g_p[nxt].get();
    if (d->timed) HIPCHK(hipEventRecord(d->ev[0], c->stream));
    hipLaunchKernelGGL(k_featdb_gather, dim3((n + 3) / 4), dim3(256), 0, c->stream, d->table(), g);
    HIPCHK(hipGetLastError());
    if (d->timed) {
      HIPCHK(hipEventRecord(d->ev[1], c->stream));
      HIPCHK(hipStreamSynchronize(c->stream));
      HIPCHK(hipEventElapsedTime(&d->ms, d->ev[0], d->ev[1]));
    }
  }
  d->cur = nxt;
  d->g_n = n;
  return 0;
}

extern "C" int ovp_featdb_triangulate(ovp_ctx* c, const ovp_triang_opts* o, double* p_FinG_out, uint8_t* ok) {
  FeatDb* d = db_of(c);
  if (!d) return c ? OVP_E_STATE : OVP_E_ARG;
  if (!o || !ok) return OVP_E_ARG;
  // the batch the context holds must be the gathered one
  if (!c->have_state || !c->have_batch || d->g_n < 0 || c->fp.uv != (const float*)d->g_uv.get() || c->n_feats != d->g_n) return OVP_E_STATE;
  const size_t F = (size_t)d->g_n;
  if (F == 0) return 0;
  StageLayout R;
  const size_t r_p = R.take(sizeof(double) * 3 * F), r_ok = R.take(F);
  if (R.bytes() > d->res_cap) return OVP_E_CAPACITY;
  HIPCHK(hipSetDevice(c->device));
  char* dr = (char*)d->dres.get();
  ovp::TriParams tp;
  tp.uvn = (const float*)d->g_uvn.get();
  tp.clone_idx = c->fp.clone_idx;
  tp.n_meas = c->fp.n_meas;
  tp.n_feats = (int)F;
  tp.max_meas = d->M;
  fill_tri_params(tp, c, o);
  tp.p_FinG = d->g_p[d->cur].get();  // the positions become the batch's linearisation points, where the batch's p_FinG already is
  tp.ok = (unsigned char*)dr + r_ok;
  if (d->timed) HIPCHK(hipEventRecord(d->ev[0], c->stream));
  HIPCHK(ovp_launch_triangulate(&tp, c->stream));
  if (d->timed) HIPCHK(hipEventRecord(d->ev[1], c->stream));
  HIPCHK(hipMemcpyAsync(dr + r_p, tp.p_FinG, sizeof(double) * 3 * F, hipMemcpyDeviceToDevice, c->stream));
  const int rp = publish_wait(c, d, R.bytes());
  if (rp) return rp;
  const char* hr = (const char*)d->hres.payload();
  if (p_FinG_out) memcpy(p_FinG_out, hr + r_p, sizeof(double) * 3 * F);
  memcpy(ok, hr + r_ok, F);
  return 0;
}

extern "C" int ovp_featdb_cleanup(ovp_ctx* c, int do_cleanup, double measurements_before_or_nan) {
  FeatDb* d = db_of(c);
  if (!d) return c ? OVP_E_STATE : OVP_E_ARG;
  d->last_cleanup.clear();
  const int n = (int)d->slot_of.size();
  const bool by_time = measurements_before_or_nan == measurements_before_or_nan;
  if (n == 0 || (!do_cleanup && !by_time)) return 0;
  StageLayout L, R;
  L.take(sizeof(int) * n);
  const size_t r_cnt = R.take(sizeof(int) * n), r_fr = R.take(sizeof(int) * n);
  if (L.bytes() > d->stage.capacity() || R.bytes() > d->res_cap) return OVP_E_CAPACITY;
  HIPCHK(hipSetDevice(c->device));
  int rs = 0;
  int* h = (int*)d->stage.begin(L.bytes(), &rs);
  if (!h) return rs;
  int k = 0;
  for (const auto& e : d->slot_of) h[k++] = e.second;
  HIPCHK(d->stage.send(L.bytes(), c->stream, Fence::Event));
  char* dr = (char*)d->dres.get();
  if (d->timed) HIPCHK(hipEventRecord(d->ev[0], c->stream));
  hipLaunchKernelGGL(k_featdb_cleanup, dim3((n + 255) / 256), dim3(256), 0, c->stream, d->table(), n, (const int*)d->stage.dev(),
                     do_cleanup ? 1 : 0, measurements_before_or_nan, (int*)(dr + r_cnt), (int*)(dr + r_fr));
  HIPCHK(hipGetLastError());
  if (d->timed) HIPCHK(hipEventRecord(d->ev[1], c->stream));
  const int rp = publish_wait(c, d, R.bytes());
  if (rp) return rp;
  ++d->version;
  // the host's map and shadow follow what the device published
  const int* cnt = (const int*)((const char*)d->hres.payload() + r_cnt);
  const int* fr = (const int*)((const char*)d->hres.payload() + r_fr);
  int i = 0;
  for (auto it = d->slot_of.begin(); it != d->slot_of.end(); ++i) {
    d->last_cleanup.insert(d->last_cleanup.end(), {(long long)it->first, (long long)cnt[i], (long long)fr[i]});
    std::vector<double>& st = d->stamps[it->second];
    if (by_time && !fr[i]) st.erase(std::remove_if(st.begin(), st.end(), [&](double x) { return x < measurements_before_or_nan; }), st.end());
    if (!fr[i] && (int)st.size() != cnt[i]) return OVP_E_STATE;  // (the shadow and the table disagree: never met)
    if (fr[i]) {
      d->release(it->second);
      it = d->slot_of.erase(it);
    } else
      ++it;
  }
  return 0;
}

extern "C" int ovp_featdb_get(ovp_ctx* c, int64_t id, int* slot, int* count, int* to_delete, double* timestamps, float* uv, float* uv_norm,
                              int cap) {
  FeatDb* d = db_of(c);
  if (!d) return c ? OVP_E_STATE : OVP_E_ARG;
  if (!count || cap < 0) return OVP_E_ARG;
  *count = -1;  // get_feature returns nullptr
  if (slot) *slot = -1;
  auto it = d->slot_of.find(id);
  if (it == d->slot_of.end()) return 0;
  const int s = it->second;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  int cnt = 0, del = 0;
  HIPCHK(hipMemcpy(&cnt, d->count.get() + s, sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(&del, d->del.get() + s, sizeof(int), hipMemcpyDeviceToHost));
  if (cnt < 0 || cnt > d->M) return OVP_E_STATE;
  *count = cnt;
  if (slot) *slot = s;
  if (to_delete) *to_delete = del;
  const int k = std::min(cnt, cap);
  const size_t at = (size_t)s * d->M;
  if (k > 0 && timestamps) HIPCHK(hipMemcpy(timestamps, d->ts.get() + at, sizeof(double) * k, hipMemcpyDeviceToHost));
  if (k > 0 && uv) HIPCHK(hipMemcpy(uv, d->uv.get() + at, sizeof(float2) * k, hipMemcpyDeviceToHost));
  if (k > 0 && uv_norm) HIPCHK(hipMemcpy(uv_norm, d->uvn.get() + at, sizeof(float2) * k, hipMemcpyDeviceToHost));
  return 0;
}

extern "C" long ovp_featdb_debug(ovp_ctx* c, const char* what, int level, void* out, long cap) {
  FeatDb* d = db_of(c);
  if (!d) return c ? OVP_E_STATE : OVP_E_ARG;
  if (!what || cap < 0) return OVP_E_ARG;
  if (!strcmp(what, "timer")) {
    d->timed = level != 0;
    return 0;
  }
  if (!out) return OVP_E_ARG;
  if (!strcmp(what, "time")) {
    if (cap < (long)sizeof(float)) return OVP_E_ARG;
    memcpy(out, &d->ms, sizeof(float));
    return sizeof(float);
  }
  if (!strcmp(what, "dims")) {
    const int v[4] = {d->S, d->M, (int)d->slot_of.size(), d->g_n};
    if (cap < (long)sizeof(v)) return OVP_E_ARG;
    memcpy(out, v, sizeof(v));
    return sizeof(v);
  }
  if (!strcmp(what, "cleanup")) {
    const size_t b = sizeof(long long) * d->last_cleanup.size();
    if ((long)b > cap) return OVP_E_ARG;
    if (b) memcpy(out, d->last_cleanup.data(), b);
    return (long)b;
  }
  if (d->g_n < 0) return OVP_E_STATE;
  const size_t F = (size_t)d->g_n, M = (size_t)d->M;
  const void* src = nullptr;
  size_t bytes = 0;
  if (!strcmp(what, "uv")) src = d->g_uv.get(), bytes = sizeof(float2) * F * M;
  else if (!strcmp(what, "uv_norm")) src = d->g_uvn.get(), bytes = sizeof(float2) * F * M;
  else if (!strcmp(what, "clone_idx")) src = d->g_ci.get(), bytes = sizeof(int) * F * M;
  else if (!strcmp(what, "n_meas")) src = d->g_nm.get(), bytes = sizeof(int) * F;
  else if (!strcmp(what, "p_FinG")) src = d->g_p[d->cur].get(), bytes = sizeof(double) * 3 * F;
  else return OVP_E_ARG;
  if ((long)bytes > cap) return OVP_E_ARG;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (bytes) HIPCHK(hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost));
  return (long)bytes;
}
