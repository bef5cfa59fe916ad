// Stand-alone check of csrc/ovp_staged.h (tests/test_staged_cpu.py builds it with -fsanitize=address,undefined and runs it).  The HIP
// calls the header needs are defined here: allocation over malloc (g_fail_at makes the k-th allocation from now on fail), and a
// stream that is a queue - hipMemcpyAsync only queues the copy, hipEventSynchronize / hipStreamSynchronize run the queue and count
// their calls.  So a host write that comes before the copy has run reaches the "device" block and is seen there.
#include "ovp_staged.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

static int g_allocs = 0, g_frees = 0, g_fail_at = 0;  // g_fail_at: 1-based countdown, 0 = never
static int g_ev_syncs = 0, g_stream_syncs = 0, g_ev_created = 0, g_ev_destroyed = 0, g_ev_records = 0;
static hipStream_t g_last_synced = nullptr;
static int g_frees_at_last_sync = -1;
struct Copy { void* dst; const void* src; size_t bytes; };
static std::vector<Copy> g_queue;
static void run_queue() {
  for (const Copy& c : g_queue) memcpy(c.dst, c.src, c.bytes);
  g_queue.clear();
}

static hipError_t fake_alloc(void** p, size_t bytes) {
  if (g_fail_at > 0 && --g_fail_at == 0) {
    *p = nullptr;
    return hipErrorOutOfMemory;
  }
  *p = malloc(bytes ? bytes : 1);
  memset(*p, 0xA5, bytes);
  ++g_allocs;
  return hipSuccess;
}
hipError_t hipMalloc(void** p, size_t bytes) { return fake_alloc(p, bytes); }
hipError_t hipFree(void* p) {
  free(p);
  ++g_frees;
  return hipSuccess;
}
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int) { return fake_alloc(p, bytes); }
hipError_t hipHostFree(void* p) {
  free(p);
  ++g_frees;
  return hipSuccess;
}
hipError_t hipHostGetDevicePointer(void** d, void* h, unsigned int) {
  *d = h;
  return hipSuccess;
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind, hipStream_t) {
  g_queue.push_back({dst, src, bytes});
  return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s) {
  ++g_stream_syncs;
  g_last_synced = s;
  g_frees_at_last_sync = g_frees;
  run_queue();
  return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) {
  *e = (hipEvent_t)malloc(1);
  ++g_ev_created;
  return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) {
  free((void*)e);
  ++g_ev_destroyed;
  return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t, hipStream_t) {
  ++g_ev_records;
  return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t) {
  ++g_ev_syncs;
  run_queue();
  return hipSuccess;
}

#define REQUIRE(x)                                               \
  do {                                                           \
    if (!(x)) {                                                  \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x);    \
      exit(1);                                                   \
    }                                                            \
  } while (0)

static long long live() { return ovp_live_bytes().pinned.load() + ovp_live_bytes().device.load(); }
static bool all_are(const char* p, size_t n, char v) {
  for (size_t i = 0; i < n; ++i)
    if (p[i] != v) return false;
  return true;
}
static hipStream_t const kStream = (hipStream_t)0x10, kOther = (hipStream_t)0x20;

int main() {
  const size_t N = 256;
  int rc = -1;
  {  // ---- event fence: two rounds with different fills ----
    Staged st;
    REQUIRE(st.dev() == nullptr && st.capacity() == 0);
    REQUIRE(st.alloc(N) == hipSuccess && st.capacity() == N && live() == 2 * (long long)N);
    REQUIRE(st.alloc(4 * N) == hipSuccess && st.capacity() == N);  // alloc on a live block: nothing
    char* h = st.begin(N, &rc);
    REQUIRE(h && rc == 0 && h == st.host() && g_ev_syncs == 0 && g_stream_syncs == 0);  // nothing to wait for in the first begin
    memset(h, 1, N);
    REQUIRE(st.send(N, kStream, Fence::Event) == hipSuccess && g_ev_created == 1 && g_ev_records == 1);
    h = st.begin(N, &rc);
    REQUIRE(h && rc == 0 && g_ev_syncs == 1 && g_stream_syncs == 0);  // exactly one event synchronisation inside the second begin
    memset(h, 2, N);
    REQUIRE(all_are(st.dev(), N, 1));  // the first fill arrived before the host wrote the second
    REQUIRE(st.send(N, kStream, Fence::Event) == hipSuccess && g_ev_created == 1 && g_ev_records == 2);  // one event, recorded again
    REQUIRE(all_are(st.dev(), N, 1));
    REQUIRE(hipStreamSynchronize(kStream) == hipSuccess);
    REQUIRE(all_are(st.dev(), N, 2));

    // ---- caller-waits fence with done(): no synchronisation of any kind inside the next begin ----
    const int ev0 = g_ev_syncs, ss0 = g_stream_syncs, rec0 = g_ev_records;
    st.done();  // (the synchronisation above stood behind the copy)
    h = st.begin(N, &rc);
    memset(h, 3, N);
    REQUIRE(st.send(N / 2, kStream, Fence::CallerWaits) == hipSuccess && g_ev_records == rec0);  // records nothing
    REQUIRE(hipStreamSynchronize(kStream) == hipSuccess);  // the caller's own wait
    st.done();
    REQUIRE(all_are(st.dev(), N / 2, 3) && all_are(st.dev() + N / 2, N / 2, 2));  // the first `bytes` bytes, no more
    h = st.begin(N, &rc);
    REQUIRE(h && g_ev_syncs == ev0 && g_stream_syncs == ss0 + 1);

    // ---- caller-waits fence without done() (a call that left early): the next begin synchronises the stored stream once ----
    memset(h, 4, N);
    REQUIRE(st.send(N, kOther, Fence::CallerWaits) == hipSuccess);
    g_last_synced = nullptr;
    h = st.begin(N, &rc);
    REQUIRE(h && rc == 0 && g_stream_syncs == ss0 + 2 && g_ev_syncs == ev0 && g_last_synced == kOther);
    memset(h, 5, N);
    REQUIRE(all_are(st.dev(), N, 4));  // the first fill arrived intact
    h = st.begin(N, &rc);
    REQUIRE(h && g_stream_syncs == ss0 + 2);  // and the fence is idle behind it

    // ---- begin above the capacity: OVP_E_CAPACITY, pinned bytes untouched, fence state unchanged ----
    memset(h, 6, N);
    REQUIRE(st.send(N, kStream, Fence::CallerWaits) == hipSuccess);
    const int ss1 = g_stream_syncs;
    rc = 0;
    REQUIRE(st.begin(N + 1, &rc) == nullptr && rc == OVP_E_CAPACITY);
    REQUIRE(g_stream_syncs == ss1 && g_ev_syncs == ev0 && !st.fence().idle() && all_are(st.host(), N, 6));
    REQUIRE(all_are(st.dev(), N, 4));  // (the copy is still queued)

    // ---- reserve: nothing at or below the capacity; a growth synchronises the given stream before it frees anything ----
    REQUIRE(st.reserve(N, 4096, kStream) == hipSuccess && st.capacity() == N && g_stream_syncs == ss1);
    st.done();
    g_queue.clear();
    const int frees0 = g_frees;
    REQUIRE(st.reserve(N + 1, 100, kOther) == hipSuccess);
    REQUIRE(g_stream_syncs == ss1 + 1 && g_last_synced == kOther && g_frees_at_last_sync == frees0 && g_frees == frees0 + 2);
    REQUIRE(st.capacity() == N + 101 && live() == 2 * (long long)(N + 101) && st.fence().idle());  // one capacity, both halves
    h = st.begin(N + 101, &rc);
    REQUIRE(h && rc == 0);
    memset(h, 7, N + 101);  // (the sanitizer checks both sizes)
    REQUIRE(st.send(N + 101, kStream, Fence::CallerWaits) == hipSuccess && hipStreamSynchronize(kStream) == hipSuccess);
    st.done();
    REQUIRE(all_are(st.dev(), N + 101, 7));

    // ---- either allocation failing during reserve: both halves empty, every byte given back, and the next reserve works ----
    for (int at = 1; at <= 2; ++at) {
      g_fail_at = at;
      REQUIRE(st.reserve(st.capacity() + 1, 0, kStream) == hipErrorOutOfMemory);
      REQUIRE(st.dev() == nullptr && st.host() == nullptr && st.capacity() == 0 && live() == 0 && st.fence().idle() && g_allocs == g_frees);
      rc = 0;
      REQUIRE(st.begin(1, &rc) == nullptr && rc == OVP_E_CAPACITY);
      REQUIRE(st.reserve(1000, 24, kStream) == hipSuccess && st.capacity() == 1024 && live() == 2048);
    }
  }
  REQUIRE(live() == 0 && g_allocs == g_frees && g_ev_created == 1 && g_ev_destroyed == 1);
  {  // ---- OvpEvent: create twice makes one event, a move leaves the source empty, creates equal destroys at exit ----
    OvpEvent a;
    REQUIRE((hipEvent_t)a == nullptr);
    REQUIRE(a.create() == hipSuccess && a.create(hipEventDisableTiming) == hipSuccess && g_ev_created == 2);
    const hipEvent_t raw = a;
    OvpEvent b(std::move(a));
    REQUIRE((hipEvent_t)a == nullptr && (hipEvent_t)b == raw && g_ev_destroyed == 1);
    OvpEvent c;
    REQUIRE(c.create() == hipSuccess && g_ev_created == 3);
    c = std::move(b);  // (the target's own event goes)
    REQUIRE((hipEvent_t)b == nullptr && (hipEvent_t)c == raw && g_ev_destroyed == 2);
    std::vector<OvpEvent> v(3);
    for (OvpEvent& e : v) REQUIRE(e.create() == hipSuccess);
    v.resize(8);  // (what the kernel timers' lists do: the events move with their owners)
    REQUIRE(g_ev_created == 6 && g_ev_destroyed == 2);
  }
  REQUIRE(g_ev_created == g_ev_destroyed && g_ev_created == 6);
  puts("ok");
  return 0;
}
