// Stand-alone check of csrc/ovp_buf.h (tests/test_ctx_buffers_cpu.py builds it with -fsanitize=address,undefined and runs it).
// The five HIP allocation calls are defined here over malloc; g_fail_at makes the k-th allocation from now on fail.
#include "ovp_buf.h"

#include <cstdio>
#include <cstdlib>

static int g_allocs = 0, g_frees = 0, g_fail_at = 0;  // g_fail_at: 1-based countdown, 0 = never
static hipError_t fake_alloc(void** p, size_t bytes) {
  if (g_fail_at > 0 && --g_fail_at == 0) {
    *p = nullptr;
    return hipErrorOutOfMemory;
  }
  *p = malloc(bytes ? bytes : 1);
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

#define REQUIRE(x)                                               \
  do {                                                           \
    if (!(x)) {                                                  \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x);    \
      exit(1);                                                   \
    }                                                            \
  } while (0)

static long long dev_bytes() { return ovp_live_bytes().device.load(); }
static long long pin_bytes() { return ovp_live_bytes().pinned.load(); }

struct Five {
  DevBuf<double> a, b, c;
  PinnedBuf<int> d{true};
  DevBuf<void> e;
  hipError_t fill() {
    if (hipError_t r = a.alloc(10)) return r;
    if (hipError_t r = b.alloc(20)) return r;
    if (hipError_t r = c.alloc(30)) return r;
    if (hipError_t r = d.alloc(40)) return r;
    return e.alloc(50);
  }
};

int main() {
  {
    DevBuf<double> b;
    REQUIRE(b.get() == nullptr && b.capacity() == 0 && !b);
    REQUIRE(b.reserve(100, 64) == hipSuccess);  // above the capacity: count + slack
    REQUIRE(b.capacity() == 164 && dev_bytes() == 164 * 8);
    double* p0 = b;
    p0[163] = 1.0;  // (the sanitizer checks the size)
    REQUIRE(b.reserve(164, 64) == hipSuccess && b.get() == p0 && b.capacity() == 164);  // at or below it: the pointer stays
    REQUIRE(b.reserve(10, 0) == hipSuccess && b.get() == p0);
    REQUIRE(b.alloc(5000) == hipSuccess && b.get() == p0 && b.capacity() == 164);  // alloc on a live buffer: nothing
    // a failed growth leaves the buffer empty, the next one works, destruction frees once
    const int frees0 = g_frees;
    g_fail_at = 1;
    REQUIRE(b.reserve(1000, 64) == hipErrorOutOfMemory);
    REQUIRE(b.get() == nullptr && b.capacity() == 0 && dev_bytes() == 0 && g_frees == frees0 + 1);
    REQUIRE(b.reserve(1000, 64) == hipSuccess && b.capacity() == 1064 && dev_bytes() == 1064 * 8);
    ((double*)b)[1063] = 2.0;
    // move and swap carry pointer and capacity
    double* p1 = b;
    DevBuf<double> m(std::move(b));
    REQUIRE(b.get() == nullptr && b.capacity() == 0 && m.get() == p1 && m.capacity() == 1064);
    DevBuf<double> o;
    REQUIRE(o.alloc(7) == hipSuccess);
    double* p2 = o;
    m.swap(o);
    REQUIRE(m.get() == p2 && m.capacity() == 7 && o.get() == p1 && o.capacity() == 1064);
    o = std::move(m);  // frees o's block, takes m's
    REQUIRE(o.get() == p2 && o.capacity() == 7 && m.get() == nullptr && dev_bytes() == 7 * 8);
    REQUIRE(g_frees == frees0 + 2);
  }
  REQUIRE(dev_bytes() == 0 && g_allocs == g_frees);
  {
    PinnedBuf<int> h(true), plain;
    REQUIRE(h.alloc(16) == hipSuccess && h.dev() == h.get() && h.capacity() == 16 && pin_bytes() == 64);
    REQUIRE(plain.reserve(8, 8) == hipSuccess && plain.dev() == nullptr && plain.capacity() == 16 && pin_bytes() == 128);
    g_fail_at = 1;
    REQUIRE(plain.reserve(100, 0) == hipErrorOutOfMemory && plain.get() == nullptr && plain.capacity() == 0 && pin_bytes() == 64);
    int* p = h;
    PinnedBuf<int> m(std::move(h));
    REQUIRE(m.get() == p && m.dev() == p && m.capacity() == 16 && h.get() == nullptr && h.dev() == nullptr);
    m.swap(plain);
    REQUIRE(plain.get() == p && plain.dev() == p && m.get() == nullptr);
    REQUIRE(m.alloc(4) == hipSuccess && m.dev() == nullptr);  // (the flag travelled with the block)
    DevBuf<void> bytes;
    REQUIRE(bytes.reserve(100, 28) == hipSuccess && bytes.capacity() == 128 && dev_bytes() == 128);
    ((char*)bytes)[127] = 1;
  }
  REQUIRE(dev_bytes() == 0 && pin_bytes() == 0 && g_allocs == g_frees);
  {
    // five buffers, the third allocation fails: the first two go with the struct
    const int a0 = g_allocs, f0 = g_frees;
    {
      Five f;
      g_fail_at = 3;
      REQUIRE(f.fill() == hipErrorOutOfMemory);
      REQUIRE(f.a && f.b && !f.c && !f.d && !f.e && g_allocs == a0 + 2 && dev_bytes() == 30 * 8);
    }
    REQUIRE(g_frees == f0 + 2);
    Five ok;
    REQUIRE(ok.fill() == hipSuccess && dev_bytes() == 60 * 8 + 50 && pin_bytes() == 160);
  }
  REQUIRE(dev_bytes() == 0 && pin_bytes() == 0 && g_allocs == g_frees);
  puts("ok");
  return 0;
}
