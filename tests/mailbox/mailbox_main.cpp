// Stand-alone check of csrc/ovp_mailbox.h (tests/test_mailbox_cpu.py builds it with -fsanitize=address,undefined and once more with
// -fsanitize=thread, and runs it).  The HIP allocation calls are defined here over malloc; g_fail_at makes the k-th allocation from
// now on fail.  A std::thread plays the device: it writes the payload, then stores the sequence word with release order.
#include "ovp_mailbox.h"

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>

static int g_allocs = 0, g_frees = 0, g_fail_at = 0, g_syncs = 0;  // g_fail_at: 1-based countdown, 0 = never
static hipError_t fake_alloc(void** p, size_t bytes) {
  if (g_fail_at > 0 && --g_fail_at == 0) {
    *p = nullptr;
    return hipErrorOutOfMemory;
  }
  *p = malloc(bytes ? bytes : 1);
  memset(*p, 0xA5, bytes);  // (hipHostMalloc promises nothing about the contents: the mailbox clears them itself)
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
hipError_t hipStreamSynchronize(hipStream_t) {
  ++g_syncs;
  return hipSuccess;
}

#define REQUIRE(x)                                               \
  do {                                                           \
    if (!(x)) {                                                  \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x);    \
      exit(1);                                                   \
    }                                                            \
  } while (0)

static long long pin_bytes() { return ovp_live_bytes().pinned.load(); }
static const std::chrono::milliseconds kShort(20);

// the device's side of a publication: payload, then the word
static void device_post(unsigned char* dst, size_t bytes, unsigned char fill, unsigned* word, unsigned seq, unsigned aux) {
  for (size_t i = 0; i < bytes; ++i) dst[i] = fill;
  word[1] = aux;
  __atomic_store_n(word, seq, __ATOMIC_RELEASE);
}

int main() {
  {
    Mailbox m;
    REQUIRE(!m && m.payload() == nullptr && m.payload_capacity() == 0 && m.capacity() == 0);
    REQUIRE(m.alloc(1000) == hipSuccess);
    // whole lines of payload, one line of channels behind them, all of it zero
    REQUIRE(m.payload_capacity() == 1024 && m.capacity() == 1024 + Mailbox::LINE && pin_bytes() == 1088);
    const unsigned char* p = (const unsigned char*)m.payload();
    for (size_t i = 0; i < m.capacity(); ++i) REQUIRE(p[i] == 0);
    for (int k = 0; k < Mailbox::CHANNELS; ++k) {
      REQUIRE((char*)m.channel(k).word_dev() == (char*)m.payload() + 1024 + 16 * k);
      REQUIRE(m.channel(k).armed() == 0);
    }
    REQUIRE(m.dev(p + 40) == (void*)(p + 40));
    REQUIRE(m.alloc(5000) == hipSuccess && m.payload_capacity() == 1024);  // alloc on a live mailbox: nothing

    // (a) wait returns 0 only after the payload is visible, several rounds on one channel
    SeqChannel& ch = m.channel(0);
    for (int round = 1; round <= 50; ++round) {
      const unsigned seq = ch.arm();
      REQUIRE(seq == (unsigned)round);
      std::thread dev(device_post, (unsigned char*)m.payload(), (size_t)1024, (unsigned char)round, ch.word_dev(), seq, 7u * round);
      REQUIRE(ch.wait(nullptr) == 0);
      for (size_t i = 0; i < 1024; ++i) REQUIRE(p[i] == (unsigned char)round);
      REQUIRE(ch.aux() == 7u * round);
      dev.join();
    }
    REQUIRE(g_syncs == 0);

    // (d) two channels of one line advance independently
    SeqChannel& c1 = m.channel(1);
    REQUIRE(c1.armed() == 0 && ch.armed() == 50);
    const unsigned s1 = c1.arm();
    REQUIRE(s1 == 1 && ch.armed() == 50);
    REQUIRE(ch.wait(nullptr, kShort) == 0);  // channel 0's last number is still posted
    {
      std::thread dev(device_post, (unsigned char*)m.payload(), (size_t)8, (unsigned char)1, c1.word_dev(), s1, 1u);
      REQUIRE(c1.wait(nullptr) == 0 && c1.aux() == 1u);
      dev.join();
    }
    const unsigned s0 = ch.arm();
    REQUIRE(s0 == 51 && c1.armed() == 1);
    REQUIRE(c1.wait(nullptr, kShort) == 0);  // and channel 1 is not disturbed by arming channel 0

    // (e) a word that never comes: one stream synchronisation, then OVP_E_STATE
    const int syncs0 = g_syncs;
    const auto t0 = std::chrono::steady_clock::now();
    REQUIRE(ch.wait(nullptr, kShort) == OVP_E_STATE);
    REQUIRE(g_syncs == syncs0 + 1 && std::chrono::steady_clock::now() - t0 >= kShort);
    __atomic_store_n(ch.word_dev(), s0, __ATOMIC_RELEASE);
    REQUIRE(ch.wait(nullptr, kShort) == 0);
  }
  REQUIRE(pin_bytes() == 0 && g_allocs == g_frees);
  {
    // (b) a payload filled with the value of the NEXT sequence number, at every offset, of a block that is first large and then
    // small, never satisfies a wait (what the sites used to guard by clearing the word before every launch)
    Mailbox m;
    REQUIRE(m.reserve(700, 0) == hipSuccess && m.payload_capacity() == 704);
    SeqChannel& ch = m.channel(0);
    for (size_t bytes : {m.payload_capacity(), (size_t)64, (size_t)4}) {
      const unsigned next = ch.armed() + 1;
      unsigned* w = (unsigned*)m.payload();
      for (size_t i = 0; i < bytes / 4; ++i) w[i] = next;  // (an earlier call's payload: no word of it is the channel's)
      REQUIRE(ch.arm() == next);
      REQUIRE(ch.wait(nullptr, kShort) == OVP_E_STATE);
      std::thread dev(device_post, (unsigned char*)m.payload(), bytes, (unsigned char)0xFF, ch.word_dev(), next, 0u);
      REQUIRE(ch.wait(nullptr) == 0);
      dev.join();
    }

    // (c) a growth rebinds every channel, zero-fills the new block and keeps the counters
    REQUIRE(m.reserve(704, 4096) == hipSuccess && m.payload_capacity() == 704);  // at or below the capacity: nothing
    const unsigned last0 = ch.armed();
    const unsigned last2 = (m.channel(2).arm(), m.channel(2).arm());
    REQUIRE(m.reserve(705, 100) == hipSuccess);
    REQUIRE(m.payload_capacity() == 832 && m.capacity() == 896 && pin_bytes() == 896);
    const unsigned char* p = (const unsigned char*)m.payload();
    for (size_t i = 0; i < m.capacity(); ++i) REQUIRE(p[i] == 0);
    for (int k = 0; k < Mailbox::CHANNELS; ++k) REQUIRE((char*)m.channel(k).word_dev() == (char*)m.payload() + 832 + 16 * k);
    REQUIRE(ch.armed() == last0 && m.channel(2).armed() == last2 && last2 == 2);
    // (the zeroed word is not the number the channel waits for next)
    const unsigned seq = ch.arm();
    REQUIRE(ch.wait(nullptr, kShort) == OVP_E_STATE);
    std::thread dev(device_post, (unsigned char*)m.payload(), m.payload_capacity(), (unsigned char)3, ch.word_dev(), seq, 0u);
    REQUIRE(ch.wait(nullptr) == 0);
    dev.join();

    // (f) a failed allocation leaves the mailbox empty and releases everything; the next one works and the counters are still there
    const int frees0 = g_frees;
    g_fail_at = 1;
    REQUIRE(m.reserve(5000, 0) == hipErrorOutOfMemory);
    REQUIRE(!m && m.payload() == nullptr && m.payload_capacity() == 0 && m.capacity() == 0 && pin_bytes() == 0 && g_frees == frees0 + 1);
    for (int k = 0; k < Mailbox::CHANNELS; ++k) REQUIRE(m.channel(k).word_dev() == nullptr);
    REQUIRE(m.reserve(5000, 0) == hipSuccess && m.payload_capacity() == 5056 && ch.armed() == seq);
    ((unsigned char*)m.payload())[5055] = 1;  // (the sanitizer checks the size)
  }
  REQUIRE(pin_bytes() == 0 && g_allocs == g_frees);
  puts("ok");
  return 0;
}
