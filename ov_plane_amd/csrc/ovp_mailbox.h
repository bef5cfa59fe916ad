// How a handful of results reaches the host without a copy command (host only, beside ovp_buf.h): the last kernel of an entry point
// writes its payload into mapped pinned memory, fences, and stores a sequence number; the host spins on that word.
//   SeqChannel  one sequence word, the auxiliary word beside it, and the word's counter
//   Mailbox     a mapped pinned block [payload | one 64-byte line of up to four channels]
// THE INVARIANT, stated here once: the last 64-byte line of a Mailbox is never payload and keeps its place for the life of the
// block, and a channel's word is written by the kernels it was armed for and by nobody else.  New memory is zero and a counter only
// ever goes up, so a word holds a number its channel has already handed out - never the next one: no site clears a word.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>

#include "ovp_buf.h"
#include "ovplane_hip.h"

// Wait for the sequence number a kernel on stream s writes into mapped pinned memory behind its payload.  Error path: after the
// bound (two seconds in the library) one stream synchronisation surfaces a fault instead of spinning forever, OVP_E_STATE when the
// word still is not there.
static inline int ovp_wait_seq(const volatile unsigned* word, unsigned seq, hipStream_t s,
                               std::chrono::nanoseconds bound = std::chrono::seconds(2)) {
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned spins = 0; __atomic_load_n((const unsigned*)word, __ATOMIC_ACQUIRE) != seq; __builtin_ia32_pause())
    if ((++spins & 0xFFFu) == 0 && std::chrono::steady_clock::now() - t0 > bound) {
      const hipError_t e = hipStreamSynchronize(s);
      if (e != hipSuccess) return (int)e;
      return __atomic_load_n((const unsigned*)word, __ATOMIC_ACQUIRE) != seq ? OVP_E_STATE : 0;
    }
  return 0;
}

class SeqChannel {
 public:
  static constexpr size_t BYTES = 16;  // [sequence word | auxiliary word | -, -]
  unsigned arm() { return ++last_; }   // the number the next publishing kernel stores
  unsigned armed() const { return last_; }
  unsigned* word_dev() const { return dev_; }  // what that kernel stores it through
  int wait(hipStream_t s, std::chrono::nanoseconds bound = std::chrono::seconds(2)) const { return ovp_wait_seq(host_, last_, s, bound); }
  unsigned aux() const { return host_[1]; }  // written in front of the sequence word by the kernel that posts it (read behind wait)

 private:
  friend class Mailbox;
  volatile unsigned* host_ = nullptr;
  unsigned* dev_ = nullptr;
  unsigned last_ = 0;
};

class Mailbox {
 public:
  static constexpr size_t LINE = 64;
  static constexpr int CHANNELS = (int)(LINE / SeqChannel::BYTES);
  // alloc: once; reserve: grow to payload_bytes + slack (rounded up to whole lines), ovp_buf.h's meaning - contents are NOT kept
  // and no stream is synchronised: the caller synchronises the stream whose kernels may still write the old block before a growth.
  // The new block is zero, the channels point into it and keep their counters.  A failure leaves the mailbox empty.
  hipError_t alloc(size_t payload_bytes) { return buf_ ? hipSuccess : reserve(payload_bytes, 0); }
  hipError_t reserve(size_t payload_bytes, size_t slack) {
    if (buf_ && payload_bytes <= payload_capacity()) return hipSuccess;
    const size_t pay = (payload_bytes + slack + LINE - 1) / LINE * LINE;
    buf_.release();
    const hipError_t e = buf_.reserve(pay + LINE, 0);
    if (e == hipSuccess) memset(buf_.get(), 0, buf_.capacity());
    for (int k = 0; k < CHANNELS; ++k) {
      ch_[k].host_ = buf_ ? (volatile unsigned*)(buf_.get() + pay + SeqChannel::BYTES * k) : nullptr;
      ch_[k].dev_ = buf_ ? (unsigned*)dev((const void*)ch_[k].host_) : nullptr;
    }
    return e;
  }
  explicit operator bool() const { return buf_.get() != nullptr; }
  void* payload() const { return buf_.get(); }
  size_t payload_capacity() const { return buf_ ? buf_.capacity() - LINE : 0; }
  size_t capacity() const { return buf_.capacity(); }  // the whole block, the channels' line included
  // device address of a host address inside the block
  void* dev(const void* host_ptr) const { return buf_.dev() + ((const char*)host_ptr - buf_.get()); }
  SeqChannel& channel(int k) { return ch_[k]; }

 private:
  PinnedBuf<char> buf_{true};
  SeqChannel ch_[CHANNELS];
};
