// How a host table reaches the device (host only, beside ovp_buf.h and ovp_mailbox.h): the host packs it into a pinned block and ONE
// asynchronous copy carries it into a device block of the same size.
//   OvpEvent     move-only owner of a hipEvent_t (timing events included: who records and reads them is the site's business)
//   UploadFence  what is known about the last copy that read a pinned block
//   Staged       a pinned block, its device block and the fence between them
//   StageLayout  offsets of the tables inside such a block
// THE INVARIANT, stated here once: a pinned block is the source of an asynchronous copy, and the host does not write it again until
// that copy has run.  Staged::begin is the only way to the host pointer for writing and it waits on the fence first.  A fence is
//   Fence::Event        an event recorded behind the copy; the entry returns without waiting and the next begin synchronises on it
//   Fence::CallerWaits  nothing recorded; the entry itself waits for something enqueued behind the copy on that stream (a mailbox
//                       word, a stream synchronisation, an event) and says so with done() directly behind that wait.  A call that
//                       left early never said it: the next begin then synchronises the stream the copy went on.
#pragma once
#include <hip/hip_runtime.h>

#include "ovp_buf.h"
#include "ovplane_hip.h"

class OvpEvent {
 public:
  OvpEvent() = default;
  OvpEvent(const OvpEvent&) = delete;
  OvpEvent& operator=(const OvpEvent&) = delete;
  OvpEvent(OvpEvent&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
  OvpEvent& operator=(OvpEvent&& o) noexcept {
    if (this != &o) {
      destroy();
      e_ = o.e_;
      o.e_ = nullptr;
    }
    return *this;
  }
  ~OvpEvent() { destroy(); }
  hipError_t create(unsigned flags = hipEventDefault) { return e_ ? hipSuccess : hipEventCreateWithFlags(&e_, flags); }
  operator hipEvent_t() const { return e_; }

 private:
  void destroy() {
    if (e_) (void)hipEventDestroy(e_);
    e_ = nullptr;
  }
  hipEvent_t e_ = nullptr;
};

enum class Fence { Event, CallerWaits };

class UploadFence {
 public:
  // the block is writable behind this, whatever it returns: the state is idle again
  hipError_t wait() {
    const State was = state_;
    state_ = Idle;
    return was == SentEvent ? hipEventSynchronize(ev_) : was == SentCallerWaits ? hipStreamSynchronize(stream_) : hipSuccess;
  }
  // a copy that reads the block has just been enqueued on s (an event that cannot be recorded leaves the stream to wait for)
  hipError_t sent(hipStream_t s, Fence kind) {
    stream_ = s;
    state_ = SentCallerWaits;
    if (kind == Fence::CallerWaits) return hipSuccess;
    hipError_t e = ev_.create(hipEventDisableTiming);
    if (e == hipSuccess && (e = hipEventRecord(ev_, s)) == hipSuccess) state_ = SentEvent;
    return e;
  }
  void done() { state_ = Idle; }  // the caller has waited for something enqueued behind the copy
  bool idle() const { return state_ == Idle; }

 private:
  enum State { Idle, SentEvent, SentCallerWaits } state_ = Idle;
  hipStream_t stream_ = nullptr;
  OvpEvent ev_;
};

class Staged {
 public:
  hipError_t alloc(size_t bytes) { return h_ ? hipSuccess : grab(bytes); }
  // grow to bytes + slack, contents NOT kept: kernels on s may still read the old device block, so s is synchronised first.  One
  // capacity stands for both halves; a failure leaves both empty and the fence idle.
  hipError_t reserve(size_t bytes, size_t slack, hipStream_t s) {
    if (bytes <= capacity()) return hipSuccess;
    hipError_t e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = fence_.wait();  // (a copy that went on another stream)
    return e != hipSuccess ? e : grab(bytes + slack);
  }
  // the host pointer, for writing `bytes` bytes: OVP_E_CAPACITY above the capacity, else behind the fence
  char* begin(size_t bytes, int* rc) {
    if (bytes > capacity()) return *rc = OVP_E_CAPACITY, nullptr;
    return (*rc = (int)fence_.wait()) ? nullptr : h_.get();
  }
  hipError_t send(size_t bytes, hipStream_t s, Fence kind) {
    const hipError_t e = hipMemcpyAsync(d_.get(), h_.get(), bytes, hipMemcpyHostToDevice, s);
    return e != hipSuccess ? e : fence_.sent(s, kind);
  }
  void done() { fence_.done(); }
  char* dev() const { return d_.get(); }
  char* host() const { return h_.get(); }  // for reading what came back into the pinned block; writing goes through begin
  size_t capacity() const { return d_.capacity(); }
  UploadFence& fence() { return fence_; }  // for a site that enqueues the copies out of host() itself (ovp_io_arena)

 private:
  hipError_t grab(size_t bytes) {
    h_.release();
    d_.release();
    fence_.done();
    hipError_t e = h_.reserve(bytes, 0);
    if (e == hipSuccess && (e = d_.reserve(bytes, 0)) != hipSuccess) h_.release();
    return e;
  }
  PinnedBuf<char> h_;
  DevBuf<char> d_;
  UploadFence fence_;
};

// Blocks of one staging buffer, each starting on a 64-byte line: take(bytes) returns the offset of the next block, bytes() the total.
struct StageLayout {
  size_t o = 0;
  static size_t al(size_t v) { return (v + 63) & ~(size_t)63; }
  size_t take(size_t bytes) {
    const size_t at = o;
    o = al(o + bytes);
    return at;
  }
  size_t bytes() const { return o; }
};
