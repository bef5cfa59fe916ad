// Owning types of the context's memory (host only): DevBuf<T> over hipMalloc / hipFree, PinnedBuf<T> over hipHostMalloc /
// hipHostFree, one template over the two.  Move-only, freed by the destructor, converting to T* so that a buffer is passed to a launch like the raw pointer it
// replaces.  alloc: once (first use); reserve: grow, contents NOT preserved and no stream synchronised (a caller whose stream may
// still read the old block synchronises it first; hipFree otherwise waits for the device itself).  Every byte these two hold is
// counted in ovp_live_bytes (ovp_debug_read "live_bytes"), and nothing else touches the counters.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <type_traits>
#include <utility>

struct OvpLiveBytes { std::atomic<long long> device{0}, pinned{0}; };
inline OvpLiveBytes& ovp_live_bytes() {
  static OvpLiveBytes b;
  return b;
}

namespace ovp_buf_detail {
template <class T> struct elem { static constexpr size_t size = sizeof(T); };
template <> struct elem<void> { static constexpr size_t size = 1; };  // a block of bytes, addressed through views
}

// where a block lives: its allocation calls and its byte counter
struct OvpDeviceMem {
  static hipError_t grab(void** p, void** dev, size_t bytes, bool) { return *dev = nullptr, hipMalloc(p, bytes); }
  static void drop(void* p) { (void)hipFree(p); }
  static std::atomic<long long>& live() { return ovp_live_bytes().device; }
};
struct OvpPinnedMem {  // mapped: hipHostMallocMapped, and *dev is the address a kernel writes the block through
  static hipError_t grab(void** p, void** dev, size_t bytes, bool mapped) {
    hipError_t e = hipHostMalloc(p, bytes, mapped ? hipHostMallocMapped : hipHostMallocDefault);
    if (e == hipSuccess && mapped && (e = hipHostGetDevicePointer(dev, *p, 0)) != hipSuccess) (void)hipHostFree(*p);
    return e;
  }
  static void drop(void* p) { (void)hipHostFree(p); }
  static std::atomic<long long>& live() { return ovp_live_bytes().pinned; }
};

template <class T, class Mem>
class OvpBuf {
 public:
  explicit OvpBuf(bool mapped = false) : mapped_(mapped) {}
  OvpBuf(const OvpBuf&) = delete;
  OvpBuf& operator=(const OvpBuf&) = delete;
  OvpBuf(OvpBuf&& o) noexcept : mapped_(o.mapped_) { swap(o); }
  OvpBuf& operator=(OvpBuf&& o) noexcept {
    if (this != &o) {
      release();
      swap(o);
    }
    return *this;
  }
  ~OvpBuf() { release(); }
  void swap(OvpBuf& o) noexcept {
    std::swap(p_, o.p_);
    std::swap(dev_, o.dev_);
    std::swap(cap_, o.cap_);
    std::swap(mapped_, o.mapped_);
  }
  operator T*() const { return p_; }
  template <class U>
  explicit operator U*() const { return (U*)p_; }  // (char*)buf, (double*)buf: the casts a raw pointer takes
  T* get() const { return p_; }
  T* dev() const { return dev_; }           // mapped pinned memory only
  size_t capacity() const { return cap_; }  // elements (bytes for T = void)
  hipError_t alloc(size_t count) { return p_ ? hipSuccess : grab(count); }
  hipError_t reserve(size_t count, size_t slack) {
    if (count <= cap_) return hipSuccess;
    release();
    return grab(count + slack);
  }
  void release() {
    if (p_) {
      Mem::drop(p_);
      Mem::live() -= (long long)(cap_ * ovp_buf_detail::elem<T>::size);
    }
    p_ = dev_ = nullptr;
    cap_ = 0;
  }

 private:
  hipError_t grab(size_t count) {  // (only ever on an empty buffer: a failure leaves it empty)
    void *p = nullptr, *d = nullptr;
    const hipError_t e = Mem::grab(&p, &d, count * ovp_buf_detail::elem<T>::size, mapped_);
    if (e != hipSuccess) return e;
    p_ = (T*)p;
    dev_ = (T*)d;
    cap_ = count;
    Mem::live() += (long long)(count * ovp_buf_detail::elem<T>::size);
    return hipSuccess;
  }
  T *p_ = nullptr, *dev_ = nullptr;
  size_t cap_ = 0;
  bool mapped_ = false;
};
template <class T> using DevBuf = OvpBuf<T, OvpDeviceMem>;
template <class T> using PinnedBuf = OvpBuf<T, OvpPinnedMem>;
