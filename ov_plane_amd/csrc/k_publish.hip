// The copy-and-post kernel of the pinned-result handshake (ovp_mailbox.h): a device block into a mailbox's payload, then the
// sequence word of one of its channels.  A hipMemcpyAsync + hipStreamSynchronize pair costs ~25 us of launch, blit and wake-up
// latency per entry, this ~5.
#include "ovp_kernels.h"

// src, dst 8-byte aligned; 8 bytes at a time, the tail byte by byte.  clear8: that many leading 8-byte words of src are zeroed
// behind the post (the point update's four flag words, cleared for the next update).
__global__ __launch_bounds__(1024) void k_publish_block(unsigned long long* __restrict__ src, unsigned long long* __restrict__ dst, int bytes,
                                                       volatile unsigned* word, unsigned seq, int clear8) {
  const int t = threadIdx.x, w = bytes >> 3;
  for (int i = t; i < w; i += 1024) dst[i] = src[i];
  for (int i = 8 * w + t; i < bytes; i += 1024)
    reinterpret_cast<unsigned char*>(dst)[i] = reinterpret_cast<const unsigned char*>(src)[i];
  __threadfence_system();
  __syncthreads();
  if (t == 0) *word = seq;
  if (t < clear8) src[t] = 0ull;
}

extern "C" hipError_t ovp_launch_publish_block(const void* src, void* dst, size_t bytes, unsigned* word, unsigned seq, int clear8,
                                               hipStream_t stream) {
  if ((((size_t)src | (size_t)dst) & 7) || bytes > (size_t)0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_publish_block, dim3(1), dim3(1024), 0, stream, (unsigned long long*)src, (unsigned long long*)dst, (int)bytes,
                     (volatile unsigned*)word, seq, clear8);
  return hipGetLastError();
}
