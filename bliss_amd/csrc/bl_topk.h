/*
 * bl_topk.h - the top-k selection the nearest-neighbour kernels share (bl_query_kernels.hip over force vectors,
 * bl_desc_kernels.hip over descriptors): a query's best 64 * KW keys sorted across the lanes of a wave, the k-th of them
 * as a wave-uniform threshold, a 64-key LDS queue for the candidates below it, and a bitonic merge when the queue is
 * full.  A key is any 64-bit unsigned whose order is the wanted one (value, then smaller index); BL_KEY_EMPTY is an empty
 * slot.  Everything is __device__ __forceinline__.
 */
#ifndef BL_TOPK_H_
#define BL_TOPK_H_

#include <hip/hip_runtime.h>

#include "bl_metric.h" /* BL_KEY_EMPTY, bl_wave_sync */

/* ascending bitonic sort of one key per lane */
__device__ __forceinline__ unsigned long long knn_sort64(unsigned long long x, int lane) {
#pragma unroll
  for (int size = 2; size <= 64; size <<= 1) {
#pragma unroll
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      const unsigned long long y = __shfl_xor(x, stride);
      const bool keep_min = ((lane & stride) == 0) == ((lane & size) == 0);
      x = keep_min ? min(x, y) : max(x, y);
    }
  }
  return x;
}

/* a bitonic sequence of 64 (one per lane) into ascending order */
__device__ __forceinline__ unsigned long long knn_clean64(unsigned long long x, int lane) {
#pragma unroll
  for (int stride = 32; stride > 0; stride >>= 1) {
    const unsigned long long y = __shfl_xor(x, stride);
    x = (lane & stride) ? max(x, y) : min(x, y);
  }
  return x;
}

/* Per-query state: the sorted list (e0 = slots 0..63, e1 = 64..127 when KW = 2), its k-th key and the queue fill. */
template <int KW> struct knn_top {
  unsigned long long e0, e1, thr;
  int qn;
  __device__ __forceinline__ void init() {
    e0 = e1 = thr = BL_KEY_EMPTY;
    qn = 0;
  }
  /* the 64 * KW smallest of the list and an ascending batch b: min against the reversed batch leaves them as one
   * bitonic sequence (positions below 64 of a 128-list meet the batch's padding, so e0 is unchanged there) */
  __device__ __forceinline__ void merge(unsigned long long b, int lane, int k) {
    const unsigned long long br = __shfl(b, 63 - lane);
    if (KW == 1) {
      e0 = knn_clean64(min(e0, br), lane);
    } else {
      const unsigned long long t1 = min(e1, br);
      const unsigned long long lo = min(e0, t1), hi = max(e0, t1);
      e0 = knn_clean64(lo, lane);
      e1 = knn_clean64(hi, lane);
    }
    thr = (KW == 1 || k <= 64) ? __shfl(e0, k - 1) : __shfl(e1, k - 65);
  }
  __device__ __forceinline__ void flush(unsigned long long *q, int lane, int k) {
    bl_wave_sync();
    unsigned long long x = lane < qn ? q[lane] : BL_KEY_EMPTY;
    bl_wave_sync();
    merge(knn_sort64(x, lane), lane, k);
    qn = 0;
  }
  /* p: this lane's key goes in (wave-uniform control flow around it) */
  __device__ __forceinline__ void push(bool p, unsigned long long key, unsigned long long *q, int lane, int k) {
    const unsigned long long m = __ballot(p);
    if (m == 0) return;
    const int cnt = __popcll(m);
    if (qn + cnt > 64) flush(q, lane, k);
    if (p) q[qn + __popcll(m & ((1ull << lane) - 1ull))] = key;
    qn += cnt;
  }
  __device__ __forceinline__ void finish(unsigned long long *q, int lane, int k) {
    if (qn > 0) flush(q, lane, k);
  }
};

#endif /* BL_TOPK_H_ */
