/*
 * bl_metric.h — the per-pair arithmetic of bl_distance / bl_cosine_similarity on the device, shared by k_pairwise
 * (bl_matrix_kernels.hip) and the vector queries (bl_query_kernels.hip), so that a value a query lists has the bits of the
 * matrix entry.  Also the 64-bit (value, song) key that gives the queries their total order, and bl_wave_sync,
 * which the frequency and envelope kernels use as well.
 * Everything is __device__ __forceinline__ and follows the reference's unfused f32 arithmetic operation by operation
 * (-ffp-contract=off): the operand order of every expression here is part of the contract.
 */
#ifndef BL_METRIC_H_
#define BL_METRIC_H_

#include <hip/hip_runtime.h>

#include "bl_cos.h"
#include "bl_sqrt.h"

/* ordering point between LDS accesses of different lanes of ONE wave: a wave's LDS
 * instructions execute in order, so only the compiler has to be told */
__device__ __forceinline__ void bl_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

/* ref analyze.c:96-100: f32 throughout, left-to-right; the sum whose root bl_distance returns */
__device__ __forceinline__ float bl_dist_sq(const float4 a, const float4 b) {
  const float d0 = a.x - b.x, d1 = a.y - b.y, d2 = a.z - b.z, d3 = a.w - b.w;
  return d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
}

__device__ __forceinline__ float bl_dist(const float4 a, const float4 b) {
  /* sqrt correctly rounded (-fhip-fp32-correctly-rounded-divide-sqrt); __fsqrt_rn is the 1-ulp native op */
  return sqrtf(bl_dist_sq(a, b));
}

/* ref analyze.c:135-140: the f32 dot product, left to right */
__device__ __forceinline__ float bl_dot(const float4 a, const float4 b) {
  return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
}

/* An empty slot of a key list: the all-ones key (index 0xFFFFFFFF is never a song) */
#define BL_KEY_EMPTY 0xFFFFFFFFFFFFFFFFull

/* ascending total order on f32 as unsigned: -0 and +0 equal, every NaN after +inf */
__device__ __forceinline__ unsigned bl_ord(float v) {
  if (v != v) return 0xFFFFFFFFu;
  const unsigned u = v == 0.f ? 0u : __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

/* (value, song) as one unsigned: high word the order of the canonical value (cosine negated: larger is nearer), low
 * word the song index, so one compare is "value, then smaller index" */
template <bool COSINE> __device__ __forceinline__ unsigned long long bl_key(float v, int j) {
  return ((unsigned long long)bl_ord(COSINE ? -v : v) << 32) | (unsigned)j;
}

/* bl_distance from the sum: bl_sqrt.h's five-instruction root in its domain, the compiler's correctly rounded
 * sqrtf elsewhere; the two agree on every f32 (bl_amd_selftest_sqrt) */
__device__ __forceinline__ float bl_root(float s) {
  return bl_sqrt_fast_ok(s) ? bl_sqrt_rn_fast<1>(s) : sqrtf(s);
}

/* bl_cosine_similarity from the prepared (root, reciprocal root) of both vectors: k_pairwise's expression */
__device__ __forceinline__ float bl_cosine(const float4 a, const double2 pa, const float4 b, const double2 pb) {
  const float dot = bl_dot(a, b);
  float c;
  if (!bl_cos_fast(dot, pa.y * pb.y, c)) {
    bl_cos_vec ca, cb;
    ca.s = pa.x;
    cb.s = pb.x;
    c = bl_cos_plain(dot, ca, cb);
  }
  return c;
}

/* Largest squared sum worth a root: with t the threshold's distance, s > t^2 (1 + 2^-20) (as computed, > t^2 (1 + 2^-21))
 * gives sqrt(s) > t (1 + 2^-22) >= t + 2 ulp(t), whose rounding exceeds t.  Below t = 2^-50 (t^2 near the subnormals),
 * for a NaN or empty threshold and on overflow the bound is +inf: everything is keyed exactly. */
__device__ __forceinline__ float bl_sq_bound(unsigned long long thr) {
  const unsigned hi = (unsigned)(thr >> 32);
  const float t = __uint_as_float(hi & 0x7FFFFFFFu);
  if (hi == 0xFFFFFFFFu || hi < 0x80000000u || t < 0x1p-50f) return __builtin_inff();
  return t * t * (1.0f + 0x1p-20f);
}

/* A pair through the metric.  bl_measure: the quantity a radius or a bound is compared with — the squared sum
 * (distance, no root yet) or the cosine itself.  bl_value_of: the matrix entry from that measure.  bl_value: both. */
template <bool COSINE>
__device__ __forceinline__ float bl_measure(const float4 a, const double2 pa, const float4 b, const double2 pb) {
  return COSINE ? bl_cosine(a, pa, b, pb) : bl_dist_sq(a, b);
}
template <bool COSINE> __device__ __forceinline__ float bl_value_of(float m) { return COSINE ? m : bl_root(m); }
template <bool COSINE>
__device__ __forceinline__ float bl_value(const float4 a, const double2 pa, const float4 b, const double2 pb) {
  return bl_value_of<COSINE>(bl_measure<COSINE>(a, pa, b, pb));
}

#endif /* BL_METRIC_H_ */
