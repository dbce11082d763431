/*
 * bl_ilog2.h — L(x): the base-2 logarithm of a 64-bit unsigned integer in 1/4096, one piece of source for the device
 * (k_mel, bl_mel_kernels.hip), the host (bl_amd_selftest_ilog2 compares the two) and tests/host/test_ilog2_host.cpp.
 *
 * Defined by this algorithm, not by libm (include/bliss_amd.h, the mel block): the integer part is the position of the
 * highest set bit; the mantissa is brought to 2^30 <= m < 2^31 (shifted up exactly, or shifted down with the low bits
 * dropped) and squared twelve times — every squaring doubles the logarithm, and whether the square passes 2 is its
 * next binary digit.  m * m < 2^62 and (m * m) >> 30 < 2^32, so everything fits 32 and 64 bits.  The truncations only
 * ever lower m, so L(x) <= 4096 log2 x, and L is non-decreasing; the error stays below 1 + 2^-10 units (about
 * 1 + 2^-17 by the analysis, tests/test_mel_reference_host.py measures it).  L(2^e) = 4096 e exactly.
 *
 * Not taken on trust: bl_amd_selftest_ilog2() runs it on the device for 2^e - 1, 2^e, 2^e + 1 of every e <= 63 and for
 * a multiplicative sequence of 2^17 values, and compares with what this same source gives on the host.
 */
#ifndef BL_ILOG2_H_
#define BL_ILOG2_H_

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BL_ILOG2_FN __host__ __device__ inline
#else
#define BL_ILOG2_FN static inline
#endif

#define BL_ILOG2_FRAC_BITS 12 /* L is in 1/4096 */

/* L(x) for 1 <= x < 2^64; x = 0 is outside the definition (the callers pass S + 1) */
BL_ILOG2_FN uint32_t bl_ilog2_q12(uint64_t x) {
  const int e = 63 - __builtin_clzll(x);
  uint32_t m = e <= 30 ? (uint32_t)(x << (30 - e)) : (uint32_t)(x >> (e - 30));
  uint32_t acc = (uint32_t)e;
  for (int i = 0; i < BL_ILOG2_FRAC_BITS; ++i) {
    const uint32_t t = (uint32_t)(((uint64_t)m * m) >> 30); /* 2^30 <= t < 2^32 */
    const uint32_t bit = t >> 31;
    m = t >> bit;
    acc = 2u * acc + bit;
  }
  return acc;
}

/* The values both self-tests run over: i < 192 are 2^e - 1, 2^e, 2^e + 1 for e = i / 3 (0 where that is no value of
 * the domain: 2^0 - 1), the rest a fixed multiplicative sequence (an odd multiplier modulo 2^64, so no value is 0). */
#define BL_ILOG2_SWEEP (192u + (1u << 17))
BL_ILOG2_FN uint64_t bl_ilog2_sweep_value(uint32_t i) {
  if (i < 192u) {
    const uint64_t p = (uint64_t)1 << (i / 3u);
    return p - 1u + i % 3u;
  }
  const uint64_t v = 0x9E3779B97F4A7C15ull * (uint64_t)(i - 191u); /* modulo 2^64 */
  return (v >> (i & 63u)) | 1u;                                     /* every magnitude from 2^64 down */
}

#endif /* BL_ILOG2_H_ */
