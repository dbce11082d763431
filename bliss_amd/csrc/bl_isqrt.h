/*
 * bl_isqrt.h — the exact floor of the square root of a 64-bit unsigned integer, one piece of source for the device
 * (k_rhythm_hops, bl_rhythm_kernels.hip) and the host (tests/host/test_isqrt_host.cpp).
 *
 * Digit by digit, base 4: `bit` runs over the even powers of two from the highest one not above x; at every step
 * r holds the root found so far, shifted, and x what is left of the radicand.  x >= r + bit asks whether the next
 * binary digit of the root is 1.  Integers only, so there is no rounding to argue about: the result r satisfies
 * r^2 <= x < (r + 1)^2 for every x < 2^64.  At most 32 steps; the rhythm pass calls it twice per hop of 128 frames on
 * values below 2^34 (17 steps).
 *
 * Not taken on trust: bl_amd_selftest_isqrt() sweeps k^2 - 1, k^2 and k^2 + 1 for every k in [1, 2^17], and 0, on the
 * device against r^2 <= x < (r + 1)^2; tests/host/test_isqrt_host.cpp does the same on the CPU.
 */
#ifndef BL_ISQRT_H_
#define BL_ISQRT_H_

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BL_ISQRT_FN __host__ __device__ inline
#else
#define BL_ISQRT_FN inline
#endif

BL_ISQRT_FN uint32_t bl_isqrt64(uint64_t x) {
  uint64_t r = 0, bit = (uint64_t)1 << 62;
  while (bit > x) bit >>= 2;
  while (bit) {
    if (x >= r + bit) {
      x -= r + bit;
      r = (r >> 1) + bit;
    } else {
      r >>= 1;
    }
    bit >>= 2;
  }
  return (uint32_t)r;
}

/* is r the floor of the square root of x?  The definition itself; r + 1 <= 2^32 so neither square overflows for
 * r < 2^32 - 1, and r = 2^32 - 1 has no upper test */
BL_ISQRT_FN bool bl_isqrt_is_floor(uint64_t x, uint32_t r) {
  const uint64_t a = (uint64_t)r * r;
  if (a > x) return false;
  if (r == 0xFFFFFFFFu) return true;
  const uint64_t b = (uint64_t)(r + 1ull) * (r + 1ull);
  return x < b;
}

#endif /* BL_ISQRT_H_ */
