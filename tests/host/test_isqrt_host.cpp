// bl_isqrt.h on the CPU: the very source k_rhythm_hops compiles, over the sweep of bl_amd_selftest_isqrt (0, and
// k^2 - 1, k^2, k^2 + 1 for every k in [1, 2^17]) against the definition r^2 <= x < (r + 1)^2 worked out here in
// 128-bit integers, then the ends of the 64-bit range and 2 000 000 seeded values.  Prints the counts and "OK".
#include <stdint.h>
#include <stdio.h>

#include "../../bliss_amd/csrc/bl_isqrt.h"

static bool is_floor(uint64_t x, uint64_t r) {
  const unsigned __int128 a = (unsigned __int128)r * r, b = (unsigned __int128)(r + 1) * (r + 1);
  return a <= x && x < b;
}

int main() {
  unsigned long long checked = 0, wrong = 0;
  auto check = [&](uint64_t x) {
    const uint32_t r = bl_isqrt64(x);
    checked += 1;
    if (!is_floor(x, r) || !bl_isqrt_is_floor(x, r)) {
      if (wrong < 10) printf("isqrt(%llu) = %u\n", (unsigned long long)x, r);
      wrong += 1;
    }
    // the checker of the device sweep refuses the neighbours of the right answer
    if (bl_isqrt_is_floor(x, r + 1u) && r != 0xFFFFFFFFu) wrong += 1;
    if (r && bl_isqrt_is_floor(x, r - 1u)) wrong += 1;
  };
  check(0);
  for (uint64_t k = 1; k <= (1ull << 17); ++k) {
    check(k * k - 1);
    check(k * k);
    check(k * k + 1);
  }
  printf("sweep: checked %llu wrong %llu\n", checked, wrong);
  if (checked != 3ull * (1ull << 17) + 1) return 1;
  // the amplitudes of the all -32768 songs: (4 * 128 * 2^32) >> 9 = 2^32 -> 2^16
  if (bl_isqrt64(1ull << 32) != 65536u) wrong += 1;
  for (int s = 2; s < 64; ++s) {
    check((1ull << s) - 1);
    check(1ull << s);
    check((1ull << s) + 1);
  }
  check(~0ull);
  check(0xFFFFFFFE00000001ull);      // (2^32 - 1)^2
  check(0xFFFFFFFE00000000ull);
  uint64_t z = 0x9E3779B97F4A7C15ull;
  for (int i = 0; i < 2000000; ++i) {
    z ^= z << 13; z ^= z >> 7; z ^= z << 17;
    check(z >> (z & 63));
  }
  printf("all: checked %llu wrong %llu\n", checked, wrong);
  if (wrong) return 1;
  printf("OK\n");
  return 0;
}
