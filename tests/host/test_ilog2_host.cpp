// bl_ilog2.h on the CPU: the very source k_mel compiles, over the values of bl_amd_selftest_ilog2
// (bl_ilog2_sweep_value: 2^e - 1, 2^e, 2^e + 1 for every e <= 63, then 2^17 values of a multiplicative sequence).
// Prints one line "x L(x)" per value (x = 0, which is outside the domain, is skipped), then the known values and
// "OK"; tests/test_mel_reference_host.py compares every line with the Python restatement of the definition.
#include <stdint.h>
#include <stdio.h>

#include "../../bliss_amd/csrc/bl_ilog2.h"

int main() {
  unsigned long long printed = 0;
  for (uint32_t i = 0; i < BL_ILOG2_SWEEP; ++i) {
    const uint64_t x = bl_ilog2_sweep_value(i);
    if (!x) continue;
    printf("%llu %u\n", (unsigned long long)x, bl_ilog2_q12(x));
    printed += 1;
  }
  if (printed != BL_ILOG2_SWEEP - 1u) return 1;
  if (bl_ilog2_q12(1) != 0u || bl_ilog2_q12(2) != 4096u || bl_ilog2_q12(3) != 6492u ||
      bl_ilog2_q12(1ull << 63) != 258048u || bl_ilog2_q12(~0ull) >= 64u * 4096u)
    return 1;
  for (int e = 0; e < 64; ++e)
    if (bl_ilog2_q12(1ull << e) != 4096u * (uint32_t)e) return 1;
  printf("OK\n");
  return 0;
}
