// bl_chroma_table.h on the CPU: the very source bl_api.c and bl_chroma_kernels.hip compile.  Builds the bank and checks
// the lengths and gains at the ends, the zero margins around every centred window, the symmetry of the window (cr is
// even and ci odd about the frame's centre, up to the +0.5 rounding's one unit), the bounds the kernel's int32 sums rest
// on (sum |c| <= 140 000 per row), the accuracy of the polynomial sine and cosine against libm, and that the two ways
// to the table (row by row, all at once with NULL outputs) agree.  Compile with -ffp-contract=off; suitable for
// -fsanitize=address,undefined.  Prints the figures and "OK".
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../bliss_amd/csrc/bl_chroma_table.h"

static int fails = 0;
#define CHECK(cond, ...)                     \
  do {                                       \
    if (!(cond)) {                           \
      if (fails < 20) { printf(__VA_ARGS__); printf("\n"); } \
      fails += 1;                            \
    }                                        \
  } while (0)

int main() {
  std::vector<int8_t> re((size_t)BL_CHROMA_PITCHES * BL_CHROMA_FRAME), im(re.size());
  uint32_t gain[BL_CHROMA_PITCHES];
  int32_t len[BL_CHROMA_PITCHES];
  bl_chroma_build(re.data(), im.data(), gain, len);
  CHECK(len[0] == 3406 && len[47] == 224, "L_0 %d L_47 %d", len[0], len[47]);
  CHECK(gain[0] == 283u && gain[47] == 65536u, "G_0 %u G_47 %u", gain[0], gain[47]);
  CHECK(bl_chroma_class(0) == 9 && bl_chroma_class(3) == 0 && bl_chroma_class(47) == 8, "pitch classes");
  long long max_abs = 0, total_len = 0;
  int max_asym = 0;
  for (int p = 0; p < BL_CHROMA_PITCHES; ++p) {
    const int8_t *r = re.data() + (size_t)p * BL_CHROMA_FRAME, *i = im.data() + (size_t)p * BL_CHROMA_FRAME;
    const int L = len[p], n0 = (BL_CHROMA_FRAME - L) / 2;
    total_len += L;
    CHECK(L == bl_chroma_len(p) && L % 2 == 0 && L >= 224 && L <= 3406, "pitch %d: L %d", p, L);
    CHECK(p == 0 || (len[p] <= len[p - 1] && gain[p] >= gain[p - 1]), "pitch %d: L or G not monotonic", p);
    CHECK(gain[p] == (uint32_t)((65536ull * 224 * 224) / ((unsigned long long)L * L)), "pitch %d: G %u", p, gain[p]);
    long long ar = 0, ai = 0;
    for (int n = 0; n < BL_CHROMA_FRAME; ++n) {
      if (n < n0 || n >= n0 + L) CHECK(r[n] == 0 && i[n] == 0, "pitch %d: entry %d outside the window is not 0", p, n);
      CHECK(r[n] >= -127 && r[n] <= 127 && i[n] >= -127 && i[n] <= 127, "pitch %d: entry %d beyond 127", p, n);
      ar += abs(r[n]);
      ai += abs(i[n]);
      // n and 4095 - n mirror about the centre: w is even, t odd, so cr is even and ci odd before rounding
      const int m = BL_CHROMA_FRAME - 1 - n;
      const int dr = abs(r[n] - r[m]), di = abs(i[n] + i[m]);
      if (dr > max_asym) max_asym = dr;
      if (di > max_asym) max_asym = di;
    }
    CHECK(ar <= BL_CHROMA_ABS_SUM_MAX && ai <= BL_CHROMA_ABS_SUM_MAX, "pitch %d: sum |c| %lld %lld", p, ar, ai);
    CHECK(ar > 127ll * L / 4 && ai > 127ll * L / 4, "pitch %d: a row that is almost empty", p);
    if (ar > max_abs) max_abs = ar;
    if (ai > max_abs) max_abs = ai;
    // the first and the last entry of the window sit where the Hann window has just left 0
    CHECK(abs(r[n0]) <= 1 && abs(i[n0]) <= 1 && abs(r[n0 + L - 1]) <= 1 && abs(i[n0 + L - 1]) <= 1, "pitch %d: window ends", p);
    // row by row gives the same bytes
    int8_t rr[BL_CHROMA_FRAME], ii[BL_CHROMA_FRAME];
    bl_chroma_row(p, rr, ii);
    CHECK(!memcmp(rr, r, BL_CHROMA_FRAME) && !memcmp(ii, i, BL_CHROMA_FRAME), "pitch %d: bl_chroma_row differs", p);
  }
  CHECK(max_asym <= 1, "asymmetry %d", max_asym);
  printf("sum L %lld, largest sum |c| %lld, largest asymmetry %d\n", total_len, max_abs, max_asym);
  bl_chroma_build(NULL, NULL, NULL, NULL);
  bl_chroma_build(NULL, im.data(), NULL, len);
  // sine and cosine against libm over a dense sweep of [0, 1] and the exact quarter points
  double worst = 0.0;
  for (int k = 0; k <= 2000000; ++k) {
    const double t = (double)k / 2000000.0;
    double c, s;
    bl_chroma_cossin(t, &c, &s);
    const double ec = fabs(c - cos(6.283185307179586 * t)), es = fabs(s - sin(6.283185307179586 * t));
    if (ec > worst) worst = ec;
    if (es > worst) worst = es;
  }
  for (int k = 0; k <= 8; ++k) {
    double c, s;
    bl_chroma_cossin(0.125 * k, &c, &s);
    if (k % 2 == 0) CHECK(fabs(c) == (k % 4 == 0 ? 1.0 : 0.0) && fabs(s) == (k % 4 == 0 ? 0.0 : 1.0), "quarter %d: %g %g", k, c, s);
  }
  printf("worst |error| of cos / sin against libm: %.3g\n", worst);
  CHECK(worst <= 1e-9, "sine or cosine off by %g", worst);
  if (fails) {
    printf("%d checks failed\n", fails);
    return 1;
  }
  printf("OK\n");
  return 0;
}
