/*
 * bl_mel_table.h — the tables of the mel call (include/bliss_amd.h: bl_amd_mel_*): the 34 band edges, the 32 triangular
 * bands' integer weights over the 255 bins of the frequency pass, and the 13 x 32 cosine table of the cepstrum.  Data,
 * built on the host; shared by bl_api.c (bl_amd_mel_table) and bl_mel_kernels.hip (the image the kernel reads).
 * Plain C.
 *
 * The edges are literals: sixteenths of a bin, equally spaced on the mel scale 2595 log10(1 + f / 700) from bin 1 to
 * bin 256 of a 512-point transform at 22 050 Hz, rounded to nearest (the nearest rounding boundary is 0.056 away, so
 * tests/mel_reference.py lands on the same integers from the formula in double).  The weights are integer floor
 * divisions of them.  The cosine is bl_chroma_cossin's (bl_chroma_table.h: IEEE double + - * / and floor only), so the
 * table comes out bit for bit the same from Python; every translation unit that includes this is compiled with
 * -ffp-contract=off.
 */
#ifndef BL_MEL_TABLE_H_
#define BL_MEL_TABLE_H_

#include <stdint.h>

#include "bl_chroma_table.h" /* bl_chroma_cossin */

#define BL_MEL_BANDS 32
#define BL_MEL_COEFFS 13
#define BL_MEL_BINS 256      /* a row of weights: bins 0 .. 255, bin 0 always 0 */
#define BL_MEL_MAX_WIDTH 41  /* non-zero weights of the widest band */

static const int32_t bl_mel_edges[BL_MEL_BANDS + 2] = {
    16,   40,   66,   95,   126,  159,  196,  236,  279,  326,  377,  432,  493,  558,  630,  707,  792,
    883,  983,  1091, 1209, 1337, 1477, 1628, 1793, 1972, 2166, 2378, 2608, 2858, 3130, 3425, 3747, 4096};

/* W[b][d]: rising over (a, c], falling over (c, z), with x = 16 d in sixteenths of a bin; 0 .. 64 */
static inline int bl_mel_weight(int b, int d) {
  const int x = 16 * d, a = bl_mel_edges[b], c = bl_mel_edges[b + 1], z = bl_mel_edges[b + 2];
  if (a < x && x <= c) return (64 * (x - a)) / (c - a);
  if (c < x && x < z) return (64 * (z - x)) / (z - c);
  return 0;
}

/* D[k][b] = floor(16384 cos(pi k (2 b + 1) / 64) + 0.5): the angle is k (2 b + 1) / 128 of a turn */
static inline int32_t bl_mel_dct(int k, int b) {
  double c, s;
  bl_chroma_cossin((double)((k * (2 * b + 1)) % 128) / 128.0, &c, &s);
  return (int32_t)floor(16384.0 * c + 0.5);
}

/* The three tables; any pointer may be NULL.  edges [34], weights [32][256], dct [13][32].  Returns 0, or -1 if the
 * weights do not have the properties the kernel's bounds rest on: every band has 3 .. 41 non-zero weights, and they
 * are contiguous; no bin feeds more than two bands; a column sums to at most 64 (so S <= 64 * 2^50 = 2^56) and bin 1,
 * where a DC offset leaks to under the Hann window, to 0; the row sums run from 90 to 1320. */
static inline int bl_mel_build(int32_t *edges, uint8_t *weights, int32_t *dct) {
  int row_min = 1 << 30, row_max = 0, bad = 0;
  int col_sum[BL_MEL_BINS] = {0}, col_n[BL_MEL_BINS] = {0};
  for (int b = 0; b < BL_MEL_BANDS; ++b) {
    int n = 0, first = 0, last = 0, sum = 0;
    for (int d = 0; d < BL_MEL_BINS; ++d) {
      const int w = d ? bl_mel_weight(b, d) : 0;
      if (weights) weights[b * BL_MEL_BINS + d] = (uint8_t)w;
      if (!w) continue;
      if (!n) first = d;
      last = d;
      n += 1;
      sum += w;
      col_sum[d] += w;
      col_n[d] += 1;
      bad |= w < 0 || w > 64;
    }
    bad |= n < 3 || n > BL_MEL_MAX_WIDTH || last - first + 1 != n;
    row_min = sum < row_min ? sum : row_min;
    row_max = sum > row_max ? sum : row_max;
  }
  for (int d = 0; d < BL_MEL_BINS; ++d) bad |= col_sum[d] > 64 || col_n[d] > 2;
  bad |= col_sum[0] != 0 || col_sum[1] != 0 || row_min != 90 || row_max != 1320;
  if (edges)
    for (int i = 0; i < BL_MEL_BANDS + 2; ++i) edges[i] = bl_mel_edges[i];
  if (dct)
    for (int k = 0; k < BL_MEL_COEFFS; ++k)
      for (int b = 0; b < BL_MEL_BANDS; ++b) dct[k * BL_MEL_BANDS + b] = bl_mel_dct(k, b);
  return bad ? -1 : 0;
}

#endif /* BL_MEL_TABLE_H_ */
