/*
 * bl_chroma_table.h — the constant-Q bank of the chroma call (include/bliss_amd.h: bl_amd_chroma_*): 48 pitches from
 * A3 to G#7, each a Hann-windowed complex exponential of its own length, centred in a frame of 4 096 samples and
 * quantised to int8, with the gain that levels the lengths.  Data, built on the host; shared by bl_api.c
 * (bl_amd_chroma_table), bl_chroma_kernels.hip (the image the kernel reads) and tests/host/test_chroma_table_host.cpp.
 * Plain C.
 *
 * The table has to come out bit for bit the same from tests/chroma_reference.py, so sine and cosine are not libm's:
 * only IEEE double + - * / and floor are used, the argument (in turns) is reduced to [-1/8, 1/8] of a turn around the
 * nearest quarter, and two fixed polynomials with literal coefficients (the Taylor terms through x^13 and x^12:
 * |x| <= pi/4, so the truncation is below 3e-14 and 5e-13) are evaluated by Horner's rule, one operation at a time.
 * Every translation unit that includes this is compiled with -ffp-contract=off: a contracted multiply-add would round
 * once where the reference rounds twice.
 */
#ifndef BL_CHROMA_TABLE_H_
#define BL_CHROMA_TABLE_H_

#include <math.h>
#include <stdint.h>
#include <string.h>

#define BL_CHROMA_FRAME 4096
#define BL_CHROMA_HOP 2048
#define BL_CHROMA_PITCHES 48
#define BL_CHROMA_RATE 22050.0
#define BL_CHROMA_ABS_SUM_MAX 140000 /* sum_n |c[p][n]| of every row stays below this (checked where the table is built) */

/* cos and sin of 2 pi t for t in [0, 1] */
static inline void bl_chroma_cossin(double t, double *c, double *s) {
  const double k = floor(4.0 * t + 0.5);         /* the nearest quarter turn, 0 .. 4 */
  const double x = 6.283185307179586 * (t - 0.25 * k); /* |x| <= pi/4 */
  const double z = x * x;
  double ps = 1.6059043836821613e-10;            /* 1/13! */
  ps = ps * z - 2.505210838544172e-08;           /* 1/11! */
  ps = ps * z + 2.7557319223985893e-06;          /* 1/9! */
  ps = ps * z - 0.0001984126984126984;           /* 1/7! */
  ps = ps * z + 0.008333333333333333;            /* 1/5! */
  ps = ps * z - 0.16666666666666666;             /* 1/3! */
  ps = ps * z + 1.0;
  ps = ps * x;
  double pc = 2.08767569878681e-09;              /* 1/12! */
  pc = pc * z - 2.755731922398589e-07;           /* 1/10! */
  pc = pc * z + 2.48015873015873e-05;            /* 1/8! */
  pc = pc * z - 0.001388888888888889;            /* 1/6! */
  pc = pc * z + 0.041666666666666664;            /* 1/4! */
  pc = pc * z - 0.5;
  pc = pc * z + 1.0;
  switch ((int)k & 3) {
    case 0: *c = pc; *s = ps; break;
    case 1: *c = -ps; *s = pc; break;
    case 2: *c = -pc; *s = -ps; break;
    default: *c = ps; *s = -pc; break;
  }
}

/* f_p: the twelve semitones from A3, doubled per octave (exact) */
static inline double bl_chroma_freq(int p) {
  static const double B[12] = {220.0,      233.081881, 246.941651, 261.625565, 277.182631, 293.664768,
                               311.126984, 329.627557, 349.228231, 369.994423, 391.995436, 415.304698};
  return B[p % 12] * (double)(1 << (p / 12));
}

/* L_p = 2 floor(374 850 / f_p): 17 periods of the pitch at 22 050 Hz, even; 3 406 for p = 0, 224 for p = 47 */
static inline int bl_chroma_len(int p) { return 2 * (int)floor(374850.0 / bl_chroma_freq(p)); }

/* G[p] = 65 536 L_47^2 / L_p^2 in integers: 283 for p = 0, 65 536 for p = 47 */
static inline uint32_t bl_chroma_gain(int p) {
  const uint64_t l47 = (uint64_t)bl_chroma_len(BL_CHROMA_PITCHES - 1), lp = (uint64_t)bl_chroma_len(p);
  return (uint32_t)((65536u * l47 * l47) / (lp * lp));
}

/* pitch class of pitch p, C = 0 (p = 0 is an A) */
static inline int bl_chroma_class(int p) { return (p + 9) % 12; }

/* the unquantised entry n (0 <= n < L_p) of row p: 127 w cos, 127 w sin */
static inline void bl_chroma_entry(int p, int n, double *re, double *im) {
  const int L = bl_chroma_len(p);
  const double fp = bl_chroma_freq(p);
  double c, s, t;
  bl_chroma_cossin(((double)n + 0.5) / (double)L, &c, &s);
  const double w = 0.5 - 0.5 * c;
  t = fp * ((double)(n - L / 2) + 0.5) / BL_CHROMA_RATE;
  t -= floor(t);
  bl_chroma_cossin(t, &c, &s);
  *re = 127.0 * w * c;
  *im = 127.0 * w * s;
}

/* row p of the bank: 4 096 int8 each of cr and ci, zero outside the centred window */
static inline void bl_chroma_row(int p, int8_t *re, int8_t *im) {
  const int L = bl_chroma_len(p), n0 = (BL_CHROMA_FRAME - L) / 2;
  memset(re, 0, BL_CHROMA_FRAME);
  memset(im, 0, BL_CHROMA_FRAME);
  for (int n = 0; n < L; ++n) {
    double a, b;
    bl_chroma_entry(p, n, &a, &b);
    re[n0 + n] = (int8_t)floor(a + 0.5);
    im[n0 + n] = (int8_t)floor(b + 0.5);
  }
}

/* the whole bank; any pointer may be NULL.  re, im: [48][4096], gain, len: [48] */
static inline void bl_chroma_build(int8_t *re, int8_t *im, uint32_t *gain, int32_t *len) {
  int8_t r[BL_CHROMA_FRAME], i[BL_CHROMA_FRAME];
  for (int p = 0; p < BL_CHROMA_PITCHES; ++p) {
    if (re || im) bl_chroma_row(p, r, i);
    if (re) memcpy(re + (size_t)p * BL_CHROMA_FRAME, r, BL_CHROMA_FRAME);
    if (im) memcpy(im + (size_t)p * BL_CHROMA_FRAME, i, BL_CHROMA_FRAME);
    if (gain) gain[p] = bl_chroma_gain(p);
    if (len) len[p] = bl_chroma_len(p);
  }
}

#endif /* BL_CHROMA_TABLE_H_ */
