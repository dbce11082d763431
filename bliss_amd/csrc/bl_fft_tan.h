/*
 * bl_fft_tan.h — the 512-point real f64 DFT of k_env_windows3 with every constant twiddle in tan form.
 *
 * Same mapping as bl_fft.h (16 lanes x 16 registers, pass 1 over m1 in registers, transpose, pass 2 over n0,
 * real-input split), fewer instructions.  A general complex multiply by a constant w costs 2 mul + 2 fma.
 * Written as w = c (1 + i t), t = tan, c = cos (Linzer-Feig / Goedecker), the multiply by (1 + i t) is 2 fma
 * and the real factor c rides along until an addition takes it as the multiplier of an fma:
 *   pass 1   lane n0 multiplies register k1 by (1 + i t(n0, k1)) only (2 fma instead of 4); the value it hands
 *            over is the true one divided by c(n0, k1) = cos(2 pi n0 k1 / 256);
 *   pass 2   lane k1 folds those factors into the first radix-4 stage: a + c becomes fma(c_c / c_a, u_c, u_a)
 *            and each output carries the factor of its group's first element; the internal twiddles absorb it,
 *            the second stage folds the rest.  Group n0 = 0 has factor cos 0 = 1: all 16 outputs are unscaled;
 *   fft16    the four general internal twiddles (exponents 1, 3, 3, 9) take the tan form too, their cosine
 *            goes into the second radix-4 stage (compile-time constants in pass 1, per-lane products in pass 2);
 *   split    W512^k, k = 0..127, has cos > 0: (t, c) replaces (cos, sin), t r / t i take 2 fma and the sums
 *            a = e + c t become fma(+-c, t, e).
 * The one pass-1 element with cos = 0 is (n0, k1) = (8, 8), w = -i.  It takes c = 2^-600, t = -2^600: c t = -1
 * exactly, c (1 + i t) = 2^-600 - i, and the huge intermediate is scaled back by the first stage of pass 2 (lane 8,
 * ratio c(8, 8) / c(0, 8) = 2^-600) — no lane mask, no instruction.  It stays finite while the pass-1 values are
 * below 2^423, i.e. for windows below 2^418.  k_env_windows3's windows are below 2^46 in every FIR mode (|s - mean|
 * < 2^16 times taps of at most 1 / (2 V) <= 2^29, V = variance / 2^30 >= 2^-30), so the intermediate is below 2^651;
 * tests/host/test_fft_tan_host.cpp runs windows of that largest scale.
 * The per-lane constants are loop-invariant: 15 t of pass 1 (which replace the 15 complex twiddles the lane kept
 * before) and the 21 folding factors of pass 2, 36 doubles per lane.
 *
 * FIR mode 2 hands the transform the exact integer filter sums Y (bl_fir_int.h) and never scales them: with f the
 * per-song factor 1 / (1e7 * 2 V'), |DFT(f Y)|^2 = f^2 |DFT(Y)|^2, and f^2 rides in the constants of the split
 * (bl_fft512_power1_sq: 12 instructions per pair, e and o never formed).  The transform starts from integers
 * (|Y| < 2^45: pass-1 values below 2^54, far below the 2^423 of the 2^-600 trick; squares below 2^110) and
 * kappa = 2 f^2 is a normal number for every admissible V' = variance / 2^15, |variance| from 1 to 2^31:
 * 2 (2^15 / 2e7)^2 ~ 5.4e-6 at one end, 2 / (1e7 * 2^17)^2 ~ 1.2e-24 at the other.
 *
 * Everything here is __host__ __device__ (tests/host/test_fft_tan_host.cpp and test_fft_sq_host.cpp run the lane code
 * on the CPU).
 */
#ifndef BL_FFT_TAN_H_
#define BL_FFT_TAN_H_

#include "bl_fft.h"

/* the folding factors of one lane's pass-2 fft16 (all 1 / compile-time constants in pass 1) */
template <typename T> struct bl_fft16_fold {
  /* first stage, group n (elements n, n + 4, n + 8, n + 12, input factors c_n .. c_(n+12)):
   * rb = c_(n+4) / c_n, rc = c_(n+8) / c_n, rd = c_(n+12) / c_(n+4); the outputs carry c_n */
  T rb[4], rc[4], rd[4];
  /* second stage, column j (elements 4 j + 0..3): factor of element b is fb[j], of c fc[j & 1], and
   * g = (factor of d) / (factor of b): g[0] for j = 0 and 2, g[1], g[2] for j = 1, 3 */
  T fb[4], fc[2], g[3];
};

/* per-lane constants of k_env_windows3's transform, as the device table holds them */
template <typename T> struct bl_fft_tan_lane {
  T t1[16];               /* pass 1, lane n0: t(n0, k1) for k1 = 1..15; t1[0] = 0 */
  bl_fft16_fold<T> fold;  /* pass 2, lane k1 */
};
#define BL_FFT_TAN_LANE_DOUBLES 37
static_assert(sizeof(bl_fft_tan_lane<double>) == 8 * BL_FFT_TAN_LANE_DOUBLES, "bl_fft_tan_lane: no padding");

/* (r, i) *= (1 + i t) */
template <typename T> BL_HD void bl_tmul(T &r, T &i, T t) {
  const T nr = bl_fma(-t, i, r), ni = bl_fma(t, r, i);
  r = nr; i = ni;
}

/* Forward 16-point DFT in place, inputs scaled by per-element real factors that `f` describes (bl_fft16_fold);
 * outputs unscaled at bl_pos16(k), as bl_fft16 leaves them. */
template <typename T> BL_HD void bl_fft16_folded(T (&re)[16], T (&im)[16], const bl_fft16_fold<T> &f) {
  /* tan of the general internal twiddles: W16^1 = C1 (1 - i S1/C1), W16^3 = S1 (1 - i C1/S1),
   * W16^9 = -C1 (1 - i S1/C1) */
  const T TA = (T)0.41421356237309504880, TB = (T)2.41421356237309504880; /* S1 / C1, C1 / S1 */
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const T ar = re[n], ai = im[n], br = re[4 + n], bi = im[4 + n];
    const T cr = re[8 + n], ci = im[8 + n], dr = re[12 + n], di = im[12 + n];
    const T rb = f.rb[n], rc = f.rc[n], rd = f.rd[n];
    const T t0r = bl_fma(rc, cr, ar), t0i = bl_fma(rc, ci, ai), t1r = bl_fma(-rc, cr, ar), t1i = bl_fma(-rc, ci, ai);
    const T u2r = bl_fma(rd, dr, br), u2i = bl_fma(rd, di, bi), u3r = bl_fma(-rd, dr, br), u3i = bl_fma(-rd, di, bi);
    re[n] = bl_fma(rb, u2r, t0r);      im[n] = bl_fma(rb, u2i, t0i);
    re[8 + n] = bl_fma(-rb, u2r, t0r); im[8 + n] = bl_fma(-rb, u2i, t0i);
    re[4 + n] = bl_fma(rb, u3i, t1r);  im[4 + n] = bl_fma(-rb, u3r, t1i);
    re[12 + n] = bl_fma(-rb, u3i, t1r); im[12 + n] = bl_fma(rb, u3r, t1i);
  }
  /* element 4 j + n holds A[n][j] / c_n; it wants W16^(n j).  The cosines of the twiddles join the carried factors
   * in fb / fc / g; here only what is left: (1 + i t), R (1 - i) and R (-1 - i) as their unscaled sums, -i as a
   * swap the second stage reads directly */
  bl_tmul(re[5], im[5], -TA);   /* exponent 1 */
  bl_tmul(re[13], im[13], -TB); /* exponent 3 */
  bl_tmul(re[7], im[7], -TB);   /* exponent 3 */
  bl_tmul(re[15], im[15], -TA); /* exponent 9 */
  { T a = re[9], b = im[9]; re[9] = a + b; im[9] = b - a; }     /* exponent 2 */
  { T a = re[6], b = im[6]; re[6] = a + b; im[6] = b - a; }     /* exponent 2 */
  { T a = re[14], b = im[14]; re[14] = b - a; im[14] = -(a + b); } /* exponent 6 */
  { T a = re[11], b = im[11]; re[11] = b - a; im[11] = -(a + b); } /* exponent 6 */
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int e = 4 * j;
    const T ar = re[e], ai = im[e], br = re[e + 1], bi = im[e + 1], dr = re[e + 3], di = im[e + 3];
    const T cr = j == 2 ? im[e + 2] : re[e + 2], ci = j == 2 ? -re[e + 2] : im[e + 2]; /* exponent 4: -i */
    const T fb = f.fb[j], fc = f.fc[j & 1], g = f.g[j == 2 ? 0 : j == 3 ? 2 : j];
    const T t0r = bl_fma(fc, cr, ar), t0i = bl_fma(fc, ci, ai), t1r = bl_fma(-fc, cr, ar), t1i = bl_fma(-fc, ci, ai);
    const T u2r = bl_fma(g, dr, br), u2i = bl_fma(g, di, bi), u3r = bl_fma(-g, dr, br), u3i = bl_fma(-g, di, bi);
    re[e] = bl_fma(fb, u2r, t0r);      im[e] = bl_fma(fb, u2i, t0i);
    re[e + 2] = bl_fma(-fb, u2r, t0r); im[e + 2] = bl_fma(-fb, u2i, t0i);
    re[e + 1] = bl_fma(fb, u3i, t1r);  im[e + 1] = bl_fma(-fb, u3r, t1i);
    re[e + 3] = bl_fma(-fb, u3i, t1r); im[e + 3] = bl_fma(fb, u3r, t1i);
  }
  /* element 4 j + k0 holds X[j + 4 k0] */
}

/* pass 1's fft16: unscaled inputs, only the internal twiddles' cosines to fold (compile-time constants: the
 * multiplications by 1 become additions) */
template <typename T> BL_HD void bl_fft16_tan(T (&re)[16], T (&im)[16]) {
  const T C1 = (T)0.92387953251128673848, S1 = (T)0.38268343236508978178;
  const T R = (T)0.70710678118654752440;
  const T TA = (T)0.41421356237309504880, TB = (T)2.41421356237309504880;
  const bl_fft16_fold<T> f = {{1, 1, 1, 1}, {1, 1, 1, 1}, {1, 1, 1, 1}, {1, C1, R, S1}, {1, R}, {1, TA, -TB}};
  bl_fft16_folded<T>(re, im, f);
}

/* pass 1 in registers (lane n0): fft16 and the twiddles (1 + i t(n0, k1)); register bl_pos16(k1) is left holding
 * the true value divided by c(n0, k1) */
template <typename T> BL_HD void bl_fft512_pass1_tan(T (&re)[16], T (&im)[16], const T (&t1)[16]) {
  bl_fft16_tan<T>(re, im);
#pragma unroll
  for (int k1 = 1; k1 < 16; ++k1) bl_tmul(re[bl_pos16(k1)], im[bl_pos16(k1)], t1[k1]);
}

/* one pair of the real-input split with w = W512^k = c (1 + i t): as bl_fft512_power1 */
template <typename T, bool QUARTER = true>
BL_HD void bl_fft512_power1_tan(T zr, T zi, T pr, T pi, bl_c2<T> tc, T &own, T &mir) {
  const T er = zr + pr, ei = zi - pi;
  const T orr = zi + pi, oi = pr - zr;
  const T tr = bl_fma(-tc.re, oi, orr), ti = bl_fma(tc.re, orr, oi);
  const T ar = bl_fma(tc.im, tr, er), ai = bl_fma(tc.im, ti, ei);
  const T br = bl_fma(-tc.im, tr, er), bi = bl_fma(-tc.im, ti, ei);
  own = bl_fma(ar, ar, ai * ai);
  mir = bl_fma(br, br, bi * bi);
  if (QUARTER) { own = (T)0.25 * own; mir = (T)0.25 * mir; }
}

/* The same pair from the squares, for an UNSCALED transform (FIR mode 2).  With z = Z_k, p = Z_(256-k), e = z + conj p,
 * o = -i (z - conj p), w = W512^k = cos a - i sin a:
 *     |e|^2 + |o|^2 = 2 (|z|^2 + |p|^2)        Re(e conj(w o)) = 2 cos a Im(z p) - sin a (|z|^2 - |p|^2)
 * so |e +- w o|^2 = 2 S +- (4 cos a M - 2 sin a Dm) with A = |z|^2, B = |p|^2, M = zr pi + zi pr, S = A + B,
 * Dm = A - B.  The caller's constants carry the square of the scale f the input was never multiplied by:
 *     kappa = 2 f^2,  cs = (c', s') = (4 f^2 cos a, -2 f^2 sin a) = (2 kappa cos a, -kappa sin a)
 * and own = f^2 |e + w o|^2, mir = f^2 |e - w o|^2: what bl_fft512_power1_tan<T, false> gives for the input f Y.
 * 12 instructions where that one takes 14.  The pair k = 0 (z = p = Z_0) needs no special case: Dm = 0 and the two
 * results are 4 f^2 (zr + zi)^2 and 4 f^2 (zr - zi)^2.  Both terms carry an absolute error of order eps times the
 * pair's energy, as there. */
template <typename T>
BL_HD void bl_fft512_power1_sq(T zr, T zi, T pr, T pi, bl_c2<T> cs, T kappa, T &own, T &mir) {
  const T A = bl_fma(zr, zr, zi * zi);
  const T B = bl_fma(pr, pr, pi * pi);
  const T M = bl_fma(zr, pi, zi * pr);
  const T S = A + B, Dm = A - B;
  const T D = bl_fma(cs.re, M, cs.im * Dm);
  own = bl_fma(kappa, S, D);
  mir = bl_fma(kappa, S, -D);
}

#if defined(__HIPCC__)
#define BL_TAN_HOST __host__ static inline
#else
#define BL_TAN_HOST static inline
#endif
/* Host: the constants, from long-double cosines and tangents.  lanes[16]: per-lane constants;
 * tw512t[128]: (t, c) of W512^k, k = 0..127. */
BL_TAN_HOST long double bl_tan_cos256_(int e) { /* c(n0, k1), e = n0 k1 */
  return e == 64 ? 0x1p-600L : cosl(2.0L * 3.14159265358979323846264338327950288L * e / 256.0L);
}
BL_TAN_HOST void bl_fft_tan_fill(bl_fft_tan_lane<double> *lanes, bl_c2<double> *tw512t) {
  const long double PI = 3.14159265358979323846264338327950288L;
  const long double C1 = cosl(PI / 8), S1 = sinl(PI / 8), R = sqrtl(0.5L);
  for (int l = 0; l < 16; ++l) {
    bl_fft_tan_lane<double> &L = lanes[l];
    L.t1[0] = 0.0;
    for (int k1 = 1; k1 < 16; ++k1) { /* w = exp(-2 pi i e / 256) = c (1 + i t), t = -tan */
      const int e = l * k1;
      L.t1[k1] = e == 64 ? -0x1p600 : (double)-tanl(2.0L * PI * e / 256.0L);
    }
    long double c[16];
    for (int n = 0; n < 16; ++n) c[n] = bl_tan_cos256_(n * l);
    bl_fft16_fold<double> &f = L.fold;
    for (int n = 0; n < 4; ++n) {
      f.rb[n] = (double)(c[n + 4] / c[n]);
      f.rc[n] = (double)(c[n + 8] / c[n]);
      f.rd[n] = (double)(c[n + 12] / c[n + 4]);
    }
    f.fb[0] = (double)c[1];
    f.fb[1] = (double)(C1 * c[1]);
    f.fb[2] = (double)(R * c[1]);
    f.fb[3] = (double)(S1 * c[1]);
    f.fc[0] = (double)c[2];
    f.fc[1] = (double)(R * c[2]);
    f.g[0] = (double)(c[3] / c[1]);
    f.g[1] = (double)((S1 * c[3]) / (C1 * c[1]));
    f.g[2] = (double)((-C1 * c[3]) / (S1 * c[1]));
  }
  for (int k = 0; k < 128; ++k) { /* W512^k = cos - i sin = c (1 + i t) */
    const long double a = 2.0L * PI * k / 512.0L;
    tw512t[k].re = (double)-tanl(a);
    tw512t[k].im = (double)cosl(a);
  }
}
/* cs512[128]: (cos a, sin a) of W512^k, k = 0..127, a = 2 pi k / 512: what k_env_windows3 scales by the song's kappa
 * into the (c', s') of bl_fft512_power1_sq */
BL_TAN_HOST void bl_fft_sq_fill(bl_c2<double> *cs512) {
  const long double PI = 3.14159265358979323846264338327950288L;
  for (int k = 0; k < 128; ++k) {
    const long double a = 2.0L * PI * k / 512.0L;
    cs512[k].re = (double)cosl(a);
    cs512[k].im = (double)sinl(a);
  }
}
/* the pair constants of one song from cs512: both products round once (2 kappa is exact) */
template <typename T> BL_HD bl_c2<T> bl_fft_sq_consts(bl_c2<T> cs, T kappa) {
  bl_c2<T> r;
  r.re = ((T)2 * kappa) * cs.re;
  r.im = -kappa * cs.im;
  return r;
}

#endif /* BL_FFT_TAN_H_ */
