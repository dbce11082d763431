/*
 * bl_fir_int.h — FIR mode 2 of k_env_windows3 (bl_env_kernels.hip) as an exact integer convolution, shared by the
 * kernel, k_song_prep (bl_stats_kernels.hip) and the host test (tests/host/test_fir_int_host.cpp).
 *
 * The taps of ref include/bandpass_coeffs.h are literals with seven decimals: c_m = C_m * 1e-7 with the integers C_m
 * below (|C_m| < 2^24, sum over the 17 taps 9 887 759).  Mode 2 filters the integers k = s - mean (|k| < 2^17), so
 *     Y_j = sum_m C_m k[j - m]       is an integer, |Y_j| < 2^45, formed without any rounding, and
 *     y_j = Y_j * sc,                sc = RN(1 / (1e7 * 2 vprime)) (bl_firi_scale), is the filter output (halved, as
 * everything in that kernel: see bl_norm in bl_fir.h) with ONE rounding where the fma form had nine and the
 * reference's about 25.  The kernel does not even form y: its DFT is linear, so it transforms Y itself and multiplies
 * the power terms by kappa = 2 sc^2 (bl_firi_power_scale; bl_fft512_power1_sq in bl_fft_tan.h).  Two routes to the same Y, hence the same bits:
 *
 *  - the f64 form (BL_FIR_INT): the nine products of the integer taps with the exact pair sums, as doubles.  Every
 *    partial sum is an integer below 2^53, so no operation rounds.  The block in front of a run and the zero-state
 *    heads use it.
 *
 *  - the int8 matrix form, for the main loop.  A sample is s = 256 h + l' + 128 with h = s >> 8 (signed high byte) and
 *    l' = (s & 255) - 128 (the low byte with its top bit flipped, read as signed); a tap is C = c0 + 2^8 c1 + 2^16 c2
 *    + 2^24 c3 with signed digits in [-128, 127] (four are needed: the centre tap 9 065 095 exceeds the three-digit
 *    range 8 355 711; c3 is 1 there and 0 elsewhere).  The byte products group by weight:
 *        a0 = sum l' c0            a1 = sum l' c1 + h c0     a2 = sum l' c2 + h c1
 *        a3 = sum l' c3 + h c2     a4 = sum h c3                                   (sums over the 17 taps)
 *        sum_m C_m (256 h + l') = a0 + 2^8 a1 + 2^16 a2 + 2^24 a3 + 2^32 a4
 *    and the rest, (128 - mean) * 9 887 759 =: K (|K| <= 32 896 * 9 887 759 < 2^39), is the same for every output
 *    that has all its 17 samples.  K = k0 + 2^16 k2 + 2^32 k4 with 0 <= k0, k2 < 2^16, |k4| <= 76 goes into the
 *    initial values of a0, a2, a4 (bl_firi_const).  Bounds, with |l'|, |h|, |c| <= 128:
 *        |a0| <= 17 * 2^14 + 2^16 < 2^19      |a1| <= 34 * 2^14 < 2^20      |a2| <= 34 * 2^14 + 2^16 < 2^20
 *        |a3| <= 34 * 2^14 < 2^20             |a4| <= 128 * 1 + 76 < 2^8    (only the centre tap has a c3)
 *        lo  = a0 + 2^8 a1            < 2^29
 *        mid = a2 + 2^8 a3 + 2^16 a4  < 2^20 + 2^28 + 2^24 < 2^29          all inside int32;
 *        Y   = (double)lo + 65536.0 * (double)mid    one fma, exact: an integer below 2^53.
 *    One 16 x 16 tile of outputs (a 256-sample block: output 16 a + b at row b, column a) is five matrix products
 *    of K = 32 samples; row b of the tap matrix holds C_(16 + b - kappa) at sample kappa (a Toeplitz band), column a
 *    of the sample matrix holds samples 16 (a - 1) + kappa of the block, kappa = 0..31.  BOTH operands are laid out by
 *    the same rule — the lane of K-group kb holds kappa = bl_firi_kappa(kb, q, e) in byte e of word q of a plane — so a
 *    product pairs equal kappa whatever order the hardware walks K in.
 */
#ifndef BL_FIR_INT_H_
#define BL_FIR_INT_H_

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BL_FIRI_HD __host__ __device__ __forceinline__
#else
#include <math.h>
#define BL_FIRI_HD static inline
#endif

/* C_m = c_m * 1e7, m = 0..8 (symmetric: C_(16 - m) = C_m): the digits of bl_fir.h's BL_C0..BL_C8 */
#define BL_CI0 (-23470.0)
#define BL_CI1 44613.0
#define BL_CI2 (-114627.0)
#define BL_CI3 226382.0
#define BL_CI4 (-405147.0)
#define BL_CI5 580037.0
#define BL_CI6 (-779167.0)
#define BL_CI7 882711.0
#define BL_CI8 9065095.0
#define BL_FIRI_TAPSUM 9887759LL /* C_8 + 2 (C_0 + .. + C_7) */
#define BL_FIRI_UNSCALE 1e7      /* exact in f64 */

/* tap m of the 17 as an integer; 0 outside 0..16 */
BL_FIRI_HD int bl_firi_tap(int m) {
  if (m < 0 || m > 16) return 0;
  switch (m > 8 ? 16 - m : m) {
    case 0: return (int)BL_CI0;
    case 1: return (int)BL_CI1;
    case 2: return (int)BL_CI2;
    case 3: return (int)BL_CI3;
    case 4: return (int)BL_CI4;
    case 5: return (int)BL_CI5;
    case 6: return (int)BL_CI6;
    case 7: return (int)BL_CI7;
    default: return (int)BL_CI8;
  }
}

/* signed base-256 digit j of c: c = d0 + 2^8 d1 + 2^16 d2 + 2^24 d3 (+ ...), every d in [-128, 127] */
BL_FIRI_HD int bl_firi_digit(int c, int j) {
  for (int i = 0; i < j; ++i) c = (c - (int)(signed char)(c & 255)) / 256; /* exact division */
  return (int)(signed char)(c & 255);
}

/* The f64 form: Y from the exact pair sums P(m) = k[j - m] + k[j - 16 + m], m = 0..7, and P(8) = k[j - 8], as
 * doubles (a sample the zero-state head does not have counts 0).  Written with fmas in the order of its neighbours in
 * bl_fir.h; none of them rounds.  BL_FIR_INT takes the samples X(m) = (double)k[j - m] instead. */
#define BL_FIR_INT_P(P)                                             \
  ({                                                                \
    double y_ = BL_CI7 * P(7);                                      \
    y_ = __builtin_fma(BL_CI6, P(6), y_);                           \
    y_ = __builtin_fma(BL_CI5, P(5), y_);                           \
    y_ = __builtin_fma(BL_CI4, P(4), y_);                           \
    y_ = __builtin_fma(BL_CI3, P(3), y_);                           \
    y_ = __builtin_fma(BL_CI2, P(2), y_);                           \
    y_ = __builtin_fma(BL_CI1, P(1), y_);                           \
    y_ = __builtin_fma(P(8), BL_CI8, y_);                           \
    y_ = __builtin_fma(BL_CI0, P(0), y_);                           \
    y_;                                                             \
  })
#define BL_FIR_INT_PAIR_(X, m) ((m) == 8 ? X(8) : X(m) + X(16 - (m)))
#define BL_FIR_INT(X)                                               \
  ({                                                                \
    const double ps_[9] = {BL_FIR_INT_PAIR_(X, 0), BL_FIR_INT_PAIR_(X, 1), BL_FIR_INT_PAIR_(X, 2),  \
                           BL_FIR_INT_PAIR_(X, 3), BL_FIR_INT_PAIR_(X, 4), BL_FIR_INT_PAIR_(X, 5),  \
                           BL_FIR_INT_PAIR_(X, 6), BL_FIR_INT_PAIR_(X, 7), BL_FIR_INT_PAIR_(X, 8)}; \
    BL_FIR_INT_P(BL_FIR_INT_PS_);                                   \
  })
#define BL_FIR_INT_PS_(m) ps_[m]

/* sc = 1 / (1e7 * 2 vprime) from the unevaluated sum rcp + rcp_lo = 1 / (2 vprime) (to ~2^-106, k_song_prep):
 * q = RN(rcp / 1e7); the remainder rcp - q * 1e7 is exact in one fma; adding rcp_lo and dividing again gives the
 * correction to a relative 2^-52 of itself, i.e. the true quotient to ~2^-104, which the last add rounds once:
 * the correctly rounded quotient unless it lies within 2^-50 ulp of a rounding boundary, and within one ulp always. */
BL_FIRI_HD double bl_firi_scale(double rcp, double rcp_lo) {
  const double q = rcp / BL_FIRI_UNSCALE;
  const double r = __builtin_fma(-q, BL_FIRI_UNSCALE, rcp) + rcp_lo;
  return q + r / BL_FIRI_UNSCALE;
}

/* kappa = 2 sc^2 = 2 / (1e7 * 2 vprime)^2, the factor FIR mode 2 applies to the power terms of the UNSCALED sums
 * (bl_fft512_power1_sq in bl_fft_tan.h) instead of sc to every sample.  From the same unevaluated rcp + rcp_lo: the
 * square in double-double (p + pe to ~2^-104), then the division by 1e14 (exact in f64) the way bl_firi_scale divides,
 * rounded once; the doubling is exact.  Not sc * sc, which would stack two roundings onto every term of a song. */
BL_FIRI_HD double bl_firi_power_scale(double rcp, double rcp_lo) {
  const double p = rcp * rcp;
  const double pe = __builtin_fma(rcp, rcp, -p) + 2.0 * (rcp * rcp_lo);
  const double q = p / 1e14;
  const double r = __builtin_fma(-q, 1e14, p) + pe;
  return 2.0 * (q + r / 1e14);
}

/* ---- the int8 matrix form ---- */

/* which of the 32 samples of a tile row byte e of word q of a plane holds on the lanes of K-group kb (0..3) */
BL_FIRI_HD int bl_firi_kappa(int kb, int q, int e) { return 8 * kb + 4 * q + e; }

BL_FIRI_HD unsigned bl_firi_perm(unsigned hi, unsigned lo, unsigned sel) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm(hi, lo, sel);
#else
  /* v_perm_b32 for selectors 0..7: result byte i is byte sel_i of the eight bytes hi:lo */
  const unsigned long long v = ((unsigned long long)hi << 32) | lo;
  unsigned r = 0;
  for (int i = 0; i < 4; ++i) r |= (unsigned)((v >> (8 * ((sel >> (8 * i)) & 7))) & 255) << (8 * i);
  return r;
#endif
}

/* The lane's 16 bytes of PCM — eight int16 samples kappa = bl_firi_kappa(kb, 0, 0) .. + 7, two to a word, as loaded —
 * into the plane of the l' (lp) and of the h (hp): byte e of word q belongs to sample 4 q + e. */
BL_FIRI_HD void bl_firi_sample_planes(const unsigned w[4], unsigned lp[2], unsigned hp[2]) {
  for (int q = 0; q < 2; ++q) {
    lp[q] = bl_firi_perm(w[2 * q + 1], w[2 * q], 0x06040200u) ^ 0x80808080u;
    hp[q] = bl_firi_perm(w[2 * q + 1], w[2 * q], 0x07050301u);
  }
}

/* The four digit planes of the tap matrix for output row b (0..15) on the lanes of K-group kb: byte e of word q of
 * plane j is digit j of the tap that meets sample kappa = bl_firi_kappa(kb, q, e), C_(16 + b - kappa). */
BL_FIRI_HD void bl_firi_tap_planes(int b, int kb, unsigned cp[4][2]) {
  for (int q = 0; q < 2; ++q) {
    unsigned v[4] = {0, 0, 0, 0};
    for (int e = 0; e < 4; ++e) {
      const int c = bl_firi_tap(16 + b - bl_firi_kappa(kb, q, e));
      for (int j = 0; j < 4; ++j) v[j] |= (unsigned)(bl_firi_digit(c, j) & 255) << (8 * e);
    }
    for (int j = 0; j < 4; ++j) cp[j][q] = v[j];
  }
}

/* K = (128 - mean) * sum C split over the initial values of a0, a2, a4 */
BL_FIRI_HD void bl_firi_const(int mean, int *k0, int *k2, int *k4) {
  const long long K = (long long)(128 - mean) * BL_FIRI_TAPSUM;
  *k0 = (int)(K & 0xFFFF);
  *k2 = (int)((K >> 16) & 0xFFFF);
  *k4 = (int)(K >> 32); /* arithmetic shift: floor */
}

/* the five weighted sums of one output -> Y (exact) */
BL_FIRI_HD double bl_firi_combine(int a0, int a1, int a2, int a3, int a4) {
  const int lo = a0 + a1 * 256;
  const int mid = a2 + a3 * 256 + a4 * 65536;
  return __builtin_fma((double)mid, 65536.0, (double)lo);
}

#endif /* BL_FIR_INT_H_ */
