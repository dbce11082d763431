/*
 * bl_fir.h — the sample arithmetic in front of the envelope DFT: the 17-tap band-pass FIR of
 * ref src/tempo_atk_sort.c:109-138 in its three forms and the normalisation that feeds it.  k_env_windows3
 * (bl_env_kernels.hip) runs it; k_song_prep (bl_stats_kernels.hip) prepares its per-song constants from the same
 * taps (bl_dstats::rcp, rcp_lo, fsc).  Must be compiled with -ffp-contract=off: the FMAs here are the explicit ones.
 */
#ifndef BL_FIR_H_
#define BL_FIR_H_

#include <hip/hip_runtime.h>
#include "bl_fir_int.h"

/* FIR taps: literal digits of ref include/bandpass_coeffs.h:1-7 (symmetric) */
#define BL_C0 (-0.0023470)
#define BL_C1 0.0044613
#define BL_C2 (-0.0114627)
#define BL_C3 0.0226382
#define BL_C4 (-0.0405147)
#define BL_C5 0.0580037
#define BL_C6 (-0.0779167)
#define BL_C7 0.0882711
#define BL_C8 0.9065095

/* ref tempo_atk_sort.c:109-114 for one sample, halved: x/2 with x = RN(((s/2^15) - (mean/2^15)) / vd)
 * = RN(k / V), k = s - mean (exact), V = variance * 2^-15 (power-of-two scalings commute with
 * rounding).  With 1 / (2V) = r + r_lo to ~2^-106, kd*r + RN(kd*r_lo) is k / (2V) with a relative
 * error below 2^-104 before the fma's single rounding; k / (2V) = k * 2^14 / variance with
 * |k| < 2^17, variance < 2^31 is either exactly representable or at least 2^-70 (relative) away
 * from the nearest rounding boundary, so the result is the correctly rounded quotient.
 * Why halved: every operation downstream (add, multiply by a constant, fma) scales exactly by a
 * power of two — nothing here comes near the subnormals — so the FIR outputs are y/2, the
 * spectrum X/2 and the power terms |X|^2 / 4 with bit-identical mantissas: the 1/4 that the
 * real-input split of the DFT owes (bl_fft512_power1) comes for free. */
__device__ __forceinline__ double bl_norm(int k, double rcp, double rcp_lo) {
  const double kd = (double)k;
  return __builtin_fma(kd, rcp, kd * rcp_lo);
}

/* ref :123-138.  The reference starts from y = 0 and adds nine products; 0 + c7 * p is c7 * p
 * bit for bit here (p = +0 gives +0: the inputs are never -0), so the first add is not issued. */
#define BL_FIR(X)                                                   \
  ({                                                                \
    double y_ = BL_C7 * (X(7) + X(9));                              \
    y_ += BL_C6 * (X(6) + X(10));                                   \
    y_ += BL_C5 * (X(5) + X(11));                                   \
    y_ += BL_C4 * (X(4) + X(12));                                   \
    y_ += BL_C3 * (X(3) + X(13));                                   \
    y_ += BL_C2 * (X(2) + X(14));                                   \
    y_ += BL_C1 * (X(1) + X(15));                                   \
    y_ += X(8) * BL_C8;                                             \
    y_ += BL_C0 * (X(0) + X(16));                                   \
    y_;                                                             \
  })

/* The same sum with each product folded into the running sum by an fma: eight roundings fewer per
 * output and eight instructions fewer (17 instead of 25).  NOT the reference's arithmetic: an
 * output differs by a few 1e-16 of its largest partial sum, which is the class of difference the
 * DFT behind it already has (ours, not FFTW's) and which the results see only through the f32
 * roundings of the ordered sum.  Selected by BL_AMD_FIR_FUSED=1; DESIGN.md §4.1 has the measured
 * flip rates that decide whether it is used. */
#define BL_FIR_FUSED(X)                                             \
  ({                                                                \
    double y_ = BL_C7 * (X(7) + X(9));                              \
    y_ = __builtin_fma(BL_C6, X(6) + X(10), y_);                    \
    y_ = __builtin_fma(BL_C5, X(5) + X(11), y_);                    \
    y_ = __builtin_fma(BL_C4, X(4) + X(12), y_);                    \
    y_ = __builtin_fma(BL_C3, X(3) + X(13), y_);                    \
    y_ = __builtin_fma(BL_C2, X(2) + X(14), y_);                    \
    y_ = __builtin_fma(BL_C1, X(1) + X(15), y_);                    \
    y_ = __builtin_fma(X(8), BL_C8, y_);                            \
    y_ = __builtin_fma(BL_C0, X(0) + X(16), y_);                    \
    y_;                                                             \
  })
/* Mode 2: the normalisation folded into the filter, on the integers.  k = s - mean is an exact integer and the taps
 * are integers times 1e-7, so the whole sum Y = sum C_m k[j - m] is formed exactly; the per-song scale
 * sc = 1e-7 / (2 vprime) (k_song_prep) is applied, squared, to the power terms of the transform of Y: no rounding
 * per output at all.  bl_fir_int.h has the two forms that give that Y —
 * BL_FIR_INT, in f64, and the int8 matrix products of the kernel's main loop — and the argument. */
#ifndef BL_FIR_FUSED_DEFAULT
#define BL_FIR_FUSED_DEFAULT 2
#endif
/* mode 2 yields the unscaled Y: k_env_windows3 applies sc squared to the power terms (bl_fft512_power1_sq) */
#define BL_FIR_SEL(MODE, X) ((MODE) == 2 ? BL_FIR_INT(X) : (MODE) == 1 ? BL_FIR_FUSED(X) : BL_FIR(X))

#endif /* BL_FIR_H_ */
