/*
 * bl_tpeak_table.h — the 4-phase, 12-tap interpolator of the true peak (include/bliss_amd.h: bl_amd_tpeak_*), in Q14.
 * It is the definition: y[4t + p] = sum over j = -5 .. 6 of BL_TPEAK_G[p][j + 5] * x[t + j].
 *
 * Provenance (tests/tpeak_reference.py regenerates the table and compares): G[p][j + 5] = floor(2^14 w(m) sinc(m / 4)
 * + 1/2) with m = 4 j - p, w(m) = (1 + cos(pi m / 24)) / 2 for |m| < 24 and 0 otherwise, sinc(0) = 1: a Hann-windowed
 * sinc at four times the rate.  Phase 0 is the sample times 2^14.  The rows sum to 16384 / 16392 / 16400 / 16392; the
 * largest row l1 norm is 30544 (phase 2), so |y| <= 30544 * 32768 = 1000865792 < 2^30.
 * Plain C, included by bl_api.c (bl_amd_tpeak_table) and bl_tpeak_kernels.hip.
 */
#ifndef BL_TPEAK_TABLE_H_
#define BL_TPEAK_TABLE_H_

#define BL_TPEAK_PHASES 4
#define BL_TPEAK_TAPS 12
#define BL_TPEAK_FRONT 5 /* frames in front of t that a frame's sums read */
#define BL_TPEAK_BACK 6  /* frames behind it */

#define BL_TPEAK_G_ROWS                                                            \
  {0, 0, 0, 0, 0, 16384, 0, 0, 0, 0, 0, 0},                                        \
  {-27, 170, -493, 1133, -2645, 14688, 4730, -1695, 758, -304, 80, -3},            \
  {-16, 170, -552, 1313, -2968, 10253, 10253, -2968, 1313, -552, 170, -16},        \
  {-3, 80, -304, 758, -1695, 4730, 14688, -2645, 1133, -493, 170, -27}

static const int BL_TPEAK_G[BL_TPEAK_PHASES][BL_TPEAK_TAPS] = {BL_TPEAK_G_ROWS};

#endif /* BL_TPEAK_TABLE_H_ */
