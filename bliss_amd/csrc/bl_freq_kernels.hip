/*
 * bl_freq_kernels.hip — gfx950 kernels and launch layer of the frequency pass: the 512-point f32 DFT of every frame in
 * libavcodec's order (bl_fft_lavc.h), the power spectrum summed in the reference's order, the band score.  Must be
 * compiled with -ffp-contract=off: everything outside bl_fft.h follows the reference's unfused arithmetic.
 *
 * Kernels (reference code each one replaces):
 *   k_freq_frames  Hann + 512-pt f32 real DFT power, summed over the frames in the
 *                  reference's order            ref src/frequency_sort.c:67-94
 *   k_freq_scan    the same with the PCM statistics riding along (bl_scan.h; k_pcm_scan's
 *                  arithmetic, bl_stats_kernels.hip): what bl_analyze launches
 *   k_freq_finish  dB spectrum, 5 bands, score  ref src/frequency_sort.c:97-139
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>

#include "bl_freq_frames.h" /* freq_frames_lavc: the body of k_freq_frames / k_freq_scan, shared with the timbre kernel */

/* ------------------------------------------------------------------------- */
/* k_freq_frames / k_freq_scan                                                */

/*
 * Hann window + 512-point f32 real DFT + per-bin power, summed over the frames in the reference's order
 * (ref src/frequency_sort.c:67-94).  k_freq_frames is the frequency analysis alone (four waves per workgroup);
 * k_freq_scan is the same body with eight waves and the statistics pass riding along (see freq_frames_lavc, bl_freq_frames.h) —
 * what bl_analyze and the batch calls launch.
 *
 * One workgroup per song.  Every 16-lane group transforms TWO frames at once: all values are
 * 2-vectors (frame A in .x, frame B in .y), so the whole transform is v_pk_add / v_pk_mul_f32
 * on register pairs with no shuffling between the halves — twice the f32 rate of
 * the scalar VALU for the same instruction count (the one-frame-per-group kernel spent 40 % of
 * its VALU stream on v_mov's that re-paired (re, im) for the packed instructions hipcc formed).
 * A wave covers 8 consecutive frames per iteration, the WAVES waves 8 * WAVES.
 *
 * ref :88-93 adds every frame's power spectrum into one f32 accumulator per bin, frame after
 * frame; f32 addition does not associate, so the order is part of the result (15 000 frames
 * leave ~1e-5 of room in `frequency`).  The running spectrum goes round the waves like a baton:
 * wave w waits for the relay word to reach WAVES * it + w, adds its eight frames bin by bin in frame
 * order (its own power values re-laid out through its private exchange space: lane j owns bins
 * j, j + 64, j + 128, j + 192) and passes it on.  No workgroup barrier in the loop; the waves
 * stagger themselves.
 *
 * LDS: 4 WAVES exchange buffers of 272 (re, im) 2-vectors (16 bytes each: every exchange access is a
 * b128), twiddles, Hann, the running spectrum, the relay word: 76.9 KB for four waves -> two workgroups per
 * CU; 159.1 KB for eight waves with the histogram behind them -> one.  Either way two waves per SIMD (the
 * kernel wants ~200 VGPRs: 64 for the data, 64 for the frames in flight).
 */

/* one workgroup per song; the channel count is uniform per workgroup, so the branch costs one
 * scalar compare and each path keeps its compiled-in input side */
__global__ __launch_bounds__(256, 2) void k_freq_frames(const int16_t *__restrict__ pcm,
                                                        const bl_dsong *__restrict__ songs,
                                                        bl_tables tb, float *spectrum) {
  const bl_dsong sg = songs[blockIdx.x];
  if (sg.channels == 2) freq_frames_lavc<true, 4, false>(pcm, sg, tb, spectrum, nullptr, nullptr);
  else freq_frames_lavc<false, 4, false>(pcm, sg, tb, spectrum, nullptr, nullptr);
}

/* k_freq_scan: k_freq_frames and k_pcm_scan in one pass over the PCM — one 512-thread workgroup per song and CU
 * (the same eight waves per CU as two k_freq_frames workgroups, one histogram) */
__global__ __launch_bounds__(64 * BL_FREQ_SCAN_WAVES) void k_freq_scan(const int16_t *__restrict__ pcm,
                                                                       const bl_dsong *__restrict__ songs,
                                                                       bl_tables tb, float *spectrum,
                                                                       bl_dstats *stats, unsigned *hist) {
  const bl_dsong sg = songs[blockIdx.x];
  bl_dstats *st = stats + blockIdx.x;
  unsigned *gh = hist + (size_t)blockIdx.x * BL_HIST_BINS;
  if (sg.channels == 2) freq_frames_lavc<true, BL_FREQ_SCAN_WAVES, true>(pcm, sg, tb, spectrum, st, gh);
  else freq_frames_lavc<false, BL_FREQ_SCAN_WAVES, true>(pcm, sg, tb, spectrum, st, gh);
}

__global__ __launch_bounds__(256) void k_freq_finish(const float *__restrict__ spectrum,
                                                     const bl_dsong *__restrict__ songs,
                                                     bl_amd_song_result *res) {
  __shared__ float ps[256];
  __shared__ float wmax[4];
  const int d = threadIdx.x, song = blockIdx.x;
  const float acc = spectrum[(size_t)song * 256 + d];
  /* ref :97-102: sqrt(ps / 512), peak over d = 1..256 (ps[256] is 0) */
  float v = d == 0 ? 0.f : (float)sqrt((double)(acc / 512));
  float m = v;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_down(m, off));
  if ((d & 63) == 0) wmax[d >> 6] = m;
  __syncthreads();
  const float peak = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
  /* ref :105-107 */
  ps[d] = (float)(20 * log10((double)(v / peak)) - 3);
  __syncthreads();
  if (d == 0) { /* ref :110-139, f32 sequential sums, divisors 50 / 57 / 115 */
    float b0 = (ps[2] + ps[4]) / 2;
    float b1 = (ps[6] + ps[8]) / 2;
    float b2 = 0, b3 = 0, b4 = 0;
    for (int i = 10; i <= 60; ++i) b2 += ps[i];
    b2 /= 50;
    for (int i = 61; i <= 118; ++i) b3 += ps[i];
    b3 /= 57;
    for (int i = 119; i <= 234; ++i) b4 += ps[i];
    b4 /= 115;
    const float sum = b4 + b3 + b2 - b0 - b1;
    bl_amd_song_result *r = res + songs[song].out_idx;
    r->freq_peak = peak;
    r->v.frequency = (float)((1. / 3.) * (double)sum + 68. / 3.);
  }
}

/* ========================================================================= */
/* launchers (declared in bl_launch.h)                                        */

int blk_freq_configure_device(void) {
  BL_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_freq_frames),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, BL_FREQ_LDS_BYTES));
  BL_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_freq_scan),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, BL_FREQ_SCAN_LDS_BYTES));
  return BL_OK;
}

/* With all three analyzers asked for, the statistics ride along with the frequency pass (k_freq_scan): two
 * passes over the PCM instead of three.  A measurement build can take them apart again (BL_AMD_FUSED_SCAN=0). */
bool blk_freq_scan_fused(int what) {
  bool fused = what == 7;
#ifdef BL_AMD_MEASURE
  if (const char *e = getenv("BL_AMD_FUSED_SCAN")) fused = fused && atoi(e) != 0;
#endif
  return fused;
}

void blk_freq_scan(const blk_analyze_args &a) {
  Mark m(a.mark, a.mark_user, PK_FREQ_SCAN, a.stream);
  hipLaunchKernelGGL(k_freq_scan, dim3(a.n_songs), dim3(64 * BL_FREQ_SCAN_WAVES), BL_FREQ_SCAN_LDS_BYTES, a.stream,
                     a.pcm, a.songs, a.tb, a.spectrum, a.stats, a.hist);
}

void blk_freq_frames(const blk_analyze_args &a, hipStream_t s) {
  Mark m(a.mark, a.mark_user, PK_FREQ, s);
  hipLaunchKernelGGL(k_freq_frames, dim3(a.n_songs), dim3(256), BL_FREQ_LDS_BYTES, s, a.pcm,
                     a.songs, a.tb, a.spectrum);
}

void blk_freq_finish(const blk_analyze_args &a, hipStream_t s) {
  Mark m(a.mark, a.mark_user, PK_FREQ_FIN, s);
  hipLaunchKernelGGL(k_freq_finish, dim3(a.n_songs), dim3(256), 0, s, a.spectrum, a.songs,
                     a.results);
}
