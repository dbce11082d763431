/*
 * bl_kernels.hip — the launch order of the per-song analysis (blk_analyze): which stage runs on which stream behind
 * which event.  The stages' kernels and their launch functions are in one translation unit each:
 *   bl_stats_kernels.hip   PCM statistics, mean / variance, amplitude, force
 *   bl_freq_kernels.hip    frequency pass (with or without the statistics riding along)
 *   bl_env_kernels.hip     envelope windows and tail
 * (and, outside the analysis, bl_matrix_kernels.hip the pairwise matrix, bl_query_kernels.hip the vector queries,
 * bl_rs_kernels.hip the rate converter).  Also here: the constant tables the stages share, and two kernels that belong
 * to no stage:
 *   k_synth        integer synthetic PCM (benchmark corpus)
 *   k_narrow_s32   same-rate S32 -> S16 narrowing
 * Written for wave64 / 160 KiB LDS / 256 CUs; no other target is supported.
 */
#include <hip/hip_runtime.h>
#include <math.h>

#include "bl_launch.h"
#include "bl_fft_lavc.h"
#include "bl_fft_tan.h"

/* ------------------------------------------------------------------------- */
/* k_synth: integer-only synthetic PCM, same bytes as oracle/orc_synth.c       */

__device__ __forceinline__ unsigned syn_mix32(unsigned x) {
  x ^= x >> 16; x *= 0x7feb352dU;
  x ^= x >> 15; x *= 0x846ca68bU;
  x ^= x >> 16;
  return x;
}
__device__ __forceinline__ int syn_psin(unsigned ph) {
  const int x = (int)(ph & 65535u) - 32768;
  const int ax = x < 0 ? -x : x;
  return -((x * (32768 - ax)) / 8192);
}
__device__ __forceinline__ short syn_sample(unsigned seed, unsigned rate, unsigned channels,
                                            unsigned i) {
  const unsigned f = i / channels, c = i - f * channels;
  const unsigned h = syn_mix32(seed * 0x9E3779B9u + 1u);
  const unsigned f1 = 110u + (h & 255u);
  const unsigned f2 = 2000u + ((h >> 8) & 2047u);
  const unsigned bpm = 90u + ((h >> 20) & 63u);
  const unsigned a1 = 3000u + ((h >> 26) & 31u) * 100u;
  const unsigned period = rate * 60u / bpm;
  const unsigned pos = f % period;
  const int env = 32768 - (int)(((unsigned long long)pos * 29491u) / period);
  const unsigned ph1 = (unsigned)((((unsigned long long)f * f1) << 16) / rate);
  const unsigned ph2 = (unsigned)((((unsigned long long)f * f2) << 16) / rate) + c * 16384u;
  const int tone = (syn_psin(ph1) * (int)a1 + syn_psin(ph2) * 2500) / 32768;
  const int sig = (tone * env) / 32768;
  const int noise = (int)(syn_mix32(seed ^ syn_mix32(i + 0x1234567u)) % 1601u) - 800;
  return (short)(sig + noise);
}

__global__ __launch_bounds__(256) void k_synth(int16_t *pcm, const bl_dsong *__restrict__ songs,
                                               unsigned seed_base, unsigned rate) {
  const bl_dsong sg = songs[blockIdx.y];
  int16_t *p = pcm + sg.pcm_off;
  const unsigned seed = seed_base + (unsigned)sg.out_idx; /* records may be length-sorted */
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < (unsigned)sg.n; i += gridDim.x * 256u)
    p[i] = syn_sample(seed, rate, (unsigned)sg.channels, i);
}

/* ------------------------------------------------------------------------- */
/* small data-movement kernels of the batch / multi-device paths                */

/* same-rate S32 -> S16 narrowing of a 32-bit source (what the reference's resampler does
 * for an S32 input at the target rate, ref src/decode.c:388-392 -> swr_convert): arithmetic
 * shift by 16.  Parity unpinned (libswresample is absent). */
__global__ __launch_bounds__(256) void k_narrow_s32(const int4 *__restrict__ in, uint2 *__restrict__ out,
                                                    size_t nvec, const int32_t *__restrict__ in_s,
                                                    int16_t *__restrict__ out_s, size_t n) {
  const size_t stride = (size_t)gridDim.x * 256u;
  const size_t t = (size_t)blockIdx.x * 256u + threadIdx.x;
  for (size_t v = t; v < nvec; v += stride) { /* 16 bytes in, 8 bytes out per lane */
    const int4 q = in[v];
    uint2 o;
    o.x = ((unsigned)q.x >> 16) | ((unsigned)q.y & 0xFFFF0000u);
    o.y = ((unsigned)q.z >> 16) | ((unsigned)q.w & 0xFFFF0000u);
    out[v] = o;
  }
  for (size_t i = 4 * nvec + t; i < n; i += stride) out_s[i] = (int16_t)(in_s[i] >> 16);
}

/* ========================================================================= */
/* launchers (declared in bl_launch.h)                                        */

size_t blk_tables_bytes(void) {
  return 256 * 16 * 2 + 512 * 4 + LV_TW_SLOTS * 16 * 8 + sizeof(bl_fft_tan_lane<double>) * 16 + 128 * 16 + 128 * 16;
}

void blk_tables_fill_host(unsigned char *h) {
  /* twiddle / window tables, computed in double on the host */
  const double pi = 3.14159265358979323846;
  c2d *t256 = reinterpret_cast<c2d *>(h);
  c2d *t512 = t256 + 256;
  float *hann = reinterpret_cast<float *>(t512 + 256);
  for (int k = 0; k < 256; ++k) {
    t256[k].re = cos(2 * pi * k / 256); t256[k].im = -sin(2 * pi * k / 256);
    t512[k].re = cos(2 * pi * k / 512); t512[k].im = -sin(2 * pi * k / 512);
  }
  /* ref frequency_sort.c:40-42 */
  for (int i = 0; i < 512; ++i) hann[i] = (float)(.5f * (1.0f - cos(2 * M_PI * i / (512 - 1))));
  /* libavcodec's cosine tables, per lane and pass (bl_fft_lavc.h) */
  float leafc[4];
  lv_fill_tables(reinterpret_cast<float(*)[2]>(hann + 512), leafc);
  /* the tan-form constants of k_env_windows3's DFT (bl_fft_tan.h), long double on the host */
  unsigned char *tan_at = reinterpret_cast<unsigned char *>(hann + 512) + LV_TW_SLOTS * 16 * 8;
  bl_fft_tan_fill(reinterpret_cast<bl_fft_tan_lane<double> *>(tan_at),
                  reinterpret_cast<c2d *>(tan_at + sizeof(bl_fft_tan_lane<double>) * 16));
  bl_fft_sq_fill(reinterpret_cast<c2d *>(tan_at + sizeof(bl_fft_tan_lane<double>) * 16) + 128);
}

bl_tables blk_tables_bind(const void *d_mem) {
  bl_tables tb;
  const unsigned char *d = static_cast<const unsigned char *>(d_mem);
  tb.tw256_d = reinterpret_cast<const c2d *>(d);
  tb.tw512_d = tb.tw256_d + 256;
  tb.hann = reinterpret_cast<const float *>(tb.tw512_d + 256);
  tb.lv_tw = reinterpret_cast<const c2f *>(tb.hann + 512);
  tb.tan_lane = reinterpret_cast<const double *>(tb.lv_tw + LV_TW_SLOTS * 16);
  tb.tw512t = reinterpret_cast<const c2d *>(tb.tan_lane + 16 * BL_FFT_TAN_LANE_DOUBLES);
  tb.cs512 = tb.tw512t + 128;
  {
    float tw[LV_TW_SLOTS * 16][2];
    lv_fill_tables(tw, tb.lv_leafc);
  }
  tb.log101 = log((double)(1 + 100.0f)); /* ref tempo_atk_sort.c:188, log(1 + mu) */
  return tb;
}

int blk_configure_device(void) {
  if (blk_env_configure_device() != BL_OK || blk_freq_configure_device() != BL_OK) return BL_UNEXPECTED;
  return BL_OK;
}

/* sum, sum of squares, histogram, trim, mean and variance: the amplitude reads the histogram and the trim, the envelope
 * mean and variance; the frequency analysis (what == 2, bl_frequency_sort) nothing of it */
static bool wants_statistics(int what) { return (what & 5) != 0; }

/* analysis of one launch group (n_songs <= 32768: gridDim.y) */
int blk_analyze(const blk_analyze_args &a) {
  const int n_songs = a.n_songs, what = a.what;
  hipStream_t stream = a.stream;
  blk_stats_init(a);
  /* With all three analyzers asked for, the statistics ride along with the frequency pass (k_freq_scan): two
   * passes over the PCM instead of three.  The frequency analysis alone reads none of them: no statistics pass. */
  const bool fused = blk_freq_scan_fused(what);
  if (fused) blk_freq_scan(a);
  else if (wants_statistics(what) && blk_pcm_scan(a) != BL_OK) return BL_UNEXPECTED;
  if (wants_statistics(what)) blk_song_prep(a);
  /* Order: the envelope windows first, then the serial envelope tail (three latency-bound waves per 64 songs: it
   * leaves the chip free) beside what is left — the amplitude kernel and, when the statistics were not fused into
   * it, the frequency pass; k_force joins the two.  The tail's 143 KB workgroups only reach a CU when the dispatcher
   * has nothing else pending for it, so they have to be resident BEFORE the kernels they run beside begin:
   *   fused    the tail follows the window kernel on the main stream; amplitude and frequency finish go to the side
   *            stream behind an event (353.9 -> 349.9 ms per 8 192 songs: launched the other way round the
   *            amplitude kernel took the CUs first and the tail ran after it, not beside it);
   *   separate the tail goes to the side stream, the main stream runs the short amplitude kernel and then the wide
   *            frequency pass (launched after that pass, the tail started ~60 ms late). */
  bool tail_async = false, head_async = false;
  hipStream_t rest_stream = stream; /* where the amplitude kernel and the frequency finish go */
  if (what & 4) {
    const int fir_mode = blk_fir_mode();
    /* the serial tail of the songs [first, first + count), on the side stream when there is something to
     * overlap it with */
    const bool side = (what & 3) && a.side;
    auto launch_tail = [&](int first, int count, bool last) -> int {
      hipStream_t ts = stream;
      if (side && !last) {
        /* the long songs of a mixed batch: their tail goes to the second side stream, behind its own event, and runs
         * under the window kernel of the rest (on the first side stream it would stand in front of the amplitude
         * kernel and the frequency finish, which only wait for the window kernel behind this one) */
        BL_HIP_CHECK(hipEventRecord(a.ev_head, stream));
        BL_HIP_CHECK(hipStreamWaitEvent(a.side2, a.ev_head, 0));
        ts = a.side2;
        head_async = true;
      } else if (side && fused) {
        /* the tail stays here; the rest waits on the side stream for the window kernel in front of it */
        BL_HIP_CHECK(hipEventRecord(a.ev_env, stream));
        BL_HIP_CHECK(hipStreamWaitEvent(a.side, a.ev_env, 0));
        rest_stream = a.side;
        tail_async = true;
      } else if (side) {
        BL_HIP_CHECK(hipEventRecord(a.ev_env, stream));
        BL_HIP_CHECK(hipStreamWaitEvent(a.side, a.ev_env, 0));
        ts = a.side;
        tail_async = true;
      }
      blk_env_tail(a, ts, first, count);
      return BL_OK;
    };
    /* Mixed lengths (records sorted longest first): the tail of a ten-minute song is a ~15 ms serial chain, and
     * launched behind the window kernel of the whole batch it outlasts the frequency pass it is meant to hide
     * behind.  The long songs [0, n_head) get their own window launch, and their tail runs on the side stream
     * under the window kernel of the rest. */
    const int n_head = (a.n_head > 0 && a.n_head < n_songs && side && a.side2) ? a.n_head : 0;
    if (n_head) {
      if (blk_env_windows(a, fir_mode, 0, n_head, a.max_n) != BL_OK || launch_tail(0, n_head, false) != BL_OK)
        return BL_UNEXPECTED;
      if (blk_env_windows(a, fir_mode, n_head, n_songs - n_head, a.max_n_rest) != BL_OK ||
          launch_tail(n_head, n_songs - n_head, true) != BL_OK)
        return BL_UNEXPECTED;
    } else {
      if (blk_env_windows(a, fir_mode, 0, n_songs, a.max_n) != BL_OK || launch_tail(0, n_songs, true) != BL_OK)
        return BL_UNEXPECTED;
    }
  }
  if (what & 1) blk_amp_finish(a, rest_stream);
  if (what & 2) {
    if (!fused) blk_freq_frames(a, rest_stream);
    blk_freq_finish(a, rest_stream);
  }
  /* whatever ran on the side stream (tails, or the amplitude / frequency finish) joins the main stream here */
  if (tail_async) {
    BL_HIP_CHECK(hipEventRecord(a.ev_tail, a.side));
    BL_HIP_CHECK(hipStreamWaitEvent(stream, a.ev_tail, 0));
  }
  if (head_async) {
    BL_HIP_CHECK(hipEventRecord(a.ev_tail2, a.side2));
    BL_HIP_CHECK(hipStreamWaitEvent(stream, a.ev_tail2, 0));
  }
  if (what == 7) blk_force(a);
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}

/* what blk_analyze(what) writes of a.spectrum, a.stats and a.hist (bl_amd_last_freq_stats) */
int blk_analyze_parts(int what) {
  return (wants_statistics(what) ? BL_AMD_PART_SUMS | BL_AMD_PART_HIST : 0) | ((what & 2) ? BL_AMD_PART_SPECTRUM : 0);
}

int blk_synth(hipStream_t s, int16_t *pcm, const bl_dsong *d_songs, int n_songs, int max_n,
              int n_cu, unsigned seed_base, unsigned rate) {
  const int gx = grid_x_for(((long long)max_n + 255) / 256, n_songs, 8, n_cu);
  hipLaunchKernelGGL(k_synth, dim3(gx, n_songs), dim3(256), 0, s, pcm, d_songs, seed_base, rate);
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}

int blk_narrow_s32(hipStream_t s, const int32_t *d_in, int16_t *d_out, size_t n, int n_cu) {
  /* the vector body needs a 16-byte aligned input and an 8-byte aligned output; anything
   * else (and the last n % 4 elements) goes element by element */
  const bool aligned = ((reinterpret_cast<size_t>(d_in) & 15) == 0) && ((reinterpret_cast<size_t>(d_out) & 7) == 0);
  const size_t nvec = aligned ? n / 4 : 0;
  const size_t work = aligned ? nvec : n;
  size_t blocks = (work + 255) / 256;
  const size_t cap = (size_t)n_cu * 16;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(k_narrow_s32, dim3((unsigned)blocks), dim3(256), 0, s,
                     reinterpret_cast<const int4 *>(d_in), reinterpret_cast<uint2 *>(d_out), nvec, d_in,
                     d_out, n);
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}
