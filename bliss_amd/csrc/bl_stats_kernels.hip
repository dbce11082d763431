/*
 * bl_stats_kernels.hip — gfx950 kernels and launch layer of the PCM statistics and of what is computed from them
 * alone: mean / variance, the amplitude score, and the force that joins the four scores.  Must be compiled with
 * -ffp-contract=off, like every kernel file: the reference's arithmetic is unfused.
 *
 * Kernels (reference code each one replaces):
 *   k_pcm_scan     sum, sum of squares, central histogram in one pass
 *                                               ref src/helpers.c:30-49,
 *                                               src/amplitude_sort.c:33-39
 *   k_trim         first / last non-zero sample  ref src/amplitude_sort.c:26-31
 *   k_song_prep    bl_mean / bl_variance values, start/end, reciprocal used by
 *                  the normalisation            ref src/tempo_atk_sort.c:101-107
 *   k_variance_wrap  exact int32-wrapping bl_variance for |mean| > 13571
 *   k_amp_finish   301-pass smoothing + integral ref src/amplitude_sort.c:41-79
 *   k_force        force, calm_or_loud          ref src/analyze.c:63-80
 * With all three analyzers asked for the scan rides along with the frequency pass instead (k_freq_scan,
 * bl_freq_kernels.hip); the per-word arithmetic both use is bl_scan.h.
 */
#include <hip/hip_runtime.h>
#include <math.h>

#include "bl_launch.h"
#include "bl_scan.h"
#include "bl_fir.h"

/* ------------------------------------------------------------------------- */
/* k_pcm_scan                                                                 */

/* sum, sum of squares and the central histogram of every song; the first / last non-zero sample is k_trim's.
 * Per 16-byte vector (8 samples): sums through v_dot2_i32_i16 (lo + hi and lo^2 + hi^2 per word; the latter read
 * as unsigned is exact up to 2^31), the histogram through scan_hist_word.  Two vectors per iteration keep two
 * loads in flight per lane. */
template <bool HIST>
__global__ __launch_bounds__(256) void k_pcm_scan(const int16_t *__restrict__ pcm,
                                                  const bl_dsong *__restrict__ songs,
                                                  bl_dstats *stats, unsigned *hist) {
  __shared__ unsigned lh[BL_HIST_BINS]; /* the only LDS of this kernel: nothing lies behind it */
  if (__builtin_amdgcn_groupstaticsize() != sizeof lh) __builtin_trap(); /* somebody added LDS: see scan_hist_word */
  const int tid = threadIdx.x;
  const bl_dsong sg = songs[blockIdx.y];
  const int16_t *p = pcm + sg.pcm_off;
  for (int i = tid; i < BL_HIST_BINS; i += 256) lh[i] = 0;
  __syncthreads();
  unsigned lds_base = (unsigned)(size_t)(bl_lds_u32 *)lh;
  asm volatile("" : "+v"(lds_base)); /* lives in a VGPR: as a scalar it is copied in front of every use */

  long long sum = 0;
  unsigned long long sq = 0;
  const unsigned nvec = (unsigned)sg.n >> 3;
  const uint4 *pv = reinterpret_cast<const uint4 *>(p);
  auto eat = [&](const uint4 q) {
    const unsigned w[4] = {q.x, q.y, q.z, q.w};
    int s32 = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) scan_word(w[k], s32, sq, lds_base, HIST);
    sum += s32;
  };
  const unsigned gstride = gridDim.x * 256u;
  unsigned v = blockIdx.x * 256u + tid;
  for (; v + gstride < nvec; v += 2 * gstride) {
    const uint4 q0 = pv[v], q1 = pv[v + gstride];
    eat(q0);
    eat(q1);
  }
  if (v < nvec) eat(pv[v]);
  if (blockIdx.x == 0 && tid < (sg.n & 7)) { /* the samples behind the last whole vector */
    const int sv = (int)p[8u * nvec + tid];
    sum += sv;
    sq += (unsigned)(sv * sv);
    const unsigned b = (unsigned)(sv + BL_HIST_BINS / 2);
    if (HIST && b < BL_HIST_BINS) atomicAdd(&lh[b], 1u);
  }
  /* wave reduction, then one pair of atomics per wave */
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    sum += __shfl_down(sum, off);
    sq += __shfl_down(sq, off);
  }
  bl_dstats *st = stats + blockIdx.y;
  if ((tid & 63) == 0) {
    atomicAdd(&st->sum, (unsigned long long)sum);
    atomicAdd(&st->sumsq, sq);
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); /* the inline-asm adds are invisible to hipcc's counters */
  __syncthreads();
  unsigned *gh = hist + (size_t)blockIdx.y * BL_HIST_BINS;
  for (int i = tid; i < BL_HIST_BINS; i += 256) {
    const unsigned c = lh[i];
    if (c) atomicAdd(&gh[i], c);
  }
}

/* k_trim: the first and the last non-zero sample of every song (ref amplitude_sort.c:26-31, the two trim loops).
 * They sit within a few thousand samples of the ends of any real recording, so this is a search, not a pass: one
 * workgroup per song, wave 0 walks forward and wave 1 backward, 1 024 samples per step, until a vector with a
 * non-zero sample turns up.  (Tracked inside k_pcm_scan's loop it cost 14 instructions per 8 samples.)  An
 * all-zero song is the only one searched to the end; it is refused anyway (k_song_prep). */
__global__ __launch_bounds__(128) void k_trim(const int16_t *__restrict__ pcm, const bl_dsong *__restrict__ songs,
                                              bl_dstats *stats) {
  const bl_dsong sg = songs[blockIdx.x];
  const int16_t *p = pcm + sg.pcm_off;
  const uint4 *pv = reinterpret_cast<const uint4 *>(p);
  const int lane = threadIdx.x & 63, n = sg.n;
  const int nvec = n >> 3;
  const bool fwd = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) == 0;
  bl_dstats *st = stats + blockIdx.x;
  /* position of the first (fwd) / last non-zero 16-bit half of a non-zero vector */
  auto locate = [&](const uint4 q) -> int {
    const unsigned w[4] = {q.x, q.y, q.z, q.w};
    int at = fwd ? 8 : -1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (fwd) {
        if (w[3 - k] >> 16) at = 2 * (3 - k) + 1;
        if (w[3 - k] & 0xFFFFu) at = 2 * (3 - k);
      } else {
        if (w[k] & 0xFFFFu) at = 2 * k;
        if (w[k] >> 16) at = 2 * k + 1;
      }
    }
    return at;
  };
  if (fwd) {
    unsigned first = 0xFFFFFFFFu;
    for (int v0 = 0; v0 < nvec; v0 += 128) {
      const int va = v0 + lane, vb = v0 + 64 + lane;
      const uint4 z = make_uint4(0, 0, 0, 0);
      const uint4 qa = va < nvec ? pv[va] : z, qb = vb < nvec ? pv[vb] : z;
      const unsigned long long ma = __ballot((qa.x | qa.y | qa.z | qa.w) != 0u);
      const unsigned long long mb = __ballot((qb.x | qb.y | qb.z | qb.w) != 0u);
      if (ma | mb) {
        const int src = ma ? __builtin_ctzll(ma) : __builtin_ctzll(mb);
        const unsigned mine = 8u * (unsigned)(ma ? va : vb) + (unsigned)locate(ma ? qa : qb);
        first = (unsigned)__shfl((int)mine, src);
        break;
      }
    }
    if (first == 0xFFFFFFFFu) /* nothing in the whole vectors: the up to seven samples behind them */
      for (int i = 8 * nvec; i < n; ++i)
        if (p[i] != 0) { first = (unsigned)i; break; }
    if (lane == 0) st->first = first;
  } else {
    int last = -1;
    for (int i = n - 1; i >= 8 * nvec; --i)
      if (p[i] != 0) { last = i; break; }
    if (last < 0)
      for (int v1 = nvec; v1 > 0; v1 -= 128) { /* vectors [v1 - 128, v1) */
        const int va = v1 - 1 - lane, vb = v1 - 65 - lane;
        const uint4 z = make_uint4(0, 0, 0, 0);
        const uint4 qa = va >= 0 ? pv[va] : z, qb = vb >= 0 ? pv[vb] : z;
        const unsigned long long ma = __ballot((qa.x | qa.y | qa.z | qa.w) != 0u);
        const unsigned long long mb = __ballot((qb.x | qb.y | qb.z | qb.w) != 0u);
        if (ma | mb) { /* lane 0 holds the highest vector of each half */
          const int src = ma ? __builtin_ctzll(ma) : __builtin_ctzll(mb);
          const int mine = 8 * (ma ? va : vb) + locate(ma ? qa : qb);
          last = __shfl(mine, src);
          break;
        }
      }
    if (lane == 0) st->last = last;
  }
}

__global__ void k_stats_init(bl_dstats *stats, int n_songs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_songs) return;
  bl_dstats s;
  s.sum = 0; s.sumsq = 0; s.first = 0xFFFFFFFFu; s.last = -1;
  s.mean = 0; s.variance = 0; s.vprime = 0; s.rcp = 0; s.rcp_lo = 0; s.fsc = 0; s.kappa = 0; s.wrap_pass = 0; s.status = BL_OK;
  s.wrap_acc = 0;
  stats[i] = s;
}

/* ------------------------------------------------------------------------- */
/* k_song_prep: one thread per song                                           */

__device__ __forceinline__ void prep_finish(bl_dstats &s, int n) {
  if (s.variance == 0) s.status = BL_UNEXPECTED; /* reference divides by zero */
  /* ref tempo_atk_sort.c:105-113: x = (s/2^15 - mean/2^15) / (var/2^30)
   *   = RN((s - mean) / (var * 2^-15)) exactly (power-of-two scalings commute
   *   with rounding); vprime and its reciprocal feed bl_norm() (bl_fir.h). */
  s.vprime = (double)s.variance / 32768.0;
  /* The envelope kernel works on x / 2 (an exact scaling: see bl_norm), so the reciprocal is
   * that of 2 * vprime, as an unevaluated sum rcp + rcp_lo accurate to ~2^-106. */
  const double v2 = 2.0 * s.vprime;
  s.rcp = 1.0 / v2;
  s.rcp_lo = __builtin_fma(-s.rcp, v2, 1.0) / v2;
  /* FIR mode 2 filters the integers with the integer taps and scales once (bl_fir_int.h): within one ulp of
   * 1e-7 / (2 vprime), correctly rounded but for near-ties */
  s.fsc = bl_firi_scale(s.rcp, s.rcp_lo);
  /* the kernel leaves the sums unscaled and multiplies the power terms instead: 2 fsc^2 from the same rcp + rcp_lo,
   * rounded once */
  s.kappa = bl_firi_power_scale(s.rcp, s.rcp_lo);
  (void)n;
}

__global__ void k_song_prep(const bl_dsong *__restrict__ songs, bl_dstats *stats, int n_songs,
                            bl_amd_song_result *res) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_songs) return;
  bl_dstats s = stats[i];
  const bl_dsong sg = songs[i];
  const int n = sg.n;
  if (s.first == 0xFFFFFFFFu) { /* all-zero PCM: the reference's trim loops never end */
    s.status = BL_UNEXPECTED;
    s.first = 0; s.last = n - 1;
  }
  /* ref helpers.c:30-37: int32 accumulator (wraps), C truncating division */
  const int wrapped = (int)(unsigned)(s.sum & 0xFFFFFFFFull);
  s.mean = wrapped / n;
  /* ref helpers.c:39-49: sum of (int32)(v*v), v = sample - mean.  Without int32
   * overflow of v*v (|v| <= 46340, guaranteed when |mean| <= 13571) this is
   * sumsq - 2*mean*sum + n*mean^2 in exact integer arithmetic. */
  const long long m = s.mean;
  if (m > 13571 || m < -13571) {
    s.wrap_pass = 1;
  } else {
    const long long acc = (long long)s.sumsq - 2 * m * (long long)s.sum + (long long)n * m * m;
    s.variance = (int)(acc / n);
    prep_finish(s, n);
  }
  stats[i] = s;
  bl_amd_song_result *r = res + sg.out_idx;
  r->start = (int)s.first; r->end = s.last;
  r->mean = s.mean; r->variance = s.variance;
  r->n_frames = sg.n_frames; r->nb_frames = sg.nb_frames; r->n_windows = sg.n_windows;
  r->status = s.status;
}

/* exact restatement of ref helpers.c:39-49 including the int32 wrap of v*v;
 * only songs flagged by k_song_prep do any work */
__global__ __launch_bounds__(256) void k_variance_wrap(const int16_t *__restrict__ pcm,
                                                       const bl_dsong *__restrict__ songs,
                                                       bl_dstats *stats) {
  bl_dstats *st = stats + blockIdx.y;
  if (!st->wrap_pass) return;
  const bl_dsong sg = songs[blockIdx.y];
  const int16_t *p = pcm + sg.pcm_off;
  const int mean = st->mean;
  long long acc = 0;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < (unsigned)sg.n; i += gridDim.x * 256u) {
    const int v = (int)p[i] - mean;
    acc += (int)((unsigned)v * (unsigned)v);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
  if ((threadIdx.x & 63) == 0)
    atomicAdd(reinterpret_cast<unsigned long long *>(&st->wrap_acc), (unsigned long long)acc);
}

__global__ void k_variance_wrap_finish(const bl_dsong *__restrict__ songs, bl_dstats *stats,
                                       int n_songs, bl_amd_song_result *res) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_songs) return;
  bl_dstats s = stats[i];
  if (!s.wrap_pass) return;
  s.variance = (int)(s.wrap_acc / songs[i].n);
  prep_finish(s, songs[i].n);
  stats[i] = s;
  res[songs[i].out_idx].variance = s.variance;
  res[songs[i].out_idx].status = s.status;
}

/* ------------------------------------------------------------------------- */
/* k_amp_finish: one block per song                                           */

#define BL_AMP_PASSES 301                         /* g = 0..300, ref amplitude_sort.c:41 */
#define BL_INT_LO ((32767 - 1000) - BL_HIST_LO)   /* local index of INTEGRAL_INF */
#define BL_INT_HI ((32767 + 1000) - BL_HIST_LO)   /* local index of INTEGRAL_SUP */

__global__ __launch_bounds__(256) void k_amp_finish(const bl_dsong *__restrict__ songs,
                                                    const bl_dstats *__restrict__ stats,
                                                    const unsigned *__restrict__ hist,
                                                    bl_amd_song_result *res) {
  __shared__ float buf[2][BL_HIST_BINS + 8];
  const int tid = threadIdx.x;
  const int song = blockIdx.x;
  const bl_dstats st = stats[song];
  const int n = songs[song].n;
  const unsigned *gh = hist + (size_t)song * BL_HIST_BINS;
  const int start = (int)st.first, end = st.last;
  if (tid < 8) { /* 3 zero cells left of bin 0, 5 right of the last bin */
    const int c = tid < 3 ? tid : BL_HIST_BINS + tid;
    buf[0][c] = 0.f; buf[1][c] = 0.f;
  }
  for (int i = tid; i < BL_HIST_BINS; i += 256) {
    unsigned c = gh[i];
    /* samples outside [start, end] are zeros and are not counted (ref :26-39) */
    if (i == BL_HIST_BINS / 2) c -= (unsigned)start + (unsigned)(n - 1 - end);
    /* float += 1 stops growing at 2^24 */
    buf[0][i + 3] = (float)min(c, 16777216u);
  }
  __syncthreads();
  int cur = 0;
  for (int g = 0; g < BL_AMP_PASSES; ++g) {
    const float *h = buf[cur] + 3;
    float *s = buf[cur ^ 1] + 3;
    /* only bins that can still reach the integral window [BL_INT_LO, BL_INT_HI] through the passes
     * that remain (3 bins per pass) are updated: from 3 807 of them in the first pass down to 2 001 */
    const int reach = 3 * (BL_AMP_PASSES - 1 - g);
    const int lo = max(BL_INT_LO - reach, 0), hi = min(BL_INT_HI + reach, BL_HIST_BINS - 1);
    for (int i = lo + tid; i <= hi; i += 256) {
      /* ref :49-55: f32 sum left to right, times (double)(1/27), stored as f32 */
      float acc = h[i - 3] + (3 * h[i - 2]);
      acc = acc + (6 * h[i - 1]);
      acc = acc + (7 * h[i]);
      acc = acc + (6 * h[i + 1]);
      acc = acc + (3 * h[i + 2]);
      acc = acc + h[i + 3];
      s[i] = (float)(1. / 27. * (double)acc);
    }
    __syncthreads();
    cur ^= 1;
  }
  /* ref :62-66 then :69-71 */
  float *s = buf[cur] + 3;
  float *v = buf[cur ^ 1] + 3;
  const float denom = (float)(start - end);
  for (int i = BL_INT_LO + tid; i <= BL_INT_HI; i += 256) {
    float t = s[i] / denom;
    t = (float)((double)t * 100.);
    v[i] = fabsf(t);
  }
  __syncthreads();
  if (tid == 0) {
    float integral = 0;
    for (int i = BL_INT_LO; i <= BL_INT_HI; ++i) integral += v[i];
    bl_amd_song_result *r = res + songs[song].out_idx;
    r->hist_integral = integral;
    r->v.amplitude = -0.2f * integral + 6.0f; /* ref :79 */
  }
}

/* ref analyze.c:63-80: force = fmax(tempo,0) + amplitude + frequency + fmax(attack,0)
 * (double sum, stored as float), then LOUD / CALM / UNKNOWN by its sign */
__global__ void k_force(bl_amd_song_result *res, int n_songs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_songs) return;
  bl_amd_song_result *r = res + i;
  const float rating = (float)(fmax((double)r->v.tempo, 0.0) + (double)r->v.amplitude +
                               (double)r->v.frequency + fmax((double)r->v.attack, 0.0));
  r->force = rating;
  r->calm_or_loud = rating > 0 ? BL_LOUD : (rating < 0 ? BL_CALM : BL_UNKNOWN);
}

/* ========================================================================= */
/* launchers (declared in bl_launch.h)                                        */

/* grid.x of the kernels that stride over the 16-byte vectors of songs of up to max_n samples */
static int scan_grid_x(int max_n, int n_songs, int n_cu) {
  return grid_x_for(((long long)max_n / 8 + 255) / 256, n_songs, 8, n_cu);
}

void blk_stats_init(const blk_analyze_args &a) {
  hipLaunchKernelGGL(k_stats_init, dim3((a.n_songs + 63) / 64), dim3(64), 0, a.stream, a.stats, a.n_songs);
}

int blk_pcm_scan(const blk_analyze_args &a) {
  BL_HIP_CHECK(hipMemsetAsync(a.hist, 0, sizeof(unsigned) * BL_HIST_BINS * (size_t)a.n_songs, a.stream));
  Mark m(a.mark, a.mark_user, PK_SCAN, a.stream);
  hipLaunchKernelGGL(k_pcm_scan<true>, dim3(scan_grid_x(a.max_n, a.n_songs, a.n_cu), a.n_songs), dim3(256), 0,
                     a.stream, a.pcm, a.songs, a.stats, a.hist);
  return BL_OK;
}

void blk_song_prep(const blk_analyze_args &a) {
  const int n_songs = a.n_songs, tb64 = (n_songs + 63) / 64;
  hipStream_t stream = a.stream;
  hipLaunchKernelGGL(k_trim, dim3(n_songs), dim3(128), 0, stream, a.pcm, a.songs, a.stats);
  hipLaunchKernelGGL(k_song_prep, dim3(tb64), dim3(64), 0, stream, a.songs, a.stats, n_songs,
                     a.results);
  hipLaunchKernelGGL(k_variance_wrap, dim3(scan_grid_x(a.max_n, n_songs, a.n_cu), n_songs), dim3(256), 0, stream,
                     a.pcm, a.songs, a.stats);
  hipLaunchKernelGGL(k_variance_wrap_finish, dim3(tb64), dim3(64), 0, stream, a.songs, a.stats,
                     n_songs, a.results);
}

void blk_amp_finish(const blk_analyze_args &a, hipStream_t s) {
  Mark m(a.mark, a.mark_user, PK_AMP, s);
  hipLaunchKernelGGL(k_amp_finish, dim3(a.n_songs), dim3(256), 0, s, a.songs, a.stats, a.hist,
                     a.results);
}

void blk_force(const blk_analyze_args &a) {
  hipLaunchKernelGGL(k_force, dim3((a.n_songs + 63) / 64), dim3(64), 0, a.stream, a.results, a.n_songs);
}

int blk_scan_one(hipStream_t s, const int16_t *pcm, const bl_dsong *d_songs, bl_dstats *d_stats,
                 unsigned *d_hist, int n, int n_cu) {
  const int gx = scan_grid_x(n, 1, n_cu);
  BL_HIP_CHECK(hipMemsetAsync(d_hist, 0, sizeof(unsigned) * BL_HIST_BINS, s));
  hipLaunchKernelGGL(k_stats_init, dim3(1), dim3(64), 0, s, d_stats, 1);
  hipLaunchKernelGGL(k_pcm_scan<true>, dim3(gx, 1), dim3(256), 0, s, pcm, d_songs, d_stats, d_hist);
  hipLaunchKernelGGL(k_trim, dim3(1), dim3(128), 0, s, pcm, d_songs, d_stats);
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}

int blk_variance_wrap_one(hipStream_t s, const int16_t *pcm, const bl_dsong *d_songs,
                          bl_dstats *d_stats, int n, int n_cu) {
  const int gx = scan_grid_x(n, 1, n_cu);
  hipLaunchKernelGGL(k_variance_wrap, dim3(gx, 1), dim3(256), 0, s, pcm, d_songs, d_stats);
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}
