/*
 * bl_tgram_kernels.hip — gfx950 kernels and launch layer of the tempo over time (bl_amd_tgram_device,
 * include/bliss_amd.h: bl_amd_tgram_frame, bl_amd_song_tgram).  Every quantity is an exact integer (the definitions are
 * in the header), so neither the cut of a song into runs nor the order in which block rows enter a frame shows in a
 * result.
 *
 * Kernels:
 *   k_tgram_blocks  one run of frames of one song per workgroup: the block rows P_b[tau] = the lag products of the S
 *                   terms of block b, a ring of the last m of them in LDS, the frame's row as a running sum, and the
 *                   pick of stage 8 on every frame's row
 *   k_tgram_songs   one wavefront per song over the frames' lags: the song record, with a 512-bin histogram in LDS for
 *                   the median and n_near
 *
 * Sharing.  Frame f is the sum of the block rows f .. f + m - 1, so R_{f+1} = R_f - P_f + P_{f+m}: the workgroup
 * keeps R in registers (the lanes that own a lag own its sum), the block rows it still has to retire in the ring, and
 * forms every block row once.  The multiply-adds of a song are those of k_rhythm_acf over the same curve, whatever m
 * is.  A run recomputes the m - 1 blocks in front of its first complete frame, so a song cut into runs of r frames
 * costs (r + m - 1) / r of that.  The subtraction is exact: R_f < 2^50, and unsigned 64-bit arithmetic has no rounding
 * to accumulate.
 *
 * Products.  The lane mapping of k_rhythm_acf: thread t of 256 has the lags 4 g .. 4 g + 3 with g = t mod 128 and every
 * second group of eight terms (t / 128); S is a multiple of 16, so the two halves take S / 16 groups each.  Per group
 * two broadcast b128 reads of the left factors and three b128 reads of the twelve right factors o[hb + 4 g .. + 11]
 * feed 32 products into four 64-bit sums.  The curve is staged tile by tile: max(1, 1024 / S) whole blocks and 512
 * hops of look-ahead, zero from hop H on.  The last term of the last frame is below T = H - 511, so no left factor
 * needs zeroing, and the highest index read is (the tile's terms) - 8 + 508 + 11, inside the staged span.
 *
 * LDS.  The ring is dynamic, m rows of 4 KB; beside it 6 KB of curve, 4 KB where the halves meet and 4 KB of the
 * frame's row for the pick: 78 KB at m = 16, which leaves room for two workgroups on a compute unit.
 */
#include <hip/hip_runtime.h>

#include "bl_tgram.h"

typedef unsigned long long bl_u64;

#define TG_LAGS BL_AMD_RHYTHM_LAGS
#define TG_STAGE (BL_TGRAM_TILE + TG_LAGS) /* hops of o a tile stages: its terms and the look-ahead */
#define TG_STATIC_LDS (4 * TG_STAGE + 16 * TG_LAGS + 128)
#define TG_NONE (1 << 30)

/* The pick of k_rhythm_pick on the row in LDS, spread over the workgroup: thread t has tau = t and t + 256.  The
 * callers' barriers: the row is complete before this is entered, and it is not written again before every thread has
 * left. */
__device__ __forceinline__ void tg_pick(const bl_u64 *row, int lag_min, int lag_max, bl_u64 *wpeak, int *wlag,
                                        int *wlag_peak, bl_amd_tgram_frame *rec) {
  const int tid = threadIdx.x, wave = tid >> 6;
  bl_u64 v[2], peak = 0;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int tau = tid + 256 * j;
    v[j] = row[tau];
    if (tau >= lag_min && tau <= lag_max && v[j] > peak) peak = v[j];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const bl_u64 o = __shfl_xor(peak, off);
    peak = o > peak ? o : peak;
  }
  if ((tid & 63) == 0) wpeak[wave] = peak;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < 4; ++w) peak = wpeak[w] > peak ? wpeak[w] : peak;
  int lag_peak = TG_NONE, lag = TG_NONE;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int tau = tid + 256 * j;
    if (tau < lag_min || tau > lag_max) continue; /* 1 <= tau <= 510: both neighbours are in the row */
    if (v[j] == peak) lag_peak = min(lag_peak, tau);
    if (v[j] >= row[tau - 1] && v[j] >= row[tau + 1] && 16 * v[j] >= 15 * peak) lag = min(lag, tau);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lag_peak = min(lag_peak, __shfl_xor(lag_peak, off));
    lag = min(lag, __shfl_xor(lag, off));
  }
  if ((tid & 63) == 0) {
    wlag[wave] = lag;
    wlag_peak[wave] = lag_peak;
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      lag = min(lag, wlag[w]);
      lag_peak = min(lag_peak, wlag_peak[w]);
    }
    if (lag == TG_NONE) lag = lag_peak;
    if (peak == 0) lag = lag_peak = 0;
    rec->r0 = row[0];
    rec->r_prev = lag ? row[lag - 1] : 0;
    rec->r_lag = lag ? row[lag] : 0;
    rec->r_next = lag ? row[lag + 1] : 0;
    rec->lag = lag;
    rec->lag_peak = lag_peak;
  }
}

/* Run blockIdx.x of song blockIdx.y: the frames [f0, f1) with f0 = blockIdx.x run_frames, which need the blocks
 * [f0, f1 - 1 + m).  Block b goes to slot b mod m of the ring, where block b - m, which leaves the frame with it,
 * stood.  The first frame is complete with block f0 + m - 1. */
__global__ __launch_bounds__(256) void k_tgram_blocks(const unsigned *__restrict__ onsets,
                                                      const bl_tgram_song *__restrict__ songs,
                                                      const bl_amd_tgram_params *__restrict__ params, int run_frames,
                                                      bl_amd_tgram_frame *frames_out, bl_u64 *gram_out) {
  extern __shared__ __attribute__((aligned(16))) bl_u64 ring[]; /* m rows of 512 */
  __shared__ __attribute__((aligned(16))) unsigned so[TG_STAGE];
  __shared__ __attribute__((aligned(16))) bl_u64 part[TG_LAGS];
  __shared__ __attribute__((aligned(16))) bl_u64 row[TG_LAGS];
  __shared__ bl_u64 wpeak[4];
  __shared__ int wlag[4], wlag_peak[4];
  const bl_tgram_song sg = songs[blockIdx.y];
  const int S = params->stride, m = params->blocks, lag_min = params->lag_min, lag_max = params->lag_max;
  const int f0 = (int)blockIdx.x * run_frames;
  if (f0 >= sg.frames) return;
  const int f1 = min(f0 + run_frames, sg.frames), b1 = f1 - 1 + m;
  const int per_tile = max(1, BL_TGRAM_TILE / S), S16 = S >> 4;
  const int tid = threadIdx.x, g4 = 4 * (tid & 127), half = tid >> 7, H = sg.hops;
  const unsigned *in = onsets + sg.onset_off;
  bl_u64 acc[4] = {0, 0, 0, 0};
  for (int t0 = f0; t0 < b1; t0 += per_tile) {
    const int nb = min(per_tile, b1 - t0), h0 = t0 * S, span = nb * S + TG_LAGS; /* span <= TG_STAGE */
    __syncthreads(); /* the products of the tile before are over */
    for (int i = tid; i < span; i += 256) {
      const int g = h0 + i;
      so[i] = g < H ? in[g] : 0u;
    }
    __syncthreads();
    for (int k = 0; k < nb; ++k) {
      const int b = t0 + k;
      bl_u64 r[4] = {0, 0, 0, 0};
      for (int q = k * S16; q < (k + 1) * S16; ++q) { /* groups of 16 terms: hb is a multiple of 8, the reads are b128 */
        const int hb = 16 * q + 8 * half;
        const uint4 l0 = *reinterpret_cast<const uint4 *>(so + hb), l1 = *reinterpret_cast<const uint4 *>(so + hb + 4);
        const uint4 r0 = *reinterpret_cast<const uint4 *>(so + hb + g4);
        const uint4 r1 = *reinterpret_cast<const uint4 *>(so + hb + g4 + 4);
        const uint4 r2 = *reinterpret_cast<const uint4 *>(so + hb + g4 + 8);
        const unsigned L[8] = {l0.x, l0.y, l0.z, l0.w, l1.x, l1.y, l1.z, l1.w};
        const unsigned R[12] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w};
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
          for (int j = 0; j < 4; ++j) r[j] += (bl_u64)L[a] * R[a + j];
      }
      if (half) {
#pragma unroll
        for (int j = 0; j < 4; ++j) part[g4 + j] = r[j];
      }
      __syncthreads();
      const bool emit = b - f0 >= m - 1; /* the same for the whole workgroup */
      if (!half) {
        bl_u64 *slot = ring + (size_t)(b % m) * TG_LAGS + g4;
        const bool retire = b - f0 >= m;
        bl_u64 *gram = gram_out && emit ? gram_out + (size_t)(sg.frame_off + (b - (m - 1))) * TG_LAGS + g4 : nullptr;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bl_u64 pb = r[j] + part[g4 + j];
          if (retire) acc[j] -= slot[j];
          acc[j] += pb;
          slot[j] = pb;
          if (emit) row[g4 + j] = acc[j];
          if (gram) gram[j] = acc[j];
        }
      }
      __syncthreads(); /* `part` has been read: the other half may write the next block's; the row is complete */
      if (emit) {
        tg_pick(row, lag_min, lag_max, wpeak, wlag, wlag_peak, frames_out + sg.frame_off + (b - (m - 1)));
      }
    }
  }
}

/* near(L, M) of the header; the operands are below 2^11 and tol at most 1000 */
__device__ __forceinline__ bool tg_near(int L, int M, int tol, int octaves) {
  if (1000 * abs(L - M) <= tol * M) return true;
  if (!octaves) return false;
  return 1000 * abs(2 * L - M) <= tol * M || 1000 * abs(L - 2 * M) <= tol * 2 * M;
}

__device__ __forceinline__ int tg_wave_sum(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
__device__ __forceinline__ int tg_wave_min(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off));
  return v;
}
__device__ __forceinline__ int tg_wave_max(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off));
  return v;
}

/* One wavefront per song, 64 frames at a time in frame order.  The frame in front of a frame that has a tempo is the
 * nearest lower lane that has one, or what the 64 frames before left (`carry`, 0: none yet).  The record is 14 int32
 * words, all written. */
__global__ __launch_bounds__(64) void k_tgram_songs(const bl_tgram_song *__restrict__ songs,
                                                    const bl_amd_tgram_params *__restrict__ params,
                                                    const bl_amd_tgram_frame *frames, bl_amd_song_tgram *out) {
  __shared__ unsigned hist[TG_LAGS];
  __shared__ int smed;
  const bl_tgram_song sg = songs[blockIdx.x];
  const int lane = threadIdx.x, F = sg.frames, tol = params->tol, octaves = params->octaves;
  int *po = reinterpret_cast<int *>(out + blockIdx.x);
  if (F == 0) { /* the whole wavefront leaves together */
    if (lane < 14) po[lane] = lane == 0 ? sg.hops : lane == 3 ? BL_UNEXPECTED : 0;
    return;
  }
  for (int i = lane; i < TG_LAGS; i += 64) hist[i] = 0u;
  __syncthreads();
  const bl_amd_tgram_frame *fr = frames + sg.frame_off;
  int carry = 0, n_tempo = 0, jumps = 0, first = TG_NONE, last = -1, lo = TG_NONE, hi = 0;
  for (int base = 0; base < F; base += 64) {
    const int f = base + lane;
    const int lag = f < F ? fr[f].lag : 0;
    const bool has = lag != 0;
    const bl_u64 mask = __ballot(has);
    const bl_u64 below = mask & ((1ull << lane) - 1ull);
    const int before = __shfl(lag, below ? 63 - __clzll((long long)below) : lane);
    const int prev = below ? before : carry;
    if (has) {
      atomicAdd(&hist[lag & (TG_LAGS - 1)], 1u); /* 1 .. 510 by construction */
      n_tempo += 1;
      first = min(first, f);
      last = max(last, f);
      lo = min(lo, lag);
      hi = max(hi, lag);
      if (prev && !tg_near(lag, prev, tol, octaves)) jumps += 1;
    }
    const int top = __shfl(lag, mask ? 63 - __clzll((long long)mask) : 0);
    if (mask) carry = top;
  }
  n_tempo = tg_wave_sum(n_tempo);
  jumps = tg_wave_sum(jumps);
  first = tg_wave_min(first);
  last = tg_wave_max(last);
  lo = tg_wave_min(lo);
  hi = tg_wave_max(hi);
  __syncthreads();
  /* the lower median: the smallest lag whose count of frames at or below it passes index (n_tempo - 1) >> 1 */
  unsigned cnt[8], mine = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    cnt[j] = hist[8 * lane + j];
    mine += cnt[j];
  }
  unsigned incl = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned o = __shfl_up(incl, off);
    if (lane >= off) incl += o;
  }
  if (lane == 0) smed = 0;
  __syncthreads();
  const unsigned want = n_tempo > 0 ? (unsigned)(n_tempo - 1) >> 1 : 0u;
  unsigned seen = incl - mine;
  if (n_tempo > 0 && seen <= want && want < incl) { /* one lane */
    int med = 8 * lane;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (seen <= want && want < seen + cnt[j]) med = 8 * lane + j;
      seen += cnt[j];
    }
    smed = med;
  }
  __syncthreads();
  const int med = smed;
  int n_near = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (cnt[j] && tg_near(8 * lane + j, med, tol, octaves)) n_near += (int)cnt[j];
  n_near = tg_wave_sum(n_near);
  if (lane == 0) {
    const bool any = n_tempo > 0;
    po[0] = sg.hops;
    po[1] = F;
    po[2] = n_tempo;
    po[3] = BL_OK;
    po[4] = any ? first : -1;
    po[5] = any ? last : -1;
    po[6] = any ? fr[first].lag : 0;
    po[7] = any ? fr[last].lag : 0;
    po[8] = any ? lo : 0;
    po[9] = any ? hi : 0;
    po[10] = any ? med : 0;
    po[11] = any ? n_near : 0;
    po[12] = jumps;
    po[13] = 0;
  }
}

/* ========================================================================= */
/* launchers (declared in bl_tgram.h)                                         */

int blk_tgram_blocks(hipStream_t s, const uint32_t *d_onsets, const bl_tgram_song *d_songs, int n_songs, int max_frames,
                     const bl_amd_tgram_params &h_params, const bl_amd_tgram_params *d_params, int n_cu,
                     bl_amd_tgram_frame *d_frames_out, uint64_t *d_gram_out, blk_mark_fn mark, void *mark_user) {
  if (max_frames < 1) return BL_OK;
  const size_t lds = sizeof(bl_u64) * TG_LAGS * (size_t)h_params.blocks;
  /* a host-side setting of the function on the current device, no device work; a failure shows as the launch's error */
  if (lds + TG_STATIC_LDS > 65536)
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_tgram_blocks), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(sizeof(bl_u64) * TG_LAGS * 16));
  /* runs of at least BL_TGRAM_RUN_FRAMES frames, and no more of them than fill the chip a few times over */
  const long long want = ((long long)n_cu * 8 + n_songs - 1) / n_songs;
  const int run_frames = (int)std::max<long long>(BL_TGRAM_RUN_FRAMES, (max_frames + want - 1) / want);
  const int gx = (max_frames + run_frames - 1) / run_frames;
  Mark m(mark, mark_user, TGK_BLOCKS, s);
  for (int b = 0; b < n_songs; b += BL_TGRAM_GRID_SONGS) {
    const int n = std::min(BL_TGRAM_GRID_SONGS, n_songs - b);
    hipLaunchKernelGGL(k_tgram_blocks, dim3((unsigned)gx, (unsigned)n), dim3(256), lds, s, d_onsets, d_songs + b, d_params,
                       run_frames, d_frames_out, reinterpret_cast<bl_u64 *>(d_gram_out));
  }
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}

int blk_tgram_songs(hipStream_t s, const bl_tgram_song *d_songs, int n_songs, const bl_amd_tgram_params *d_params,
                    const bl_amd_tgram_frame *d_frames, bl_amd_song_tgram *d_out, blk_mark_fn mark, void *mark_user) {
  Mark m(mark, mark_user, TGK_SONGS, s);
  hipLaunchKernelGGL(k_tgram_songs, dim3((unsigned)n_songs), dim3(64), 0, s, d_songs, d_params, d_frames, d_out);
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}
