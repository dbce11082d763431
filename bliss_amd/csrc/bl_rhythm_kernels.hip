/*
 * bl_rhythm_kernels.hip — gfx950 kernels and launch layer of the per-song tempo (bl_amd_rhythm_batch_device,
 * bl_amd_rhythm_from_onsets, include/bliss_amd.h: bl_amd_song_rhythm).  Nothing of the reference's analysis is restated
 * here: its `tempo` is a rating that cannot be turned into beats per minute, and "BPM" / "Beat loudness" are rows of
 * its author's ROADMAP.md.  Every quantity is an exact integer (the definitions are in the header), so neither the
 * split of a song over workgroups nor the order of the atomics that join them shows in a result.
 *
 * Kernels:
 *   k_rhythm_hops   streaming pass over the PCM: the hop energies A_h, B_h, the windowed amplitudes and the novelty
 *                   n_h, 4 bytes per hop of 128 frames to scratch
 *   k_rhythm_acf    local-mean removal and smoothing on the way into LDS (the onset curve o_h), then the 512 lag
 *                   products R[tau] of one chunk of terms, joined by 64-bit integer atomics
 *   k_rhythm_pick   one wave per song: the pick over [lag_min, lag_max] and the record
 *   k_isqrt_sweep   bl_amd_selftest_isqrt
 *
 * Bounds.  m = l + r (stereo) or 2 s (mono): |m| <= 2^16, so m^2 <= 2^32 does NOT fit 32 bits (the all -32768 stereo
 * song reaches it); d = m[i] - m[i-1]: |d| <= 2^17 - 2, d^2 < 2^34.  Both squares are 32 x 32 -> 64-bit
 * multiply-adds into 64-bit sums (v_mad_i64_i32).  A hop has 128 frames: A_h <= 2^39, B_h < 2^41; a window of four:
 * < 2^41, < 2^43; >> 9: <= 2^32, < 2^34, whose roots are a_h <= 2^16, b_h < 2^17.  n_h <= a_h + b_h < 2^18;
 * 16 n_h and the 16-term sum are < 2^22; q_h <= n_h, o_h <= max q < 2^18.  A product o o' < 2^36, H < 2^24 terms:
 * R < 2^60 and 16 R < 2^64.
 *
 * Lane mapping of k_rhythm_hops.  pcm_offset is a multiple of 8 samples, so a 16-byte vector never straddles a hop: a
 * stereo hop is 512 bytes = 32 consecutive lanes, a mono hop 256 bytes = 16.  A lane squares the 4 (stereo) or 8
 * (mono) frames of its vector; the predecessor frame of the vector's first frame is the word in front of it in memory,
 * which the lane loads itself (the "seams" of bl_level_kernels.hip); vector 0 of the song has none and takes its own
 * first frame, which makes d[0] = 0.  Eight lanes share a hop, each with every eighth vector of it, and join their
 * sums in three DPP steps: no atomics, and LDS only behind the hop.
 *
 * Run split.  A workgroup owns a contiguous run of tiles of RH_TILE hops.  n_h needs a_h and a_{h-1}, that is
 * A_{h-4} .. A_h: the workgroup computes the energies of the four hops in front of its run itself (for a run that
 * starts at hop 0 they are 0 by definition) and carries the last four of a tile into the next.  So n_h is the same
 * bits whatever the split.
 */
#include <hip/hip_runtime.h>

#include "bl_isqrt.h"
#include "bl_launch.h"

typedef unsigned long long bl_u64;
typedef short bl_s2 __attribute__((ext_vector_type(2)));

#define RH_TILE 64                 /* hops per tile of k_rhythm_hops */
#define RA_CH 1024                 /* terms h per chunk of k_rhythm_acf */
#define RA_W (RA_CH + BL_AMD_RHYTHM_LAGS) /* hops of o a chunk stages: its terms and 511 of look-ahead, rounded up */

__device__ __forceinline__ bl_s2 rh_s2(unsigned w) { bl_s2 v; __builtin_memcpy(&v, &w, 4); return v; }

/* cross-lane move inside every group of eight lanes: 0xB1 = quad_perm [1,0,3,2] (lane ^ 1), 0x4E = quad_perm [2,3,0,1]
 * (lane ^ 2), 0x141 = row_half_mirror (lane 7 - i: the other quad, which is all a step needs once the quads are
 * uniform).  Taken in this order every lane of the eight ends with their sum. */
template <int CTRL> __device__ __forceinline__ bl_u64 rh_dpp(bl_u64 v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)v, CTRL, 0xF, 0xF, true);
  const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(v >> 32), CTRL, 0xF, 0xF, true);
  return ((bl_u64)hi << 32) | lo;
}
__device__ __forceinline__ bl_u64 rh_sum8(bl_u64 v) {
  v += rh_dpp<0xB1>(v);
  v += rh_dpp<0x4E>(v);
  v += rh_dpp<0x141>(v);
  return v;
}

/* One 16-byte vector; before: the word in front of q.x in memory, or what stands in for it in vector 0.  The squares
 * are signed 32 x 32 -> 64-bit multiply-adds (v_mad_i64_i32): no magnitudes to take. */
template <bool MONO> __device__ __forceinline__ void rh_eat(const uint4 q, unsigned before, long long &A, long long &B) {
  const unsigned w[4] = {q.x, q.y, q.z, q.w};
  const bl_s2 one = {1, 1};
  int mp = MONO ? 2 * ((int)before >> 16) : __builtin_amdgcn_sdot2(rh_s2(before), one, 0, false);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int m[2];
    if (MONO) {
      m[0] = 2 * (int)(short)(w[k] & 0xFFFFu);
      m[1] = 2 * ((int)w[k] >> 16);
    } else {
      m[0] = __builtin_amdgcn_sdot2(rh_s2(w[k]), one, 0, false);
    }
#pragma unroll
    for (int j = 0; j < (MONO ? 2 : 1); ++j) {
      const int d = m[j] - mp;
      mp = m[j];
      A += (long long)m[j] * m[j];
      B += (long long)d * d;
    }
  }
}

/* The energies of hops [first, first + cnt), cnt <= RH_TILE, into sA / sB[slot0 ..].  Eight lanes per hop, 32 hops per
 * turn of the workgroup; lane `sub` of the eight takes the hop's vectors sub, sub + 8, ... (four of a stereo hop, two of
 * a mono one, all loaded before the first is used), so a wave's load instruction reads whole 128-byte lines, and the
 * cross-lane sum comes once per hop and lane, not once per vector.  Every lane of the workgroup takes the same number
 * of turns and a lane without a hop eats zeros, so the cross-lane steps see whole groups. */
template <bool MONO>
__device__ __forceinline__ void rh_hops(const int16_t *p, int first, int cnt, bl_u64 *sA, bl_u64 *sB, int slot0) {
  constexpr int VPH = MONO ? 16 : 32, NV = VPH / 8; /* vectors per hop, per lane */
  const uint4 *pv = reinterpret_cast<const uint4 *>(p);
  const unsigned *pw = reinterpret_cast<const unsigned *>(p);
  const int sub = threadIdx.x & 7;
  for (int base = 0; base < cnt; base += 32) {
    const int hl = base + (int)(threadIdx.x >> 3);
    const bool live = hl < cnt;
    uint4 q[NV];
    unsigned b[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      q[j] = make_uint4(0, 0, 0, 0);
      b[j] = 0;
      if (live) {
        const unsigned v = (unsigned)(first + hl) * VPH + 8u * j + sub;
        q[j] = pv[v];
        b[j] = pw[v ? 4u * v - 1u : 0u];
        if (!v) b[j] = MONO ? q[j].x << 16 : q[j].x; /* the song's first frame has no predecessor: d[0] = 0 */
      }
    }
    long long A = 0, B = 0;
#pragma unroll
    for (int j = 0; j < NV; ++j) rh_eat<MONO>(q[j], b[j], A, B);
    const bl_u64 hA = rh_sum8((bl_u64)A), hB = rh_sum8((bl_u64)B);
    if (live && sub == 0) {
      sA[slot0 + hl] = hA;
      sB[slot0 + hl] = hB;
    }
  }
}

template <bool MONO>
__device__ __forceinline__ void rh_song(const int16_t *p, int H, unsigned *n_out, bl_u64 *sA, bl_u64 *sB, unsigned *sa,
                                        unsigned *sb) {
  const int tid = threadIdx.x;
  const int ntile = (H + RH_TILE - 1) / RH_TILE;
  const int per = (ntile + (int)gridDim.x - 1) / (int)gridDim.x;
  const int t_begin = (int)blockIdx.x * per, t_end = min(t_begin + per, ntile);
  if (t_begin >= t_end) return;
  /* slots 0..3: the four hops in front of the run */
  if (t_begin == 0) {
    if (tid < 4) sA[tid] = sB[tid] = 0;
  } else {
    rh_hops<MONO>(p, t_begin * RH_TILE - 4, 4, sA, sB, 0);
  }
  for (int t = t_begin; t < t_end; ++t) {
    const int h0 = t * RH_TILE, cnt = min(RH_TILE, H - h0);
    rh_hops<MONO>(p, h0, cnt, sA, sB, 4);
    __syncthreads();
    /* amplitudes of hops h0 - 1 .. h0 + cnt - 1: thread j has hop h0 - 1 + j, its window is slots j .. j + 3 */
    if (tid <= cnt) sa[tid] = bl_isqrt64((sA[tid] + sA[tid + 1] + sA[tid + 2] + sA[tid + 3]) >> 9);
    if (tid >= 128 && tid - 128 <= cnt) { /* b on the workgroup's other half: the two roots run side by side */
      const int j = tid - 128;
      sb[j] = bl_isqrt64((sB[j] + sB[j + 1] + sB[j + 2] + sB[j + 3]) >> 9);
    }
    bl_u64 cA = 0, cB = 0;
    if (tid < 4) { cA = sA[RH_TILE + tid]; cB = sB[RH_TILE + tid]; } /* the next tile's slots 0..3 (cnt == RH_TILE then) */
    __syncthreads();
    if (tid < cnt) {
      const unsigned a1 = sa[tid + 1], a0 = sa[tid], b1 = sb[tid + 1], b0 = sb[tid];
      const unsigned nh = (a1 > a0 ? a1 - a0 : 0u) + (b1 > b0 ? b1 - b0 : 0u);
      n_out[h0 + tid] = (h0 + tid) ? nh : 0u; /* n_0 = 0 */
    }
    if (tid < 4) { sA[tid] = cA; sB[tid] = cB; }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_rhythm_hops(const int16_t *__restrict__ pcm,
                                                     const bl_rhythm_song *__restrict__ songs,
                                                     unsigned *__restrict__ n_out) {
  __shared__ bl_u64 sA[RH_TILE + 4], sB[RH_TILE + 4];
  __shared__ unsigned sa[RH_TILE + 1], sb[RH_TILE + 1];
  const bl_rhythm_song sg = songs[blockIdx.y];
  const int16_t *p = pcm + sg.pcm_off;
  unsigned *out = n_out + sg.hop_off;
  if (sg.channels == 1) rh_song<true>(p, sg.hops, out, sA, sB, sa, sb);
  else rh_song<false>(p, sg.hops, out, sA, sB, sa, sb);
}

/* k_rhythm_acf.  Chunk c of a song holds the terms h in [c RA_CH, min((c + 1) RA_CH, T)); index i of its LDS arrays
 * is hop h0 + i, h0 = c RA_CH.  Staging: n over [h0 - 9, h0 + RA_W + 8) (q_g needs n_{g-8} .. n_{g+7}, o_h needs
 * q_{h-1} .. q_{h+1}: 9 hops before, 8 after), q over [h0 - 1, h0 + RA_W + 1), o over [h0, h0 + RA_W); everything
 * outside [0, H) is 0.  CURVE: `src` is the caller's onset curve (bl_amd_rhythm_from_onsets) and goes to `so` as it is.
 * A hop is owned by the chunk whose terms contain it, the hops from T on by the last chunk: the owner writes it to
 * onsets_out and counts it in onset_sum / onset_max.
 *
 * Products.  Thread t of 256: lags 4 g .. 4 g + 3 with g = t mod 128, and every second block of eight terms (t / 128).
 * Per block: the eight left factors (two broadcast b128 reads of `sl`, which is o with the terms from T on zeroed) and
 * the twelve right factors o[hb + 4 g .. + 11] (three b128 reads, 16-byte aligned since hb and 4 g are multiples of 4;
 * consecutive lanes read consecutive 16 bytes) feed 32 products into four 64-bit sums.  The highest index read is
 * RA_CH - 8 + 508 + 11 = RA_W - 1.  The two halves meet in LDS and 512 atomics per chunk go to the song's row. */
struct bl_rhythm_acc { /* per song of a launch group, zeroed by the launcher */
  bl_u64 onset_sum;
  unsigned onset_max, pad;
};

template <bool CURVE>
__global__ __launch_bounds__(256) void k_rhythm_acf(const unsigned *__restrict__ src,
                                                    const bl_rhythm_song *__restrict__ songs, bl_u64 *rows,
                                                    int rows_by_out_idx, bl_rhythm_acc *acc, unsigned *onsets_out) {
  __shared__ __attribute__((aligned(16))) unsigned so[RA_W];
  __shared__ __attribute__((aligned(16))) unsigned sl[RA_CH];
  __shared__ unsigned sn[CURVE ? 1 : RA_W + 17], sq[CURVE ? 1 : RA_W + 2];
  __shared__ bl_u64 part[BL_AMD_RHYTHM_LAGS];
  const bl_rhythm_song sg = songs[blockIdx.y];
  const int H = sg.hops, T = H >= BL_AMD_RHYTHM_LAGS ? H - (BL_AMD_RHYTHM_LAGS - 1) : 0;
  const int nchunk = T > 0 ? (T + RA_CH - 1) / RA_CH : 1;
  if ((int)blockIdx.x >= nchunk) return;
  const bool last = (int)blockIdx.x == nchunk - 1;
  const int h0 = (int)blockIdx.x * RA_CH, tid = threadIdx.x;
  const unsigned *in = src + (CURVE ? sg.onset_off : sg.hop_off);
  if (!CURVE) {
    for (int i = tid; i < RA_W + 17; i += 256) {
      const int g = h0 - 9 + i;
      sn[i] = g >= 0 && g < H ? in[g] : 0u;
    }
    __syncthreads();
    for (int i = tid; i < RA_W + 2; i += 256) { /* hop g = h0 - 1 + i is sn[i + 8] */
      const int g = h0 - 1 + i;
      unsigned sum = 0;
#pragma unroll
      for (int k = 0; k < 16; ++k) sum += sn[i + k];
      const unsigned c = 16u * sn[i + 8];
      sq[i] = g >= 0 && g < H && c > sum ? (c - sum) >> 4 : 0u;
    }
    __syncthreads();
  }
  bl_u64 osum = 0;
  unsigned omax = 0;
  for (int i = tid; i < RA_W; i += 256) {
    const int g = h0 + i;
    unsigned o = 0;
    if (g < H) o = CURVE ? in[g] : (sq[i] + 2u * sq[i + 1] + sq[i + 2]) >> 2;
    so[i] = o;
    if (i < RA_CH) sl[i] = g < T ? o : 0u;
    if (g < H && (i < RA_CH || last)) {
      if (onsets_out) onsets_out[sg.onset_off + g] = o;
      osum += o;
      omax = max(omax, o);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    osum += __shfl_down(osum, off);
    omax = max(omax, __shfl_down(omax, off));
  }
  if ((tid & 63) == 0) {
    atomicAdd(&acc[blockIdx.y].onset_sum, osum);
    atomicMax(&acc[blockIdx.y].onset_max, omax);
  }
  if (T <= 0) return; /* a short song: no terms */
  __syncthreads();
  const int cnt = min(RA_CH, T - h0), g4 = 4 * (tid & 127), half = tid >> 7;
  bl_u64 r[4] = {0, 0, 0, 0};
  for (int hb = 8 * half; hb < cnt; hb += 16) {
    const uint4 l0 = *reinterpret_cast<const uint4 *>(sl + hb), l1 = *reinterpret_cast<const uint4 *>(sl + hb + 4);
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
  if (!half) {
    bl_u64 *row = rows + (size_t)BL_AMD_RHYTHM_LAGS * (rows_by_out_idx ? (unsigned)sg.out_idx : blockIdx.y);
#pragma unroll
    for (int j = 0; j < 4; ++j) atomicAdd(row + g4 + j, r[j] + part[g4 + j]);
  }
}

/* k_rhythm_pick: one wave per song; lane l holds R[l + 64 j], j = 0..7.  The record's every byte is written. */
__global__ __launch_bounds__(64) void k_rhythm_pick(const bl_rhythm_song *__restrict__ songs, const bl_u64 *rows,
                                                    int rows_by_out_idx, const bl_rhythm_acc *acc, int lag_min,
                                                    int lag_max, bl_amd_song_rhythm *out) {
  const bl_rhythm_song sg = songs[blockIdx.x];
  const int lane = threadIdx.x, H = sg.hops;
  bl_amd_song_rhythm *rec = out + sg.out_idx;
  if (H < BL_AMD_RHYTHM_LAGS) { /* a short song: its row stays 0 */
    if (lane == 0) {
      rec->r0 = rec->r_prev = rec->r_lag = rec->r_next = rec->r_peak = rec->onset_sum = 0;
      rec->onset_max = 0;
      rec->hops = H;
      rec->terms = rec->lag = rec->lag_peak = 0;
      rec->status = BL_UNEXPECTED;
    }
    return;
  }
  const bl_u64 *row = rows + (size_t)BL_AMD_RHYTHM_LAGS * (rows_by_out_idx ? (unsigned)sg.out_idx : blockIdx.x);
  bl_u64 R[8], peak = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int tau = lane + 64 * j;
    R[j] = row[tau];
    if (tau >= lag_min && tau <= lag_max && R[j] > peak) peak = R[j];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const bl_u64 o = __shfl_xor(peak, off);
    peak = o > peak ? o : peak;
  }
  const int none = 1 << 30;
  int lag_peak = none, lag = none;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int tau = lane + 64 * j;
    if (tau < lag_min || tau > lag_max) continue; /* 1 <= tau <= 510: both neighbours are in the row */
    if (R[j] == peak) lag_peak = min(lag_peak, tau);
    if (R[j] >= row[tau - 1] && R[j] >= row[tau + 1] && 16 * R[j] >= 15 * peak) lag = min(lag, tau);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lag_peak = min(lag_peak, __shfl_xor(lag_peak, off));
    lag = min(lag, __shfl_xor(lag, off));
  }
  if (lag == none) lag = lag_peak;
  if (peak == 0) lag = lag_peak = 0;
  if (lane == 0) {
    rec->r0 = row[0];
    rec->r_prev = lag ? row[lag - 1] : 0;
    rec->r_lag = lag ? row[lag] : 0;
    rec->r_next = lag ? row[lag + 1] : 0;
    rec->r_peak = peak;
    rec->onset_sum = acc[blockIdx.x].onset_sum;
    rec->onset_max = acc[blockIdx.x].onset_max;
    rec->hops = H;
    rec->terms = H - (BL_AMD_RHYTHM_LAGS - 1);
    rec->lag = lag;
    rec->lag_peak = lag_peak;
    rec->status = BL_OK;
  }
}

/* bl_amd_selftest_isqrt: x = 0, and k^2 - 1, k^2, k^2 + 1 for k in [1, 2^17]; counts[0] += checked, [1] += wrong */
__global__ __launch_bounds__(256) void k_isqrt_sweep(bl_u64 *counts) {
  const unsigned n = 3u * (1u << 17) + 1u;
  unsigned checked = 0, wrong = 0;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
    bl_u64 x = 0;
    if (i) {
      const bl_u64 k = (i - 1u) / 3u + 1u;
      x = k * k - 1u + (i - 1u) % 3u;
    }
    checked += 1;
    wrong += !bl_isqrt_is_floor(x, bl_isqrt64(x));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    checked += __shfl_down(checked, off);
    wrong += __shfl_down(wrong, off);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&counts[0], (bl_u64)checked);
    atomicAdd(&counts[1], (bl_u64)wrong);
  }
}

/* ========================================================================= */
/* launchers (declared in bl_launch.h)                                        */

size_t blk_rhythm_rows_bytes(int n_songs, bool own_rows) {
  return ((size_t)n_songs * sizeof(bl_rhythm_acc) + 255) / 256 * 256 +
         (own_rows ? (size_t)n_songs * BL_AMD_RHYTHM_LAGS * sizeof(bl_u64) : 0);
}

int blk_rhythm_group(hipStream_t s, const int16_t *d_pcm, const uint32_t *d_curve, const bl_rhythm_song *d_songs,
                     int n_songs, int max_hops, int lag_min, int lag_max, int n_cu, uint32_t *d_n, void *d_rows,
                     bl_amd_song_rhythm *d_songs_out, uint32_t *d_onsets_out, uint64_t *d_acf_out, blk_mark_fn mark,
                     void *mark_user) {
  bl_rhythm_acc *acc = static_cast<bl_rhythm_acc *>(d_rows);
  const size_t acc_bytes = blk_rhythm_rows_bytes(n_songs, false);
  bl_u64 *rows = d_acf_out ? reinterpret_cast<bl_u64 *>(d_acf_out)
                           : reinterpret_cast<bl_u64 *>(static_cast<char *>(d_rows) + acc_bytes);
  /* the sums start from zero; the caller's rows were zeroed once for the whole call */
  BL_HIP_CHECK(hipMemsetAsync(d_rows, 0, blk_rhythm_rows_bytes(n_songs, !d_acf_out), s));
  if (!d_curve) {
    Mark m(mark, mark_user, PK_RHYTHM_HOPS, s);
    const int gx = grid_x_for((max_hops + RH_TILE - 1) / RH_TILE, n_songs, 8, n_cu);
    hipLaunchKernelGGL(k_rhythm_hops, dim3(gx, n_songs), dim3(256), 0, s, d_pcm, d_songs, d_n);
  }
  const int T = max_hops - (BL_AMD_RHYTHM_LAGS - 1), gx = T > 0 ? (T + RA_CH - 1) / RA_CH : 1;
  {
    Mark m(mark, mark_user, PK_RHYTHM_ACF, s);
    if (d_curve)
      hipLaunchKernelGGL(k_rhythm_acf<true>, dim3(gx, n_songs), dim3(256), 0, s, d_curve, d_songs, rows,
                         d_acf_out ? 1 : 0, acc, d_onsets_out);
    else
      hipLaunchKernelGGL(k_rhythm_acf<false>, dim3(gx, n_songs), dim3(256), 0, s, d_n, d_songs, rows,
                         d_acf_out ? 1 : 0, acc, d_onsets_out);
  }
  {
    Mark m(mark, mark_user, PK_RHYTHM_PICK, s);
    hipLaunchKernelGGL(k_rhythm_pick, dim3(n_songs), dim3(64), 0, s, d_songs, rows, d_acf_out ? 1 : 0, acc, lag_min,
                       lag_max, d_songs_out);
  }
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}

int blk_isqrt_sweep(hipStream_t s, unsigned long long *d_counts, int n_cu) {
  hipLaunchKernelGGL(k_isqrt_sweep, dim3(n_cu), dim3(256), 0, s, d_counts);
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}
