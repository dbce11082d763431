/*
 * bl_tbeats_kernels.hip — gfx950 kernels and launch layer of the beat grid that follows the tempo over time
 * (bl_amd_tbeats_device, bl_amd_tbeats_host, include/bliss_amd.h: bl_amd_song_tbeats): the dynamic programme of
 * bl_amd_beats_* (bl_beat_kernels.hip) with the period a function of the hop, taken from per-frame lags such as the
 * tempogram's.  Exact integers throughout (the definition is in the header), so that neither the split of the hops
 * over lanes, the cut into runs and blocks nor the order of a reduction shows in a result.
 *
 * Kernels:
 *   k_tbeats_track   stages 1 to 3, one workgroup of 256 per song: which frames are valid, the nearest valid frame of
 *                    every other one, the fold, the counts
 *   k_tbeats         stages 4 to 8, one workgroup of 256 per song: the scale, then run by run the penalty table and the
 *                    scores C and links P block by block, the end, the back-trace and the record
 *
 * k_tbeats_track.  A tile is 256 frames, one per lane.  The forward pass leaves, per frame, the index of the last
 * valid frame at or before it: inside a wave from the ballot of the valid lanes, across the waves of a tile from four
 * words in LDS, across tiles from a carry every lane holds.  It parks that index in the track (each lane reads back
 * only what it wrote itself).  The backward pass finds the first valid frame at or behind every frame the same way,
 * tiles taken from the last to the first, chooses between the two by distance with ties to the earlier, fetches that
 * frame's lag, folds and writes q.  Every index is one of a valid frame of the song, so every fetch stays inside its
 * F lags.
 *
 * k_tbeats.  A run is a maximal stretch of hops with one period L.  Its end is found from the track: every wave looks
 * at the next 64 frames at a time for the first whose q differs (all four waves read the same words and reach the same
 * answer, so no LDS and no barrier is needed for it), and never looks past the frame of hop H - 1.  At a run's start
 * the workgroup rebuilds the penalty table for L: at most 766 entries, three per lane; the barrier behind the previous
 * run's last block has already parted its readers from the writers.  Inside a run the blocks are those of k_beats:
 * lo = (L + 1) >> 1 hops whose sources t - d, d >= lo, lie below the block's start, G = 256 / (lo rounded up to a power
 * of two) lanes per hop, one barrier per block.  A block ends at the run's end at the latest, so lo, hi, G and the
 * table are those of every hop in it.  The ring of 2048 scores (1024 C[t] at t mod 2048) carries over between runs
 * unchanged: whatever L, a block reads at most 2 * 510 = 1020 hops back and writes at most 255, a span of 1275 < 2048.
 *
 * Bounds: those of k_beats.  pen < 2^26, C < 2^42, the key 1024 v + (1023 - d) fits 53 bits.  A source has
 * 0 <= t - d (the window is clipped at d <= t) and d - lo <= 765; a frame index is clamped to [0, F - 1] and F >= 1
 * wherever the track is read; a link P[t] = d <= t, so the back-trace never leaves [0, H).
 *
 * The cross-lane maximum is k_beats's (bl_beat_lanes.h).
 */
#include <hip/hip_runtime.h>

#include "bl_beat_lanes.h"
#include "bl_ilog2.h"
#include "bl_tbeats.h"

#define TB_RING BL_TBEATS_RING
#define TB_TILE BL_TBEATS_TRACK_TILE
#define TB_PEN 768
#define TB_NONE (-0x7FFFFFFFFFFFFFFFll - 1) /* the least key: a lane or a hop without a candidate */

__device__ __forceinline__ int tb_wave_sum(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
__device__ __forceinline__ bool tb_lag_ok(int L) { return L >= 2 && L <= BL_AMD_BEATS_PERIOD_MAX; }

/* ========================================================================= */
/* stages 1 to 3: the period of every frame                                   */

__global__ __launch_bounds__(256) void k_tbeats_track(const bl_tbeats_song *__restrict__ songs, const char *lag,
                                                      int lag_stride, const char *anchor, int anchor_stride,
                                                      const bl_amd_tbeats_params *__restrict__ params, int32_t *track,
                                                      bl_amd_song_tbeats *out) {
  __shared__ int wv[4];
  __shared__ int red[2][4];
  const bl_tbeats_song sg = songs[blockIdx.x];
  const int F = sg.frames, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const char *lg = lag + (size_t)sg.frame_off * (size_t)lag_stride;
  int32_t *tr = track + sg.frame_off;
  bl_amd_song_tbeats *rec = out + sg.out_idx;
  auto lag_of = [&](int f) { return *reinterpret_cast<const int *>(lg + (size_t)f * (size_t)lag_stride); };
  /* forward: the last valid frame at or before f, -1 where there is none; carry: that of the tiles so far */
  int carry = -1;
  for (int base = 0; base < F; base += TB_TILE) {
    const int f = base + tid;
    const bool valid = f < F && tb_lag_ok(lag_of(f));
    const bl_u64 mask = __ballot(valid);
    const bl_u64 below = mask & ((2ull << lane) - 1ull); /* lanes 0 .. lane; lane 63: every lane */
    if (lane == 0) wv[wave] = mask ? base + 64 * wave + 63 - __clzll((long long)mask) : -1;
    __syncthreads();
    int p = below ? base + 64 * wave + 63 - __clzll((long long)below) : -1;
    for (int w = wave - 1; p < 0 && w >= 0; --w) p = wv[w];
    if (p < 0) p = carry;
    if (f < F) tr[f] = p;
#pragma unroll
    for (int w = 0; w < 4; ++w)
      if (wv[w] >= 0) carry = wv[w];
    __syncthreads();
  }
  if (carry < 0) { /* F == 0 or no valid frame: no tempo */
    for (int f = tid; f < F; f += 256) tr[f] = 0;
    if (tid == 0) {
      rec->frames = F;
      rec->status = BL_UNEXPECTED;
      rec->n_filled = rec->n_folded = rec->reserved = 0;
    }
    return;
  }
  int A = 0;
  if (params->fold && anchor) A = *reinterpret_cast<const int *>(anchor + (size_t)sg.out_idx * (size_t)anchor_stride);
  const bool folding = tb_lag_ok(A);
  /* backward: the first valid frame at or behind f, the choice, the fold */
  int n_filled = 0, n_folded = 0;
  carry = -1;
  for (int base = (F - 1) / TB_TILE * TB_TILE; base >= 0; base -= TB_TILE) {
    const int f = base + tid;
    const int own = f < F ? lag_of(f) : 0;
    const bool valid = f < F && tb_lag_ok(own);
    const bl_u64 mask = __ballot(valid);
    const bl_u64 above = mask & (~0ull << lane); /* lanes lane .. 63 */
    if (lane == 0) wv[wave] = mask ? base + 64 * wave + __builtin_ctzll(mask) : -1;
    __syncthreads();
    int n = above ? base + 64 * wave + __builtin_ctzll(above) : -1;
    for (int w = wave + 1; n < 0 && w < 4; ++w) n = wv[w];
    if (n < 0) n = carry;
    if (f < F) {
      int q = own;
      if (!valid) {
        const int p = tr[f]; /* this lane's own word of the forward pass */
        n_filled += 1;
        q = lag_of(p >= 0 && (n < 0 || f - p <= n - f) ? p : n); /* one of the two exists: the song has a valid frame */
      }
      if (folding) {
        int q2 = q;
        if (3 * q <= 2 * A) q2 = 2 * q;
        else if (3 * q > 4 * A) q2 = q >> 1;
        if (q2 != q && tb_lag_ok(q2)) {
          q = q2;
          n_folded += 1;
        }
      }
      tr[f] = q;
    }
#pragma unroll
    for (int w = 3; w >= 0; --w)
      if (wv[w] >= 0) carry = wv[w];
    __syncthreads();
  }
  n_filled = tb_wave_sum(n_filled);
  n_folded = tb_wave_sum(n_folded);
  if (lane == 0) { red[0][wave] = n_filled; red[1][wave] = n_folded; }
  __syncthreads();
  if (tid == 0) {
    rec->frames = F;
    rec->status = BL_OK;
    rec->n_filled = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    rec->n_folded = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    rec->reserved = 0;
  }
}

/* ========================================================================= */
/* stages 4 to 8: the grid                                                    */

__global__ __launch_bounds__(256) void k_tbeats(const unsigned *__restrict__ onsets,
                                                const bl_tbeats_song *__restrict__ songs,
                                                const bl_amd_tbeats_params *__restrict__ params, const int32_t *track,
                                                bl_amd_song_tbeats *out, uint8_t *flags, uint16_t *links,
                                                uint16_t *link_scratch, bl_i64 *scores) {
  __shared__ bl_i64 ring[TB_RING];
  __shared__ bl_i64 pen[TB_PEN]; /* 1024 pen(d) - (1023 - d) of the run */
  __shared__ bl_i64 red_v[4];
  __shared__ int red_t[4];
  __shared__ unsigned red_m[4];
  const bl_tbeats_song sg = songs[blockIdx.x];
  const int H = sg.hops, F = sg.frames, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int seg = params->seg, origin = params->origin, tight = params->tight;
  const unsigned *o = onsets + sg.onset_off;
  const int32_t *q = track + sg.frame_off;
  uint8_t *fl = flags + sg.onset_off;
  uint16_t *P = links ? links + sg.onset_off : link_scratch + sg.hop_off;
  bl_i64 *Cg = scores ? scores + sg.onset_off : nullptr;
  bl_amd_song_tbeats *rec = out + sg.out_idx;
  if (rec->status != BL_OK) { /* no tempo (k_tbeats_track says so): the record says so, the arrays are 0 */
    for (int h = tid; h < H; h += 256) {
      fl[h] = 0;
      if (links) P[h] = 0;
      if (Cg) Cg[h] = 0;
    }
    if (tid == 0) {
      rec->score = 0;
      rec->pen_scale = 0;
      rec->hops = H;
      rec->n_beats = rec->first = rec->last = 0;
      rec->period_first = rec->period_last = rec->n_runs = 0;
    }
    return;
  }
  /* g(t), for 0 <= t < H; F >= 1 here */
  auto frame_of = [&](int t) { return t < origin ? 0 : min((t - origin) / seg, F - 1); };
  /* the scale: omax over the whole curve */
  unsigned m = 0;
  for (int h = tid; h < H; h += 256) m = max(m, o[h]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, off));
  if (lane == 0) red_m[wave] = m;
  for (int i = tid; i < TB_RING; i += 256) ring[i] = 0;
  __syncthreads();
  const bl_u64 W = (bl_u64)tight * max(max(red_m[0], red_m[1]), max(red_m[2], red_m[3]));
  const int g_last = frame_of(H - 1);
  int L = 0, n_runs = 0;
  for (int r0 = 0; r0 < H;) {
    /* the run that starts at hop r0: its period and its end */
    const int g0 = frame_of(r0);
    L = q[g0];
    int r1 = H;
    for (int ge = g0 + 1; ge <= g_last; ge += 64) {
      const int f = ge + lane;
      const bl_u64 differs = __ballot(f <= g_last && q[f] != L);
      if (differs) { /* frame ge' <= g_last starts at origin + ge' seg <= H - 1 */
        r1 = origin + (ge + __builtin_ctzll(differs)) * seg;
        break;
      }
    }
    r1 = __builtin_amdgcn_readfirstlane(r1);
    n_runs += 1;
    const int lo = (L + 1) >> 1, hi = 2 * L;
    {
      const int lL = (int)bl_ilog2_q12((bl_u64)L);
      for (int i = tid; i <= hi - lo; i += 256) { /* hi - lo <= 765 */
        const int e = (int)bl_ilog2_q12((bl_u64)(lo + i)) - lL;
        pen[i] = (bl_i64)((W * (bl_u64)(e * e)) >> 28) * 1024 - (1023 - (lo + i));
      }
    }
    __syncthreads();
    int gs = 0; /* G = 1 << gs lanes per hop, nt = 256 >> gs hops side by side */
    while (gs < 6 && (lo << (gs + 1)) <= 256) ++gs;
    const int G = 1 << gs, nt = 256 >> gs, sub = tid & (G - 1), j = tid >> gs;
    for (int t0 = r0; t0 < r1; t0 += lo) {
      const int cnt = min(lo, r1 - t0);
      for (int base = 0; base < cnt; base += nt) {
        const int t = t0 + base + j;
        const bool live = base + j < cnt;
        const unsigned ot = live ? o[t] : 0u;
        bl_i64 key = TB_NONE;
        if (live) {
          const int dmax = min(hi, t);
          for (int d = lo + sub; d <= dmax; d += G) key = bt_max(key, ring[(t - d) & (TB_RING - 1)] - pen[d - lo]);
        }
        key = bt_group_max(key, G);
        if (live && sub == 0) {
          const bl_i64 best = key >> 10; /* floor: v itself; far below 0 when there was no candidate */
          bl_i64 c = (bl_i64)ot;
          int p = 0;
          if (best > 0) {
            c += best;
            p = 1023 - (int)(key & 1023);
          }
          ring[t & (TB_RING - 1)] = c * 1024;
          P[t] = (uint16_t)p;
          fl[t] = 0;
          if (Cg) Cg[t] = c;
        }
      }
      __syncthreads();
    }
    r0 = r1;
  }
  /* the end: the largest C over the last L(H - 1) hops (all of them still in the ring), ties to the largest t */
  bl_i64 bv = -1;
  int bt = -1;
  for (int t = max(0, H - L) + tid; t < H; t += 256) {
    const bl_i64 c = ring[t & (TB_RING - 1)] >> 10;
    if (c >= bv) { bv = c; bt = t; }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const bl_i64 ov = __shfl_xor(bv, off);
    const int ot = __shfl_xor(bt, off);
    if (ov > bv || (ov == bv && ot > bt)) { bv = ov; bt = ot; }
  }
  if (lane == 0) { red_v[wave] = bv; red_t[wave] = bt; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w)
      if (red_v[w] > bv || (red_v[w] == bv && red_t[w] > bt)) { bv = red_v[w]; bt = red_t[w]; }
    int n = 0, first = -1, last = -1;
    if (bv != 0) {
      int t = last = bt;
      for (;;) {
        fl[t] = 1;
        ++n;
        const int p = P[t];
        if (p == 0 || p > t) break; /* p <= t by construction */
        t -= p;
      }
      first = t;
    }
    rec->score = bv;
    rec->pen_scale = W;
    rec->hops = H;
    rec->n_beats = n;
    rec->first = first;
    rec->last = last;
    rec->period_first = n ? q[frame_of(first)] : 0;
    rec->period_last = n ? q[frame_of(last)] : 0;
    rec->n_runs = n_runs;
  }
}

/* ========================================================================= */
/* launchers (declared in bl_tbeats.h)                                        */

int blk_tbeats_track(hipStream_t s, const bl_tbeats_song *d_songs, int n_songs, const void *d_lag, int lag_stride,
                     const void *d_anchor, int anchor_stride, const bl_amd_tbeats_params *d_params, int32_t *d_track,
                     bl_amd_song_tbeats *d_songs_out, blk_mark_fn mark, void *mark_user) {
  Mark m(mark, mark_user, TBK_TRACK, s);
  hipLaunchKernelGGL(k_tbeats_track, dim3((unsigned)n_songs), dim3(256), 0, s, d_songs, static_cast<const char *>(d_lag),
                     lag_stride, static_cast<const char *>(d_anchor), anchor_stride, d_params, d_track, d_songs_out);
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}

int blk_tbeats_group(hipStream_t s, const uint32_t *d_onsets, const bl_tbeats_song *d_songs, int n_songs,
                     const bl_amd_tbeats_params *d_params, const int32_t *d_track, bl_amd_song_tbeats *d_songs_out,
                     uint8_t *d_flags_out, uint16_t *d_links_out, uint16_t *d_link_scratch, int64_t *d_scores_out,
                     blk_mark_fn mark, void *mark_user) {
  Mark m(mark, mark_user, TBK_BEATS, s);
  hipLaunchKernelGGL(k_tbeats, dim3((unsigned)n_songs), dim3(256), 0, s, d_onsets, d_songs, d_params, d_track,
                     d_songs_out, d_flags_out, d_links_out, d_link_scratch, reinterpret_cast<bl_i64 *>(d_scores_out));
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}
