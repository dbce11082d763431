/*
 * bl_beat_kernels.hip — gfx950 kernel and launch layer of the per-song beat grid (bl_amd_beats_device,
 * bl_amd_beats_host, include/bliss_amd.h: bl_amd_song_beats): Ellis's dynamic-programming beat tracker over the onset
 * curve of the tempo call, stated in exact integers (the definition is in the header), so that neither the split of
 * the hops over lanes nor the order of a reduction shows in a result.
 *
 * Kernel:
 *   k_beats   one workgroup of 256 threads per song: the scale, the penalty table, the scores C and links P block by
 *             block, the end, the back-trace and the record
 *
 * Structure.  C[t] needs C[t - d] for d in [lo, hi], lo = (L + 1) >> 1, hi = 2 L.  For t in a block [t0, t0 + lo)
 * every source t - d <= t0 - 1 lies in an earlier block: the lo scores of a block do not depend on each other and only
 * the blocks are serial, one barrier each.
 *
 * State in LDS.  pen[d - lo] for d in [lo, hi]: at most 766 entries of 8 bytes.  C lives in a ring of BT_RING = 2048 entries,
 * C[t] at t mod 2048: a block reads [t0 - 2 L, t0 - 1] and writes [t0, t0 + lo - 1], a span of at most
 * 1020 + 255 = 1275 < 2048 hops, so within a block no slot is both read and written and the one barrier behind a block
 * is all the ordering there is.  C goes to memory only when the caller asks for the scores.
 *
 * Lane mapping.  G = 2^k consecutive lanes own one hop t and scan its window in strides of G; 256 / G hops run side by
 * side.  G = 256 / (lo rounded up to a power of two), at most a wave: lo <= 4 gives a wave per hop, lo in 65 .. 128 two
 * lanes, lo > 128 one lane per hop.  A candidate is the key 1024 v + (1023 - d) with v = C[t - d] - pen(d): v >= -2^26
 * and v < 2^42, d <= 1020, so the key fits 53 bits and its maximum is the largest v with the smallest d.  The ring
 * holds 1024 C and the table 1024 pen(d) - (1023 - d), so a key is one 64-bit subtraction.  The group
 * joins its keys by DPP inside a row of 16 lanes and by two wave shuffles beyond it; every lane of the workgroup takes
 * every step (a lane without a hop carries the least key), so the cross-lane moves see whole groups.
 *
 * Bounds.  o < 2^18, tight <= 4096: W = tight omax < 2^30; e <= 4096 for every L in 2 .. 510 and d in [lo, hi]
 * (tests/test_beat_reference_host.py checks all of them), so W e^2 < 2^54 and pen < 2^26.  C grows by less than 2^18
 * per hop: C < 2^42.  Every index: a source t - d has 0 <= t - d (the window is clipped at d <= t) and d - lo < 766;
 * a link P[t] = d <= t, so the back-trace never leaves [0, H).
 *
 * Back-trace.  One lane chases P from the end; it runs behind the barrier that follows the last block, by which time
 * the workgroup has written every flag of the song as 0 and every P.  Its loads depend on each other: it is the
 * serial rest of the kernel, about H / L loads.
 */
#include <hip/hip_runtime.h>

#include "bl_beat_lanes.h"
#include "bl_ilog2.h"
#include "bl_launch.h"

#define BT_RING 2048
#define BT_PEN 768
#define BT_NONE (-0x7FFFFFFFFFFFFFFFll - 1) /* the least key: a lane or a hop without a candidate */

__global__ __launch_bounds__(256) void k_beats(const unsigned *__restrict__ onsets,
                                               const bl_beat_song *__restrict__ songs, const char *__restrict__ period,
                                               int period_stride, int tight, bl_amd_song_beats *out, uint8_t *flags,
                                               uint16_t *links, uint16_t *link_scratch, bl_i64 *scores) {
  __shared__ bl_i64 ring[BT_RING];
  __shared__ bl_i64 pen[BT_PEN]; /* 1024 pen(d) - (1023 - d) */
  __shared__ bl_i64 red_v[4];
  __shared__ int red_t[4];
  __shared__ unsigned red_m[4];
  const bl_beat_song sg = songs[blockIdx.x];
  const int H = sg.hops, tid = threadIdx.x, wave = tid >> 6;
  const unsigned *o = onsets + sg.onset_off;
  uint8_t *fl = flags + sg.onset_off;
  uint16_t *P = links ? links + sg.onset_off : link_scratch + sg.hop_off;
  bl_i64 *Cg = scores ? scores + sg.onset_off : nullptr;
  bl_amd_song_beats *rec = out + sg.out_idx;
  const int L = *reinterpret_cast<const int *>(period + (size_t)sg.out_idx * (size_t)period_stride);
  if (L < 2 || L > BL_AMD_BEATS_PERIOD_MAX) { /* no tempo: the record says so, the arrays are 0 */
    for (int h = tid; h < H; h += 256) {
      fl[h] = 0;
      if (links) P[h] = 0;
      if (Cg) Cg[h] = 0;
    }
    if (tid == 0) {
      rec->score = 0;
      rec->pen_scale = 0;
      rec->hops = H;
      rec->period = L;
      rec->n_beats = rec->first = rec->last = 0;
      rec->status = BL_UNEXPECTED;
    }
    return;
  }
  /* the scale: omax over the whole curve */
  unsigned m = 0;
  for (int h = tid; h < H; h += 256) m = max(m, o[h]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, off));
  if ((tid & 63) == 0) red_m[wave] = m;
  for (int i = tid; i < BT_RING; i += 256) ring[i] = 0;
  __syncthreads();
  const bl_u64 W = (bl_u64)tight * max(max(red_m[0], red_m[1]), max(red_m[2], red_m[3]));
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
  for (int t0 = 0; t0 < H; t0 += lo) {
    const int cnt = min(lo, H - t0);
    for (int base = 0; base < cnt; base += nt) {
      const int t = t0 + base + j;
      const bool live = base + j < cnt;
      const unsigned ot = live ? o[t] : 0u;
      bl_i64 key = BT_NONE;
      if (live) {
        const int dmax = min(hi, t);
        for (int d = lo + sub; d <= dmax; d += G) key = bt_max(key, ring[(t - d) & (BT_RING - 1)] - pen[d - lo]);
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
        ring[t & (BT_RING - 1)] = c * 1024;
        P[t] = (uint16_t)p;
        fl[t] = 0;
        if (Cg) Cg[t] = c;
      }
    }
    __syncthreads();
  }
  /* the end: the largest C over the last L hops (all of them still in the ring), ties to the largest t */
  bl_i64 bv = -1;
  int bt = -1;
  for (int t = max(0, H - L) + tid; t < H; t += 256) {
    const bl_i64 c = ring[t & (BT_RING - 1)] >> 10;
    if (c >= bv) { bv = c; bt = t; }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const bl_i64 ov = __shfl_xor(bv, off);
    const int ot = __shfl_xor(bt, off);
    if (ov > bv || (ov == bv && ot > bt)) { bv = ov; bt = ot; }
  }
  if ((tid & 63) == 0) { red_v[wave] = bv; red_t[wave] = bt; }
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
    rec->period = L;
    rec->n_beats = n;
    rec->first = first;
    rec->last = last;
    rec->status = BL_OK;
  }
}

/* ========================================================================= */
/* launcher (declared in bl_launch.h)                                         */

int blk_beats_group(hipStream_t s, const uint32_t *d_onsets, const bl_beat_song *d_songs, int n_songs,
                    const void *d_period, int period_stride, int tight, bl_amd_song_beats *d_songs_out,
                    uint8_t *d_flags_out, uint16_t *d_links_out, uint16_t *d_link_scratch, int64_t *d_scores_out,
                    blk_mark_fn mark, void *mark_user) {
  Mark m(mark, mark_user, PK_BEATS, s);
  hipLaunchKernelGGL(k_beats, dim3(n_songs), dim3(256), 0, s, d_onsets, d_songs, static_cast<const char *>(d_period),
                     period_stride, tight, d_songs_out, d_flags_out, d_links_out, d_link_scratch,
                     reinterpret_cast<bl_i64 *>(d_scores_out));
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}
