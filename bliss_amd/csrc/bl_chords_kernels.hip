/*
 * bl_chords_kernels.hip — gfx950 kernels and launch layer of the chord sequences (bl_amd_chords_device; the definition
 * is the block in include/bliss_amd.h).  Every quantity is an exact integer and no atomics touch global memory: what a
 * song gets is written once, by the one wavefront that owns the song.
 *
 * Kernels:
 *   k_chords_forward<SPW>  the recurrence: SPW songs per wavefront (64 / SPW lanes each), a workgroup of one wavefront,
 *                    no barrier.  A lane is a label c and holds the column cost[.][c] in 25 registers as
 *                    K[a] = 32 cost[a][c] - (31 - a), and W = 32 (V[c] - base).  A candidate is W of lane a minus K[a]
 *                    = 32 (V[a] - cost[a][c]) + (31 - a): one integer maximum over the 25 gives the value (its bits
 *                    above the fifth) and the smallest a that attains it (31 minus its low five bits).  W of lane a
 *                    comes by v_readlane_b32 with a constant lane (SPW 1) or by ds_bpermute_b32 with the song's first
 *                    lane plus a (SPW 2).  The emission is three v_dot4_u32_u8 of the unit's three words against the
 *                    lane's masks, which hold 32 in the bytes of the triad's three classes.  Units come four at a time,
 *                    one round ahead of their use; the four backpointers of a lane make one word, and a round's 32
 *                    words (128 bytes) are one store.  After a round W of label 24 is taken off every W of the song and
 *                    added to the song's base.  At the end a maximum over W + (31 - c) gives the score and the last
 *                    label, which the song's first lane leaves for the back-trace.
 *   k_chords_trace   one wavefront per song.  From the last BL_CHORDS_TRACE_UNITS units backwards: the lanes copy the
 *                    units' backpointers to LDS, lane 0 walks L_{t-1} = B_t[L_t] through them and leaves the labels in
 *                    LDS, and the lanes write the labels, count the changes and add to the 25 counts (LDS atomics).
 *                    Then a wave maximum over (count, 31 - label) picks `top`, and the record and the counts are written.
 *
 * Bounds.  max V_t - min V_t <= 1024 + 381 for t >= 1 (the header's argument: every V_t[c] lies between
 * max V_{t-1} - 1024 and max V_{t-1} + 381) and <= 381 for t = 0.  W is taken relative to label 24 once a round, so
 * within a round |V[c] - base| <= 1405 + 4 x 1024: |W| < 2^18, a candidate lies within 2^18 + 32 x 1024 + 31 < 2^19, and
 * the base, a true score, has |base| < 2^30.  All of it is int32 without a wrap.
 *
 * What is read.  A unit is addressed through its song's record and only for t < U; a backpointer word only inside the
 * song's own rounds.  A wavefront's second song may be missing (an odd count): its lanes carry U = 0, load nothing and
 * store nothing.  The backpointer bytes of lanes 25 .. 31 and of the units past U in a song's last round are never
 * written and never used: the walk only follows labels below 25.
 */
#include <hip/hip_runtime.h>
#include <limits.h>

#include "bl_chords.h"

#define CH_LANES 64
#define CH_LABELS BL_CHORDS_LABELS
#define CH_STEP BL_CHORDS_STEP_UNITS
#define CH_TRACE BL_CHORDS_TRACE_UNITS
#define CH_BPW BL_CHORDS_BP_WORDS

static_assert(sizeof(bl_amd_chords_params) == 1264, "the parameters are 1264 bytes");
static_assert(sizeof(bl_amd_song_chords) == 32, "the record is 32 bytes");
static_assert(sizeof(bl_chords_song) == 24 && sizeof(bl_chords_end) == 8, "the workspace records");
static_assert(CH_LABELS == 25 && CH_STEP == 4 && CH_BPW == 32, "a label per lane of 32, a backpointer byte per unit of a round");
static_assert(CH_TRACE % CH_STEP == 0 && CH_TRACE / CH_STEP * CH_BPW * 4 <= 16 * 1024, "the back-trace's rounds fit static LDS");

/* ========================================================================= */
/* forward                                                                    */

/* W of label a of the lane's own song; a: a constant */
template <int SPW>
__device__ __forceinline__ int ch_prev(int w, int first_lane_bytes, int a) {
  if (SPW == 1) return __builtin_amdgcn_readlane(w, a);
  return __builtin_amdgcn_ds_bpermute(first_lane_bytes + 4 * a, w);
}

template <int SPW>
__global__ __launch_bounds__(CH_LANES) void k_chords_forward(const uint4 *__restrict__ units,
                                                             const bl_chords_song *__restrict__ songs, int n_songs,
                                                             const bl_amd_chords_params *__restrict__ prm,
                                                             uint32_t *__restrict__ bp, bl_chords_end *__restrict__ end) {
  constexpr int LPS = CH_LANES / SPW; /* lanes per song */
  const int lane = threadIdx.x;
  const int half = lane / LPS, c = lane % LPS;
  const long long song = (long long)blockIdx.x * SPW + half;
  const bool live = song < n_songs;
  const bool lab = c < CH_LABELS;
  bl_chords_song sg;
  sg.unit_off = 0, sg.bp_off = 0, sg.units = 0, sg.reserved = 0;
  if (live) sg = songs[song];
  const int U = sg.units;
  const uint4 *__restrict__ up = units + sg.unit_off;
  uint32_t *__restrict__ pb = bp + sg.bp_off * CH_BPW;
  const int first = half * LPS * 4;

  /* the lane's column of the costs and its template */
  const int cc = lab ? c : CH_LABELS - 1;
  int K[CH_LABELS];
#pragma unroll
  for (int a = 0; a < CH_LABELS; ++a) K[a] = 32 * (int)prm->cost[a * CH_LABELS + cc] - (31 - a);
  uint32_t m0 = 0u, m1 = 0u, m2 = 0u;
  if (c < 24) {
    const int r = c % 12;
    const int p[3] = {r, (r + (c < 12 ? 4 : 3)) % 12, (r + 7) % 12};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const uint32_t bit = 32u << (8 * (p[k] & 3));
      if ((p[k] >> 2) == 0) m0 |= bit;
      else if ((p[k] >> 2) == 1) m1 |= bit;
      else m2 |= bit;
    }
  }
  const uint32_t n32 = c == 24 ? 32u * (uint32_t)prm->none : 0u;

  int Umax = U;
  if (SPW == 2) Umax = max(U, __shfl_xor(U, 32));
  Umax = __builtin_amdgcn_readfirstlane(Umax);

  const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
  int W = 0, base = 0;
  uint4 nx[CH_STEP];
#pragma unroll
  for (int k = 0; k < CH_STEP; ++k) nx[k] = k < U ? up[k] : zero4;

  for (int t0 = 0; t0 < Umax; t0 += CH_STEP) {
    uint4 cu[CH_STEP];
#pragma unroll
    for (int k = 0; k < CH_STEP; ++k) {
      cu[k] = nx[k];
      const int tn = t0 + CH_STEP + k; /* the next round's unit; none past U - 1 is fetched */
      nx[k] = tn < U ? up[tn] : zero4;
    }
    uint32_t bpw = 0u;
#pragma unroll
    for (int k = 0; k < CH_STEP; ++k) {
      const int t = t0 + k;
      const uint32_t e32 = __builtin_amdgcn_udot4(
          cu[k].x, m0, __builtin_amdgcn_udot4(cu[k].y, m1, __builtin_amdgcn_udot4(cu[k].z, m2, n32, false), false), false);
      int m = ch_prev<SPW>(W, first, 0) - K[0];
#pragma unroll
      for (int a = 1; a < CH_LABELS; ++a) m = max(m, ch_prev<SPW>(W, first, a) - K[a]);
      const int keep = t == 0 ? 0 : ~31; /* V_0 = E_0: no transition into the first unit */
      const int wn = (m & keep) + (int)e32;
      if (t < U) W = wn;
      bpw |= (uint32_t)(31 - (m & 31)) << (8 * k);
    }
    if (lab && t0 < U) pb[(long long)(t0 / CH_STEP) * CH_BPW + c] = bpw;
    const int d = ch_prev<SPW>(W, first, CH_LABELS - 1); /* a multiple of 32, as every W */
    W -= d;
    base += d >> 5;
  }

  int key = lab ? W + (31 - c) : INT_MIN;
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) key = max(key, __shfl_xor(key, o)); /* stays inside a song's 32 label lanes */
  if (c == 0 && U > 0) {
    bl_chords_end e;
    e.score = base + (key >> 5);
    e.last = 31 - (key & 31);
    end[song] = e;
  }
}

/* ========================================================================= */
/* back-trace, record, counts                                                 */

__device__ __forceinline__ int ch_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ uint32_t ch_wave_max(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
  return v;
}

__global__ __launch_bounds__(CH_LANES) void k_chords_trace(const bl_chords_song *__restrict__ songs,
                                                           const uint32_t *__restrict__ bp,
                                                           const bl_chords_end *__restrict__ end,
                                                           bl_amd_song_chords *__restrict__ out,
                                                           uint8_t *__restrict__ labels_out,
                                                           uint32_t *__restrict__ hist_out) {
  __shared__ uint32_t sbp[CH_TRACE / CH_STEP * CH_BPW]; /* the backpointers of CH_TRACE units */
  __shared__ uint8_t slab[CH_TRACE];                    /* their labels */
  __shared__ uint32_t shist[32];
  __shared__ int scarry; /* the label of the unit before the block */
  const long long song = blockIdx.x;
  const int lane = threadIdx.x;
  const bl_chords_song sg = songs[song];
  const int U = sg.units;
  int32_t *po = reinterpret_cast<int32_t *>(out + song);
  uint32_t *ph = hist_out ? hist_out + CH_LABELS * song : nullptr;

  if (U <= 0) { /* the whole wavefront leaves together */
    if (lane < 8) po[lane] = lane == 1 ? BL_AMD_CHORDS_EMPTY : lane == 4 ? -1 : 0;
    if (ph && lane < CH_LABELS) ph[lane] = 0u;
    return;
  }
  const bl_chords_end e = end[song];
  const uint32_t *__restrict__ pb = bp + sg.bp_off * CH_BPW;
  uint8_t *pl = labels_out ? labels_out + sg.unit_off : nullptr;
  const uint8_t *b8 = reinterpret_cast<const uint8_t *>(sbp);
  if (lane < 32) shist[lane] = 0u;
  int L = e.last & 31, changes = 0;
  __syncthreads();

  for (int t0 = (U - 1) / CH_TRACE * CH_TRACE; t0 >= 0; t0 -= CH_TRACE) {
    const int n = min(CH_TRACE, U - t0);
    const int words = (n + CH_STEP - 1) / CH_STEP * CH_BPW; /* the song's own rounds, no word past them */
    for (int i = lane; i < words; i += CH_LANES) sbp[i] = pb[(long long)(t0 / CH_STEP) * CH_BPW + i];
    __syncthreads();
    if (lane == 0) {
      for (int i = n - 1; i >= 0; --i) {
        slab[i] = (uint8_t)L;
        if (t0 + i > 0) L = b8[(i >> 2) * (CH_BPW * 4) + L * 4 + (i & 3)] & 31; /* below 25 by construction */
      }
      scarry = L;
    }
    __syncthreads();
    for (int i = lane; i < n; i += CH_LANES) {
      const int l = slab[i];
      const int before = i > 0 ? (int)slab[i - 1] : scarry;
      if (t0 + i > 0 && l != before) ++changes;
      atomicAdd(&shist[l], 1u);
      if (pl) pl[t0 + i] = (uint8_t)l;
    }
    __syncthreads();
  }

  changes = ch_wave_sum(changes);
  const uint32_t cnt = lane < CH_LABELS ? shist[lane] : 0u;                     /* below 2^20 */
  const uint32_t top = ch_wave_max(lane < CH_LABELS ? (cnt << 5) | (uint32_t)(31 - lane) : 0u);
  if (ph && lane < CH_LABELS) ph[lane] = cnt;
  if (lane == 0) {
    po[0] = U;
    po[1] = 0;
    po[2] = e.score;
    po[3] = changes;
    po[4] = 31 - (int)(top & 31u);
    po[5] = (int)(top >> 5);
    po[6] = (int)shist[BL_AMD_CHORDS_NONE];
    po[7] = 0;
  }
}

/* ========================================================================= */
/* launchers (declared in bl_chords.h)                                        */

int blk_chords_forward(hipStream_t s, const uint4 *d_units, const bl_chords_song *d_songs, int n_songs,
                       const bl_amd_chords_params *d_params, int spw, uint32_t *d_bp, bl_chords_end *d_end,
                       blk_mark_fn mark, void *mark_user) {
  Mark m(mark, mark_user, CHK_FORWARD, s);
  if (spw == 2)
    hipLaunchKernelGGL(k_chords_forward<2>, dim3((unsigned)((n_songs + 1) / 2)), dim3(CH_LANES), 0, s, d_units, d_songs,
                       n_songs, d_params, d_bp, d_end);
  else
    hipLaunchKernelGGL(k_chords_forward<1>, dim3((unsigned)n_songs), dim3(CH_LANES), 0, s, d_units, d_songs, n_songs,
                       d_params, d_bp, d_end);
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}

int blk_chords_trace(hipStream_t s, const bl_chords_song *d_songs, int n_songs, const uint32_t *d_bp,
                     const bl_chords_end *d_end, bl_amd_song_chords *d_out, uint8_t *d_labels_out, uint32_t *d_hist_out,
                     blk_mark_fn mark, void *mark_user) {
  Mark m(mark, mark_user, CHK_TRACE, s);
  hipLaunchKernelGGL(k_chords_trace, dim3((unsigned)n_songs), dim3(CH_LANES), 0, s, d_songs, d_bp, d_end, d_out,
                     d_labels_out, d_hist_out);
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}
