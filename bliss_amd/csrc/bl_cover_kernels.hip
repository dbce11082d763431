/*
 * bl_cover_kernels.hip — gfx950 kernels and launch layer of the cover and version matching (bl_amd_cover_match_device;
 * the definition is the block in include/bliss_amd.h).  Every quantity is an exact integer and no atomics touch global
 * memory: a record is written once, by the one wavefront that owns its pair.
 *
 * Kernels:
 *   k_cover_profile  one wavefront per song of either set.  A lane sums the twelve classes of every 64th unit (a byte of
 *                    a word is v_dot4_u32_u8 against a one in that byte), the wave adds the lanes' sums and lane 0
 *                    writes the twelve uint32 g[k].
 *   k_cover_align    one wavefront per pair, a workgroup of 64 lanes, no barrier.  Lanes 0 .. 11 compute C(r) and a wave
 *                    maximum picks r.  The 64 lanes own 64 consecutive columns of b (a strip); a lane holds its column's
 *                    unit in three registers, rotated by r over the twelve bytes.  The rows of a pass through the lanes
 *                    as a skewed wavefront: at step s lane t works on cell (s - t, j0 + t).  It takes the unit of a, H
 *                    and O of lane t - 1 from the previous step by a whole-wave shift (v_mov_b32_dpp wave_shr:1); H_diag
 *                    is the previous step's H_left and H_up the lane's own.  Lane 0 has no left neighbour: the units of
 *                    a and the (H, O) the previous strip's last lane left in LDS are fetched 64 rows at a time, one row
 *                    per lane and one block ahead, and lane 0 takes row s out of them with v_readlane_b32.  S is three
 *                    v_dot4_u32_u8.  The last lane writes (H, O) of every row to LDS (8 bytes a row) while a further
 *                    strip follows.  Every lane keeps its best 64-bit key and the cell's origin; one wave maximum at the
 *                    end gives the record, which the lane that holds the key writes.
 *
 * What is read.  A unit is addressed through its song's record only and every index is checked against the pair's own
 * Ua and Ub: a lane outside the matrix loads nothing, contributes key 0 and hands on zeros.  A pair index outside its set
 * reads no record.
 *
 * LDS order.  Row i of the strip edge is read no later than step 64 floor(i / 64) of a strip (a block ahead of its use)
 * and written at step i + 63 of the same strip, by the same wavefront: the read of a row always precedes its next write,
 * and the write its next read, in program order.
 *
 * Untuned: first forms.  A strip costs Ua + 63 steps for Ua rows, 63 of them skew (the last strip of a pair runs only
 * as far as its columns go); the longer song is not put on the rows, so a short b leaves lanes idle for a whole pass;
 * a workgroup holds one pair, so a call of short songs keeps one wavefront per workgroup slot.
 */
#include <hip/hip_runtime.h>

#include "bl_cover.h"

typedef unsigned long long cv_u64;

#define CV_LANES BL_COVER_LANES
#define CV_UMAX BL_COVER_UNITS_MAX
#define CV_LOW13 8191u

static_assert(sizeof(bl_amd_cover_match) == 40, "the record is 40 bytes");
static_assert(sizeof(bl_amd_cover_params) == 16, "the parameters are 16 bytes");
static_assert(CV_LANES == 64 && BL_COVER_STRIP == CV_LANES && BL_COVER_ROWS == CV_LANES, "one column and row per lane");
static_assert(CV_UMAX == 8192 && CV_UMAX * 8 <= 64 * 1024, "the strip edge of the longest song fits the default LDS");

__device__ __forceinline__ uint32_t cv_wave_sum(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

__device__ __forceinline__ cv_u64 cv_wave_max(cv_u64 k) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const cv_u64 o = __shfl_xor(k, off);
    k = o > k ? o : k;
  }
  return k;
}

/* ========================================================================= */
/* profile                                                                    */

__global__ __launch_bounds__(CV_LANES) void k_cover_profile(const uint4 *__restrict__ units_a,
                                                            const uint4 *__restrict__ units_b,
                                                            const bl_cover_seq *__restrict__ seq, int n_a,
                                                            uint32_t *__restrict__ prof) {
  const int song = blockIdx.x, lane = threadIdx.x;
  const bl_cover_seq sq = seq[song];
  const uint4 *__restrict__ up = (song < n_a ? units_a : units_b) + sq.off;
  const int U = sq.count > CV_UMAX ? 0 : sq.count; /* a song that is too long has no profile: g stays below 2^20 */
  uint32_t g[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) g[k] = 0u;
  for (int u = lane; u < U; u += CV_LANES) {
    const uint4 v = up[u];
#pragma unroll
    for (int k = 0; k < 12; ++k)
      g[k] = __builtin_amdgcn_udot4(k < 4 ? v.x : k < 8 ? v.y : v.z, 1u << (8 * (k & 3)), g[k], false);
  }
#pragma unroll
  for (int k = 0; k < 12; ++k) g[k] = cv_wave_sum(g[k]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 12; ++k) prof[12 * (long long)song + k] = g[k];
  }
}

/* ========================================================================= */
/* alignment                                                                  */

/* every lane takes v of the lane below it; lane 0 keeps its own (and replaces it) */
__device__ __forceinline__ uint32_t cv_from_below(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
}

__device__ __forceinline__ uint32_t cv_lane_value(uint32_t v, int l) { /* l: the same in every lane */
  return (uint32_t)__builtin_amdgcn_readlane((int)v, l);
}

/* byte k of the result is byte (k + r) mod 12 of the unit's twelve; r: the same in every lane, 0 .. 11 */
__device__ __forceinline__ void cv_rotate(const uint4 v, int r, uint32_t &o0, uint32_t &o1, uint32_t &o2) {
  const int ws = r >> 2, bs = 8 * (r & 3);
  const uint32_t a = ws == 0 ? v.x : ws == 1 ? v.y : v.z;
  const uint32_t b = ws == 0 ? v.y : ws == 1 ? v.z : v.x;
  const uint32_t c = ws == 0 ? v.z : ws == 1 ? v.x : v.y;
  o0 = (uint32_t)((((cv_u64)b << 32) | a) >> bs);
  o1 = (uint32_t)((((cv_u64)c << 32) | b) >> bs);
  o2 = (uint32_t)((((cv_u64)a << 32) | c) >> bs);
}

__global__ __launch_bounds__(CV_LANES) void k_cover_align(const uint4 *__restrict__ units_a,
                                                          const uint4 *__restrict__ units_b,
                                                          const bl_cover_seq *__restrict__ seq, int n_a, int n_b,
                                                          const uint32_t *__restrict__ prof,
                                                          const int32_t *__restrict__ pairs, int thr, int gap,
                                                          int transpose, bl_amd_cover_match *__restrict__ out) {
  extern __shared__ uint2 edge[]; /* (H, O) of the strip's last column, one per row of a */
  const int lane = threadIdx.x;
  const long long p = blockIdx.x;
  const int ia = pairs[2 * p], ib = pairs[2 * p + 1];
  int32_t *po = reinterpret_cast<int32_t *>(out + p);

  if (ia < 0 || ia >= n_a || ib < 0 || ib >= n_b) { /* the whole wavefront leaves together, here and below */
    if (lane < 10) po[lane] = lane == 8 ? BL_AMD_COVER_BAD_INDEX : 0;
    return;
  }
  const bl_cover_seq sa = seq[ia], sb = seq[n_a + ib];
  const int Ua = sa.count, Ub = sb.count;
  if (Ua > CV_UMAX || Ub > CV_UMAX) {
    if (lane < 10) po[lane] = lane == 6 ? Ua : lane == 7 ? Ub : lane == 8 ? BL_AMD_COVER_TOO_LONG : 0;
    return;
  }
  if (Ua == 0 || Ub == 0) {
    if (lane < 10) po[lane] = lane == 6 ? Ua : lane == 7 ? Ub : lane == 8 ? BL_AMD_COVER_NO_MATCH : 0;
    return;
  }

  /* transposition: lane r < 12 has C(r); the largest C, then the smallest r */
  int r = transpose;
  if (transpose < 0) {
    cv_u64 key = 0ull;
    if (lane < 12) {
      const uint32_t *ga = prof + 12 * (long long)ia, *gb = prof + 12 * ((long long)n_a + ib);
      cv_u64 c = 0ull;
#pragma unroll
      for (int k = 0; k < 12; ++k) {
        const int kk = k + lane;
        c += (cv_u64)ga[k] * (cv_u64)gb[kk >= 12 ? kk - 12 : kk]; /* below 2^40 each */
      }
      key = (c << 4) | (cv_u64)(15 - lane); /* C < 2^44 */
    }
    r = 15 - (int)(cv_wave_max(key) & 15ull);
  }

  const uint4 *__restrict__ pa = units_a + sa.off;
  const uint4 *__restrict__ pb = units_b + sb.off;
  const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
  cv_u64 best = 0ull;
  uint32_t best_o = 0u;

  for (int j0 = 0; j0 < Ub; j0 += BL_COVER_STRIP) {
    const int ncol = min(BL_COVER_STRIP, Ub - j0); /* below 64 only in the last strip */
    const bool more = j0 + BL_COVER_STRIP < Ub;    /* a further strip reads this one's edge */
    const bool left_edge = j0 > 0;
    const int j = j0 + lane;
    const bool col = lane < ncol;
    uint32_t b0, b1, b2;
    cv_rotate(col ? pb[j] : zero4, r, b0, b1, b2);
    const uint32_t cj = CV_LOW13 - (uint32_t)(j & (int)CV_LOW13);
    const int steps = Ua + ncol - 1;

    /* what the lane hands on: the unit of a it used, its H and O; and what it was handed one step ago */
    uint32_t a0 = 0u, a1 = 0u, a2 = 0u, h = 0u, o = 0u, hl_prev = 0u, ol_prev = 0u;
    /* rows s0 + lane of a and of the edge, a block ahead */
    uint4 na = lane < Ua ? pa[lane] : zero4;
    uint2 ne = left_edge && lane < Ua ? edge[lane] : make_uint2(0u, 0u);
    for (int s0 = 0; s0 < steps; s0 += BL_COVER_ROWS) {
      const uint4 ca = na;
      const uint2 ce = ne;
      const int nr = s0 + BL_COVER_ROWS + lane; /* the next block's row; none past Ua - 1 is fetched */
      na = nr < Ua ? pa[nr] : zero4;
      ne = left_edge && nr < Ua ? edge[nr] : make_uint2(0u, 0u);
      const int kend = min(BL_COVER_ROWS, steps - s0);
      for (int k = 0; k < kend; ++k) {
        const int i = s0 + k - lane;
        /* from the lane below, as it stood after the previous step; lane 0 from row s0 + k of the block */
        uint32_t x0 = cv_from_below(a0), x1 = cv_from_below(a1), x2 = cv_from_below(a2);
        uint32_t hl = cv_from_below(h), ol = cv_from_below(o);
        const uint32_t f0 = cv_lane_value(ca.x, k), f1 = cv_lane_value(ca.y, k), f2 = cv_lane_value(ca.z, k);
        const uint32_t fh = cv_lane_value(ce.x, k), fo = cv_lane_value(ce.y, k);
        if (lane == 0) x0 = f0, x1 = f1, x2 = f2, hl = fh, ol = fo;

        const uint32_t S = __builtin_amdgcn_udot4(x0, b0, __builtin_amdgcn_udot4(x1, b1, __builtin_amdgcn_udot4(x2, b2, 0u, false), false), false);
        const int hd = (int)hl_prev;
        const int d = hd + (int)S - thr, u = (int)h - gap, l = (int)hl - gap; /* h: the lane's own, one row up */
        int H = max(max(d, u), max(l, 0));
        uint32_t O = d == H ? (hd == 0 ? ((uint32_t)i << 13) | (uint32_t)j : ol_prev) : u == H ? o : ol;
        const bool cell = col && i >= 0 && i < Ua;
        if (!cell || H <= 0) H = 0, O = 0u;

        const cv_u64 key = ((cv_u64)(uint32_t)H << 26) | (cv_u64)(((CV_LOW13 - (uint32_t)(i & (int)CV_LOW13)) << 13) | cj);
        if (H > 0 && key > best) best = key, best_o = O;
        if (more && lane == CV_LANES - 1 && i >= 0 && i < Ua) edge[i] = make_uint2((uint32_t)H, O);

        hl_prev = hl, ol_prev = ol;
        a0 = x0, a1 = x1, a2 = x2, h = (uint32_t)H, o = O;
      }
    }
  }

  const cv_u64 top = cv_wave_max(best);
  if (top == 0ull) {
    if (lane < 10)
      po[lane] = lane == 5 ? r : lane == 6 ? Ua : lane == 7 ? Ub : lane == 8 ? BL_AMD_COVER_NO_MATCH : 0;
    return;
  }
  if (best == top) { /* one lane: a key names its cell */
    const uint32_t low = (uint32_t)(top & ((1u << 26) - 1u));
    po[0] = (int32_t)(uint32_t)(top >> 26);
    po[1] = (int32_t)(best_o >> 13);
    po[2] = (int32_t)(CV_LOW13 - (low >> 13));
    po[3] = (int32_t)(best_o & CV_LOW13);
    po[4] = (int32_t)(CV_LOW13 - (low & CV_LOW13));
    po[5] = r;
    po[6] = Ua;
    po[7] = Ub;
    po[8] = 0;
    po[9] = 0;
  }
}

/* ========================================================================= */
/* launchers (declared in bl_cover.h)                                         */

int blk_cover_profile(hipStream_t s, const uint4 *d_units_a, const uint4 *d_units_b, const bl_cover_seq *d_seq, int n_a,
                      int n_seq, uint32_t *d_prof, blk_mark_fn mark, void *mark_user) {
  Mark m(mark, mark_user, CVK_PROFILE, s);
  hipLaunchKernelGGL(k_cover_profile, dim3((unsigned)n_seq), dim3(CV_LANES), 0, s, d_units_a, d_units_b, d_seq, n_a,
                     d_prof);
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}

int blk_cover_align(hipStream_t s, const uint4 *d_units_a, const uint4 *d_units_b, const bl_cover_seq *d_seq, int n_a,
                    int n_b, const uint32_t *d_prof, const int32_t *d_pairs, int n_pairs, int max_units_a,
                    const bl_amd_cover_params &p, bl_amd_cover_match *d_out, blk_mark_fn mark, void *mark_user) {
  if (max_units_a < 1) max_units_a = 1;
  if (max_units_a > CV_UMAX) max_units_a = CV_UMAX;
  const size_t lds = sizeof(uint2) * (size_t)max_units_a; /* at most 64 KB: no attribute is needed */
  Mark m(mark, mark_user, CVK_ALIGN, s);
  hipLaunchKernelGGL(k_cover_align, dim3((unsigned)n_pairs), dim3(CV_LANES), lds, s, d_units_a, d_units_b, d_seq, n_a,
                     n_b, d_prof, d_pairs, p.thr, p.gap, p.transpose, d_out);
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}
