/*
 * bl_fprint_kernels.hip — gfx950 kernels and launch layer of the audio fingerprints (bl_amd_fprint_words_device,
 * bl_amd_fprint_match_device; the definition is the block in include/bliss_amd.h).  Every quantity is an exact
 * integer and no atomics touch global memory: a result is written once, by the one workgroup that owns it.
 *
 * Kernels:
 *   k_fprint_words  one workgroup per (song, run of 256 words), one lane per word.  The run's 256 + 15 frames are copied
 *                   to LDS with coalesced loads; every lane sums 8 frames (H_t = X_t + .. + X_t+7), the sums go back to
 *                   LDS over the frames, and word t is compared out of H_t (S1) and H_t+8 (S2).
 *   k_fprint_match  one workgroup per pair.  It walks the offsets in chunks and `a` in tiles (bl_fprint_geom), so
 *                   neither a sequence nor an offset range has to fit anything; the errors of all offsets of a chunk
 *                   stay in registers over the tiles, are joined in LDS, and the best key is reduced at the end.
 *
 * The match's inner loop.  A lane owns 4 consecutive offsets d .. d + 3 and walks its strip of `a` 4 words at a time:
 * the 16 word pairs of such a step need a[i .. i + 3] and the 7 words b[i + d .. i + d + 6], so a step costs one
 * 16-byte LDS read of `a` (the lanes of a row read one address: a broadcast), one of `b` (the upper four of this step
 * are the lower four of the next; lanes read consecutive 16-byte pieces) and 16 x (v_xor, v_bcnt with accumulate).
 * d and i are multiples of 4 away from the tile's origin, so every LDS read is aligned.
 *
 * What is read.  A tile of `a` and the window of `b` under it are copied to LDS with a range check per word against
 * the song's own count: a word outside [0, W) is a zero in LDS and is never fetched, so a neighbour in the
 * concatenated words cannot leak in.  A step whose 16 pairs all lie inside both songs takes the plain path; any other
 * step tests each pair (0 <= i < Wa, 0 <= i + d < Wb), so the zeros never count.  n(d) is arithmetic.
 *
 * Untuned: a first form.  One workgroup per pair leaves a call with few pairs of long songs on few CUs; with
 * max_shift = 64 a workgroup keeps 231 of its 256 lanes busy, with 1024 it keeps 171 and its tiles are 64 words.
 */
#include <hip/hip_runtime.h>

#include "bl_fprint.h"

typedef unsigned long long fp_u64;

#define FP_FRAMES BL_AMD_FPRINT_FRAMES                       /* 16 */
#define FP_HALF (FP_FRAMES / 2)                              /* 8 */
#define FP_BLOCK BL_FPRINT_BLOCK_WORDS                       /* 256 */
#define FP_ROWS (FP_BLOCK + FP_FRAMES - 1)                   /* frames under a run of words: 271 */
#define FP_PITCH 13 /* uint64 per LDS row: 12 and one of padding, so that lanes one row apart are 26 banks apart */

static_assert(sizeof(bl_amd_frame_chroma) == 96, "a frame record is twelve uint64");
static_assert(FP_FRAMES == 16 && FP_BLOCK + FP_HALF <= 2 * FP_BLOCK, "k_fprint_words sums in two rounds at most");

__global__ __launch_bounds__(FP_BLOCK) void k_fprint_words(const bl_amd_frame_chroma *__restrict__ frames,
                                                           const bl_fprint_song *__restrict__ songs, int n_songs,
                                                           uint32_t *__restrict__ words) {
  /* this workgroup's song: the last record whose group_off <= g (a record without words shares its offset with the
   * next) */
  const long long g = blockIdx.x;
  int lo = 0, hi = n_songs;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (songs[mid].group_off <= g) lo = mid;
    else hi = mid;
  }
  const bl_fprint_song sg = songs[lo];
  const int t0 = (int)(g - sg.group_off) * FP_BLOCK;
  const int rows = min(FP_ROWS, sg.frames - t0); /* frames of this song under the run: never one of the next song */
  const int tid = threadIdx.x;

  __shared__ fp_u64 sh[FP_ROWS * FP_PITCH];
  const fp_u64 *src = reinterpret_cast<const fp_u64 *>(frames + sg.frame_off + t0);
  for (int e = tid; e < rows * 12; e += FP_BLOCK) sh[(e / 12) * FP_PITCH + e % 12] = src[e];
  __syncthreads();

  /* H_j = rows j .. j + 7, for every j that has them; lane tid owns j = tid and, the first 8 lanes, j = 256 + tid */
  fp_u64 h[2][12];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int j = tid + r * FP_BLOCK;
#pragma unroll
    for (int k = 0; k < 12; ++k) h[r][k] = 0ull;
    if (j + FP_HALF <= rows && (r == 0 || tid < FP_HALF))
      for (int f = 0; f < FP_HALF; ++f)
#pragma unroll
        for (int k = 0; k < 12; ++k) h[r][k] += sh[(j + f) * FP_PITCH + k];
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int j = tid + r * FP_BLOCK;
    if (j + FP_HALF <= rows && (r == 0 || tid < FP_HALF))
#pragma unroll
      for (int k = 0; k < 12; ++k) sh[j * FP_PITCH + k] = h[r][k];
  }
  __syncthreads();

  if (t0 + tid >= sg.words) return; /* word t needs rows tid .. tid + 15: H of tid and of tid + 8 exist */
  fp_u64 s1[12], s2[12], a[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    s1[k] = h[0][k];
    s2[k] = sh[(tid + FP_HALF) * FP_PITCH + k];
    a[k] = s1[k] + s2[k];
  }
  uint32_t w = 0u;
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    const int n = (k + 1) % 12;
    w |= (uint32_t)(s2[k] > s1[k]) << k;
    w |= (uint32_t)(a[k] > a[n]) << (12 + k);
    if (k < 8) w |= (uint32_t)(s1[k] + s2[n] > s2[k] + s1[n]) << (24 + k);
  }
  words[sg.word_off + t0 + tid] = w;
}

/* ========================================================================= */
/* match                                                                      */

#define FP_U BL_FPRINT_UNIT
#define FP_STRIP BL_FPRINT_STRIP_WORDS
#define FP_TILE_MAX (FP_STRIP * BL_FPRINT_STRIPS_MAX)     /* 2048 */
#define FP_WIN_MAX (FP_TILE_MAX + 64)                     /* 64 strips + 4 groups + 4 words at most, see below */
#define FP_NO_KEY 0xFFFFFFFFFFFFFFFFull

static_assert(FP_U == 4, "a step is a 4 x 4 block of word pairs read as 16-byte pieces");

/* strips * 64 + 4 * groups + 4 with strips = min(32, 256 / groups) is largest at groups = 8: 2 084 */
constexpr bool fp_win_fits() {
  for (int groups = 1; groups <= BL_FPRINT_LANES; ++groups) {
    int strips = BL_FPRINT_LANES / groups;
    if (strips > BL_FPRINT_STRIPS_MAX) strips = BL_FPRINT_STRIPS_MAX;
    if (strips * FP_STRIP + FP_U * groups + FP_U > FP_WIN_MAX) return false;
  }
  return true;
}
static_assert(fp_win_fits(), "the window of b under a tile fits its LDS array");

__device__ __forceinline__ int fp_overlap(int wa, int wb, int d) {
  const int n = min(wa, wb - d) - max(0, -d);
  return n > 0 ? n : 0;
}

struct fp_best {
  fp_u64 key;
  uint32_t e, n;
  int d;
};

__global__ __launch_bounds__(BL_FPRINT_LANES) void k_fprint_match(
    const uint32_t *__restrict__ words_a, const bl_fprint_seq *__restrict__ seq_a, int n_a,
    const uint32_t *__restrict__ words_b, const bl_fprint_seq *__restrict__ seq_b, int n_b,
    const int32_t *__restrict__ pairs, int D, int min_overlap, bl_fprint_geom geo, bl_amd_fprint_match *__restrict__ out,
    uint32_t *__restrict__ profile) {
  const long long p = blockIdx.x;
  const int tid = threadIdx.x;
  const int nd = 2 * D + 1;
  const int ia = pairs[2 * p], ib = pairs[2 * p + 1];
  bl_amd_fprint_match none;
  none.errors = none.overlap = 0u;
  none.offset = 0;
  none.score = 0xFFFFFFFFu;
  none.status = BL_UNEXPECTED;
  none.reserved = 0;
  if ((unsigned)ia >= (unsigned)n_a || (unsigned)ib >= (unsigned)n_b) { /* the whole workgroup leaves together */
    if (tid == 0) out[p] = none;
    if (profile)
      for (int t = tid; t < 2 * nd; t += BL_FPRINT_LANES) profile[p * 2 * nd + t] = 0u;
    return;
  }
  const bl_fprint_seq qa = seq_a[ia], qb = seq_b[ib];
  const int wa = qa.count, wb = qb.count;
  const uint32_t *__restrict__ pa = words_a + qa.off;
  const uint32_t *__restrict__ pb = words_b + qb.off;

  __shared__ uint4 sa4[FP_TILE_MAX / 4], sb4[FP_WIN_MAX / 4];
  __shared__ uint32_t se[FP_U * BL_FPRINT_LANES];
  __shared__ fp_u64 sk[BL_FPRINT_LANES / 64];
  uint32_t *sa = reinterpret_cast<uint32_t *>(sa4), *sb = reinterpret_cast<uint32_t *>(sb4);

  const int tile = geo.strips * FP_STRIP;
  const int win = tile + FP_U * geo.groups + FP_U;
  const int row = tid / geo.groups, col = tid - row * geo.groups; /* the lane's strip and its group in the chunk */
  const bool lane_on = row < geo.strips;

  fp_best best = {FP_NO_KEY, 0u, 0u, 0};
  for (int c = 0; c < geo.chunks; ++c) {
    const int d_chunk = -D + FP_U * geo.groups * c; /* the chunk's first offset */
    const int dl = d_chunk + FP_U * col;            /* this lane's first */
    uint32_t e[FP_U] = {0u, 0u, 0u, 0u};
    for (int i0 = 0; i0 < wa; i0 += tile) {
      __syncthreads(); /* the previous tile, or chunk, has been read */
      for (int j = tid; j < tile; j += BL_FPRINT_LANES) sa[j] = i0 + j < wa ? pa[i0 + j] : 0u;
      for (int j = tid; j < win; j += BL_FPRINT_LANES) {
        const int bi = i0 + d_chunk + j;
        sb[j] = bi >= 0 && bi < wb ? pb[bi] : 0u;
      }
      __syncthreads();
      if (lane_on && dl <= D) {
        const int is = row * FP_STRIP;            /* in the tile */
        const int bs = (is + FP_U * col) / FP_U;  /* b[i0 + is + dl] as a 16-byte piece of the window */
        uint4 blo = sb4[bs];
        for (int m = 0; m < FP_STRIP / FP_U; ++m) {
          const int i = i0 + is + FP_U * m;
          if (i >= wa) break;
          const uint4 bhi = sb4[bs + m + 1], a4 = sa4[is / FP_U + m];
          const uint32_t av[4] = {a4.x, a4.y, a4.z, a4.w};
          const uint32_t bv[7] = {blo.x, blo.y, blo.z, blo.w, bhi.x, bhi.y, bhi.z};
          if (i + 3 < wa && i + dl >= 0 && i + dl + 6 < wb) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
              for (int q = 0; q < 4; ++q) e[q] += __popc(av[r] ^ bv[r + q]);
          } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
              for (int q = 0; q < 4; ++q) {
                const int bi = i + r + dl + q;
                if (i + r < wa && bi >= 0 && bi < wb) e[q] += __popc(av[r] ^ bv[r + q]);
              }
          }
          blo = bhi;
        }
      }
    }
    /* the strips' shares of the chunk's offsets are joined in LDS; then lane t owns offset d_chunk + t */
    __syncthreads();
    for (int t = tid; t < FP_U * geo.groups; t += BL_FPRINT_LANES) se[t] = 0u;
    __syncthreads();
    if (lane_on && dl <= D)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (e[q]) atomicAdd(&se[FP_U * col + q], e[q]);
    __syncthreads();
    for (int t = tid; t < FP_U * geo.groups; t += BL_FPRINT_LANES) {
      const int d = d_chunk + t;
      if (d > D) continue;
      const uint32_t ed = se[t], n = (uint32_t)fp_overlap(wa, wb, d);
      if (profile) {
        profile[(p * nd + (d + D)) * 2] = ed;
        profile[(p * nd + (d + D)) * 2 + 1] = n;
      }
      if (n < (uint32_t)min_overlap) continue; /* min_overlap >= 1: an empty overlap is no candidate */
      const fp_u64 s = ((fp_u64)ed << 16) / n;
      const fp_u64 key = (s << 32) | (fp_u64)(uint32_t)(d < 0 ? -2 * d - 1 : 2 * d);
      if (key < best.key) best = {key, ed, n, d};
    }
  }

  /* the smallest key of the workgroup; keys of different offsets differ, so one lane at most holds it */
  fp_u64 k = best.key;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const fp_u64 o = __shfl_xor(k, off);
    k = o < k ? o : k;
  }
  if ((tid & 63) == 0) sk[tid >> 6] = k;
  __syncthreads();
  k = sk[0];
  for (int w = 1; w < BL_FPRINT_LANES / 64; ++w) k = sk[w] < k ? sk[w] : k;
  if (k == FP_NO_KEY) {
    if (tid == 0) out[p] = none;
  } else if (best.key == k) {
    bl_amd_fprint_match o;
    o.errors = best.e;
    o.overlap = best.n;
    o.offset = best.d;
    o.score = (uint32_t)(k >> 32);
    o.status = BL_OK;
    o.reserved = 0;
    out[p] = o;
  }
}

/* ========================================================================= */
/* launchers (declared in bl_fprint.h)                                        */

int blk_fprint_words(hipStream_t s, const bl_amd_frame_chroma *d_frames, const bl_fprint_song *d_songs, int n_songs,
                     long long n_groups, uint32_t *d_words, blk_mark_fn mark, void *mark_user) {
  if (n_groups < 1) return BL_OK;
  Mark m(mark, mark_user, FK_WORDS, s);
  hipLaunchKernelGGL(k_fprint_words, dim3((unsigned)n_groups), dim3(FP_BLOCK), 0, s, d_frames, d_songs, n_songs,
                     d_words);
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}

int blk_fprint_match(hipStream_t s, const uint32_t *d_words_a, const bl_fprint_seq *d_seq_a, int n_a,
                     const uint32_t *d_words_b, const bl_fprint_seq *d_seq_b, int n_b, const int32_t *d_pairs,
                     int n_pairs, int max_shift, int min_overlap, bl_amd_fprint_match *d_out, uint32_t *d_profile,
                     blk_mark_fn mark, void *mark_user) {
  Mark m(mark, mark_user, FK_MATCH, s);
  hipLaunchKernelGGL(k_fprint_match, dim3((unsigned)n_pairs), dim3(BL_FPRINT_LANES), 0, s, d_words_a, d_seq_a, n_a,
                     d_words_b, d_seq_b, n_b, d_pairs, max_shift, min_overlap, fprint_geom(max_shift), d_out,
                     d_profile);
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}
