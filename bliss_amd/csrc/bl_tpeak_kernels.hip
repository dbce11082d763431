/*
 * bl_tpeak_kernels.hip — gfx950 kernels and launch layer of the true peak (bl_amd_tpeak_batch_device; the definition
 * is the block in include/bliss_amd.h, the interpolator bl_tpeak_table.h).  Every quantity is an exact integer, so the
 * atomics that join the lanes of a song do not disturb determinism.
 *
 * Kernels:
 *   k_tpeak_scan    one workgroup per (song, group of 4 096 frames), one lane per run of 16 consecutive frames.  Per
 *                   frame and channel: the three interpolated points (phase 0 is the sample itself), their magnitudes,
 *                   the points above the ceiling, the largest magnitude with its first position, the sample peak and,
 *                   with a profile, the block maxima.
 *   k_tpeak_finish  one lane per song: unpacks the joined keys into the record; also writes the records of songs
 *                   without a frame.
 *
 * Layout of the arithmetic.  The sums are packed int16 dot products with an int32 accumulator (v_dot2c_i32_i16): a
 * 32-bit register holds two consecutive samples of ONE channel, the taps are wave-uniform packed pairs, and a point is
 * six of them: 18 per sample for the three phases.  |y| <= 30544 * 32768 < 2^30, so nothing saturates or wraps.
 *   mono    a word of the stream is already a pair (x[2i], x[2i+1]); the pairs that start at an odd frame are this
 *           word and the next one shifted by 16 bits (v_alignbit_b32), as in the level pass.
 *   stereo  a word is one frame of two channels; two neighbouring words are regrouped by halves (v_perm_b32) into one
 *           pair per channel.
 * A frame t reads the pairs that start at t-5, t-3, .. t+5, whatever its parity.
 *
 * What is read.  A lane owns frames [t0, t0 + 16) of its song, t0 a multiple of 16, and reads 8 frames in front of
 * them and 8 behind (the sums need 5 and 6) in aligned 16-byte pieces.  A piece in front of the song is not loaded: it
 * is zeros.  A piece is loaded whole only when it ends at or before the song's last sample that belongs to a frame;
 * the piece that straddles that end is read sample by sample up to it; pieces behind it are zeros.  So nothing outside
 * [pcm_off, pcm_off + F channels) is touched and zeros stand outside the song, as the definition says.  Every sample
 * is loaded twice (by its owner and as a neighbour's halo), the second time from a line the wave is loading anyway.
 *
 * The largest magnitude.  Inside a frame the four magnitudes are compared as 32-bit keys (|y| << 2) | (3 - phase), so
 * one maximum picks the largest with the smallest phase; a lane replaces its best frame only by a strictly larger
 * magnitude, so the first frame wins.  The lane's result becomes the 64-bit key (|y| << 33) | (2^33 - 1 - i), the
 * waves and then the workgroup reduce it by maximum and join the song with one atomicMax per workgroup and channel: the
 * order of the joins cannot matter.  The counts above the ceiling join by integer atomicAdd, the sample peak and the blocks that span lanes by
 * atomicMax; a block that lies inside one lane's run is stored.
 *
 * Untuned: the run length, the private halo loads and the per-frame bookkeeping are first choices.
 */
#include <hip/hip_runtime.h>

#include "bl_tpeak.h"
#include "bl_tpeak_table.h"

typedef unsigned long long tp_u64;
typedef short tp_s2 __attribute__((ext_vector_type(2)));

#define TP_L BL_TPEAK_LANE_FRAMES
#define TP_INDEX_BITS 33
#define TP_INDEX_MASK ((1ull << TP_INDEX_BITS) - 1ull)

static_assert(TP_L == 16, "the windows below are laid out for runs of 16 frames");

__device__ __forceinline__ tp_s2 tp_as_s2(unsigned w) { tp_s2 v; __builtin_memcpy(&v, &w, 4); return v; }
constexpr unsigned tp_pack(int lo, int hi) { return ((unsigned)lo & 0xFFFFu) | ((unsigned)hi << 16); }

/* the 16-byte piece at element `a` (a multiple of 8, may be negative) of a song of `ne` elements (see "What is read") */
__device__ __forceinline__ uint4 tp_piece(const int16_t *__restrict__ p, long long a, long long ne) {
  uint4 q = make_uint4(0u, 0u, 0u, 0u);
  if (a >= 0 && a + 8 <= ne) {
    q = *reinterpret_cast<const uint4 *>(p + a);
  } else if (a >= 0 && a < ne) {
    unsigned w[4] = {0u, 0u, 0u, 0u};
    for (int k = 0; k < 8; ++k)
      if (a + k < ne) w[k >> 1] |= (unsigned)(unsigned short)p[a + k] << (16 * (k & 1));
    q = make_uint4(w[0], w[1], w[2], w[3]);
  }
  return q;
}

/* per-channel state of one lane */
struct tp_ch {
  unsigned best; /* (|y| << 2) | (3 - phase) of the best point so far */
  int best_i;    /* its frame, relative to the lane's first */
  unsigned overs, peak;
};

/* One frame of one channel.  pr[k] = (x[t-5+2k], x[t-4+2k]), k = 0..5; i: the frame's position in the lane's run;
 * thr = ceiling << 14.  Returns the frame's largest magnitude. */
__device__ __forceinline__ unsigned tp_frame(tp_ch &c, const unsigned (&pr)[6], int i, unsigned thr) {
  constexpr int G[BL_TPEAK_PHASES][BL_TPEAK_TAPS] = {BL_TPEAK_G_ROWS};
  unsigned a[4];
  const int x = (int)pr[2] >> 16; /* x[t], the high half of (x[t-1], x[t]): phase 0 is x << 14 */
  const unsigned ax = (unsigned)(x < 0 ? -x : x);
  a[0] = ax << 14;
#pragma unroll
  for (int ph = 1; ph < 4; ++ph) {
    int y = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k)
      y = __builtin_amdgcn_sdot2(tp_as_s2(pr[k]), tp_as_s2(tp_pack(G[ph][2 * k], G[ph][2 * k + 1])), y, false);
    a[ph] = (unsigned)(y < 0 ? -y : y);
  }
  c.peak = max(c.peak, ax);
  c.overs += (unsigned)(a[0] > thr) + (unsigned)(a[1] > thr) + (unsigned)(a[2] > thr) + (unsigned)(a[3] > thr);
  const unsigned key = max(max((a[0] << 2) | 3u, (a[1] << 2) | 2u), max((a[2] << 2) | 1u, a[3] << 2));
  if (key > (c.best | 3u)) { /* a strictly larger magnitude: the first frame keeps an equal one */
    c.best = key;
    c.best_i = i;
  }
  return key >> 2;
}

/* the block bookkeeping of one lane (only with a profile) */
struct tp_blk {
  uint32_t *out;      /* the song's first block, nullptr without a profile */
  unsigned bi;        /* the block the next frame belongs to */
  int left;           /* frames until that block ends */
  int block;
  bool started_in;    /* that block began inside this lane's run */
  bool pend;          /* m holds frames that have not been written */
  unsigned m[2];
};

template <bool MONO>
__device__ __forceinline__ void tp_blk_frame(tp_blk &b, unsigned f0, unsigned f1) {
  b.m[0] = max(b.m[0], f0);
  b.m[1] = max(b.m[1], f1);
  b.pend = true;
  if (--b.left == 0) { /* the block ends with this frame */
    uint32_t *o = b.out + 2ull * b.bi;
    if (b.started_in) {
      o[0] = b.m[0];
      if (!MONO) o[1] = b.m[1];
    } else {
      atomicMax(&o[0], b.m[0]);
      if (!MONO) atomicMax(&o[1], b.m[1]);
    }
    b.bi += 1u;
    b.left = b.block;
    b.started_in = true;
    b.pend = false;
    b.m[0] = b.m[1] = 0u;
  }
}

/* the lane's run [t0, t0 + nf) of a song of F frames at p; nf in 1..16 */
template <bool MONO>
__device__ __forceinline__ void tp_run(const int16_t *__restrict__ p, long long F, long long t0, int nf, unsigned thr,
                                       tp_ch &c0, tp_ch &c1, tp_blk &b) {
  if (MONO) {
    /* word w holds frames t0 - 8 + 2w and the next one */
    unsigned xw[16], od[15];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint4 q = tp_piece(p, t0 - 8 + 8 * k, F);
      xw[4 * k] = q.x; xw[4 * k + 1] = q.y; xw[4 * k + 2] = q.z; xw[4 * k + 3] = q.w;
    }
#pragma unroll
    for (int w = 0; w < 15; ++w) od[w] = __builtin_amdgcn_alignbit(xw[w + 1], xw[w], 16);
#pragma unroll
    for (int i = 0; i < TP_L; ++i) {
      if (i < nf) {
        const int r = i + 3; /* the first pair starts at frame t - 5 = (t0 - 8) + r */
        unsigned pr[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) pr[k] = (r & 1) ? od[(r - 1) / 2 + k] : xw[r / 2 + k];
        const unsigned f0 = tp_frame(c0, pr, i, thr);
        if (b.out) tp_blk_frame<true>(b, f0, 0u);
      }
    }
  } else {
    /* word w holds frame t0 - 8 + w; pa / pb [v]: the pair of channel 0 / 1 that starts at frame t0 - 5 + v */
    unsigned xw[32], pa[26], pb[26];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const uint4 q = tp_piece(p, 2 * (t0 - 8) + 8 * k, 2 * F);
      xw[4 * k] = q.x; xw[4 * k + 1] = q.y; xw[4 * k + 2] = q.z; xw[4 * k + 3] = q.w;
    }
#pragma unroll
    for (int v = 0; v < 26; ++v) {
      pa[v] = __builtin_amdgcn_perm(xw[v + 4], xw[v + 3], 0x05040100u);
      pb[v] = __builtin_amdgcn_perm(xw[v + 4], xw[v + 3], 0x07060302u);
    }
#pragma unroll
    for (int i = 0; i < TP_L; ++i) {
      if (i < nf) {
        unsigned p0[6], p1[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          p0[k] = pa[i + 2 * k];
          p1[k] = pb[i + 2 * k];
        }
        const unsigned f0 = tp_frame(c0, p0, i, thr);
        const unsigned f1 = tp_frame(c1, p1, i, thr);
        if (b.out) tp_blk_frame<false>(b, f0, f1);
      }
    }
  }
}

__device__ __forceinline__ tp_u64 tp_key(const tp_ch &c, long long t0) {
  const long long i = 4 * (t0 + c.best_i) + (3 - (int)(c.best & 3u));
  return ((tp_u64)(c.best >> 2) << TP_INDEX_BITS) | (TP_INDEX_MASK - (tp_u64)i);
}

__global__ __launch_bounds__(BL_TPEAK_GROUP_LANES) void k_tpeak_scan(const int16_t *__restrict__ pcm,
                                                                     const bl_tpeak_song *__restrict__ songs,
                                                                     int n_songs, unsigned thr, int block,
                                                                     bl_tpeak_acc *acc, uint32_t *blocks) {
  /* this workgroup's song: the last record whose group_off <= g (a record without groups shares its offset with the
   * next) */
  const long long g = blockIdx.x;
  int lo = 0, hi = n_songs; /* songs[lo].group_off <= g < songs[hi].group_off, with songs[n_songs] = infinity */
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (songs[mid].group_off <= g) lo = mid;
    else hi = mid;
  }
  const bl_tpeak_song sg = songs[lo];
  const int16_t *p = pcm + sg.pcm_off;
  const long long F = sg.frames;
  const bool mono = sg.channels == 1;
  const long long t0 = (g - sg.group_off) * BL_TPEAK_GROUP_FRAMES + (long long)threadIdx.x * TP_L;
  const int nf = F - t0 >= TP_L ? TP_L : (F > t0 ? (int)(F - t0) : 0);

  tp_ch c0 = {3u, 0, 0u, 0u}, c1 = c0; /* magnitude 0 at phase 0 of the run's first frame */
  tp_blk b;
  b.out = blocks ? blocks + 2 * sg.blk_off : nullptr;
  b.block = block;
  b.bi = 0u;
  b.left = 0;
  b.started_in = false;
  b.pend = false;
  b.m[0] = b.m[1] = 0u;
  if (blocks && nf > 0) {
    const unsigned ut0 = (unsigned)t0, rem = ut0 % (unsigned)block; /* t0 < F + 4096 < 2^32 */
    b.bi = ut0 / (unsigned)block;
    b.left = block - (int)rem;
    b.started_in = rem == 0u;
  }
  if (nf > 0) {
    if (mono) tp_run<true>(p, F, t0, nf, thr, c0, c1, b);
    else tp_run<false>(p, F, t0, nf, thr, c0, c1, b);
  }

  /* the block a lane's run ends in and does not finish: when all of a wave's open blocks are one block, the wave
   * reduces them and joins once */
  if (blocks) {
    const bool has = b.pend;
    const tp_u64 mask = __ballot(has);
    if (mask) {
      const unsigned bi_s = __shfl(b.bi, (int)__builtin_ctzll(mask));
      unsigned m0 = has ? b.m[0] : 0u, m1 = has ? b.m[1] : 0u;
      if (__all(!has || b.bi == bi_s)) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          m0 = max(m0, __shfl_down(m0, off));
          m1 = max(m1, __shfl_down(m1, off));
        }
        if ((threadIdx.x & 63) == 0) {
          uint32_t *o = b.out + 2ull * bi_s;
          atomicMax(&o[0], m0);
          if (!mono) atomicMax(&o[1], m1);
        }
      } else if (has) {
        uint32_t *o = b.out + 2ull * b.bi;
        atomicMax(&o[0], m0);
        if (!mono) atomicMax(&o[1], m1);
      }
    }
  }

  /* the song's records: wave reduction, then one integer atomic per workgroup and field that has something to say */
  tp_u64 k0 = nf > 0 ? tp_key(c0, t0) : 0ull, k1 = nf > 0 && !mono ? tp_key(c1, t0) : 0ull;
  tp_u64 ov0 = c0.overs, ov1 = c1.overs;
  int pk0 = (int)c0.peak, pk1 = (int)c1.peak;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const tp_u64 o0 = __shfl_down(k0, off), o1 = __shfl_down(k1, off);
    k0 = o0 > k0 ? o0 : k0;
    k1 = o1 > k1 ? o1 : k1;
    ov0 += __shfl_down(ov0, off);
    ov1 += __shfl_down(ov1, off);
    pk0 = max(pk0, __shfl_down(pk0, off));
    pk1 = max(pk1, __shfl_down(pk1, off));
  }
  /* the four waves through LDS, so that a workgroup joins once: the workgroups in flight mostly belong to one song, and
   * at a song's start every one of them has something to say to the same line */
  __shared__ tp_u64 sh_k[2][BL_TPEAK_GROUP_LANES / 64], sh_ov[2][BL_TPEAK_GROUP_LANES / 64];
  __shared__ int sh_pk[2][BL_TPEAK_GROUP_LANES / 64];
  if ((threadIdx.x & 63) == 0) {
    const int w = threadIdx.x >> 6;
    sh_k[0][w] = k0; sh_k[1][w] = k1;
    sh_ov[0][w] = ov0; sh_ov[1][w] = ov1;
    sh_pk[0][w] = pk0; sh_pk[1][w] = pk1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < BL_TPEAK_GROUP_LANES / 64; ++w) {
      k0 = sh_k[0][w] > k0 ? sh_k[0][w] : k0;
      k1 = sh_k[1][w] > k1 ? sh_k[1][w] : k1;
      ov0 += sh_ov[0][w];
      ov1 += sh_ov[1][w];
      pk0 = max(pk0, sh_pk[0][w]);
      pk1 = max(pk1, sh_pk[1][w]);
    }
    bl_tpeak_acc *a = acc + lo;
    /* the joined values only grow, so a value that is not above what is there already cannot change it */
    if (k0 > __hip_atomic_load(&a->key[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&a->key[0], k0);
    if (k1 > __hip_atomic_load(&a->key[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&a->key[1], k1);
    if (ov0) atomicAdd(&a->overs[0], ov0);
    if (ov1) atomicAdd(&a->overs[1], ov1);
    if (pk0 > __hip_atomic_load(&a->peak[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&a->peak[0], pk0);
    if (pk1 > __hip_atomic_load(&a->peak[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&a->peak[1], pk1);
  }
}

__global__ __launch_bounds__(256) void k_tpeak_finish(const bl_tpeak_song *__restrict__ songs, int n_songs,
                                                      const bl_tpeak_acc *__restrict__ acc,
                                                      bl_amd_song_tpeak *__restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_songs) return;
  const bl_tpeak_song sg = songs[i];
  const bl_tpeak_acc a = acc[i];
  bl_amd_song_tpeak o;
  for (int c = 0; c < 2; ++c) {
    const bool live = sg.frames > 0 && c < sg.channels;
    o.at[c] = live ? (int64_t)(TP_INDEX_MASK - (a.key[c] & TP_INDEX_MASK)) : -1;
    o.overs[c] = live ? (int64_t)a.overs[c] : 0;
    o.tpeak[c] = live ? (uint32_t)(a.key[c] >> TP_INDEX_BITS) : 0u;
    o.peak[c] = live ? a.peak[c] : 0;
  }
  o.frames = sg.frames;
  o.status = BL_OK;
  out[i] = o;
}

/* ========================================================================= */
/* launcher (declared in bl_tpeak.h)                                          */

int blk_tpeak(hipStream_t s, const int16_t *d_pcm, const bl_tpeak_song *d_songs, int n_songs, long long n_groups,
              int ceiling, int block, bl_tpeak_acc *d_acc, bl_amd_song_tpeak *d_songs_out, uint32_t *d_blocks,
              long long n_blocks, blk_mark_fn mark, void *mark_user) {
  BL_HIP_CHECK(hipMemsetAsync(d_acc, 0, sizeof(bl_tpeak_acc) * (size_t)n_songs, s));
  if (d_blocks && n_blocks > 0) BL_HIP_CHECK(hipMemsetAsync(d_blocks, 0, 8 * (size_t)n_blocks, s));
  if (n_groups > 0) {
    Mark m(mark, mark_user, TK_SCAN, s);
    hipLaunchKernelGGL(k_tpeak_scan, dim3((unsigned)n_groups), dim3(BL_TPEAK_GROUP_LANES), 0, s, d_pcm, d_songs,
                       n_songs, (unsigned)ceiling << 14, block, d_acc, d_blocks);
    BL_HIP_CHECK(hipGetLastError());
  }
  Mark m(mark, mark_user, TK_FINISH, s);
  hipLaunchKernelGGL(k_tpeak_finish, dim3((unsigned)((n_songs + 255) / 256)), dim3(256), 0, s, d_songs, n_songs, d_acc,
                     d_songs_out);
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}
