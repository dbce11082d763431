/*
 * bl_loud_kernels.hip — gfx950 kernels and launch layer of the K-weighted gated loudness (bl_amd_loud_batch_device,
 * bl_amd_loud_from_hops; the definition is the numbered block in include/bliss_amd.h).
 *
 * Kernels:
 *   k_loud_filter  stages 1 to 3: one lane per (song, chunk of 16 hops).  The K-weighting is a recursive filter; the
 *                  definition cuts it into chunks that start from zero state `warm` frames early, so a chunk is a pure
 *                  function of its own frames and the lanes are independent.  A stereo lane runs both channels: they
 *                  are the same bytes, and the two independent recurrences give the f64 chain its instruction-level
 *                  parallelism.  The arithmetic is plain C++ in the header's order; the Makefile's -ffp-contract=off
 *                  keeps it unfused, and f64 denormals are on by default on this target.
 *   k_loud_gate    stages 4 to 6: one workgroup per song over its hop energies Z: block sums, the two gates with
 *                  128-bit sums in two limbs, short-term sums, and the two percentiles of the range by an MSB-first
 *                  radix select (one count per bit, no sort).
 *
 * Staging.  The lanes of a wave stream from addresses hundreds of KB apart, and a lane-private 16-byte load would use an
 * eighth of every line it touches.  So a wave (one workgroup = one wave) moves 128 bytes per lane and round through
 * LDS: eight lanes load the eight 16-byte pieces of one lane's row side by side, each lane then reads its own row.
 * The row of the next round is loaded into registers before the current one is consumed.
 *
 * What is read.  A lane's stream is [start, end) in int16 elements of the arena, start = pcm_off + f_start * channels,
 * end = pcm_off + 16 (k + 1) hop * channels clipped to H hop * channels.  Rows are cut at multiples of 8 elements, so
 * the first row begins up to 7 elements in front of start: still inside the song, because pcm_off is a multiple of 8
 * and start >= pcm_off.  A 16-byte piece is loaded whole only when it ends at or before `end`; the piece that straddles
 * `end` is read element by element up to `end`; pieces behind it are not read.  Nothing outside
 * [pcm_off, pcm_off + H hop channels) is touched.
 *
 * Untuned: the row size, one wave per workgroup and the lane-per-chunk shape are first choices; a batch with fewer
 * chunks than the chip has lanes (1 024 songs of 30 s) leaves most of it idle.
 */
#include <hip/hip_runtime.h>

#include "bl_loud.h"

typedef unsigned long long lk_u64;

#define LK_ROW_ELEMS 64                    /* int16 elements a lane consumes per round: 128 bytes */
#define LK_ROW_PITCH (LK_ROW_ELEMS + 8)    /* the row's pitch in LDS, 144 bytes: rows start 36 banks apart */

struct lk_state { double x1, x2, v1, v2, y1, y2; };

/* one frame of one channel: stage 2 of the header, in its order */
__device__ __forceinline__ double lk_step(const bl_amd_loud_params &p, lk_state &s, double x) {
  const double v = ((((p.s1_b[0] * x + p.s1_b[1] * s.x1) + p.s1_b[2] * s.x2) - p.s1_a[1] * s.v2) - p.s1_a[0] * s.v1);
  const double y = ((((v - (s.v1 + s.v1)) + s.v2) - p.s2_a[1] * s.y2) - p.s2_a[0] * s.y1);
  s.x2 = s.x1; s.x1 = x;
  s.v2 = s.v1; s.v1 = v;
  s.y2 = s.y1; s.y1 = y;
  return y;
}

/* the 16-byte piece at element `a` of a stream that ends at element `end` (see "What is read") */
__device__ __forceinline__ uint4 lk_piece(const int16_t *__restrict__ pcm, long long a, long long end) {
  uint4 q = make_uint4(0u, 0u, 0u, 0u);
  if (a + 8 <= end) {
    q = *reinterpret_cast<const uint4 *>(pcm + a);
  } else if (a < end) {
    unsigned w[4] = {0u, 0u, 0u, 0u};
    for (int k = 0; k < 8; ++k)
      if (a + k < end) w[k >> 1] |= (unsigned)(unsigned short)pcm[a + k] << (16 * (k & 1));
    q = make_uint4(w[0], w[1], w[2], w[3]);
  }
  return q;
}

/* the next row of all 64 lanes: piece (lane & 7) of the rows of lanes 8 i + (lane >> 3) */
__device__ __forceinline__ void lk_fetch(const int16_t *__restrict__ pcm, long long cur, long long end, int lane,
                                         uint4 (&nxt)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int t = 8 * i + (lane >> 3);
    const long long ct = __shfl(cur, t), et = __shfl(end, t);
    nxt[i] = lk_piece(pcm, ct + 8 * (lane & 7), et);
  }
}

__global__ __launch_bounds__(64) void k_loud_filter(const int16_t *__restrict__ pcm,
                                                    const bl_loud_song *__restrict__ songs, int n_songs,
                                                    long long n_chunks, const bl_amd_loud_params p,
                                                    lk_u64 *__restrict__ z) {
  __shared__ __attribute__((aligned(16))) int16_t rows[64 * LK_ROW_PITCH];
  const int lane = threadIdx.x;
  const long long g = (long long)blockIdx.x * 64 + lane;

  /* this lane's chunk: the last record whose chunk_off <= g (a record without chunks shares its offset with the next) */
  long long cur = 0, end = 0, z_at = 0;
  int ch = 2, skip = 0, warm_left = 0;
  if (g < n_chunks) {
    int lo = 0, hi = n_songs; /* songs[lo].chunk_off <= g < songs[hi].chunk_off, with songs[n_songs] = infinity */
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (songs[mid].chunk_off <= g) lo = mid;
      else hi = mid;
    }
    const bl_loud_song sg = songs[lo];
    const long long k = g - sg.chunk_off;
    const long long h0 = BL_AMD_LOUD_CHUNK * k;
    const long long h1 = h0 + BL_AMD_LOUD_CHUNK < sg.hops ? h0 + BL_AMD_LOUD_CHUNK : sg.hops;
    const long long f_first = h0 * p.hop, f_start = f_first > p.warm ? f_first - p.warm : 0;
    ch = sg.channels;
    warm_left = (int)(f_first - f_start);
    cur = (long long)sg.pcm_off + f_start * ch;
    end = (long long)sg.pcm_off + h1 * p.hop * ch;
    skip = (int)(cur & 7);
    cur -= skip;
    z_at = 2 * (sg.hop_off + h0);
  }

  lk_state s0 = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, s1 = s0;
  double e0 = 0.0, e1 = 0.0;
  int in_hop = 0;
  uint4 nxt[8];
  lk_fetch(pcm, cur, end, lane, nxt);
  while (__any(cur < end)) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
      *reinterpret_cast<uint4 *>(&rows[(8 * i + (lane >> 3)) * LK_ROW_PITCH + 8 * (lane & 7)]) = nxt[i];
    __syncthreads();
    const long long left = end - cur; /* elements of this row and behind it */
    const int avail = left < LK_ROW_ELEMS ? (left > 0 ? (int)left : 0) : LK_ROW_ELEMS;
    cur += LK_ROW_ELEMS;
    lk_fetch(pcm, cur, end, lane, nxt);
    const int16_t *row = &rows[lane * LK_ROW_PITCH];
    int pos = skip;
    skip = 0;
    /* a frame never straddles rows: pcm_off is a multiple of 8 and a stereo frame starts at an even element */
    while (__any(pos < avail)) {
      if (pos < avail) {
        const double y0 = lk_step(p, s0, (double)row[pos]);
        double y1 = 0.0;
        if (ch == 2) y1 = lk_step(p, s1, (double)row[pos + 1]);
        pos += ch;
        if (warm_left > 0) {
          --warm_left;
        } else {
          e0 = e0 + y0 * y0;
          e1 = e1 + y1 * y1;
          if (++in_hop == p.hop) {
            z[z_at] = (lk_u64)e0;
            z[z_at + 1] = (lk_u64)e1;
            z_at += 2;
            e0 = e1 = 0.0;
            in_hop = 0;
          }
        }
      }
    }
    __syncthreads();
  }
}

/* ---- stages 4 to 6 ------------------------------------------------------------------ */

struct lk_u128 { lk_u64 lo, hi; };
__device__ __forceinline__ lk_u128 lk_add(lk_u128 a, lk_u128 b) {
  lk_u128 r;
  r.lo = a.lo + b.lo;
  r.hi = a.hi + b.hi + (r.lo < a.lo ? 1ull : 0ull); /* the carry of the low limb */
  return r;
}
__device__ __forceinline__ lk_u128 lk_mul(lk_u64 a, lk_u64 b) {
  lk_u128 r;
  r.lo = a * b;
  r.hi = __umul64hi(a, b);
  return r;
}
__device__ __forceinline__ bool lk_gt(lk_u128 a, lk_u128 b) { return a.hi != b.hi ? a.hi > b.hi : a.lo > b.lo; }

/* the sum over both channels and `len` hops from hop j */
__device__ __forceinline__ lk_u64 lk_window(const lk_u64 *__restrict__ z, long long j, int len) {
  lk_u64 sum = 0;
  for (int k = 0; k < 2 * len; ++k) sum += z[2 * j + k];
  return sum;
}

struct lk_part { lk_u128 sum; lk_u64 mx; unsigned n; };

/* the workgroup's total of `mine` in every thread */
__device__ lk_part lk_reduce(lk_part mine, lk_part *sh) {
  const int tid = threadIdx.x;
  sh[tid] = mine;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) {
      const lk_part a = sh[tid], b = sh[tid + w];
      lk_part r;
      r.sum = lk_add(a.sum, b.sum);
      r.mx = a.mx > b.mx ? a.mx : b.mx;
      r.n = a.n + b.n;
      sh[tid] = r;
    }
    __syncthreads();
  }
  const lk_part r = sh[0];
  __syncthreads();
  return r;
}

#define LK_NONE (~0ull) /* a short-term start that a gate has removed: ST < 2^54, so no sum is this value */

__global__ __launch_bounds__(256) void k_loud_gate(const lk_u64 *__restrict__ z_all,
                                                   const bl_loud_song *__restrict__ songs, lk_u64 abs_gate,
                                                   lk_u64 *__restrict__ st_all, bl_amd_song_loud *__restrict__ out) {
  __shared__ lk_part sh[256];
  __shared__ unsigned cnt[64][2];
  const bl_loud_song sg = songs[blockIdx.x];
  const int tid = threadIdx.x;
  const lk_u64 *z = z_all + 2 * sg.hop_off;
  lk_u64 *st = st_all + sg.st_off;
  const long long H = sg.hops, nb = H >= 4 ? H - 3 : 0, ns = H >= 30 ? H - 29 : 0, nst = blk_loud_starts(H);
  const lk_part none = {{0ull, 0ull}, 0ull, 0u};
  if (tid < 128) cnt[tid >> 1][tid & 1] = 0u;

  /* absolute gate */
  lk_part a = none;
  for (long long j = tid; j < nb; j += 256) {
    const lk_u64 P = lk_window(z, j, 4);
    a.mx = P > a.mx ? P : a.mx;
    if (P > abs_gate) {
      a.n += 1u;
      a.sum = lk_add(a.sum, lk_u128{P, 0ull});
    }
  }
  const lk_part abs_ = lk_reduce(a, sh);
  /* relative gate, -10 LU: P 10 N1 > S1 */
  lk_part g = none;
  for (long long j = tid; j < nb; j += 256) {
    const lk_u64 P = lk_window(z, j, 4);
    if (P > abs_gate && lk_gt(lk_mul(P * 10ull, abs_.n), abs_.sum)) {
      g.n += 1u;
      g.sum = lk_add(g.sum, lk_u128{P, 0ull});
    }
  }
  const lk_part gated = lk_reduce(g, sh);
  /* short-term sums: the maximum over every start, the absolute gate over the starts 0, 10, 20, ... */
  lk_part t = none;
  for (long long j = tid; j < ns; j += 256) {
    const lk_u64 ST = lk_window(z, j, 30);
    t.mx = ST > t.mx ? ST : t.mx;
    if (j % 10 == 0) {
      const bool in = 2ull * ST > 15ull * abs_gate;
      st[j / 10] = in ? ST : LK_NONE;
      if (in) {
        t.n += 1u;
        t.sum = lk_add(t.sum, lk_u128{ST, 0ull});
      }
    }
  }
  const lk_part st_abs = lk_reduce(t, sh); /* its barriers also order the writes to st before the reads below */
  /* relative gate, -20 LU: ST 100 N > S */
  lk_part r = none;
  for (long long i = tid; i < nst; i += 256) {
    const lk_u64 v = st[i];
    if (v == LK_NONE) continue;
    if (lk_gt(lk_mul(v * 100ull, st_abs.n), st_abs.sum)) r.n += 1u;
    else st[i] = LK_NONE;
  }
  const long long M = lk_reduce(r, sh).n;
  /* the values of rank r_lo and r_hi among the survivors, bit by bit from the top */
  lk_u64 v_lo = 0, v_hi = 0;
  if (M > 0) {
    long long r_lo = (10 * (M - 1) + 50) / 100, r_hi = (95 * (M - 1) + 50) / 100;
    for (int b = 63; b >= 0; --b) {
      unsigned c_lo = 0, c_hi = 0; /* survivors that agree with the prefix above bit b and have bit b clear */
      for (long long i = tid; i < nst; i += 256) {
        const lk_u64 v = st[i];
        if (v == LK_NONE || ((v >> b) & 1ull)) continue;
        const lk_u64 top = ~((2ull << b) - 1ull); /* the bits above b; 2 << 63 wraps to 0: no bits */
        c_lo += ((v ^ v_lo) & top) == 0ull;
        c_hi += ((v ^ v_hi) & top) == 0ull;
      }
      if (c_lo) atomicAdd(&cnt[b][0], c_lo);
      if (c_hi) atomicAdd(&cnt[b][1], c_hi);
      __syncthreads();
      const long long n_lo = cnt[b][0], n_hi = cnt[b][1];
      if (r_lo >= n_lo) { r_lo -= n_lo; v_lo |= 1ull << b; }
      if (r_hi >= n_hi) { r_hi -= n_hi; v_hi |= 1ull << b; }
    }
  }
  if (tid == 0) {
    bl_amd_song_loud o;
    o.gated_sum[0] = gated.sum.lo; o.gated_sum[1] = gated.sum.hi;
    o.abs_sum[0] = abs_.sum.lo; o.abs_sum[1] = abs_.sum.hi;
    o.momentary_max = abs_.mx;
    o.st_max = st_abs.mx;
    o.lra_lo = v_lo;
    o.lra_hi = v_hi;
    o.gated_count = (int32_t)gated.n;
    o.abs_count = (int32_t)abs_.n;
    o.st_gated = (int32_t)M;
    o.hops = (int32_t)H;
    o.blocks = (int32_t)nb;
    o.status = BL_OK;
    out[sg.out_idx] = o;
  }
}

/* ========================================================================= */
/* launchers (declared in bl_loud.h)                                          */

int blk_loud_filter(hipStream_t s, const int16_t *d_pcm, const bl_loud_song *d_songs, int n_songs, long long n_chunks,
                    const bl_amd_loud_params &p, unsigned long long *d_z, blk_mark_fn mark, void *mark_user) {
  if (n_chunks < 1) return BL_OK;
  Mark m(mark, mark_user, LK_FILTER, s);
  hipLaunchKernelGGL(k_loud_filter, dim3((unsigned)((n_chunks + 63) / 64)), dim3(64), 0, s, d_pcm, d_songs, n_songs,
                     n_chunks, p, d_z);
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}

int blk_loud_gate(hipStream_t s, const unsigned long long *d_z, const bl_loud_song *d_songs, int n_songs,
                  unsigned long long abs_gate, unsigned long long *d_st, bl_amd_song_loud *d_songs_out,
                  blk_mark_fn mark, void *mark_user) {
  Mark m(mark, mark_user, LK_GATE, s);
  hipLaunchKernelGGL(k_loud_gate, dim3((unsigned)n_songs), dim3(256), 0, s, d_z, d_songs, abs_gate, d_st, d_songs_out);
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}
