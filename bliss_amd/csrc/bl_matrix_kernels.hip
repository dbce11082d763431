/*
 * bl_matrix_kernels.hip — gfx950 kernels and launch layer of what works on whole arrays of force vectors without
 * being a query: the N x N distance / cosine matrix, the seeded playlist, moving vectors in and out of result
 * records, and the exhaustive self-tests of the arithmetic the matrix rests on.  The per-pair arithmetic is
 * bl_metric.h, shared with the vector queries (bl_query_kernels.hip).  Must be compiled with -ffp-contract=off.
 *
 * Kernels (reference code each one replaces):
 *   k_pairwise     bl_distance / bl_cosine_similarity matrix
 *                                               ref src/analyze.c:96-100,135-140
 *   k_seed_dist, k_seed_dist_vec, k_rank_order  seeded playlist  ref python/examples/make_m3u_playlist.py:62-72
 *   k_scatter_vecs, k_extract_vecs  force vectors between result records, shard order and caller order
 *   k_sqrt_sweep, k_cos_sweep  self-tests of bl_sqrt.h and bl_cos.h on the device
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>

#include "bl_launch.h"
#include "bl_metric.h"

/* ------------------------------------------------------------------------- */
/* k_pairwise (bl_dist_sq, bl_dist, bl_dot: bl_metric.h)                        */

/* A workgroup owns BL_PW_ROWS rows x 1024 columns: every thread keeps its four column
 * vectors in registers and walks down the rows (the row vector is wave-uniform: scalar
 * loads), so a vector is fetched once per 16 outputs instead of once per output and the
 * index arithmetic is paid once.  Output: 16-byte stores, each row segment contiguous. */
#define BL_PW_ROWS 16
#ifndef BL_SQRT_VARIANT
#define BL_SQRT_VARIANT 1
#endif
/* SQ: 0 = the compiler's correctly rounded sqrtf everywhere, 1 / 2 = bl_sqrt_rn_fast<SQ> in its domain */
template <bool COSINE, int SQ = BL_SQRT_VARIANT>
__global__ __launch_bounds__(256) void k_pairwise(const float4 *__restrict__ vecs, int n,
                                                  int row_begin, int n_rows,
                                                  float *__restrict__ out) {
  const int j0 = (blockIdx.x * 256 + threadIdx.x) * 4;
  const int r0 = blockIdx.y * BL_PW_ROWS;
  const int r1 = min(r0 + BL_PW_ROWS, n_rows);
  /* cosine: what depends on one vector only — squared norm, its double root, the root's reciprocal (bl_cos.h) —
   * once per row of the workgroup (LDS) and once per column of the thread, not once per output */
  __shared__ double row_s[COSINE ? BL_PW_ROWS : 1], row_r[COSINE ? BL_PW_ROWS : 1];
  if (COSINE) {
    if ((int)threadIdx.x < r1 - r0) {
      const bl_cos_vec p = bl_cos_prep(vecs[row_begin + r0 + threadIdx.x]);
      row_s[threadIdx.x] = p.s;
      row_r[threadIdx.x] = p.r;
    }
    __syncthreads();
  }
  if (j0 >= n) return;
  float4 b[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) b[k] = vecs[min(j0 + k, n - 1)];
  bl_cos_vec cb[COSINE ? 4 : 1];
  if (COSINE) {
#pragma unroll
    for (int k = 0; k < 4; ++k) cb[k] = bl_cos_prep(b[k]);
  }
  const bool vec_ok = j0 + 4 <= n && (n & 3) == 0 && ((reinterpret_cast<size_t>(out) & 15) == 0);
  for (int row = r0; row < r1; ++row) {
    const float4 a = vecs[row_begin + row];
    float *orow = out + (size_t)row * n;
    float r[4];
    if (SQ == 3) { /* measurement builds only (BL_AMD_MEASURE): the store stream alone, no arithmetic */
#pragma unroll
      for (int k = 0; k < 4; ++k) r[k] = a.x;
    } else if (COSINE) {
      /* q' = dot * (ra * rb) where its float is provably the reference's (bl_cos.h); a wave with any output
       * near a float rounding boundary, a zero dot product or a degenerate norm takes the plain expression */
      const double ra = row_r[row - r0];
      float dot[4];
      bool fast = true;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        dot[k] = bl_dot(a, b[k]);
        fast = bl_cos_fast(dot[k], ra * cb[k].r, r[k]) && fast;
      }
      if (!__all(fast)) {
        bl_cos_vec ca;
        ca.s = row_s[row - r0];
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = bl_cos_plain(dot[k], ca, cb[k]);
      }
    } else {
      /* the five-instruction root where every sum of the wave is in its domain (bl_sqrt.h), the
       * compiler's sqrtf otherwise: a zero (the diagonal, duplicate songs), a tiny or a non-finite
       * sum — about one wave-row in forty at N = 10 000.  Both are the correctly rounded root. */
      float q[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) q[k] = bl_dist_sq(a, b[k]);
      const unsigned worst = max(max(bl_sqrt_fast_key(q[0]), bl_sqrt_fast_key(q[1])),
                                 max(bl_sqrt_fast_key(q[2]), bl_sqrt_fast_key(q[3])));
      if (SQ != 0 && __all(worst <= BL_SQRT_FAST_SPAN)) {
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = bl_sqrt_rn_fast<SQ == 2 ? 2 : 1>(q[k]);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = sqrtf(q[k]);
      }
    }
    if (vec_ok) { /* plain stores: with the non-temporal hint the same stream is 6 % slower (70.8 vs 66.6 us) */
      *reinterpret_cast<float4 *>(orow + j0) = make_float4(r[0], r[1], r[2], r[3]);
    } else {
      for (int k = 0; k < 4 && j0 + k < n; ++k) orow[j0 + k] = r[k];
    }
  }
}

/* Exhaustive check of bl_sqrt_rn_fast: every f32 bit pattern in [first, first + count) that lies
 * in the fast domain against (float)sqrt((double)s); counts[0] += values checked, counts[1] +=
 * mismatches, counts[2] += mismatches of the compiler's sqrtf over ALL patterns of the range
 * (zero, denormals, infinities included; NaN results compare equal to NaN). */
template <int V>
__global__ __launch_bounds__(256) void k_sqrt_sweep(unsigned long long first, unsigned long long count,
                                                    unsigned long long *counts) {
  unsigned long long checked = 0, bad_fast = 0, bad_slow = 0;
  for (unsigned long long i = blockIdx.x * 256ull + threadIdx.x; i < count; i += gridDim.x * 256ull) {
    const float s = __uint_as_float((unsigned)(first + i));
    const float want = (float)sqrt((double)s);
    const float slow = sqrtf(s);
    if (!(slow == want || (slow != slow && want != want))) ++bad_slow;
    if (bl_sqrt_fast_ok(s)) {
      ++checked;
      if (__float_as_uint(bl_sqrt_rn_fast<V>(s)) != __float_as_uint(want)) ++bad_fast;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    checked += __shfl_down(checked, off);
    bad_fast += __shfl_down(bad_fast, off);
    bad_slow += __shfl_down(bad_slow, off);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&counts[0], checked);
    atomicAdd(&counts[1], bad_fast);
    atomicAdd(&counts[2], bad_slow);
  }
}

/* ------------------------------------------------------------------------- */
/* seeded playlist: ref python/examples/make_m3u_playlist.py:62-72                */
/* distances from one seed vector to every song (bl_distance arithmetic), then the songs
 * in order of increasing distance.  The order is the stable argsort: rank(i) = number of
 * songs that are closer, or equally close with a smaller index (a NaN distance: farther than
 * every number, as close as another NaN) — an exact, deterministic
 * O(n^2) count (4.3e9 comparisons at n = 65 536, a few ms) instead of a comparison sort. */
__global__ __launch_bounds__(256) void k_seed_dist(const float4 *__restrict__ vecs, int n, int seed,
                                                   float *__restrict__ dist) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j < n) dist[j] = bl_dist(vecs[seed], vecs[j]);
}

/* the same from a seed that is no song of the library: the vector itself is the kernel's argument */
__global__ __launch_bounds__(256) void k_seed_dist_vec(const float4 *__restrict__ vecs, int n, float4 seed,
                                                       float *__restrict__ dist) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j < n) dist[j] = bl_dist(seed, vecs[j]);
}

__global__ __launch_bounds__(256) void k_rank_order(const float *__restrict__ dist, int n,
                                                    int *__restrict__ order) {
  /* compared as bl_ord keys, the total order of the queries: every NaN distance after +inf and equal to every other
   * NaN, so the NaN songs take the last ranks in index order (numpy's stable argsort) and every rank is taken once;
   * a plain float compare is false both ways for a NaN and would rank all of them 0 */
  __shared__ unsigned tile[256];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const unsigned ki = i < n ? bl_ord(dist[i]) : 0u;
  int rank = 0;
  for (int j0 = 0; j0 < n; j0 += 256) {
    const int j = j0 + threadIdx.x;
    tile[threadIdx.x] = j < n ? bl_ord(dist[j]) : 0u;
    __syncthreads();
    const int lim = min(256, n - j0);
    for (int k = 0; k < lim; ++k) {
      const unsigned kj = tile[k];
      rank += (kj < ki || (kj == ki && j0 + k < i)) ? 1 : 0;
    }
    __syncthreads();
  }
  if (i < n) order[rank] = i;
}

/* Sweep of bl_cos_fast against the plain expression over pseudo-random (dot, na, nb): norms over 2^-40..2^40
 * (a quarter of them within 2^-4..2^16, where force vectors live), dot = u * sqrt(na nb) with u in [-1, 1], and for
 * each such triple the 8 neighbouring floats of dot.  counts: [0] triples, [1] triples the fast path accepts,
 * [2] accepted triples whose float differs from the plain expression's (must be 0), [3] largest |q' - q| seen,
 * in ulp of the double quotient (provable bound: < 6), [4] triples whose q lies within 64 ulp of a float rounding
 * boundary, [5] of those, how many the unguarded (float)q' would get wrong. */
__global__ __launch_bounds__(256) void k_cos_sweep(unsigned long long seed, int per_thread, unsigned long long *counts) {
  unsigned long long st = seed + 0x9E3779B97F4A7C15ull * (blockIdx.x * 256ull + threadIdx.x + 1);
  auto next = [&]() -> unsigned {
    st ^= st << 13; st ^= st >> 7; st ^= st << 17;
    return (unsigned)(st >> 32) ^ (unsigned)st;
  };
  auto rnd_norm = [&]() -> float {
    const unsigned r = next();
    const int span = (r & 3u) ? 80 : 20, base = (r & 3u) ? -40 : -4;
    const int e = base + (int)((r >> 2) % (unsigned)span);
    return ldexpf(1.0f + (float)(next() >> 9) * (1.0f / 8388608.0f), e);
  };
  unsigned long long n = 0, n_fast = 0, bad = 0, max_ulp = 0, near = 0, near_bad = 0;
  for (int it = 0; it < per_thread; ++it) {
    bl_cos_vec a, b;
    a.n = rnd_norm(); b.n = rnd_norm();
    a.s = sqrt((double)a.n); a.r = 1.0 / a.s;
    b.s = sqrt((double)b.n); b.r = 1.0 / b.s;
    const float u = (float)((int)next()) * (1.0f / 2147483648.0f);
    const float d0 = (float)((double)u * (a.s * b.s));
    for (int j = -4; j < 4; ++j) {
      const float dot = __uint_as_float(__float_as_uint(d0) + (unsigned)j);
      const float want = bl_cos_plain(dot, a, b);
      float got;
      const bool ok = bl_cos_fast(dot, a.r * b.r, got);
      const double q = (double)dot / (a.s * b.s), qf = (double)dot * (a.r * b.r);
      const long long bq = __double_as_longlong(q), bf = __double_as_longlong(qf);
      ++n;
      if (ok) {
        ++n_fast;
        if (__float_as_uint(got) != __float_as_uint(want)) ++bad;
      }
      if (q == q && qf == qf && q != 0.0 && (bq >> 63) == (bf >> 63)) {
        const unsigned long long d = (unsigned long long)(bq > bf ? bq - bf : bf - bq);
        if (d < (1ull << 40)) max_ulp = max(max_ulp, d);
        const unsigned lo = (unsigned)bq & 0x1FFFFFFFu;
        if (lo - (0x10000000u - 64u) <= 128u) {
          ++near;
          if (__float_as_uint(got) != __float_as_uint(want)) ++near_bad;
        }
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    n += __shfl_down(n, off); n_fast += __shfl_down(n_fast, off); bad += __shfl_down(bad, off);
    near += __shfl_down(near, off); near_bad += __shfl_down(near_bad, off);
    max_ulp = max(max_ulp, (unsigned long long)__shfl_down(max_ulp, off));
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&counts[0], n); atomicAdd(&counts[1], n_fast); atomicAdd(&counts[2], bad);
    atomicMax(&counts[3], max_ulp); atomicAdd(&counts[4], near); atomicAdd(&counts[5], near_bad);
  }
}

/* ------------------------------------------------------------------------- */
/* force vectors of the batch / multi-device paths                              */

__global__ __launch_bounds__(256) void k_scatter_vecs(const float4 *__restrict__ in,
                                                      const int32_t *__restrict__ order,
                                                      float4 *__restrict__ out, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n && order[i] >= 0) out[order[i]] = in[i]; /* -1: padding slot of a short shard */
}

__global__ __launch_bounds__(256) void k_extract_vecs(const bl_amd_song_result *__restrict__ res,
                                                      float4 *__restrict__ out, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const struct force_vector_s v = res[i].v;
    out[i] = make_float4(v.tempo, v.amplitude, v.frequency, v.attack);
  }
}

/* ========================================================================= */
/* launchers (declared in bl_launch.h)                                        */

/* Which root the distance kernel uses: the compiled default BL_SQRT_VARIANT (bl_sqrt.h).  Only a
 * measurement build (make measure: -DBL_AMD_MEASURE, tools/dist_bench.py) also reads
 * BL_AMD_SQRT_VARIANT=0|1|2|3 at run time — 0 = the compiler's sqrtf only, 3 = no arithmetic at
 * all, the store stream alone (results invalid).  The product build ignores the variable.
 * rocprofv3 at N = 10 000, us per launch: 78.9 / 71.2 / 70.7 / 66.6 (profiles/r03_distance.json). */
static int blk_sqrt_variant() {
#ifdef BL_AMD_MEASURE
  const char *e = getenv("BL_AMD_SQRT_VARIANT");
  const int v = e && *e ? atoi(e) : BL_SQRT_VARIANT;
  return v < 0 || v > 3 ? BL_SQRT_VARIANT : v;
#else
  return BL_SQRT_VARIANT;
#endif
}

/* every k_pairwise<COSINE, SQ> the build has (the cosine has no root to vary), as PW_X(COSINE, SQ) */
#ifdef BL_AMD_MEASURE
#define PW_INSTANCES PW_X(true, 0) PW_X(false, 0) PW_X(false, 1) PW_X(false, 2) PW_X(false, 3)
#else
#define PW_INSTANCES PW_X(true, 0) PW_X(false, BL_SQRT_VARIANT)
#endif

int blk_pairwise(hipStream_t s, const struct force_vector_s *d_vecs, int n, int row_begin,
                 int n_rows, float *d_out, bool cosine, blk_mark_fn mark, void *mark_user) {
  const float4 *v = reinterpret_cast<const float4 *>(d_vecs);
  const int gx = (n + 1023) / 1024;
  const int chunk = 65535 * BL_PW_ROWS; /* rows per launch (gridDim.y limit) */
  for (int r0 = 0; r0 < n_rows; r0 += chunk) {
    const int cnt = n_rows - r0 < chunk ? n_rows - r0 : chunk;
    const int gy = (cnt + BL_PW_ROWS - 1) / BL_PW_ROWS;
    Mark m(mark, mark_user, PK_DIST, s);
    const int sq = cosine ? 0 : blk_sqrt_variant();
#define PW_X(C, SQ)                                                                                   \
  if (cosine == (C) && sq == (SQ))                                                                    \
    hipLaunchKernelGGL((k_pairwise<C, SQ>), dim3(gx, gy), dim3(256), 0, s, v, n, row_begin + r0, cnt, \
                       d_out + (size_t)r0 * n);
    PW_INSTANCES
#undef PW_X
  }
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}

int blk_cos_sweep(hipStream_t s, unsigned long long seed, int per_thread, unsigned long long *d_counts, int n_cu) {
  hipLaunchKernelGGL(k_cos_sweep, dim3(n_cu * 8), dim3(256), 0, s, seed, per_thread, d_counts);
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}

int blk_sqrt_sweep(hipStream_t s, unsigned long long first, unsigned long long count,
                   unsigned long long *d_counts, int n_cu) {
  if (blk_sqrt_variant() == 2)
    hipLaunchKernelGGL(k_sqrt_sweep<2>, dim3(n_cu * 8), dim3(256), 0, s, first, count, d_counts);
  else /* variant 0 ships no fast form; the sweep then checks form 1 and the fallback */
    hipLaunchKernelGGL(k_sqrt_sweep<1>, dim3(n_cu * 8), dim3(256), 0, s, first, count, d_counts);
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}

int blk_playlist(hipStream_t s, const struct force_vector_s *d_vecs, int n, int seed_index,
                 int32_t *d_order, float *d_dist) {
  const int gx = (n + 255) / 256;
  hipLaunchKernelGGL(k_seed_dist, dim3(gx), dim3(256), 0, s, reinterpret_cast<const float4 *>(d_vecs),
                     n, seed_index, d_dist);
  hipLaunchKernelGGL(k_rank_order, dim3(gx), dim3(256), 0, s, d_dist, n, d_order);
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}

int blk_playlist_vec(hipStream_t s, const struct force_vector_s *d_vecs, int n, struct force_vector_s seed,
                     int32_t *d_order, float *d_dist) {
  const int gx = (n + 255) / 256;
  hipLaunchKernelGGL(k_seed_dist_vec, dim3(gx), dim3(256), 0, s, reinterpret_cast<const float4 *>(d_vecs), n,
                     make_float4(seed.tempo, seed.amplitude, seed.frequency, seed.attack), d_dist);
  hipLaunchKernelGGL(k_rank_order, dim3(gx), dim3(256), 0, s, d_dist, n, d_order);
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}

int blk_scatter_vecs(hipStream_t s, const struct force_vector_s *d_in, const int32_t *d_order,
                     struct force_vector_s *d_out, int n) {
  hipLaunchKernelGGL(k_scatter_vecs, dim3((n + 255) / 256), dim3(256), 0, s,
                     reinterpret_cast<const float4 *>(d_in), d_order, reinterpret_cast<float4 *>(d_out), n);
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}

int blk_extract_vecs(hipStream_t s, const bl_amd_song_result *d_res, struct force_vector_s *d_out,
                     int n) {
  hipLaunchKernelGGL(k_extract_vecs, dim3((n + 255) / 256), dim3(256), 0, s, d_res,
                     reinterpret_cast<float4 *>(d_out), n);
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}
