/*
 * bl_query_kernels.hip — gfx950 kernels and launch layer of the vector queries over force vectors: answers that
 * would otherwise be read off the N x N matrix of k_pairwise (bl_matrix_kernels.hip), without building it.  The queries
 * share one design: a listed value has the bits of the matrix entry (bl_metric.h), a 64-bit (value, song) key gives
 * the order, the cosine takes a per-song "prep" array computed once per call, and with few query rows the columns are
 * split over blockIdx.y.  Must be compiled with -ffp-contract=off, like every kernel file.
 *
 * Kernels:
 *   k_knn_prep     cosine: (root, reciprocal root) of |v|^2 per song
 *   k_knn, k_knn_merge  the k nearest songs of each query   ref python/examples/make_m3u_playlist.py:62-72
 *                  k_knn, k_knn_merge, k_radius_count and k_radius_fill carry a flag CROSS: false for queries that
 *                  are songs of the library, true for vectors outside it (bl_amd_cross_*), of which no candidate is
 *                  excluded; the self form passes the library as its own query array
 *   k_chain, k_chain_init, k_chain_step  song-to-song chains: every next song the nearest unplayed one
 *   k_mix, k_mix_init, k_mix_step  siblings of those under rules (bl_amd_mix_*): excluded songs, a gap between songs
 *                  of one tag, seeds that are vectors
 *   k_radius_count, k_radius_offsets, k_radius_split_scan, k_radius_fill  the songs within a radius of each query
 *                  as CSR lists
 *   k_groups_init, k_groups_union, k_groups_compress  duplicate groups: connected components of the within-radius
 *                  graph, union-find on the output
 */
#include <hip/hip_runtime.h>
#include <algorithm>

#include "bl_launch.h"
#include "bl_metric.h"
#include "bl_topk.h"

/* ------------------------------------------------------------------------- */
/* k_knn: the k nearest songs of each query without the N x N matrix            */
/* Values: bl_distance / bl_cosine_similarity with k_pairwise's arithmetic (bl_dist_sq + a correctly rounded root,
 * bl_cos.h's guarded quotient), so a listed value has the bits of the matrix entry.  Order: a 64-bit key per
 * (value, song) — high word the order-preserving bits of the canonical value (-0 -> +0, every NaN -> 0xFFFFFFFF,
 * cosine negated so that larger is nearer), low word the song index — so one unsigned compare is the contract's
 * total order (value, then smaller index).  An empty slot is the all-ones key (index 0xFFFFFFFF is never a song).
 *
 * A wave owns KNN_QPW queries (wave-uniform vectors) and streams 64 candidate columns per step, one per lane.  Each
 * query keeps its best 64 * KW keys sorted across the lanes (KW = 1 for k <= 64, 2 up to 128) and the k-th of them
 * as a wave-uniform threshold: a candidate below it goes to the query's 64-key LDS queue, and a full queue is sorted
 * (bitonic, 21 shuffle steps) and merged into the list (6 or 7 more).  For the distance the filter runs on the squared
 * sum against a bound taken from the threshold (bl_sq_bound) and only survivors take the root.  With few queries the
 * columns are split over blockIdx.y; each split writes its sorted partial list and k_knn_merge streams those keys
 * through the same filter and queue. */
#define KNN_QPW 4       /* queries per wave */
#define KNN_WAVES 4     /* waves per workgroup */
/* knn_sort64, knn_clean64 and knn_top<KW>, the list, threshold, queue and merge: bl_topk.h */

/* slots [0, k) of row r: index and recomputed value (same function as the key's, so the same bits) */
template <int KW, bool COSINE>
__device__ __forceinline__ void knn_emit(const knn_top<KW> &t, int lane, int k, size_t r, const float4 a,
                                         const double2 pa, const float4 *__restrict__ vecs,
                                         const double2 *__restrict__ prep, int32_t *__restrict__ out_index,
                                         float *__restrict__ out_value) {
#pragma unroll
  for (int w = 0; w < KW; ++w) {
    const int slot = w * 64 + lane;
    if (slot >= k) continue;
    const unsigned long long key = w == 0 ? t.e0 : t.e1;
    int idx = -1;
    float val = __builtin_nanf("");
    if (key != BL_KEY_EMPTY) {
      idx = (int)(unsigned)key;
      val = bl_value<COSINE>(a, pa, vecs[idx], COSINE ? prep[idx] : make_double2(0.0, 0.0));
    }
    out_index[r * k + slot] = idx;
    out_value[r * k + slot] = val;
  }
}

/* cosine: the per-vector part of bl_cos.h once per song: (sqrt((double)|v|^2), its reciprocal) */
__global__ __launch_bounds__(256) void k_knn_prep(const float4 *__restrict__ vecs, int n, double2 *__restrict__ prep) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const bl_cos_vec p = bl_cos_prep(vecs[i]);
    prep[i] = make_double2(p.s, p.r);
  }
}

/* blockIdx.x: KNN_WAVES * KNN_QPW query rows, blockIdx.y: column split [y * cols, (y + 1) * cols).  n_split == 1:
 * the final lists go to out_index / out_value; otherwise the first k keys of each list go to
 * part[(row * n_split + split) * k ...].  Query r is qvecs[row_begin + r] with its prep qprep[row_begin + r].
 *   CROSS = false  the queries are songs of the library: the launch passes vecs / prep as qvecs / qprep, and a
 *                  query's own column is no candidate.
 *   CROSS = true   the queries are vectors outside the library (bl_amd_cross_knn_device): they start at row 0
 *                  (row_begin is not read) and every column is a candidate.
 * One kernel with a flag, not two: the flag on the kernel itself leaves both forms' registers and occupancy what
 * the two copies had; a body inlined into two kernels did not. */
template <int KW, bool COSINE, bool CROSS>
__global__ __launch_bounds__(256) void k_knn(const float4 *__restrict__ qvecs, const double2 *__restrict__ qprep,
                                             const float4 *__restrict__ vecs, const double2 *__restrict__ prep, int n,
                                             int row_begin, int n_rows, int k, int cols, int n_split,
                                             unsigned long long *__restrict__ part, int32_t *__restrict__ out_index,
                                             float *__restrict__ out_value) {
  __shared__ unsigned long long queue[KNN_WAVES][KNN_QPW][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r0 = (blockIdx.x * KNN_WAVES + wave) * KNN_QPW;
  if (r0 >= n_rows) return;
  const int nq = min(KNN_QPW, n_rows - r0);
  const int c0 = blockIdx.y * cols, c1 = min(n, c0 + cols);
  const int q0 = (CROSS ? 0 : row_begin) + r0; /* the wave's first row in qvecs */
  float4 a[KNN_QPW];
  double2 pa[KNN_QPW];
  float bnd[KNN_QPW];
  knn_top<KW> top[KNN_QPW];
#pragma unroll
  for (int q = 0; q < KNN_QPW; ++q) {
    const int row = q0 + min(q, nq - 1);
    a[q] = qvecs[row];
    pa[q] = COSINE ? qprep[row] : make_double2(0.0, 0.0);
    /* held in VGPRs: the same in every lane, but as scalars (16 + 16 SGPRs for the cosine) they overflowed the
     * SGPR budget and spilled in the candidate loop; the empty asm only moves them to vector registers */
    asm volatile("" : "+v"(a[q].x), "+v"(a[q].y), "+v"(a[q].z), "+v"(a[q].w));
    if (COSINE) asm volatile("" : "+v"(pa[q].x), "+v"(pa[q].y));
    bnd[q] = __builtin_inff();
    top[q].init();
  }
  for (int j0 = c0; j0 < c1; j0 += 64) {
    const int j = j0 + lane;
    const bool valid = j < c1;
    const int jj = valid ? j : c1 - 1;
    const float4 b = vecs[jj];
    const double2 pb = COSINE ? prep[jj] : make_double2(0.0, 0.0);
#pragma unroll
    for (int q = 0; q < KNN_QPW; ++q) {
      if (q >= nq) break;
      const bool cand = valid && (CROSS || j != q0 + q);
      if (COSINE) {
        const unsigned long long key = bl_key<true>(bl_cosine(a[q], pa[q], b, pb), j);
        top[q].push(cand && key < top[q].thr, key, queue[wave][q], lane, k);
      } else {
        const float s = bl_dist_sq(a[q], b);
        const bool p = cand && !(s > bnd[q]);
        if (__ballot(p) == 0) continue;
        const float d = __all(!p || bl_sqrt_fast_ok(s)) ? bl_sqrt_rn_fast<1>(s) : sqrtf(s);
        const unsigned long long key = bl_key<false>(d, j);
        top[q].push(p && key < top[q].thr, key, queue[wave][q], lane, k);
        bnd[q] = bl_sq_bound(top[q].thr);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < KNN_QPW; ++q) {
    if (q >= nq) break;
    top[q].finish(queue[wave][q], lane, k);
    const size_t r = (size_t)(r0 + q);
    if (n_split == 1) {
      knn_emit<KW, COSINE>(top[q], lane, k, r, a[q], pa[q], vecs, prep, out_index, out_value);
    } else {
      unsigned long long *dst = part + (r * n_split + blockIdx.y) * k;
#pragma unroll
      for (int w = 0; w < KW; ++w)
        if (w * 64 + lane < k) dst[w * 64 + lane] = w == 0 ? top[q].e0 : top[q].e1;
    }
  }
}

/* one wave per query row: the n_split partial lists of the row, read as one stream of keys, through the filter; the
 * emitted values are computed from the query array again, indexed as in k_knn */
template <int KW, bool COSINE, bool CROSS>
__global__ __launch_bounds__(256) void k_knn_merge(const float4 *__restrict__ qvecs, const double2 *__restrict__ qprep,
                                                   const float4 *__restrict__ vecs, const double2 *__restrict__ prep,
                                                   int row_begin, int n_rows, int k, int n_split,
                                                   const unsigned long long *__restrict__ part,
                                                   int32_t *__restrict__ out_index, float *__restrict__ out_value) {
  __shared__ unsigned long long queue[KNN_WAVES][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = blockIdx.x * KNN_WAVES + wave;
  if (r >= n_rows) return;
  const unsigned long long *src = part + (size_t)r * n_split * k;
  const int total = n_split * k;
  knn_top<KW> top;
  top.init();
  for (int o = 0; o < total; o += 4 * 64) {
    unsigned long long key[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = o + u * 64 + lane;
      key[u] = i < total ? src[i] : BL_KEY_EMPTY;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) top.push(key[u] < top.thr, key[u], queue[wave], lane, k);
  }
  top.finish(queue[wave], lane, k);
  const int row = (CROSS ? 0 : row_begin) + r;
  knn_emit<KW, COSINE>(top, lane, k, (size_t)r, qvecs[row], COSINE ? qprep[row] : make_double2(0.0, 0.0), vecs, prep,
                       out_index, out_value);
}

/* ------------------------------------------------------------------------- */
/* k_chain: song-to-song chains (bl_amd_chain_device)                           */
/* Slot t + 1 of a chain is the unplayed song nearest to the song of slot t: `length` dependent steps of an argmin
 * over n candidates.  Values and order are k_knn's (bl_dist_sq + bl_root or bl_cosine, bl_key), the pick is the
 * minimum key and the stored value is computed again at the store by the function its key came from.  Two shapes,
 * same bytes:
 *   k_chain       one workgroup per chain.  Lane `tid` owns the columns j = tid (mod blockDim.x) for the whole chain,
 *                 so their played bits are the lane's own words (LDS, or the workspace when n bits do not fit) and need
 *                 no atomics.  A step: every lane's minimum key over its unplayed columns, a wave min by shuffles,
 *                 one LDS word per wave, one barrier (the words are double-buffered by the step's parity).
 *   k_chain_step  few chains over many songs: one launch per step, blockIdx.x a column slice, blockIdx.y the chain.
 *                 A slice's minimum key goes into the chain's `best` by an agent-scope atomic min; once that has
 *                 returned the workgroup adds to the chain's arrival counter, and the workgroup whose add came last
 *                 takes `best` (an atomic exchange that also re-arms it), writes the slot, sets the played bit and
 *                 publishes the current song for the next launch.  Nobody waits for anybody: no polling.  Only
 *                 8-byte and 4-byte agent-scope atomics carry data between workgroups of one launch; everything
 *                 else (current song, played bits) crosses a kernel boundary. */
#define CHAIN_MAX_WAVES 16
#define CHAIN_BATCH 8 /* candidate loads a lane keeps in flight */
#define CHAIN_LDS_HEAD (2 * CHAIN_MAX_WAVES * 8) /* bytes of wave minima in front of the LDS bitmap */
#define CHAIN_LDS_MAX (160 * 1024)

struct chain_state { /* one per chain of the column-split shape; `best` and `count` on different 128-byte lines */
  unsigned long long best;
  unsigned pad0[30];
  unsigned count;
  int cur;
  unsigned pad1[30];
};

/* candidate j into a lane's running minimum.  Distance: a sum above bl_sq_bound(best) has a root above best's, so
 * only sums at or below it (and NaN) take the root. */
template <bool COSINE>
__device__ __forceinline__ void chain_visit(const float4 a, const double2 pa, const float4 b, const double2 pb, int j,
                                            unsigned long long &best, float &bnd) {
  if (COSINE) {
    best = min(best, bl_key<true>(bl_cosine(a, pa, b, pb), j));
  } else {
    const float s = bl_dist_sq(a, b);
    if (!(s > bnd)) {
      const unsigned long long key = bl_key<false>(bl_root(s), j);
      if (key < best) {
        best = key;
        bnd = bl_sq_bound(best);
      }
    }
  }
}

__device__ __forceinline__ unsigned long long chain_wave_min(unsigned long long x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x = min(x, (unsigned long long)__shfl_xor(x, off));
  return x;
}

/* blockDim.x = 1 << lb threads (a multiple of 64, at most 1024).  `words` 32-column words of played bits per lane:
 * word w of lane tid at bits[w * blockDim.x + tid] covers the columns tid + (32 w + i) * blockDim.x. */
template <bool COSINE, bool LDS_BITS>
__global__ __launch_bounds__(1024) void k_chain(const float4 *__restrict__ vecs, const double2 *__restrict__ prep, int n,
                                                const int32_t *__restrict__ seeds, int length, int lb, int words,
                                                unsigned *__restrict__ g_bits, int32_t *__restrict__ out_order,
                                                float *__restrict__ out_value) {
  extern __shared__ __attribute__((aligned(16))) unsigned char chain_smem[];
  unsigned long long *wmin = reinterpret_cast<unsigned long long *>(chain_smem);
  const int B = 1 << lb, tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wave_mask = (B >> 6) - 1;
  unsigned *bits = LDS_BITS ? reinterpret_cast<unsigned *>(chain_smem + CHAIN_LDS_HEAD)
                            : g_bits + (size_t)blockIdx.x * words * B;
  int32_t *order = out_order + (size_t)blockIdx.x * length;
  float *value = out_value + (size_t)blockIdx.x * length;
  const int steps = min(length, n);
  int cur = seeds[blockIdx.x];
  const bool ok = cur >= 0 && cur < n;
  for (int t = (ok ? steps : 0) + tid; t < length; t += B) {
    order[t] = -1;
    value[t] = __builtin_nanf("");
  }
  if (!ok) return;
  const int cols = tid < n ? ((n - 1 - tid) >> lb) + 1 : 0; /* columns of this lane */
  for (int w = 0; w < words; ++w) bits[w * B + tid] = 0u;
  if ((cur & (B - 1)) == tid) bits[((cur >> lb) >> 5) * B + tid] = 1u << ((cur >> lb) & 31);
  for (int t = 0; t < steps; ++t) {
    float4 a = vecs[cur];
    double2 pa = COSINE ? prep[cur] : make_double2(0.0, 0.0);
    /* wave-uniform, but held in VGPRs like k_knn's queries: as scalars they crowd the SGPR file in the loop */
    asm volatile("" : "+v"(a.x), "+v"(a.y), "+v"(a.z), "+v"(a.w));
    if (COSINE) asm volatile("" : "+v"(pa.x), "+v"(pa.y));
    if (t == 0) {
      if (tid == 0) {
        order[0] = cur;
        value[0] = bl_value<COSINE>(a, pa, a, pa);
      }
      continue;
    }
    unsigned long long best = BL_KEY_EMPTY;
    float bnd = __builtin_inff();
    for (int i0 = 0; i0 < cols; i0 += 32) {
      const unsigned played = bits[(i0 >> 5) * B + tid];
      for (int u0 = 0; u0 < 32 && i0 + u0 < cols; u0 += CHAIN_BATCH) {
        /* CHAIN_BATCH loads in flight, then the arithmetic: one load per visit leaves the step latency-bound */
        float4 b[CHAIN_BATCH];
        double2 pb[CHAIN_BATCH];
#pragma unroll
        for (int u = 0; u < CHAIN_BATCH; ++u) {
          const int j = tid + (min(i0 + u0 + u, cols - 1) << lb);
          b[u] = vecs[j];
          pb[u] = COSINE ? prep[j] : make_double2(0.0, 0.0);
        }
#pragma unroll
        for (int u = 0; u < CHAIN_BATCH; ++u)
          if (i0 + u0 + u < cols && !((played >> (u0 + u)) & 1u))
            chain_visit<COSINE>(a, pa, b[u], pb[u], tid + ((i0 + u0 + u) << lb), best, bnd);
      }
    }
    best = chain_wave_min(best);
    unsigned long long *slot = wmin + (t & 1) * CHAIN_MAX_WAVES;
    if (lane == 0) slot[wave] = best;
    __syncthreads();
    unsigned long long m = slot[lane & wave_mask];
#pragma unroll
    for (int off = CHAIN_MAX_WAVES / 2; off > 0; off >>= 1) m = min(m, (unsigned long long)__shfl_xor(m, off));
    if (m == BL_KEY_EMPTY) break; /* cannot happen while t < n: a song is left */
    const int pick = __builtin_amdgcn_readfirstlane((int)(unsigned)m);
    if ((pick & (B - 1)) == tid) bits[((pick >> lb) >> 5) * B + tid] |= 1u << ((pick >> lb) & 31);
    if (tid == 0) {
      order[t] = pick;
      value[t] = bl_value<COSINE>(a, pa, vecs[pick], COSINE ? prep[pick] : make_double2(0.0, 0.0));
    }
    cur = pick;
  }
}

/* column-split shape, start of a call: played bits (word w of chain c at bits[c * words + w], bit j & 31 of word
 * j >> 5 = song j), the chain's state, slot 0 and the padding.  grid (any, n_chains). */
template <bool COSINE>
__global__ __launch_bounds__(256) void k_chain_init(const float4 *__restrict__ vecs, const double2 *__restrict__ prep,
                                                    int n, const int32_t *__restrict__ seeds, int length, int words,
                                                    chain_state *__restrict__ state, unsigned *__restrict__ bits,
                                                    int32_t *__restrict__ out_order, float *__restrict__ out_value) {
  const int c = blockIdx.y;
  const int seed = seeds[c];
  const bool ok = seed >= 0 && seed < n;
  const int steps = min(length, n);
  const unsigned g = blockIdx.x * 256u + threadIdx.x, stride = gridDim.x * 256u;
  for (unsigned w = g; w < (unsigned)words; w += stride)
    bits[(size_t)c * words + w] = (ok && w == (unsigned)seed >> 5) ? 1u << (seed & 31) : 0u;
  for (unsigned t = (ok ? steps : 0) + g; t < (unsigned)length; t += stride) {
    out_order[(size_t)c * length + t] = -1;
    out_value[(size_t)c * length + t] = __builtin_nanf("");
  }
  if (g == 0) {
    state[c].best = BL_KEY_EMPTY;
    state[c].count = 0u;
    state[c].cur = ok ? seed : -1;
    if (ok) {
      const float4 a = vecs[seed];
      const double2 pa = COSINE ? prep[seed] : make_double2(0.0, 0.0);
      out_order[(size_t)c * length] = seed;
      out_value[(size_t)c * length] = bl_value<COSINE>(a, pa, a, pa);
    }
  }
}

/* slot t of every chain.  grid (n_groups, n_chains); workgroup x scans the columns [x * cols, (x + 1) * cols). */
template <bool COSINE>
__global__ __launch_bounds__(256) void k_chain_step(const float4 *__restrict__ vecs, const double2 *__restrict__ prep,
                                                    int n, int cols, int t, int length, int words,
                                                    chain_state *__restrict__ state, unsigned *__restrict__ bits_all,
                                                    int32_t *__restrict__ out_order, float *__restrict__ out_value) {
  __shared__ unsigned long long wmin[4];
  const int c = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  chain_state *st = state + c;
  const int cur = st->cur; /* published by the previous launch */
  if (cur < 0) return;     /* a seed outside [0, n): the whole grid row leaves, nobody arrives */
  const unsigned *bits = bits_all + (size_t)c * words;
  float4 a = vecs[cur];
  double2 pa = COSINE ? prep[cur] : make_double2(0.0, 0.0);
  asm volatile("" : "+v"(a.x), "+v"(a.y), "+v"(a.z), "+v"(a.w));
  if (COSINE) asm volatile("" : "+v"(pa.x), "+v"(pa.y));
  const unsigned c0 = (unsigned)blockIdx.x * (unsigned)cols; /* n_groups * cols < n + cols <= 2^31 + 2^23 */
  const unsigned c1 = min((unsigned)n, c0 + (unsigned)cols);
  unsigned long long best = BL_KEY_EMPTY;
  float bnd = __builtin_inff();
  for (unsigned j0 = c0 + tid; j0 < c1; j0 += 256u * CHAIN_BATCH) {
    unsigned played[CHAIN_BATCH];
    float4 b[CHAIN_BATCH];
    double2 pb[CHAIN_BATCH];
#pragma unroll
    for (int u = 0; u < CHAIN_BATCH; ++u) {
      const unsigned j = j0 + 256u * u < c1 ? j0 + 256u * u : j0;
      played[u] = bits[j >> 5];
      b[u] = vecs[j];
      pb[u] = COSINE ? prep[j] : make_double2(0.0, 0.0);
    }
#pragma unroll
    for (int u = 0; u < CHAIN_BATCH; ++u) {
      const unsigned j = j0 + 256u * u;
      if (j < c1 && !((played[u] >> (j & 31u)) & 1u)) chain_visit<COSINE>(a, pa, b[u], pb[u], (int)j, best, bnd);
    }
  }
  best = chain_wave_min(best);
  if (lane == 0) wmin[wave] = best;
  __syncthreads();
  if (tid != 0) return;
  const unsigned long long m = min(min(wmin[0], wmin[1]), min(wmin[2], wmin[3]));
  if (m != BL_KEY_EMPTY) (void)__hip_atomic_fetch_min(&st->best, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  /* the min has been performed before the arrival is counted */
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const unsigned ticket = __hip_atomic_fetch_add(&st->count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (ticket != gridDim.x - 1u) return;
  /* every slice's min was performed before its add, and every add before this one returned */
  const unsigned long long key = __hip_atomic_exchange(&st->best, BL_KEY_EMPTY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&st->count, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (key == BL_KEY_EMPTY) { /* cannot happen while t < n */
    __hip_atomic_store(&st->cur, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  const int pick = (int)(unsigned)key;
  atomicOr(bits_all + (size_t)c * words + (pick >> 5), 1u << (pick & 31));
  out_order[(size_t)c * length + t] = pick;
  out_value[(size_t)c * length + t] =
      bl_value<COSINE>(a, pa, vecs[pick], COSINE ? prep[pick] : make_double2(0.0, 0.0));
  __hip_atomic_store(&st->cur, pick, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

/* ------------------------------------------------------------------------- */
/* k_mix: chains under rules (bl_amd_mix_device)                                */
/* A chain whose step takes the nearest *allowed* song: not played, not excluded, and (gap > 0) of a tag that none of
 * the last `gap` slots carries.  Siblings of k_chain, k_chain_init and k_chain_step over the same pieces (bl_metric.h,
 * chain_wave_min, the chain's bit layouts and its arrival protocol), not a flag on them: their registers stay theirs.
 *   Exclusion   costs nothing per step: the played bits start from the mask instead of from zero.
 *   Tags        the tags of the last `gap` slots are a wave-uniform history (mix_hist), newest first, -1 where there
 *               is none.  k_mix keeps it in registers, every thread pushing the tag of the pick it has just read from
 *               LDS; in the split shape it lives in the chain's state, written by the last-arriving workgroup and read
 *               by the next launch, like `cur`.  A candidate's tag is fetched with its vector (TAGS) but tested only
 *               once its key has passed the squared-sum bound and would become the lane's best: a blocked candidate
 *               changes neither `best` nor `bnd`, so it cannot prune an allowed one behind it.
 *   Vector seed slot 0 is the same scan with the seed vector as the query (its cosine prep by bl_cos_prep, as
 *               k_knn_prep makes a song's) and an empty history, so no tag blocks; the value has the seed as first
 *               operand.
 *   The end     no allowed song: the minimum is the empty key, and the rest of the row is -1 / NaN.
 * With TAGS = false, no mask and index seeds the arithmetic per candidate is k_chain's. */
struct mix_state { /* chain_state with the tag history on the line of `count` and `cur` */
  unsigned long long best;
  unsigned pad0[30];
  unsigned count;
  int cur;
  int hist[BL_AMD_MIX_MAX_GAP];
  unsigned pad1[30 - BL_AMD_MIX_MAX_GAP];
};
static_assert(sizeof(mix_state) == sizeof(chain_state), "blk_mix_scratch_bytes is blk_chain_scratch_bytes");

/* tags of the last `gap` slots, h[0] the newest; entries at and past `gap` stay -1, which no tag >= 0 equals */
struct mix_hist {
  int h[BL_AMD_MIX_MAX_GAP];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int k = 0; k < BL_AMD_MIX_MAX_GAP; ++k) h[k] = -1;
  }
  __device__ __forceinline__ void push(int tag, int gap) { /* gap >= 1 */
#pragma unroll
    for (int k = BL_AMD_MIX_MAX_GAP - 1; k > 0; --k)
      if (k < gap) h[k] = h[k - 1];
    h[0] = tag;
  }
  /* k_mix holds the history in VGPRs: sixteen more scalars in its candidate loop overflow the SGPR file, as the
   * query vectors do in k_knn */
  __device__ __forceinline__ void to_vgprs() {
#pragma unroll
    for (int k = 0; k < BL_AMD_MIX_MAX_GAP; ++k) asm volatile("" : "+v"(h[k]));
  }
  __device__ __forceinline__ bool blocks(int tag) const {
    bool m = false;
#pragma unroll
    for (int k = 0; k < BL_AMD_MIX_MAX_GAP; ++k) m |= h[k] == tag;
    return tag >= 0 && m;
  }
};

/* chain_visit with the tag rule: candidate j of tag `tag` into the lane's minimum unless the history blocks it */
template <bool COSINE, bool TAGS>
__device__ __forceinline__ void mix_visit(const float4 a, const double2 pa, const float4 b, const double2 pb, int j,
                                          int tag, const mix_hist &hist, unsigned long long &best, float &bnd) {
  if (COSINE) {
    const unsigned long long key = bl_key<true>(bl_cosine(a, pa, b, pb), j);
    if (key < best && !(TAGS && hist.blocks(tag))) best = key;
  } else {
    const float s = bl_dist_sq(a, b);
    if (!(s > bnd)) {
      const unsigned long long key = bl_key<false>(bl_root(s), j);
      if (key < best && !(TAGS && hist.blocks(tag))) {
        best = key;
        bnd = bl_sq_bound(best);
      }
    }
  }
}

/* the query of a step: song `cur`, or (q != nullptr: slot 0 of a vector seed) the vector *q with its own prep */
template <bool COSINE>
__device__ __forceinline__ void mix_query(const float4 *__restrict__ vecs, const double2 *__restrict__ prep, int cur,
                                          const float4 *__restrict__ q, float4 &a, double2 &pa) {
  pa = make_double2(0.0, 0.0);
  if (q) {
    a = *q;
    if (COSINE) {
      const bl_cos_vec p = bl_cos_prep(a);
      pa = make_double2(p.s, p.r);
    }
  } else {
    a = vecs[cur];
    if (COSINE) pa = prep[cur];
  }
  /* in VGPRs, as in k_chain */
  asm volatile("" : "+v"(a.x), "+v"(a.y), "+v"(a.z), "+v"(a.w));
  if (COSINE) asm volatile("" : "+v"(pa.x), "+v"(pa.y));
}

/* k_chain's launch and bit layout.  Exactly one of seeds / qvecs (n_chains seed vectors) is non-null; tags is
 * non-null exactly when TAGS; exclude is null or n bytes, non-zero = never picked. */
template <bool COSINE, bool LDS_BITS, bool TAGS>
__global__ __launch_bounds__(1024) void k_mix(const float4 *__restrict__ vecs, const double2 *__restrict__ prep, int n,
                                              const int32_t *__restrict__ seeds, const float4 *__restrict__ qvecs,
                                              int length, int lb, int words, const int32_t *__restrict__ tags, int gap,
                                              const unsigned char *__restrict__ exclude, unsigned *__restrict__ g_bits,
                                              int32_t *__restrict__ out_order, float *__restrict__ out_value) {
  extern __shared__ __attribute__((aligned(16))) unsigned char chain_smem[];
  unsigned long long *wmin = reinterpret_cast<unsigned long long *>(chain_smem);
  const int B = 1 << lb, tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wave_mask = (B >> 6) - 1;
  unsigned *bits = LDS_BITS ? reinterpret_cast<unsigned *>(chain_smem + CHAIN_LDS_HEAD)
                            : g_bits + (size_t)blockIdx.x * words * B;
  int32_t *order = out_order + (size_t)blockIdx.x * length;
  float *value = out_value + (size_t)blockIdx.x * length;
  const int steps = min(length, n);
  int cur = qvecs ? 0 : seeds[blockIdx.x];
  const bool ok = cur >= 0 && cur < n;
  for (int t = (ok ? steps : 0) + tid; t < length; t += B) {
    order[t] = -1;
    value[t] = __builtin_nanf("");
  }
  if (!ok) return;
  const int cols = tid < n ? ((n - 1 - tid) >> lb) + 1 : 0; /* columns of this lane */
  for (int w = 0; w < words; ++w) {
    unsigned x = 0u;
    if (exclude && cols > 0) { /* bit i of word w: column tid + (32 w + i) * B; integer arithmetic only, eight
                                * bytes in flight: as compares the 32 bits of a word took the SGPR file */
#pragma unroll 1
      for (int i0 = 0; i0 < 32; i0 += 8) {
        unsigned e[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) e[u] = exclude[tid + (min(32 * w + i0 + u, cols - 1) << lb)];
#pragma unroll
        for (int u = 0; u < 8; ++u) x |= ((e[u] + 255u) >> 8) << (i0 + u);
      }
      const int left = cols - 32 * w; /* columns this word has; the bits past them repeat the last column's */
      if (left < 32) x &= left > 0 ? (1u << left) - 1u : 0u;
    }
    bits[w * B + tid] = x;
  }
  mix_hist hist;
  hist.clear();
  /* the query of the first scan: the seed vector, or the seed song, which also takes slot 0 whatever the mask says
   * and is the first entry of the history */
  float4 a;
  double2 pa;
  mix_query<COSINE>(vecs, prep, cur, qvecs ? qvecs + blockIdx.x : nullptr, a, pa);
  int t = 0;
  if (!qvecs) {
    if ((cur & (B - 1)) == tid) bits[((cur >> lb) >> 5) * B + tid] |= 1u << ((cur >> lb) & 31);
    if (TAGS) hist.push(tags[cur], gap);
    if (tid == 0) {
      order[0] = cur;
      value[0] = bl_value<COSINE>(a, pa, a, pa);
    }
    t = 1;
  }
  if (TAGS) hist.to_vgprs();
  for (; t < steps; ++t) {
    unsigned long long best = BL_KEY_EMPTY;
    float bnd = __builtin_inff();
    for (int i0 = 0; i0 < cols; i0 += 32) {
      const unsigned played = bits[(i0 >> 5) * B + tid];
      for (int u0 = 0; u0 < 32 && i0 + u0 < cols; u0 += CHAIN_BATCH) {
        float4 b[CHAIN_BATCH];
        double2 pb[CHAIN_BATCH];
        int tg[CHAIN_BATCH];
#pragma unroll
        for (int u = 0; u < CHAIN_BATCH; ++u) {
          const int j = tid + (min(i0 + u0 + u, cols - 1) << lb);
          b[u] = vecs[j];
          pb[u] = COSINE ? prep[j] : make_double2(0.0, 0.0);
          tg[u] = TAGS ? tags[j] : -1;
        }
#pragma unroll
        for (int u = 0; u < CHAIN_BATCH; ++u)
          if (i0 + u0 + u < cols && !((played >> (u0 + u)) & 1u))
            mix_visit<COSINE, TAGS>(a, pa, b[u], pb[u], tid + ((i0 + u0 + u) << lb), tg[u], hist, best, bnd);
      }
    }
    best = chain_wave_min(best);
    unsigned long long *slot = wmin + (t & 1) * CHAIN_MAX_WAVES;
    if (lane == 0) slot[wave] = best;
    __syncthreads();
    unsigned long long m = slot[lane & wave_mask];
#pragma unroll
    for (int off = CHAIN_MAX_WAVES / 2; off > 0; off >>= 1) m = min(m, (unsigned long long)__shfl_xor(m, off));
    if (m == BL_KEY_EMPTY) break; /* no song is allowed: the chain ends here, for every thread alike */
    const int pick = __builtin_amdgcn_readfirstlane((int)(unsigned)m);
    if ((pick & (B - 1)) == tid) bits[((pick >> lb) >> 5) * B + tid] |= 1u << ((pick >> lb) & 31);
    float4 an; /* the pick is the next query */
    double2 pan;
    mix_query<COSINE>(vecs, prep, pick, nullptr, an, pan);
    if (tid == 0) {
      order[t] = pick;
      value[t] = bl_value<COSINE>(a, pa, an, pan);
    }
    if (TAGS) {
      hist.push(tags[pick], gap);
      hist.to_vgprs();
    }
    a = an;
    pa = pan;
  }
  for (int u = t + tid; u < steps; u += B) { /* the slots of a chain that ended early; nobody else wrote them */
    order[u] = -1;
    value[u] = __builtin_nanf("");
  }
}

/* column-split shape, start of a call: k_chain_init with the played bits taken from the mask (a wave's ballot over
 * 64 songs is two words), the whole row padded (a chain may end at any slot), and the history.  An index seed takes
 * slot 0 here; a vector seed (seeds == nullptr) leaves it to the step launched with t = 0.  grid (any, n_chains).
 * Unlike k_chain_init, which clears all `words`, only the words that cover songs below n are written, on purpose:
 * words == ceil(n / 32) today and no step reads a bit at or past n.  If `words` is ever padded beyond that, the words
 * past the last song hold stale bits and must be cleared here before anything may read them. */
template <bool COSINE>
__global__ __launch_bounds__(256) void k_mix_init(const float4 *__restrict__ vecs, const double2 *__restrict__ prep,
                                                  int n, const int32_t *__restrict__ seeds, int length, int words,
                                                  const int32_t *__restrict__ tags,
                                                  const unsigned char *__restrict__ exclude,
                                                  mix_state *__restrict__ state, unsigned *__restrict__ bits,
                                                  int32_t *__restrict__ out_order, float *__restrict__ out_value) {
  const int c = blockIdx.y, lane = threadIdx.x & 63;
  const int seed = seeds ? seeds[c] : 0;
  const bool ok = seed >= 0 && seed < n;
  const bool at_seed = seeds && ok; /* slot 0 is the seed song */
  const unsigned g = blockIdx.x * 256u + threadIdx.x, stride = gridDim.x * 256u;
  for (unsigned j0 = g - lane; j0 < (unsigned)n; j0 += stride) { /* j0: a multiple of 64, the same in the whole wave */
    const unsigned j = j0 + lane;
    unsigned long long m = __ballot(exclude && j < (unsigned)n && exclude[min(j, (unsigned)n - 1u)] != 0);
    if (at_seed && (unsigned)seed - j0 < 64u) m |= 1ull << ((unsigned)seed - j0);
    const unsigned w = (j0 >> 5) + lane;
    if (lane < 2 && w < (unsigned)words) bits[(size_t)c * words + w] = (unsigned)(m >> (32 * lane));
  }
  for (unsigned t = (at_seed ? 1u : 0u) + g; t < (unsigned)length; t += stride) {
    out_order[(size_t)c * length + t] = -1;
    out_value[(size_t)c * length + t] = __builtin_nanf("");
  }
  if (g == 0) {
    state[c].best = BL_KEY_EMPTY;
    state[c].count = 0u;
    state[c].cur = ok ? seed : -1;
#pragma unroll
    for (int k = 0; k < BL_AMD_MIX_MAX_GAP; ++k) state[c].hist[k] = -1;
    if (at_seed) {
      if (tags) state[c].hist[0] = tags[seed];
      const float4 a = vecs[seed];
      const double2 pa = COSINE ? prep[seed] : make_double2(0.0, 0.0);
      out_order[(size_t)c * length] = seed;
      out_value[(size_t)c * length] = bl_value<COSINE>(a, pa, a, pa);
    }
  }
}

/* slot t of every chain: k_chain_step with the tag rule.  qvecs != nullptr (t = 0 of a call with vector seeds): the
 * query of chain c is qvecs[c].  grid (n_groups, n_chains). */
template <bool COSINE, bool TAGS>
__global__ __launch_bounds__(256) void k_mix_step(const float4 *__restrict__ vecs, const double2 *__restrict__ prep,
                                                  int n, int cols, int t, int length, int words,
                                                  const int32_t *__restrict__ tags, int gap,
                                                  const float4 *__restrict__ qvecs, mix_state *__restrict__ state,
                                                  unsigned *__restrict__ bits_all, int32_t *__restrict__ out_order,
                                                  float *__restrict__ out_value) {
  __shared__ unsigned long long wmin[4];
  const int c = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  mix_state *st = state + c;
  const int cur = st->cur; /* published by the previous launch */
  if (cur < 0) return;     /* a seed outside [0, n), or a chain that has ended: nobody arrives */
  mix_hist hist;
  hist.clear();
  if (TAGS) {
#pragma unroll
    for (int k = 0; k < BL_AMD_MIX_MAX_GAP; ++k) hist.h[k] = st->hist[k];
  }
  const unsigned *bits = bits_all + (size_t)c * words;
  float4 a;
  double2 pa;
  mix_query<COSINE>(vecs, prep, cur, qvecs ? qvecs + c : nullptr, a, pa);
  const unsigned c0 = (unsigned)blockIdx.x * (unsigned)cols;
  const unsigned c1 = min((unsigned)n, c0 + (unsigned)cols);
  unsigned long long best = BL_KEY_EMPTY;
  float bnd = __builtin_inff();
  for (unsigned j0 = c0 + tid; j0 < c1; j0 += 256u * CHAIN_BATCH) {
    unsigned played[CHAIN_BATCH];
    float4 b[CHAIN_BATCH];
    double2 pb[CHAIN_BATCH];
    int tg[CHAIN_BATCH];
#pragma unroll
    for (int u = 0; u < CHAIN_BATCH; ++u) {
      const unsigned j = j0 + 256u * u < c1 ? j0 + 256u * u : j0;
      played[u] = bits[j >> 5];
      b[u] = vecs[j];
      pb[u] = COSINE ? prep[j] : make_double2(0.0, 0.0);
      tg[u] = TAGS ? tags[j] : -1;
    }
#pragma unroll
    for (int u = 0; u < CHAIN_BATCH; ++u) {
      const unsigned j = j0 + 256u * u;
      if (j < c1 && !((played[u] >> (j & 31u)) & 1u))
        mix_visit<COSINE, TAGS>(a, pa, b[u], pb[u], (int)j, tg[u], hist, best, bnd);
    }
  }
  best = chain_wave_min(best);
  if (lane == 0) wmin[wave] = best;
  __syncthreads();
  if (tid != 0) return;
  const unsigned long long m = min(min(wmin[0], wmin[1]), min(wmin[2], wmin[3]));
  if (m != BL_KEY_EMPTY) (void)__hip_atomic_fetch_min(&st->best, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  /* the min has been performed before the arrival is counted */
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const unsigned ticket = __hip_atomic_fetch_add(&st->count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (ticket != gridDim.x - 1u) return;
  /* every slice's min was performed before its add, and every add before this one returned */
  const unsigned long long key = __hip_atomic_exchange(&st->best, BL_KEY_EMPTY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&st->count, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (key == BL_KEY_EMPTY) { /* no song is allowed: the chain has ended, the row keeps k_mix_init's padding */
    __hip_atomic_store(&st->cur, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  const int pick = (int)(unsigned)key;
  atomicOr(bits_all + (size_t)c * words + (pick >> 5), 1u << (pick & 31));
  out_order[(size_t)c * length + t] = pick;
  out_value[(size_t)c * length + t] =
      bl_value<COSINE>(a, pa, vecs[pick], COSINE ? prep[pick] : make_double2(0.0, 0.0));
  if (TAGS) { /* every workgroup of this launch has read the history before it arrived */
    hist.push(tags[pick], gap);
#pragma unroll
    for (int k = 0; k < BL_AMD_MIX_MAX_GAP; ++k)
      __hip_atomic_store(&st->hist[k], hist.h[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __hip_atomic_store(&st->cur, pick, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

/* ------------------------------------------------------------------------- */
/* k_radius_*, k_groups_*: fixed-radius neighbourhoods (bl_amd_radius_*, bl_amd_groups_*) */
/* Song j is within the radius of query i when the matrix entry passes a plain f32 compare: bl_distance <= radius or
 * bl_cosine_similarity >= radius.  The distance is decided on the squared sum: the correctly rounded root is monotone,
 * so rn(sqrt(s)) <= radius exactly when s <= s_max, the largest f32 whose rounded root is <= radius, which the host
 * computes once per call (bl_amd_radius_bound) — no root in the count pass, and a NaN sum fails the compare as the NaN
 * entry would.  The cosine compares bl_cosine's f32.  `bound` is s_max or the cosine radius.
 *
 * Layout: k_knn's.  A wave owns RAD_QPW queries (wave-uniform vectors in VGPRs) and walks 64 candidate columns per
 * step in ascending order; a query's hits of a step are one ballot, from which the tail lanes of the last step and
 * the query's own column are masked off as scalars.  Count adds the popcount; fill writes the hit lanes at the row's
 * running base plus their rank among the hits, which is ascending song order.  With few query rows the columns are
 * split over blockIdx.y: a split's count goes to part[row * n_split + split], and fill starts a split at the row's
 * offset plus the counts of the splits before it.  Every count is an integer function of the predicate alone, so the
 * result depends neither on the row range nor on the split. */
#define RAD_QPW 8   /* queries per wave */
#define RAD_WAVES 4 /* waves per workgroup */

template <bool COSINE>
__device__ __forceinline__ void radius_load_queries(const float4 *__restrict__ vecs, const double2 *__restrict__ prep,
                                                    int row0, int nq, float4 (&a)[RAD_QPW], double2 (&pa)[RAD_QPW]) {
#pragma unroll
  for (int q = 0; q < RAD_QPW; ++q) {
    const int row = row0 + min(q, nq - 1);
    a[q] = vecs[row];
    pa[q] = COSINE ? prep[row] : make_double2(0.0, 0.0);
    /* in VGPRs, as in k_knn: as scalars they crowd the SGPR file in the candidate loop */
    asm volatile("" : "+v"(a[q].x), "+v"(a[q].y), "+v"(a[q].z), "+v"(a[q].w));
    if (COSINE) asm volatile("" : "+v"(pa[q].x), "+v"(pa[q].y));
  }
}

/* m: bl_measure of the pair */
template <bool COSINE> __device__ __forceinline__ bool radius_within(float m, float bound) {
  return COSINE ? m >= bound : m <= bound;
}

/* the hit lanes of query `row` among the columns j0 .. j0 + 63; vmask: the lanes whose column exists.  CROSS: no
 * column is the query's own, so the hits are the ballot under the tail mask alone */
template <bool COSINE, bool CROSS>
__device__ __forceinline__ unsigned long long radius_hits(float m, float bound, unsigned long long vmask, int row, int j0) {
  unsigned long long hits = __ballot(radius_within<COSINE>(m, bound)) & vmask;
  if (!CROSS) {
    const unsigned self = (unsigned)(row - j0);
    if (self < 64u) hits &= ~(1ull << self);
  }
  return hits;
}

/* grid (query tiles of RAD_WAVES * RAD_QPW rows, n_split); part[row * n_split + split] = hits of the split.  Query r
 * is qvecs[row_begin + r] with its prep qprep[row_begin + r], as in k_knn: the self form (CROSS = false) is launched
 * with the library as its own query array; the cross form's queries (bl_amd_cross_radius_*_device) start at row 0.
 * k_radius_offsets and k_radius_split_scan serve both forms. */
template <bool COSINE, bool CROSS>
__global__ __launch_bounds__(256) void k_radius_count(const float4 *__restrict__ qvecs, const double2 *__restrict__ qprep,
                                                      const float4 *__restrict__ vecs, const double2 *__restrict__ prep,
                                                      int n, int row_begin, int n_rows, int cols, int n_split,
                                                      float bound, unsigned *__restrict__ part) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r0 = (blockIdx.x * RAD_WAVES + wave) * RAD_QPW;
  if (r0 >= n_rows) return;
  const int nq = min(RAD_QPW, n_rows - r0);
  const int c0 = blockIdx.y * cols, c1 = min(n, c0 + cols);
  const int q0 = (CROSS ? 0 : row_begin) + r0; /* the wave's first row in qvecs */
  float4 a[RAD_QPW];
  double2 pa[RAD_QPW];
  radius_load_queries<COSINE>(qvecs, qprep, q0, nq, a, pa);
  unsigned cnt[RAD_QPW];
#pragma unroll
  for (int q = 0; q < RAD_QPW; ++q) cnt[q] = 0;
  int jn = min(c0 + lane, c1 - 1);
  float4 b = vecs[jn];
  double2 pb = COSINE ? prep[jn] : make_double2(0.0, 0.0);
  for (int j0 = c0; j0 < c1; j0 += 64) {
    const float4 bc = b;
    const double2 pbc = pb;
    jn = min(j0 + 64 + lane, c1 - 1); /* the next step's column, fetched under this step's arithmetic */
    b = vecs[jn];
    if (COSINE) pb = prep[jn];
    const unsigned long long vmask = __ballot(j0 + lane < c1);
#pragma unroll
    for (int q = 0; q < RAD_QPW; ++q) /* rows past nq repeat the last query; their counts are not stored */
      cnt[q] += __popcll(radius_hits<COSINE, CROSS>(bl_measure<COSINE>(a[q], pa[q], bc, pbc), bound, vmask,
                                                    q0 + q, j0));
  }
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < RAD_QPW; ++q)
      if (q < nq) part[(size_t)(r0 + q) * n_split + blockIdx.y] = cnt[q];
  }
}

/* offset[r] = hits of the rows before r, offset[n_rows] = the total, from the rows' counts: one workgroup, thread t
 * owns a contiguous run of rows, the runs' sums are scanned through LDS, int64 throughout */
__global__ __launch_bounds__(1024) void k_radius_offsets(const unsigned *__restrict__ counts, int n_rows,
                                                         long long *__restrict__ offset) {
  __shared__ long long run_sum[1024];
  const int t = threadIdx.x;
  const long long per = ((long long)n_rows + 1023) / 1024;
  const long long r_lo = min((long long)t * per, (long long)n_rows), r_hi = min(r_lo + per, (long long)n_rows);
  long long sum = 0;
  for (long long r = r_lo; r < r_hi; ++r) sum += counts[r];
  run_sum[t] = sum;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) { /* inclusive scan */
    const long long add = t >= d ? run_sum[t - d] : 0;
    __syncthreads();
    run_sum[t] += add;
    __syncthreads();
  }
  long long run = run_sum[t] - sum;
  for (long long r = r_lo; r < r_hi; ++r) {
    offset[r] = run;
    run += counts[r];
  }
  if (t == 1023) offset[n_rows] = run_sum[1023];
}

/* column split, one wave per row: the row's per-split counts into the exclusive prefix fill starts each split at,
 * and their sum into rowsum[r] */
__global__ __launch_bounds__(256) void k_radius_split_scan(unsigned *__restrict__ part, int n_rows, int n_split,
                                                           unsigned *__restrict__ rowsum) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n_rows) return;
  unsigned *p = part + (size_t)r * n_split;
  unsigned run = 0;
  for (int s0 = 0; s0 < n_split; s0 += 64) {
    const int s = s0 + lane;
    const unsigned c = s < n_split ? p[s] : 0u;
    unsigned x = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned y = __shfl_up(x, d);
      if (lane >= d) x += y;
    }
    if (s < n_split) p[s] = run + x - c;
    run += __shfl(x, 63);
  }
  if (lane == 0) rowsum[r] = run;
}

/* grid as k_radius_count; row r's hits of split y go to out_*[offset[r] + before[r * n_split + y] ...] in ascending
 * song order (before == nullptr: one split).  The stored value is computed from the measure that decided the hit. */
template <bool COSINE, bool VALUES, bool CROSS>
__global__ __launch_bounds__(256) void k_radius_fill(const float4 *__restrict__ qvecs, const double2 *__restrict__ qprep,
                                                     const float4 *__restrict__ vecs, const double2 *__restrict__ prep,
                                                     int n, int row_begin, int n_rows, int cols, int n_split, float bound,
                                                     const unsigned *__restrict__ before,
                                                     const long long *__restrict__ offset, int32_t *__restrict__ out_index,
                                                     float *__restrict__ out_value) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r0 = (blockIdx.x * RAD_WAVES + wave) * RAD_QPW;
  if (r0 >= n_rows) return;
  const int nq = min(RAD_QPW, n_rows - r0);
  const int c0 = blockIdx.y * cols, c1 = min(n, c0 + cols);
  const int q0 = (CROSS ? 0 : row_begin) + r0; /* the wave's first row in qvecs */
  float4 a[RAD_QPW];
  double2 pa[RAD_QPW];
  radius_load_queries<COSINE>(qvecs, qprep, q0, nq, a, pa);
  long long base[RAD_QPW];
#pragma unroll
  for (int q = 0; q < RAD_QPW; ++q) {
    const size_t r = (size_t)(r0 + min(q, nq - 1));
    base[q] = offset[r] + (before ? (long long)before[r * n_split + blockIdx.y] : 0);
  }
  const unsigned long long below = (1ull << lane) - 1ull;
  int jn = min(c0 + lane, c1 - 1);
  float4 b = vecs[jn];
  double2 pb = COSINE ? prep[jn] : make_double2(0.0, 0.0);
  for (int j0 = c0; j0 < c1; j0 += 64) {
    const float4 bc = b;
    const double2 pbc = pb;
    jn = min(j0 + 64 + lane, c1 - 1);
    b = vecs[jn];
    if (COSINE) pb = prep[jn];
    const unsigned long long vmask = __ballot(j0 + lane < c1);
#pragma unroll
    for (int q = 0; q < RAD_QPW; ++q) {
      if (q >= nq) break;
      const float m = bl_measure<COSINE>(a[q], pa[q], bc, pbc);
      const unsigned long long hits = radius_hits<COSINE, CROSS>(m, bound, vmask, q0 + q, j0);
      if (hits == 0) continue;
      if ((hits >> lane) & 1ull) {
        const long long pos = base[q] + __popcll(hits & below);
        out_index[pos] = j0 + lane;
        if (VALUES) out_value[pos] = bl_value_of<COSINE>(m);
      }
      base[q] += __popcll(hits);
    }
  }
}

/* Duplicate groups: the weakly connected components of the "within the radius" graph, by a lock-free union-find on
 * the output itself.  parent[x] <= x always; only roots (parent[r] == r) are hooked, the larger root under the
 * smaller by a compare-and-swap that is retried with the value found when it loses, so the root of a tree is the
 * smallest index of its component.  Reads are agent-scope atomic loads: a value read was the entry's at some time,
 * and an entry that has stopped being a root never becomes one again, so an out-of-date read costs a retry, never
 * a wrong hook.  Path halving stores an ancestor over an ancestor, which keeps both properties. */
__device__ __forceinline__ int groups_load(const int *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int groups_find(int *parent, int x) {
  for (;;) {
    const int p = groups_load(parent + x);
    if (p == x) return x;
    const int g = groups_load(parent + p);
    if (g == p) return p;
    __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = g;
  }
}

__device__ __forceinline__ void groups_union(int *parent, int x, int y) {
  /* two entries that hold the same value are in that song's tree: nothing to do (the dense case ends here) */
  if (groups_load(parent + x) == groups_load(parent + y)) return;
  for (;;) {
    x = groups_find(parent, x);
    y = groups_find(parent, y);
    if (x == y) return;
    const int hi = max(x, y), lo = min(x, y);
    int seen = hi;
    if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT))
      return;
    x = seen; /* hi was hooked under `seen` in between: join that tree with lo's */
    y = lo;
  }
}

__global__ __launch_bounds__(256) void k_groups_init(int *__restrict__ parent, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) parent[i] = i;
}

/* grid as k_radius_count over all n rows.  Both matrices are bitwise symmetric (bl_dist_sq squares differences;
 * bl_cosine multiplies commutatively and adds in component order), so a wave visits the columns above its rows only. */
template <bool COSINE>
__global__ __launch_bounds__(256) void k_groups_union(const float4 *__restrict__ vecs, const double2 *__restrict__ prep,
                                                      int n, int cols, float bound, int *parent) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r0 = (blockIdx.x * RAD_WAVES + wave) * RAD_QPW;
  if (r0 >= n) return;
  const int nq = min(RAD_QPW, n - r0);
  const int c1 = min(n, (int)blockIdx.y * cols + cols);
  const int c0 = max((int)blockIdx.y * cols, (r0 + 1) & ~63); /* cols is a multiple of 64 */
  if (c0 >= c1) return;
  float4 a[RAD_QPW];
  double2 pa[RAD_QPW];
  radius_load_queries<COSINE>(vecs, prep, r0, nq, a, pa);
  for (int j0 = c0; j0 < c1; j0 += 64) {
    const int j = j0 + lane;
    const int jj = min(j, c1 - 1);
    const float4 b = vecs[jj];
    const double2 pb = COSINE ? prep[jj] : make_double2(0.0, 0.0);
#pragma unroll
    for (int q = 0; q < RAD_QPW; ++q) {
      if (q >= nq) break;
      const int row = r0 + q;
      if (j < c1 && j > row && radius_within<COSINE>(bl_measure<COSINE>(a[q], pa[q], b, pb), bound))
        groups_union(parent, row, j);
    }
  }
}

/* after the union launch: every entry to its root */
__global__ __launch_bounds__(256) void k_groups_compress(int *parent, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int x = i;
  for (;;) {
    const int p = groups_load(parent + x);
    if (p == x) break;
    x = p;
  }
  __hip_atomic_store(parent + i, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

/* ------------------------------------------------------------------------- */
/* launch layer                                                                 */

int blk_query_configure_device(void) {
  for (const void *fn : {reinterpret_cast<const void *>(k_chain<false, true>),
                         reinterpret_cast<const void *>(k_chain<true, true>),
                         reinterpret_cast<const void *>(k_mix<false, true, false>),
                         reinterpret_cast<const void *>(k_mix<false, true, true>),
                         reinterpret_cast<const void *>(k_mix<true, true, false>),
                         reinterpret_cast<const void *>(k_mix<true, true, true>)})
    BL_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, CHAIN_LDS_MAX));
  return BL_OK;
}

/* Column split of a call whose waves own `qpw` query rows each: one split while the query waves alone fill the chip
 * (16 per CU), else enough splits to reach that many waves, each of at least `min_cols` columns.  cols is a multiple
 * of 64.  kNN: 4 096 columns at least (a split's list fills with its first k candidates, so short splits would spend
 * their time filling); radius and groups: 1 024. */
void blk_split_plan(int n, int n_rows, int n_cu, int qpw, int min_cols, int *n_split, int *cols) {
  const long long waves = ((long long)n_rows + qpw - 1) / qpw;
  const long long target = (long long)n_cu * 16;
  long long split = 1;
  if (waves < target) split = std::min(std::min((target + waves - 1) / waves, std::max(1LL, (long long)n / min_cols)), 1024LL);
  *cols = (int)((((long long)n + split - 1) / split + 63) / 64 * 64);
  *n_split = (int)(((long long)n + *cols - 1) / *cols);
}

#define RAD_SPLIT_MIN_COLS 1024 /* KNN_SPLIT_MIN_COLS: bl_launch.h, the descriptor kNN splits by it too */

/* the cosine prep sits at the front of every query's scratch: double2[n] rounded up to 256 bytes, nothing otherwise */
static size_t prep_bytes(int n, bool cosine) {
  return cosine ? (sizeof(double2) * (size_t)n + 255) / 256 * 256 : 0;
}

/* fills it (cosine only) and returns it, nullptr for the distance */
static double2 *launch_prep(hipStream_t s, const float4 *v, int n, bool cosine, void *d_scratch) {
  if (!cosine) return nullptr;
  double2 *prep = static_cast<double2 *>(d_scratch);
  hipLaunchKernelGGL(k_knn_prep, dim3((n + 255) / 256), dim3(256), 0, s, v, n, prep);
  return prep;
}

/* The two sides of a query.  The queries are q[row_begin .. row_begin + n_rows).  A cross query (d_queries != nullptr:
 * n_q vectors outside the library, row_begin = 0) keeps the queries' prep behind the library's.  The self forms have
 * d_queries == nullptr: q is v, the library as its own query array, and qprep is prep; the kernels only read through
 * either name, so the same array under two __restrict__ pointers is as sound as a cross call whose queries alias the
 * library.  `cross` picks the kernels' CROSS instantiation and is derived here, nowhere else. */
struct query_preps {
  const float4 *q;
  const double2 *prep, *qprep;
  char *rest;
  bool cross;
};

static size_t cross_prep_bytes(const void *d_queries, int n_q, bool cosine) {
  return d_queries ? prep_bytes(n_q, cosine) : 0;
}

/* fills what the cosine needs and returns where the rest of the scratch begins */
static query_preps launch_preps(hipStream_t s, const struct force_vector_s *d_queries, int n_q, const float4 *v, int n,
                                bool cosine, void *d_scratch) {
  query_preps p;
  char *base = static_cast<char *>(d_scratch);
  p.cross = d_queries != nullptr;
  p.q = p.cross ? reinterpret_cast<const float4 *>(d_queries) : v;
  p.prep = launch_prep(s, v, n, cosine, base);
  p.qprep = p.cross ? launch_prep(s, p.q, n_q, cosine, base + prep_bytes(n, cosine)) : p.prep;
  p.rest = base + prep_bytes(n, cosine) + cross_prep_bytes(d_queries, n_q, cosine);
  return p;
}

size_t blk_knn_scratch_bytes(const struct force_vector_s *d_queries, int n, int n_rows, int k, bool cosine, int n_cu) {
  int n_split, cols;
  blk_split_plan(n, n_rows, n_cu, KNN_QPW, KNN_SPLIT_MIN_COLS, &n_split, &cols);
  const size_t part = n_split > 1 ? sizeof(unsigned long long) * (size_t)n_rows * n_split * k : 0;
  return prep_bytes(n, cosine) + cross_prep_bytes(d_queries, n_rows, cosine) + part;
}

template <int KW, bool COSINE>
static void knn_launch(hipStream_t s, const float4 *v, const query_preps &p, int n, int row_begin, int n_rows, int k,
                       int n_split, int cols, unsigned long long *part, int32_t *d_index, float *d_value) {
  const int per_block = KNN_WAVES * KNN_QPW;
  const dim3 grid((n_rows + per_block - 1) / per_block, n_split), merge_grid((n_rows + KNN_WAVES - 1) / KNN_WAVES);
  const dim3 block(64 * KNN_WAVES);
  const auto knn = p.cross ? k_knn<KW, COSINE, true> : k_knn<KW, COSINE, false>;
  const auto merge = p.cross ? k_knn_merge<KW, COSINE, true> : k_knn_merge<KW, COSINE, false>;
  hipLaunchKernelGGL(knn, grid, block, 0, s, p.q, p.qprep, v, p.prep, n, row_begin, n_rows, k, cols, n_split, part,
                     d_index, d_value);
  if (n_split > 1)
    hipLaunchKernelGGL(merge, merge_grid, block, 0, s, p.q, p.qprep, v, p.prep, row_begin, n_rows, k, n_split, part,
                       d_index, d_value);
}

int blk_knn(hipStream_t s, const struct force_vector_s *d_queries, const struct force_vector_s *d_vecs, int n,
            int row_begin, int n_rows, int k, bool cosine, int n_cu, void *d_scratch, int32_t *d_index, float *d_value) {
  if (d_queries && row_begin) return BL_UNEXPECTED;
  const float4 *v = reinterpret_cast<const float4 *>(d_vecs);
  int n_split, cols;
  blk_split_plan(n, n_rows, n_cu, KNN_QPW, KNN_SPLIT_MIN_COLS, &n_split, &cols);
  const query_preps p = launch_preps(s, d_queries, n_rows, v, n, cosine, d_scratch);
  unsigned long long *part = n_split > 1 ? reinterpret_cast<unsigned long long *>(p.rest) : nullptr;
  if (k > 64) {
    if (cosine) knn_launch<2, true>(s, v, p, n, row_begin, n_rows, k, n_split, cols, part, d_index, d_value);
    else knn_launch<2, false>(s, v, p, n, row_begin, n_rows, k, n_split, cols, part, d_index, d_value);
  } else {
    if (cosine) knn_launch<1, true>(s, v, p, n, row_begin, n_rows, k, n_split, cols, part, d_index, d_value);
    else knn_launch<1, false>(s, v, p, n, row_begin, n_rows, k, n_split, cols, part, d_index, d_value);
  }
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}

/* Shape of a chain call (see k_chain).  Column split (2) when the corpus is large enough for a step's scan by one
 * workgroup to cost more than a launch boundary with its two atomics, and the chains are few enough that their
 * launches do not: the constants are the measured crossovers of DESIGN §4.7 (tools/chain_bench.py).  `force`: 0 = this
 * rule, 1 / 2 = that shape (tools and tests). */
#define CHAIN_SPLIT_MIN_N 8192      /* fewer songs: one workgroup per chain */
#define CHAIN_SPLIT_FILL 2          /* split while n_chains * this <= CUs */
#define CHAIN_SPLIT_COLS 2048       /* columns of a slice, at least */
#define CHAIN_SPLIT_MAX_GROUPS 128  /* slices of a chain, at most: every slice costs two atomics on the chain's state */
#define CHAIN_SPLIT_MAX_CHAINS 65535 /* gridDim.y */

struct chain_plan {
  int shape;
  /* 1 */
  int lb, words;
  bool lds_bits;
  size_t lds_bytes;
  /* 2 */
  int groups, cols, bit_words;
};

static chain_plan chain_make_plan(int n, int n_chains, int n_cu, int force) {
  chain_plan p{};
  p.shape = (n >= CHAIN_SPLIT_MIN_N && (long long)n_chains * CHAIN_SPLIT_FILL <= n_cu) ? 2 : 1;
  if (force == 1 || force == 2) p.shape = force;
  if (n_chains > CHAIN_SPLIT_MAX_CHAINS) p.shape = 1;
  if (p.shape == 1) {
    p.lb = n <= 16384 ? 8 : 10;
    const long long per_lane = ((long long)n + (1 << p.lb) - 1) >> p.lb;
    p.words = (int)((per_lane + 31) / 32);
    p.lds_bytes = CHAIN_LDS_HEAD + sizeof(unsigned) * ((size_t)p.words << p.lb);
    p.lds_bits = p.lds_bytes <= CHAIN_LDS_MAX;
    if (!p.lds_bits) p.lds_bytes = CHAIN_LDS_HEAD;
  } else {
    const long long want = ((long long)n + CHAIN_SPLIT_COLS - 1) / CHAIN_SPLIT_COLS;
    const long long cap = std::min((long long)CHAIN_SPLIT_MAX_GROUPS, std::max(1LL, 4LL * n_cu / n_chains));
    const long long groups = std::max(1LL, std::min(want, cap));
    p.cols = (int)((((long long)n + groups - 1) / groups + 255) / 256 * 256);
    p.groups = (int)(((long long)n + p.cols - 1) / p.cols);
    p.bit_words = (int)(((long long)n + 31) / 32);
  }
  return p;
}

int blk_chain_shape(int n, int n_chains, int n_cu, int force) { return chain_make_plan(n, n_chains, n_cu, force).shape; }

size_t blk_chain_scratch_bytes(int n, int n_chains, bool cosine, int n_cu, int force) {
  const chain_plan p = chain_make_plan(n, n_chains, n_cu, force);
  size_t bytes = prep_bytes(n, cosine);
  if (p.shape == 1) {
    if (!p.lds_bits) bytes += sizeof(unsigned) * ((size_t)p.words << p.lb) * n_chains;
  } else {
    bytes += sizeof(chain_state) * (size_t)n_chains + sizeof(unsigned) * (size_t)p.bit_words * n_chains;
  }
  return bytes;
}

template <bool COSINE>
static void chain_launch(hipStream_t s, const chain_plan &p, const float4 *v, const double2 *prep, void *rest, int n,
                         const int32_t *d_seeds, int n_chains, int length, int32_t *d_order, float *d_value) {
  if (p.shape == 1) {
    unsigned *g_bits = static_cast<unsigned *>(rest);
    if (p.lds_bits)
      hipLaunchKernelGGL((k_chain<COSINE, true>), dim3(n_chains), dim3(1 << p.lb), p.lds_bytes, s, v, prep, n, d_seeds,
                         length, p.lb, p.words, g_bits, d_order, d_value);
    else
      hipLaunchKernelGGL((k_chain<COSINE, false>), dim3(n_chains), dim3(1 << p.lb), p.lds_bytes, s, v, prep, n,
                         d_seeds, length, p.lb, p.words, g_bits, d_order, d_value);
    return;
  }
  chain_state *state = static_cast<chain_state *>(rest);
  unsigned *bits = reinterpret_cast<unsigned *>(state + n_chains);
  const int fill = std::max(p.bit_words, length);
  hipLaunchKernelGGL((k_chain_init<COSINE>), dim3(std::min(256, (fill + 255) / 256), n_chains), dim3(256), 0, s, v,
                     prep, n, d_seeds, length, p.bit_words, state, bits, d_order, d_value);
  const int steps = std::min(length, n);
  for (int t = 1; t < steps; ++t)
    hipLaunchKernelGGL((k_chain_step<COSINE>), dim3(p.groups, n_chains), dim3(256), 0, s, v, prep, n, p.cols, t,
                       length, p.bit_words, state, bits, d_order, d_value);
}

int blk_chain(hipStream_t s, const struct force_vector_s *d_vecs, int n, const int32_t *d_seeds, int n_chains,
              int length, bool cosine, int n_cu, int force, void *d_scratch, int32_t *d_order, float *d_value) {
  const float4 *v = reinterpret_cast<const float4 *>(d_vecs);
  const chain_plan p = chain_make_plan(n, n_chains, n_cu, force);
  void *rest = static_cast<char *>(d_scratch) + prep_bytes(n, cosine);
  const double2 *prep = launch_prep(s, v, n, cosine, d_scratch);
  if (cosine) chain_launch<true>(s, p, v, prep, rest, n, d_seeds, n_chains, length, d_order, d_value);
  else chain_launch<false>(s, p, v, prep, rest, n, d_seeds, n_chains, length, d_order, d_value);
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}

/* Chains under rules (k_mix): the plan, the shapes and the scratch layout are the chain's (sizeof(mix_state) ==
 * sizeof(chain_state)).  d_tags is nullptr when gap == 0, which picks the kernels without the tag rule. */
size_t blk_mix_scratch_bytes(int n, int n_chains, bool cosine, int n_cu, int force) {
  return blk_chain_scratch_bytes(n, n_chains, cosine, n_cu, force);
}

template <bool COSINE, bool TAGS>
static void mix_launch(hipStream_t s, const chain_plan &p, const float4 *v, const double2 *prep, void *rest, int n,
                       const int32_t *d_seeds, const float4 *q, int n_chains, int length, const int32_t *d_tags, int gap,
                       const unsigned char *d_exclude, int32_t *d_order, float *d_value) {
  if (p.shape == 1) {
    unsigned *g_bits = static_cast<unsigned *>(rest);
    if (p.lds_bits)
      hipLaunchKernelGGL((k_mix<COSINE, true, TAGS>), dim3(n_chains), dim3(1 << p.lb), p.lds_bytes, s, v, prep, n,
                         d_seeds, q, length, p.lb, p.words, d_tags, gap, d_exclude, g_bits, d_order, d_value);
    else
      hipLaunchKernelGGL((k_mix<COSINE, false, TAGS>), dim3(n_chains), dim3(1 << p.lb), p.lds_bytes, s, v, prep, n,
                         d_seeds, q, length, p.lb, p.words, d_tags, gap, d_exclude, g_bits, d_order, d_value);
    return;
  }
  mix_state *state = static_cast<mix_state *>(rest);
  unsigned *bits = reinterpret_cast<unsigned *>(state + n_chains);
  const int fill = std::max(n, length);
  hipLaunchKernelGGL((k_mix_init<COSINE>), dim3(std::min(256, (fill + 255) / 256), n_chains), dim3(256), 0, s, v, prep,
                     n, d_seeds, length, p.bit_words, d_tags, d_exclude, state, bits, d_order, d_value);
  const int steps = std::min(length, n);
  for (int t = q ? 0 : 1; t < steps; ++t) /* a vector seed's slot 0 is a step of its own, the query from q */
    hipLaunchKernelGGL((k_mix_step<COSINE, TAGS>), dim3(p.groups, n_chains), dim3(256), 0, s, v, prep, n, p.cols, t,
                       length, p.bit_words, d_tags, gap, t == 0 ? q : nullptr, state, bits, d_order, d_value);
}

int blk_mix(hipStream_t s, const struct force_vector_s *d_vecs, int n, const int32_t *d_seeds,
            const struct force_vector_s *d_seed_vecs, int n_chains, int length, bool cosine, const int32_t *d_tags,
            int gap, const uint8_t *d_exclude, int n_cu, int force, void *d_scratch, int32_t *d_order, float *d_value) {
  const float4 *v = reinterpret_cast<const float4 *>(d_vecs), *q = reinterpret_cast<const float4 *>(d_seed_vecs);
  const chain_plan p = chain_make_plan(n, n_chains, n_cu, force);
  void *rest = static_cast<char *>(d_scratch) + prep_bytes(n, cosine);
  const double2 *prep = launch_prep(s, v, n, cosine, d_scratch);
  const int32_t *tags = gap > 0 ? d_tags : nullptr;
  if (cosine) {
    if (tags) mix_launch<true, true>(s, p, v, prep, rest, n, d_seeds, q, n_chains, length, tags, gap, d_exclude, d_order, d_value);
    else mix_launch<true, false>(s, p, v, prep, rest, n, d_seeds, q, n_chains, length, tags, gap, d_exclude, d_order, d_value);
  } else {
    if (tags) mix_launch<false, true>(s, p, v, prep, rest, n, d_seeds, q, n_chains, length, tags, gap, d_exclude, d_order, d_value);
    else mix_launch<false, false>(s, p, v, prep, rest, n, d_seeds, q, n_chains, length, tags, gap, d_exclude, d_order, d_value);
  }
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}

size_t blk_radius_scratch_bytes(const struct force_vector_s *d_queries, int n, int n_rows, bool cosine, int n_cu) {
  int n_split, cols;
  blk_split_plan(n, n_rows, n_cu, RAD_QPW, RAD_SPLIT_MIN_COLS, &n_split, &cols);
  /* counts per (row, split), and with a column split the rows' sums behind them */
  return prep_bytes(n, cosine) + cross_prep_bytes(d_queries, n_rows, cosine) +
         sizeof(unsigned) * (size_t)n_rows * (n_split + (n_split > 1 ? 1 : 0));
}

static dim3 radius_grid(int n_rows, int n_split) {
  const int per_block = RAD_WAVES * RAD_QPW;
  return dim3((n_rows + per_block - 1) / per_block, n_split);
}

/* the per-(row, split) counts into p.rest, which is returned */
template <bool COSINE>
static unsigned *radius_count_launch(hipStream_t s, const float4 *v, const query_preps &p, int n, int row_begin,
                                     int n_rows, float bound, int n_split, int cols) {
  unsigned *part = reinterpret_cast<unsigned *>(p.rest);
  const auto count = p.cross ? k_radius_count<COSINE, true> : k_radius_count<COSINE, false>;
  hipLaunchKernelGGL(count, radius_grid(n_rows, n_split), dim3(64 * RAD_WAVES), 0, s, p.q, p.qprep, v, p.prep, n,
                     row_begin, n_rows, cols, n_split, bound, part);
  return part;
}

int blk_radius_count(hipStream_t s, const struct force_vector_s *d_queries, const struct force_vector_s *d_vecs, int n,
                     int row_begin, int n_rows, bool cosine, float bound, int n_cu, void *d_scratch,
                     long long *d_offset) {
  if (d_queries && row_begin) return BL_UNEXPECTED;
  const float4 *v = reinterpret_cast<const float4 *>(d_vecs);
  int n_split, cols;
  blk_split_plan(n, n_rows, n_cu, RAD_QPW, RAD_SPLIT_MIN_COLS, &n_split, &cols);
  const query_preps p = launch_preps(s, d_queries, n_rows, v, n, cosine, d_scratch);
  unsigned *part = cosine ? radius_count_launch<true>(s, v, p, n, row_begin, n_rows, bound, n_split, cols)
                          : radius_count_launch<false>(s, v, p, n, row_begin, n_rows, bound, n_split, cols);
  const unsigned *counts = part;
  if (n_split > 1) {
    unsigned *rowsum = part + (size_t)n_rows * n_split;
    hipLaunchKernelGGL(k_radius_split_scan, dim3((n_rows + 3) / 4), dim3(256), 0, s, part, n_rows, n_split, rowsum);
    counts = rowsum;
  }
  hipLaunchKernelGGL(k_radius_offsets, dim3(1), dim3(1024), 0, s, counts, n_rows, d_offset);
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}

/* One split: a row's list starts at its offset, nothing else is needed.  Column split: the per-split counts are
 * computed again here (the scratch may have served another call since the count), so fill depends on nothing but
 * its arguments. */
template <bool COSINE>
static void radius_fill_run(hipStream_t s, const struct force_vector_s *d_queries, const float4 *v, int n, int row_begin,
                            int n_rows, float bound, int n_cu, void *d_scratch, const long long *d_offset,
                            int32_t *d_index, float *d_value) {
  int n_split, cols;
  blk_split_plan(n, n_rows, n_cu, RAD_QPW, RAD_SPLIT_MIN_COLS, &n_split, &cols);
  const query_preps p = launch_preps(s, d_queries, n_rows, v, n, COSINE, d_scratch);
  unsigned *before = nullptr;
  if (n_split > 1) {
    before = radius_count_launch<COSINE>(s, v, p, n, row_begin, n_rows, bound, n_split, cols);
    hipLaunchKernelGGL(k_radius_split_scan, dim3((n_rows + 3) / 4), dim3(256), 0, s, before, n_rows, n_split,
                       before + (size_t)n_rows * n_split);
  }
  const dim3 grid = radius_grid(n_rows, n_split), block(64 * RAD_WAVES);
  const auto fill = d_value ? (p.cross ? k_radius_fill<COSINE, true, true> : k_radius_fill<COSINE, true, false>)
                            : (p.cross ? k_radius_fill<COSINE, false, true> : k_radius_fill<COSINE, false, false>);
  hipLaunchKernelGGL(fill, grid, block, 0, s, p.q, p.qprep, v, p.prep, n, row_begin, n_rows, cols, n_split, bound, before,
                     d_offset, d_index, d_value);
}

int blk_radius_fill(hipStream_t s, const struct force_vector_s *d_queries, const struct force_vector_s *d_vecs, int n,
                    int row_begin, int n_rows, bool cosine, float bound, int n_cu, void *d_scratch,
                    const long long *d_offset, int32_t *d_index, float *d_value) {
  if (d_queries && row_begin) return BL_UNEXPECTED;
  const float4 *v = reinterpret_cast<const float4 *>(d_vecs);
  if (cosine) radius_fill_run<true>(s, d_queries, v, n, row_begin, n_rows, bound, n_cu, d_scratch, d_offset, d_index, d_value);
  else radius_fill_run<false>(s, d_queries, v, n, row_begin, n_rows, bound, n_cu, d_scratch, d_offset, d_index, d_value);
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}

size_t blk_groups_scratch_bytes(int n, bool cosine) { return prep_bytes(n, cosine); }

int blk_groups(hipStream_t s, const struct force_vector_s *d_vecs, int n, bool cosine, float bound, int n_cu,
               void *d_scratch, int32_t *d_group) {
  const float4 *v = reinterpret_cast<const float4 *>(d_vecs);
  int n_split, cols;
  blk_split_plan(n, n, n_cu, RAD_QPW, RAD_SPLIT_MIN_COLS, &n_split, &cols);
  const dim3 flat((n + 255) / 256);
  hipLaunchKernelGGL(k_groups_init, flat, dim3(256), 0, s, d_group, n);
  const double2 *prep = launch_prep(s, v, n, cosine, d_scratch);
  if (cosine) {
    hipLaunchKernelGGL((k_groups_union<true>), radius_grid(n, n_split), dim3(64 * RAD_WAVES), 0, s, v, prep, n, cols,
                       bound, d_group);
  } else {
    hipLaunchKernelGGL((k_groups_union<false>), radius_grid(n, n_split), dim3(64 * RAD_WAVES), 0, s, v, prep, n, cols,
                       bound, d_group);
  }
  hipLaunchKernelGGL(k_groups_compress, flat, dim3(256), 0, s, d_group, n);
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}
