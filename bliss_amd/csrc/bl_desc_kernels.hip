/*
 * bl_desc_kernels.hip — gfx950 kernels and launch layer of the library-normalised descriptors (bl_amd_desc_*,
 * include/bliss_amd.h: bl_amd_desc, bl_amd_desc_range).  A descriptor is 32 int16, one 64-byte line per song, and the
 * squared distance of two of them an exact integer, so no result depends on the reduction order, the column split or
 * the row range.  Must be compiled with -ffp-contract=off, like every kernel file: the quantiser's f64 arithmetic is
 * unfused by contract.
 *
 * Kernels:
 *   k_desc_range, k_desc_range_finish  column-wise minimum, maximum and count of the finite entries
 *   k_desc_quantize                    one thread per entry: the header's f64 expression, ties to even
 *   k_desc_knn<KW, CROSS>              the k nearest descriptors of each query by (d^2, index), int8 matrix products
 *   k_desc_merge<KW>                   joins the partial lists of a column split, one wave per query
 *
 * Pair arithmetic.  q = 256 h + l with h = (q + 128) >> 8 in [-127, 127] and l the low byte of q as a signed byte
 * (|q| <= 32512 keeps h a signed byte), so with H and L the byte planes of a tile
 *     a . b = 65536 HH + 256 (HL + LH) + LL
 * as three exact int32 products: HL + LH is one v_mfma_i32_16x16x64_i8 with A = [h | l] and B = [l | h], HH and LL one
 * v_mfma_i32_16x16x32_i8 each.  |HH|, |LL| <= 32 * 128^2 = 2^19 and |HL + LH| <= 2 * 32 * 127 * 128 < 2^20.  Then
 * d^2 = |a|^2 + |b|^2 - 2 a . b in int64, the norms summed from the int16 themselves in the same kernel.
 *
 * Operand layout.  Lane group g = lane >> 4 loads the 16 bytes that hold dimensions 8 g .. 8 g + 7 of its vector, query
 * (A, row lane & 15) and candidate (B, column lane & 15) alike, and splits them into the planes h8 and l8 of 8 bytes.
 * BOTH operands of every product are laid out by that one rule — byte j of a group's K slice is dimension
 * 8 g + (j & 7), in the 16-byte slices the first 8 bytes [h | l] for A and [l | h] for B — so a product pairs equal
 * dimensions whatever order the hardware walks K in.  Result register r of lane (col, g): query row 4 g + r against
 * candidate col.
 *
 * Selection.  bl_topk.h: per query a sorted list across the lanes, its k-th key as the threshold, an LDS queue and a
 * bitonic merge.  The key is (d^2 << 27) | index (d^2 < 2^37, n < 2^27), the filter one 64-bit compare; a lane keeps the
 * thresholds of its four rows, and a tile none of whose 256 pairs passes costs one ballot.
 */
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bl_desc_pair.h"
#include "bl_launch.h"
#include "bl_topk.h"

#define DS_QPW 16       /* queries per wave: the rows of a tile */
#define DS_WAVES 4      /* waves per workgroup */
/* DS_TILE, DS_IDX_BITS, DS_IDX_MASK, ds_u64, ds_v4i: bl_desc_pair.h */

/* ------------------------------------------------------------------------- */
/* range                                                                       */

#define DS_RANGE_ROWS 8 /* rows of x a workgroup of 256 reads per pass: thread (row, column) = (tid >> 5, tid & 31) */

struct ds_range_part { float lo, hi; unsigned cnt; };

__device__ __forceinline__ bool ds_finite(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }

__device__ __forceinline__ void ds_range_join(ds_range_part &a, const ds_range_part b) {
  a.lo = b.lo < a.lo ? b.lo : a.lo;
  a.hi = b.hi > a.hi ? b.hi : a.hi;
  a.cnt += b.cnt;
}

/* workgroup b takes the rows b * 8 + (tid >> 5) + i * 8 * gridDim.x; part[b * 32 + c] = its share of column c */
__global__ __launch_bounds__(256) void k_desc_range(const float *__restrict__ x, int n, int d,
                                                    ds_range_part *__restrict__ part) {
  __shared__ ds_range_part sh[DS_RANGE_ROWS][BL_AMD_DESC_DIMS];
  const int c = threadIdx.x & 31, rr = threadIdx.x >> 5;
  ds_range_part p = {__builtin_inff(), -__builtin_inff(), 0u};
  if (c < d) {
    const long long stride = (long long)DS_RANGE_ROWS * gridDim.x;
    for (long long r = (long long)blockIdx.x * DS_RANGE_ROWS + rr; r < n; r += stride) {
      const float v = x[(size_t)r * d + c];
      if (ds_finite(v)) ds_range_join(p, ds_range_part{v, v, 1u});
    }
  }
  sh[rr][c] = p;
  __syncthreads();
  if (rr == 0) {
#pragma unroll
    for (int i = 1; i < DS_RANGE_ROWS; ++i) ds_range_join(p, sh[i][c]);
    part[(size_t)blockIdx.x * BL_AMD_DESC_DIMS + c] = p;
  }
}

/* one workgroup: the n_part shares of every column into the record; every byte of it is written */
__global__ __launch_bounds__(256) void k_desc_range_finish(const ds_range_part *__restrict__ part, int n_part,
                                                           bl_amd_desc_range *__restrict__ out) {
  __shared__ ds_range_part sh[DS_RANGE_ROWS][BL_AMD_DESC_DIMS];
  const int c = threadIdx.x & 31, rr = threadIdx.x >> 5;
  ds_range_part p = {__builtin_inff(), -__builtin_inff(), 0u};
  for (int i = rr; i < n_part; i += DS_RANGE_ROWS) ds_range_join(p, part[(size_t)i * BL_AMD_DESC_DIMS + c]);
  sh[rr][c] = p;
  __syncthreads();
  if (rr == 0) {
#pragma unroll
    for (int i = 1; i < DS_RANGE_ROWS; ++i) ds_range_join(p, sh[i][c]);
    const bool any = p.cnt != 0u;
    out->lo[c] = any && p.lo != 0.f ? p.lo : 0.f; /* a zero is stored as +0 */
    out->hi[c] = any && p.hi != 0.f ? p.hi : 0.f;
    out->n_finite[c] = p.cnt;
  }
}

/* ------------------------------------------------------------------------- */
/* quantise                                                                    */

/* the header's expression, operation by operation in f64 */
__device__ __forceinline__ int ds_quantize(float x, float lo, float hi, unsigned scale) {
  if (!(ds_finite(x) && ds_finite(lo) && ds_finite(hi) && hi > lo)) return 0;
  const double t = ((double)x - (double)lo) / ((double)hi - (double)lo);
  double u = 2.0 * t - 1.0;
  u = u < -1.0 ? -1.0 : u;
  u = u > 1.0 ? 1.0 : u;
  return (int)__builtin_rint(u * (double)scale);
}

/* thread i: entry (row, column) = (i >> 5, i & 31) of the output */
__global__ __launch_bounds__(256) void k_desc_quantize(const float *__restrict__ x, int n, int d,
                                                       const bl_amd_desc_range *__restrict__ range,
                                                       const blk_desc_scale scale, int16_t *__restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t row = i >> 5;
  const int c = (int)(i & 31);
  if (row >= (size_t)n) return;
  int q = 0;
  if (c < d) q = ds_quantize(x[row * d + c], range->lo[c], range->hi[c], scale.s[c]);
  out[i] = (int16_t)q;
}

/* ------------------------------------------------------------------------- */
/* kNN                                                                         */

/* ds_planes, ds_norm, ds_pack: bl_desc_pair.h, shared with the chains of bl_desc_chain_kernels.hip */

/* slots [0, k) of output row r from the sorted keys */
template <int KW>
__device__ __forceinline__ void ds_emit(const knn_top<KW> &t, int lane, int k, size_t r, int32_t *__restrict__ out_index,
                                        ds_u64 *__restrict__ out_d2) {
#pragma unroll
  for (int w = 0; w < KW; ++w) {
    const int slot = w * 64 + lane;
    if (slot >= k) continue;
    const ds_u64 key = w == 0 ? t.e0 : t.e1;
    const bool empty = key == BL_KEY_EMPTY;
    out_index[r * k + slot] = empty ? -1 : (int)((unsigned)key & DS_IDX_MASK);
    out_d2[r * k + slot] = empty ? BL_KEY_EMPTY : key >> DS_IDX_BITS;
  }
}

/* blockIdx.x: DS_WAVES * DS_QPW query rows, blockIdx.y: column split [y * cols, (y + 1) * cols).  n_split == 1: the
 * final lists go to out_index / out_d2; otherwise the first k keys of each list go to part[(row * n_split + split) * k].
 * Query r is qv[row_begin + r] (CROSS = false: qv is the library, and a query's own column is no candidate) or qv[r]
 * (CROSS = true: row_begin is not read, every column is a candidate).  A vector is four uint4. */
template <int KW, bool CROSS>
__global__ __launch_bounds__(256) void k_desc_knn(const uint4 *__restrict__ qv, const uint4 *__restrict__ lib, int n,
                                                  int row_begin, int n_rows, int k, int cols, int n_split,
                                                  ds_u64 *__restrict__ part, int32_t *__restrict__ out_index,
                                                  ds_u64 *__restrict__ out_d2) {
  __shared__ ds_u64 queue[DS_WAVES][DS_QPW][64];
  __shared__ ds_u64 qnorm[DS_WAVES][DS_QPW];
  const int lane = threadIdx.x & 63, col = lane & 15, grp = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r0 = (blockIdx.x * DS_WAVES + wave) * DS_QPW;
  if (r0 >= n_rows) return;
  const int nq = min(DS_QPW, n_rows - r0);
  const int c0 = blockIdx.y * cols, c1 = min(n, c0 + cols);
  const int q0 = (CROSS ? 0 : row_begin) + r0; /* the wave's first row in qv */
  /* A: row `col` of the tile is query q0 + col (the last one again behind the end) */
  const uint4 aw = qv[(size_t)(q0 + min(col, nq - 1)) * 4 + grp];
  int ah[2], al[2];
  ds_planes(aw, ah, al);
  const ds_v4i a64 = {ah[0], ah[1], al[0], al[1]};
  const long ahh = ds_pack(ah), all_ = ds_pack(al);
  {
    const ds_u64 an = ds_norm(aw);
    if (grp == 0) qnorm[wave][col] = an;
    bl_wave_sync();
  }
  ds_u64 na[4], thr4[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    na[r] = qnorm[wave][4 * grp + r];
    thr4[r] = BL_KEY_EMPTY;
  }
  knn_top<KW> top[DS_QPW];
#pragma unroll
  for (int q = 0; q < DS_QPW; ++q) top[q].init();
  const ds_v4i zero = {0, 0, 0, 0};
  uint4 bw = lib[(size_t)min(c0 + col, c1 - 1) * 4 + grp];
  for (int j0 = c0; j0 < c1; j0 += DS_TILE) {
    const int j = j0 + col;
    const bool valid = j < c1;
    const uint4 cur = bw;
    bw = lib[(size_t)min(j + DS_TILE, c1 - 1) * 4 + grp]; /* the next tile's, in flight under this one's products */
    int bh[2], bl[2];
    ds_planes(cur, bh, bl);
    const ds_v4i b64 = {bl[0], bl[1], bh[0], bh[1]};
    const ds_u64 nb = ds_norm(cur);
    const ds_v4i x = __builtin_amdgcn_mfma_i32_16x16x64_i8(a64, b64, zero, 0, 0, 0);
    const ds_v4i hh = __builtin_amdgcn_mfma_i32_16x16x32_i8(ahh, ds_pack(bh), zero, 0, 0, 0);
    const ds_v4i ll = __builtin_amdgcn_mfma_i32_16x16x32_i8(all_, ds_pack(bl), zero, 0, 0, 0);
    ds_u64 key[4];
    bool pr[4], any = false;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long long dot = ((long long)hh[r] << 16) + ((long long)x[r] << 8) + (long long)ll[r];
      const ds_u64 d2 = na[r] + nb - (ds_u64)(2 * dot);
      key[r] = (d2 << DS_IDX_BITS) | (unsigned)j;
      const int row = 4 * grp + r;
      pr[r] = (int)valid & (int)(row < nq) & (int)(CROSS || j != q0 + row) & (int)(key[r] < thr4[r]); /* no branches */
      any |= pr[r];
    }
    if (__ballot(any) == 0) continue;
#pragma unroll
    for (int q = 0; q < DS_QPW; ++q) {
      const bool mine = grp == (q >> 2);
      top[q].push(mine && pr[q & 3], key[q & 3], queue[wave][q], lane, k);
      if (mine) thr4[q & 3] = top[q].thr;
    }
  }
#pragma unroll
  for (int q = 0; q < DS_QPW; ++q) {
    if (q < nq) { /* not a break: the loop must unroll for top[] to stay in registers */
      top[q].finish(queue[wave][q], lane, k);
      const size_t r = (size_t)(r0 + q);
      if (n_split == 1) {
        ds_emit<KW>(top[q], lane, k, r, out_index, out_d2);
      } else {
        ds_u64 *dst = part + (r * n_split + blockIdx.y) * k;
#pragma unroll
        for (int w = 0; w < KW; ++w)
          if (w * 64 + lane < k) dst[w * 64 + lane] = w == 0 ? top[q].e0 : top[q].e1;
      }
    }
  }
}

/* one wave per query row: the n_split partial lists of the row as one stream of keys through the filter.  The keys
 * carry value and index, so no vector is read. */
template <int KW>
__global__ __launch_bounds__(256) void k_desc_merge(int n_rows, int k, int n_split, const ds_u64 *__restrict__ part,
                                                    int32_t *__restrict__ out_index, ds_u64 *__restrict__ out_d2) {
  __shared__ ds_u64 queue[DS_WAVES][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = blockIdx.x * DS_WAVES + wave;
  if (r >= n_rows) return;
  const ds_u64 *src = part + (size_t)r * n_split * k;
  const int total = n_split * k;
  knn_top<KW> top;
  top.init();
  for (int o = 0; o < total; o += 4 * 64) {
    ds_u64 key[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = o + u * 64 + lane;
      key[u] = i < total ? src[i] : BL_KEY_EMPTY;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) top.push(key[u] < top.thr, key[u], queue[wave], lane, k);
  }
  top.finish(queue[wave], lane, k);
  ds_emit<KW>(top, lane, k, (size_t)r, out_index, out_d2);
}

/* ========================================================================= */
/* launchers (declared in bl_launch.h)                                        */

static int ds_range_blocks(int n, int n_cu) {
  const long long want = ((long long)n + DS_RANGE_ROWS - 1) / DS_RANGE_ROWS;
  return (int)std::max(1LL, std::min(want, (long long)n_cu * 8));
}

size_t blk_desc_range_scratch_bytes(int n, int n_cu) {
  return sizeof(ds_range_part) * BL_AMD_DESC_DIMS * (size_t)ds_range_blocks(n, n_cu);
}

int blk_desc_range(hipStream_t s, const float *d_x, int n, int d, int n_cu, void *d_scratch, bl_amd_desc_range *d_range,
                   blk_mark_fn mark, void *mark_user) {
  Mark m(mark, mark_user, PK_DESC_RANGE, s);
  const int blocks = ds_range_blocks(n, n_cu);
  ds_range_part *part = static_cast<ds_range_part *>(d_scratch);
  hipLaunchKernelGGL(k_desc_range, dim3(blocks), dim3(256), 0, s, d_x, n, d, part);
  hipLaunchKernelGGL(k_desc_range_finish, dim3(1), dim3(256), 0, s, part, blocks, d_range);
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}

int blk_desc_quantize(hipStream_t s, const float *d_x, int n, int d, const bl_amd_desc_range *d_range,
                      const blk_desc_scale &scale, bl_amd_desc *d_out, blk_mark_fn mark, void *mark_user) {
  Mark m(mark, mark_user, PK_DESC_QUANTIZE, s);
  const unsigned blocks = (unsigned)(((size_t)n * BL_AMD_DESC_DIMS + 255) / 256); /* n is an int: below 2^28 */
  hipLaunchKernelGGL(k_desc_quantize, dim3(blocks), dim3(256), 0, s, d_x, n, d, d_range, scale,
                     reinterpret_cast<int16_t *>(d_out));
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}

size_t blk_desc_knn_scratch_bytes(int n, int n_rows, int k, int n_cu) {
  int n_split, cols;
  blk_split_plan(n, n_rows, n_cu, DS_QPW, KNN_SPLIT_MIN_COLS, &n_split, &cols);
  return n_split > 1 ? sizeof(ds_u64) * (size_t)n_rows * n_split * k : 0;
}

template <int KW>
static void ds_knn_launch(hipStream_t s, const uint4 *q, bool cross, const uint4 *lib, int n, int row_begin, int n_rows,
                          int k, int n_split, int cols, ds_u64 *part, int32_t *d_index, ds_u64 *d_d2, blk_mark_fn mark,
                          void *mark_user) {
  const int per_block = DS_WAVES * DS_QPW;
  const dim3 grid((n_rows + per_block - 1) / per_block, n_split), merge_grid((n_rows + DS_WAVES - 1) / DS_WAVES);
  const dim3 block(64 * DS_WAVES);
  const auto knn = cross ? k_desc_knn<KW, true> : k_desc_knn<KW, false>;
  const auto merge = k_desc_merge<KW>;
  {
    Mark m(mark, mark_user, PK_DESC_KNN, s);
    hipLaunchKernelGGL(knn, grid, block, 0, s, q, lib, n, row_begin, n_rows, k, cols, n_split, part, d_index, d_d2);
  }
  if (n_split > 1) {
    Mark m(mark, mark_user, PK_DESC_MERGE, s);
    hipLaunchKernelGGL(merge, merge_grid, block, 0, s, n_rows, k, n_split, part, d_index, d_d2);
  }
}

int blk_desc_knn(hipStream_t s, const bl_amd_desc *d_queries, const bl_amd_desc *d_lib, int n, int row_begin, int n_rows,
                 int k, int n_cu, void *d_scratch, int32_t *d_index, uint64_t *d_dist2, blk_mark_fn mark,
                 void *mark_user) {
  if (d_queries && row_begin) return BL_UNEXPECTED;
  if (n < 1 || (unsigned)n > DS_IDX_MASK) return BL_UNEXPECTED; /* the index bits of a key */
  const uint4 *lib = reinterpret_cast<const uint4 *>(d_lib);
  const uint4 *q = d_queries ? reinterpret_cast<const uint4 *>(d_queries) : lib;
  int n_split, cols;
  blk_split_plan(n, n_rows, n_cu, DS_QPW, KNN_SPLIT_MIN_COLS, &n_split, &cols);
  ds_u64 *part = n_split > 1 ? static_cast<ds_u64 *>(d_scratch) : nullptr;
  ds_u64 *d2 = reinterpret_cast<ds_u64 *>(d_dist2);
  if (k > 64) ds_knn_launch<2>(s, q, d_queries != nullptr, lib, n, row_begin, n_rows, k, n_split, cols, part, d_index, d2, mark, mark_user);
  else ds_knn_launch<1>(s, q, d_queries != nullptr, lib, n, row_begin, n_rows, k, n_split, cols, part, d_index, d2, mark, mark_user);
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}
