/*
 * bl_form_kernels.hip — gfx950 kernels and launch layer of the song structure (bl_amd_form_device; the definition is
 * the block in include/bliss_amd.h).  Every quantity is an exact integer and no atomics touch global memory: a result
 * is written once, by the one workgroup that owns it.
 *
 * Kernels:
 *   k_form_units    one workgroup per (song, run of 256 units), one lane per unit.  The frames under floor(256 / P)
 *                   units at a time are copied to LDS with coalesced loads; a lane sums its P frames, shifts the sums
 *                   below 2^20, takes bl_isqrt64 of their squares and divides each class once, in 32 bits.
 *   k_form_thumb    one workgroup per song, the song's units in LDS (16 bytes each, at most 128 KB).  The lags go in
 *                   chunks of one per lane; a lane walks the starts u of its lag with the sliding sum F += S(new) -
 *                   S(old) in a register and keeps its best (F, u); the 64-bit keys are reduced across the lanes at the
 *                   end.  S is three v_dot4_u32_u8 (q is 0 .. 127, so the unsigned form is exact).  The lanes of a wave
 *                   read one address for the unit at u (a broadcast) and consecutive 16-byte pieces for the one at
 *                   u + l.  With rep (a variant of its own, so the plain call does not pay for it) every step ends in a
 *                   maximum across the wave, 64 steps are joined across the waves in LDS, and lane u % 64 of the first
 *                   wave owns rep[u] over all chunks: chunks come in rising lag, so only a larger F replaces.
 *   k_form_novelty  one workgroup per song, one lane per unit and round: the tapered difference directly (2 L units of
 *                   16 bytes, which neighbouring lanes share in the cache), the maximum as a 64-bit key, then the peak
 *                   rule over the song's own novelty values, which the workgroup wrote itself.
 *
 * What is read.  A kernel addresses frames and units through its song's record only and checks every index against
 * the song's own T or U: a unit of a neighbour in the concatenated arrays is never fetched.
 *
 * Untuned: first forms.  The thumbnail kernel computes every S twice (once entering, once leaving the window) and M
 * more per lag for the first window; a lane's last chunk is partly idle; one workgroup per song leaves a call with few
 * long songs on few CUs.
 */
#include <hip/hip_runtime.h>

#include "bl_form.h"
#include "bl_isqrt.h"

typedef unsigned long long fm_u64;

#define FM_BLOCK BL_FORM_BLOCK_UNITS /* 256 */
#define FM_LANES BL_FORM_LANES       /* 256 */
#define FM_WAVES (FM_LANES / 64)
#define FM_PITCH 13 /* uint64 per LDS row: 12 and one of padding */
#define FM_UMAX BL_AMD_FORM_UNITS_MAX
#define FM_LOW20 0xFFFFFull
#define FM_LDS_DEFAULT (64 * 1024) /* dynamic LDS a kernel may ask for without an attribute */

static_assert(sizeof(bl_amd_frame_chroma) == 96, "a frame record is twelve uint64");
static_assert(sizeof(bl_amd_song_form) == 48, "the record is 48 bytes");
static_assert(FM_UMAX * 16 == 128 * 1024 && FM_UMAX <= (1 << 20), "one song's units fit a workgroup's LDS");

/* ========================================================================= */
/* units                                                                      */

__global__ __launch_bounds__(FM_BLOCK) void k_form_units(const bl_amd_frame_chroma *__restrict__ frames,
                                                         const bl_form_song *__restrict__ songs, int n_songs, int P,
                                                         uint4 *__restrict__ units) {
  /* this workgroup's song: the last record whose group_off <= g (a record without units shares its offset with the
   * next) */
  const long long g = blockIdx.x;
  int lo = 0, hi = n_songs;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (songs[mid].group_off <= g) lo = mid;
    else hi = mid;
  }
  const bl_form_song sg = songs[lo];
  const int u0 = (int)(g - sg.group_off) * FM_BLOCK;
  const int nu = min(FM_BLOCK, sg.units - u0); /* units of this song in the run: the last frame read is u0 P + nu P - 1 < T */
  const int tid = threadIdx.x;
  const int per_pass = FM_BLOCK / P; /* units whose frames fit the 256 rows: 256 .. 16 */

  __shared__ fm_u64 sh[FM_BLOCK * FM_PITCH];
  const fm_u64 *src = reinterpret_cast<const fm_u64 *>(frames + sg.frame_off + (long long)u0 * P);
  for (int b = 0; b < nu; b += per_pass) {
    const int n = min(per_pass, nu - b), rows = n * P;
    __syncthreads(); /* the previous pass has been read */
    for (int e = tid; e < rows * 12; e += FM_BLOCK) sh[(e / 12) * FM_PITCH + e % 12] = src[(long long)b * P * 12 + e];
    __syncthreads();
    if (tid >= n) continue;
    fm_u64 Y[12], m = 0ull;
#pragma unroll
    for (int k = 0; k < 12; ++k) Y[k] = 0ull;
    for (int j = 0; j < P; ++j)
#pragma unroll
      for (int k = 0; k < 12; ++k) Y[k] += sh[(tid * P + j) * FM_PITCH + k];
#pragma unroll
    for (int k = 0; k < 12; ++k) m = Y[k] > m ? Y[k] : m;
    uint32_t qw[3] = {0u, 0u, 0u};
    if (m) {
      const int s = max(0, 64 - __clzll((long long)m) - 20);
      uint32_t y[12];
      fm_u64 ss = 0ull;
#pragma unroll
      for (int k = 0; k < 12; ++k) {
        y[k] = (uint32_t)(Y[k] >> s);
        ss += (fm_u64)y[k] * y[k];
      }
      const uint32_t r = bl_isqrt64(ss); /* >= y of the largest class >= 1 */
#pragma unroll
      for (int k = 0; k < 12; ++k) qw[k >> 2] |= ((127u * y[k]) / r) << (8 * (k & 3));
    }
    units[sg.unit_off + u0 + b + tid] = make_uint4(qw[0], qw[1], qw[2], 0u);
  }
}

/* ========================================================================= */
/* thumbnail                                                                  */

__device__ __forceinline__ uint32_t fm_sim(const uint4 a, const uint4 b) {
  return __builtin_amdgcn_udot4(a.x, b.x, __builtin_amdgcn_udot4(a.y, b.y, __builtin_amdgcn_udot4(a.z, b.z, 0u, false), false),
                                false);
}

__device__ __forceinline__ fm_u64 fm_wave_max(fm_u64 k) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const fm_u64 o = __shfl_xor(k, off);
    k = o > k ? o : k;
  }
  return k;
}

/* the largest key of the workgroup, in every lane; sk: FM_WAVES slots nobody else is using */
__device__ __forceinline__ fm_u64 fm_block_max(fm_u64 k, fm_u64 *sk) {
  k = fm_wave_max(k);
  if ((threadIdx.x & 63) == 0) sk[threadIdx.x >> 6] = k;
  __syncthreads();
  k = sk[0];
#pragma unroll
  for (int w = 1; w < FM_WAVES; ++w) k = sk[w] > k ? sk[w] : k;
  return k;
}

template <bool REP>
__global__ __launch_bounds__(FM_LANES) void k_form_thumb(const uint4 *__restrict__ units,
                                                         const bl_form_song *__restrict__ songs, int M, int minlag,
                                                         bl_amd_song_form *__restrict__ out, uint32_t *rep) {
  extern __shared__ uint4 su[]; /* the song's U units */
  __shared__ fm_u64 sk[FM_WAVES];
  __shared__ fm_u64 srep[REP ? FM_WAVES : 1][REP ? 64 : 1]; /* the waves' maxima of 64 steps; next to nothing without rep */
  __shared__ uint32_t s_self;
  const int tid = threadIdx.x;
  const bl_form_song sg = songs[blockIdx.x];
  const int U = sg.units;
  const bool too_long = U > FM_UMAX;
  uint32_t *rp = REP ? rep + 2 * sg.unit_off : nullptr;

  bl_amd_song_form o; /* the fields this kernel owns; k_form_novelty writes the others */
  o.units = U;
  o.status = BL_AMD_FORM_NO_THUMB | (too_long ? BL_AMD_FORM_TOO_LONG : 0);
  o.thumb_start = o.thumb_lag = 0;
  o.thumb_score = o.thumb_self = 0u;
  bl_amd_song_form *po = out + blockIdx.x;

  /* lane u % 64 of the first wave owns rep[u] from here to the end */
  if (REP && tid < 64)
    for (int u = tid; u < U; u += 64) rp[2 * u] = rp[2 * u + 1] = 0u;
  if (too_long || U < M + minlag) { /* the whole workgroup leaves together */
    if (tid == 0) {
      po->units = o.units, po->status = o.status, po->thumb_start = 0, po->thumb_lag = 0;
      po->thumb_score = 0u, po->thumb_self = 0u;
    }
    return;
  }
  const uint4 *__restrict__ up = units + sg.unit_off;
  for (int u = tid; u < U; u += FM_LANES) su[u] = up[u];
  if (tid == 0) s_self = 0u;
  __syncthreads();

  const int lmax = U - M; /* >= minlag */
  fm_u64 best = 0ull;
  for (int l0 = minlag; l0 <= lmax; l0 += FM_LANES) {
    const int l = l0 + tid;
    const int ulast = U - M - l;   /* this lane's last start; negative: the lane has no lag in this chunk */
    const int ulast0 = U - M - l0; /* the chunk's: lane 0's */
    uint32_t F = 0u, bestF = 0u;
    int bestu = 0;
    if (ulast >= 0)
      for (int j = 0; j < M; ++j) F += fm_sim(su[j], su[l + j]); /* l + j <= U - 1 */
    for (int u = 0; u <= ulast0; ++u) {
      const bool live = u <= ulast;
      if (live && F > bestF) bestF = F, bestu = u;
      if (REP) {
        const fm_u64 k = fm_wave_max(live ? ((fm_u64)F << 20) | (FM_LOW20 - (fm_u64)l) : 0ull);
        if ((tid & 63) == 0) srep[tid >> 6][u & 63] = k;
        if ((u & 63) == 63 || u == ulast0) { /* the same for every lane */
          __syncthreads();
          const int ut = (u & ~63) + tid;
          if (tid < 64 && ut <= u) {
            fm_u64 kk = srep[0][tid];
#pragma unroll
            for (int w = 1; w < FM_WAVES; ++w) kk = srep[w][tid] > kk ? srep[w][tid] : kk;
            const uint32_t R = (uint32_t)(kk >> 20);
            if (R > rp[2 * ut]) { /* a later chunk's lags are larger: a tie stays with the smaller */
              rp[2 * ut] = R;
              rp[2 * ut + 1] = (uint32_t)(FM_LOW20 - (kk & FM_LOW20));
            }
          }
          __syncthreads();
        }
      }
      if (u < ulast) F += fm_sim(su[u + M], su[u + l + M]) - fm_sim(su[u], su[u + l]); /* u + l + M <= U - 1 */
    }
    if (bestF) {
      const fm_u64 key = ((fm_u64)bestF << 40) | ((FM_LOW20 - (fm_u64)l) << 20) | (FM_LOW20 - (fm_u64)bestu);
      best = key > best ? key : best;
    }
  }

  const fm_u64 k = fm_block_max(best, sk);
  if (k >> 40) {
    const int us = (int)(FM_LOW20 - (k & FM_LOW20)), ls = (int)(FM_LOW20 - ((k >> 20) & FM_LOW20));
    uint32_t self = 0u;
    for (int j = tid; j < M; j += FM_LANES) self += fm_sim(su[us + j], su[us + j]);
    if (self) atomicAdd(&s_self, self);
    __syncthreads();
    o.status = 0;
    o.thumb_start = us;
    o.thumb_lag = ls;
    o.thumb_score = (uint32_t)(k >> 40);
    o.thumb_self = s_self;
  }
  if (tid == 0) {
    po->units = o.units, po->status = o.status, po->thumb_start = o.thumb_start, po->thumb_lag = o.thumb_lag;
    po->thumb_score = o.thumb_score, po->thumb_self = o.thumb_self;
  }
}

/* ========================================================================= */
/* novelty                                                                    */

__device__ __forceinline__ int fm_byte(const uint4 v, int k) {
  const uint32_t w = k < 4 ? v.x : k < 8 ? v.y : v.z;
  return (int)((w >> (8 * (k & 3))) & 0xFFu);
}

__global__ __launch_bounds__(FM_LANES) void k_form_novelty(const uint4 *__restrict__ units,
                                                           const bl_form_song *__restrict__ songs, int L, int pnum,
                                                           int pden, bl_amd_song_form *__restrict__ out, fm_u64 *nov,
                                                           uint8_t *__restrict__ flags) {
  __shared__ fm_u64 sk[FM_WAVES];
  __shared__ int s_count;
  const int tid = threadIdx.x;
  const bl_form_song sg = songs[blockIdx.x];
  const int U = sg.units;
  const bool too_long = U > FM_UMAX;
  const uint4 *__restrict__ up = units + sg.unit_off;
  fm_u64 *nv = nov + sg.unit_off;
  if (tid == 0) s_count = 0;

  fm_u64 best = 0ull;
  for (int u = tid; u < U; u += FM_LANES) {
    fm_u64 N = 0ull;
    if (!too_long && u >= L && u <= U - L) { /* units u - L .. u + L - 1, all inside [0, U) */
      int D[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) D[k] = 0;
      for (int a = 1; a <= L; ++a) {
        const int w = L + 1 - a;
        const uint4 p = up[u - a], g = up[u + a - 1];
#pragma unroll
        for (int k = 0; k < 12; ++k) D[k] += w * (fm_byte(p, k) - fm_byte(g, k));
      }
#pragma unroll
      for (int k = 0; k < 12; ++k) N += (fm_u64)((long long)D[k] * D[k]);
    }
    nv[u] = N;
    if (N) {
      const fm_u64 key = (N << 20) | (FM_LOW20 - (fm_u64)u); /* N < 2^40 */
      best = key > best ? key : best;
    }
  }
  __threadfence_block();
  const fm_u64 kmax = fm_block_max(best, sk); /* its barrier also stands between the novelty's writes and reads */
  const fm_u64 Nmax = kmax >> 20;

  int count = 0;
  for (int u = tid; u < U; u += FM_LANES) {
    const fm_u64 n = nv[u];
    bool b = n > 0ull && n * (fm_u64)pden >= Nmax * (fm_u64)pnum; /* below 2^48 */
    if (b) {
      const int v0 = max(0, u - L), v1 = min(U - 1, u + L);
      for (int v = v0; v < u && b; ++v) b = nv[v] < n;
      for (int v = u + 1; v <= v1 && b; ++v) b = nv[v] <= n;
    }
    if (flags) flags[sg.unit_off + u] = b ? 1 : 0;
    count += b ? 1 : 0;
  }
  if (count) atomicAdd(&s_count, count);
  __syncthreads();
  if (tid == 0) {
    bl_amd_song_form *po = out + blockIdx.x;
    po->boundaries = s_count;
    po->nov_max_unit = Nmax ? (int)(FM_LOW20 - (kmax & FM_LOW20)) : 0;
    po->nov_max = Nmax;
    po->reserved = 0ull;
  }
}

/* ========================================================================= */
/* launchers (declared in bl_form.h)                                          */

int blk_form_units(hipStream_t s, const bl_amd_frame_chroma *d_frames, const bl_form_song *d_songs, int n_songs,
                   long long n_groups, int pool, uint4 *d_units, blk_mark_fn mark, void *mark_user) {
  if (n_groups < 1) return BL_OK;
  Mark m(mark, mark_user, FMK_UNITS, s);
  hipLaunchKernelGGL(k_form_units, dim3((unsigned)n_groups), dim3(FM_BLOCK), 0, s, d_frames, d_songs, n_songs, pool,
                     d_units);
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}

int blk_form_thumb(hipStream_t s, const uint4 *d_units, const bl_form_song *d_songs, int n_songs, int max_units, int seg,
                   int min_lag, bl_amd_song_form *d_out, uint32_t *d_rep, blk_mark_fn mark, void *mark_user) {
  if (max_units < 1) max_units = 1;
  if (max_units > FM_UMAX) max_units = FM_UMAX;
  const size_t lds = sizeof(uint4) * (size_t)max_units;
  const auto kernel = d_rep ? k_form_thumb<true> : k_form_thumb<false>;
  /* a host-side setting of the function on the current device, no device work; a failure shows as the launch's error */
  if (lds > FM_LDS_DEFAULT)
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(sizeof(uint4) * FM_UMAX));
  Mark m(mark, mark_user, FMK_THUMB, s);
  hipLaunchKernelGGL(kernel, dim3((unsigned)n_songs), dim3(FM_LANES), lds, s, d_units, d_songs, seg, min_lag, d_out,
                     d_rep);
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}

int blk_form_novelty(hipStream_t s, const uint4 *d_units, const bl_form_song *d_songs, int n_songs, int nov,
                     int peak_num, int peak_den, bl_amd_song_form *d_out, unsigned long long *d_nov, uint8_t *d_flags,
                     blk_mark_fn mark, void *mark_user) {
  Mark m(mark, mark_user, FMK_NOVELTY, s);
  hipLaunchKernelGGL(k_form_novelty, dim3((unsigned)n_songs), dim3(FM_LANES), 0, s, d_units, d_songs, nov, peak_num,
                     peak_den, d_out, d_nov, d_flags);
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}
