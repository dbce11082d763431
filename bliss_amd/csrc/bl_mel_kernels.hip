/*
 * bl_mel_kernels.hip — gfx950 kernels and launch layer of the mel call (bl_amd_mel_batch_device, include/bliss_amd.h:
 * bl_amd_frame_mel, bl_amd_song_mel): per frame the 32 log-mel band levels, 13 cepstral coefficients and the spectral
 * flatness, summed over the song.  The frames, the window, the transform and the power values are the frequency
 * pass's own (freq_frames_lavc, bl_freq_frames.h, compiled here in its per-frame form, as k_timbre does); what is new
 * is the stage behind the transform.  Must be compiled with -ffp-contract=off.
 *
 * Kernels:
 *   k_mel           one workgroup of four waves per song.  A wave transforms eight frames per iteration; once their 255
 *                   power values each lie in the wave's staging rows, bl_mel_frames::frames turns every frame into band
 *                   sums, band levels, coefficients and flatness and keeps the song's sums in registers; the workgroup
 *                   joins them at the end (::finish).
 *   k_ilog2_sweep   bl_amd_selftest_ilog2
 *
 * Everything behind the power values is an integer (Q[d] = floor(16 P[d]) as a uint64, bl_ilog2.h, bl_mel_table.h), so
 * no result depends on the order of a reduction or the shape of the launch.
 *
 * LDS.  freq_frames_lavc's layout of four waves (BL_FREQ_LDS_BYTES, 76 864 bytes) is left as it is; the kernel asks
 * for BL_MEL_IMAGE_BYTES = 2 368 more behind it (where k_freq_scan keeps its histogram, which the per-frame form does
 * not have) and copies the table image there before the transform's first barrier: 2 x 79 232 = 158 464 <= 163 840, so
 * two workgroups still share a CU.  The image (mel_build_image): 32 bands x 48 bytes {first bin, length, 0, 0, 44
 * weights, zero behind the length}, then the cosine table as [8 lanes][13 k][4 bands] int16.  ::finish puts the waves'
 * sums (4 x 61 x 8 = 1 952 bytes, more than the 1 KB freq_frames_lavc hands over) into the exchange buffers, which are
 * free behind the barrier in front of it.  bl_freq_frames.h is unchanged.
 *
 * Lane mapping of the per-frame stage.  Eight lanes per frame (lane = 8 frame + s).
 *   energy     as k_timbre: 32 consecutive bins per lane, eight b128 reads (2-way conflicted, see there), three DPP
 *              steps
 *   band sums  lane s takes bands s, 15 - s, 16 + s, 31 - s, one after the other: the eight lanes of a step then hold
 *              eight neighbouring bands, whose lengths differ little (3 .. 6, 6 .. 11, 12 .. 22, 23 .. 41 bins), and the
 *              step's loop runs to the longest of them in groups of four bins: 2 + 3 + 6 + 11 = 22 groups per
 *              iteration, against 16 if the 481 non-zero weights were spread evenly.  A group is one b32 read of four
 *              weight bytes and four b32 reads of power values.  The weight word of band b, group g is dword
 *              12 b + 1 + g of the image: the lanes of a frame read eight neighbouring bands, 12 b mod 32 takes eight
 *              different multiples of 4, the eight frames read the same addresses (broadcast) — conflict-free.  A
 *              power value of frame f, bin d is dword 264 f + d of the staging rows, bank (8 f + d) mod 32; a b32 read
 *              is served in two halves of 32 lanes = 4 frames x 8 bands, and two of its lanes meet on a bank when
 *              8 (f - f') + (d - d') is a multiple of 32.  Counted over this table's addresses: every read of the first
 *              three steps is at most 2-way, the worst of the last step 3-way, 2.05 LDS cycles per half on average
 *              over the 88 reads of an iteration; derived from the addresses, not measured.
 *   levels     E = L(S + 1) for the lane's four bands, L(T) from the eight-lane sum T (bl_ilog2.h: 12 squarings each)
 *   cepstrum   the lane's share of all 13 sums (52 multiply-adds into 64-bit sums from 13 8-byte entries of the cosine
 *              table, which hipcc reads in pairs: the eight lanes of a frame read eight addresses 26 dwords apart, two
 *              banks each, all different under the 32-bank and the 64-bank rule alike; the frames read the same —
 *              conflict-free), then a reduce-scatter over the eight lanes (8 + 4 + 2 exchanges): lane s ends with
 *              coefficients s and 8 + s, lane 5's second slot takes the flatness
 * Every lane stores its two values of the frame record and its four band levels, and adds them to its own sums, so the
 * song's 60 sums cost eight 64-bit registers per lane.
 */
#include <hip/hip_runtime.h>

#include <vector>

#include "bl_freq_frames.h"
#include "bl_ilog2.h"
#include "bl_mel_table.h"

typedef unsigned long long bl_u64;

#define BL_MEL_WAVES 4 /* waves per workgroup: BL_FREQ_LDS_BYTES is the layout of four */
#define BL_MEL_BAND_STRIDE 48
#define BL_MEL_BAND_GROUPS 11 /* groups of four weights per band: 44 >= BL_MEL_MAX_WIDTH */
#define BL_MEL_DCT_OFF (BL_MEL_BANDS * BL_MEL_BAND_STRIDE)
#define BL_MEL_IMAGE_BYTES (BL_MEL_DCT_OFF + 8 * BL_MEL_COEFFS * 4 * 2)
#define BL_MEL_LDS_BYTES (BL_FREQ_LDS_BYTES + BL_MEL_IMAGE_BYTES)
#define BL_MEL_SUMS 61 /* 64-bit values a wave hands to ::finish: the record's 60 sums and `used` */
static_assert(4 + 4 * BL_MEL_BAND_GROUPS == BL_MEL_BAND_STRIDE && 4 * BL_MEL_BAND_GROUPS >= BL_MEL_MAX_WIDTH,
              "a band's header and its weights, padded to whole groups, fill its stride");
static_assert(BL_MEL_IMAGE_BYTES % 16 == 0 && BL_FREQ_LDS_BYTES % 16 == 0 && 2 * BL_MEL_LDS_BYTES <= 160 * 1024,
              "the image lies 16-byte aligned behind the transform's layout and two workgroups fit a CU");
static_assert(BL_MEL_SUMS * 8 * BL_MEL_WAVES <= BL_FREQ_XCH_BYTES(BL_MEL_WAVES), "the waves' sums fit the exchange buffers");
static_assert(sizeof(bl_amd_frame_mel) == 56 && sizeof(bl_amd_song_mel) == 496 &&
                  offsetof(bl_amd_song_mel, frames) == 8 * (BL_MEL_SUMS - 1),
              "the song record is 60 64-bit sums and four int32");

/* the band of lane s in step q: s, 15 - s, 16 + s, 31 - s */
__host__ __device__ constexpr int mel_band(int s, int q) { return (q & 1) ? 8 * q + 7 - s : 8 * q + s; }

/* cross-lane moves inside every group of eight lanes (CTRL as in bl_timbre_kernels.hip: 0xB1 lane ^ 1, 0x4E lane ^ 2,
 * 0x141 the other quad) */
template <int CTRL> __device__ __forceinline__ unsigned mel_dpp(unsigned v) {
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
}
template <int CTRL> __device__ __forceinline__ bl_u64 mel_dpp(bl_u64 v) {
  return ((bl_u64)mel_dpp<CTRL>((unsigned)(v >> 32)) << 32) | mel_dpp<CTRL>((unsigned)v);
}
template <int CTRL> __device__ __forceinline__ long long mel_dpp(long long v) { return (long long)mel_dpp<CTRL>((bl_u64)v); }
/* the sum over the eight lanes of a frame, in all of them */
template <class T> __device__ __forceinline__ T mel_sum8(T v) {
  v += mel_dpp<0xB1>(v);
  v += mel_dpp<0x4E>(v);
  v += mel_dpp<0x141>(v); /* the quads are uniform by now */
  return v;
}
/* lane ^ 4: no DPP pattern does it inside a row of 16 */
__device__ __forceinline__ long long mel_xor4(long long v) { return __shfl_xor(v, 4); }

/* the per-frame form of freq_frames_lavc's PF: the song's records and this lane's share of its sums */
struct bl_mel_frames {
  static constexpr bool per_frame = true;
  bl_amd_frame_mel *rec; /* the song's first frame record, or nullptr */
  uint32_t *bands;       /* the song's first row of 32 band levels, or nullptr */
  bl_amd_song_mel *song;
  bl_u64 min_energy;
  int n_frames;
  const unsigned char *image; /* LDS: the table image */
  unsigned char *smem;        /* LDS: the workgroup's base (the exchange buffers) */
  /* lane (frame, s): coefficient s, slot 8 + s (coefficients 8 .. 12, the flatness for s = 5, nothing for s = 6, 7) and
   * bands mel_band(s, 0 .. 3) */
  long long vsum[2] = {0, 0};
  bl_u64 vsq[2] = {0, 0}, bsum[4] = {0, 0, 0, 0};
  unsigned used = 0;

  /* the wave's frames [first, first + 8) lie in stage[8][BL_FREQ_SROW]; the first n_live of them belong to the song */
  __device__ __forceinline__ void frames(const float *stage, int lane, int first, int n_live) {
    const int fr = lane >> 3, s = lane & 7;
    const float *row = stage + fr * BL_FREQ_SROW;
    /* energy: the sum of Q over bins 1 .. 255, as k_timbre takes it */
    bl_u64 energy = 0;
    {
      const float4 *seg = reinterpret_cast<const float4 *>(row + 32 * s);
      float4 pv[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) pv[q] = seg[q];
#pragma unroll
      for (int j = 0; j < 32; ++j) {
        const float4 v = pv[j >> 2];
        float pw = (j & 3) == 0 ? v.x : (j & 3) == 1 ? v.y : (j & 3) == 2 ? v.z : v.w;
        if (j == 0) pw = s == 0 ? 0.f : pw; /* bin 0 takes no part */
        /* 16 P is exact and below 2^50: the conversion truncates, which is the floor of a value >= 0 */
        energy += (bl_u64)(pw * 16.f);
      }
      energy = mel_sum8(energy);
    }
    /* band sums: S = sum W Q <= 64 * sum Q < 64 * 2^50 = 2^56 (a column of W sums to at most 64), T < 32 * 2^56 + 32 */
    unsigned E[4];
    bl_u64 T = 0;
    unsigned G = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const unsigned char *bd = image + mel_band(s, q) * BL_MEL_BAND_STRIDE;
      const unsigned head = *reinterpret_cast<const unsigned *>(bd);
      const int d0 = (int)(head & 0xFFu), groups = ((int)((head >> 8) & 0xFFu) + 3) >> 2;
      const unsigned *wt = reinterpret_cast<const unsigned *>(bd + 4);
      bl_u64 S = 0;
      for (int g = 0; g < groups; ++g) {
        const unsigned w4 = wt[g];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          /* the weights behind the band's length are 0; their bins are read inside the row all the same */
          const int d = min(d0 + 4 * g + i, 255);
          S += (bl_u64)(row[d] * 16.f) * ((w4 >> (8 * i)) & 0xFFu);
        }
      }
      E[q] = bl_ilog2_q12(S + 1u);
      T += S + 1u;
      G += E[q];
    }
    T = mel_sum8(T);
    G = mel_sum8(G);
    /* 32 * 4096 * log2(arithmetic mean / geometric mean) of the 32 values S + 1 */
    const int flat = (int)(32u * bl_ilog2_q12(T)) - 160 * 4096 - (int)G;
    /* cepstrum: this lane's four terms of every sum, |D E| < 2^14 * 2^18, then the reduce-scatter: a step halves what
     * a lane keeps and adds its partner's share of it */
    long long c16[16];
    {
      const uint2 *dl = reinterpret_cast<const uint2 *>(image + BL_MEL_DCT_OFF) + s * BL_MEL_COEFFS;
#pragma unroll
      for (int k = 0; k < BL_MEL_COEFFS; ++k) {
        const uint2 d4 = dl[k];
        const int d0 = (int)(short)(d4.x & 0xFFFFu), d1 = (int)(short)(d4.x >> 16);
        const int d2 = (int)(short)(d4.y & 0xFFFFu), d3 = (int)(short)(d4.y >> 16);
        c16[k] = (long long)d0 * (int)E[0] + (long long)d1 * (int)E[1] + (long long)d2 * (int)E[2] +
                 (long long)d3 * (int)E[3];
      }
      c16[13] = c16[14] = c16[15] = 0;
    }
    const bool p1 = (s & 1) != 0, p2 = (s & 2) != 0, p4 = (s & 4) != 0;
    long long c8[8], c4[4], c2[2];
#pragma unroll
    for (int i = 0; i < 8; ++i) /* slot 2 i + (s & 1) */
      c8[i] = (p1 ? c16[2 * i + 1] : c16[2 * i]) + mel_dpp<0xB1>(p1 ? c16[2 * i] : c16[2 * i + 1]);
#pragma unroll
    for (int i = 0; i < 4; ++i) /* slot 4 i + (s & 3) */
      c4[i] = (p2 ? c8[2 * i + 1] : c8[2 * i]) + mel_dpp<0x4E>(p2 ? c8[2 * i] : c8[2 * i + 1]);
#pragma unroll
    for (int i = 0; i < 2; ++i) /* slot 8 i + s */
      c2[i] = (p4 ? c4[2 * i + 1] : c4[2 * i]) + mel_xor4(p4 ? c4[2 * i] : c4[2 * i + 1]);
    /* floor(sum / 2^14): an arithmetic shift; |sum| < 32 * 2^32, so the result fits an int */
    const int v0 = (int)(c2[0] >> 14), v1 = s == 5 ? flat : (int)(c2[1] >> 14);
    if (fr < n_live) {
      const size_t t = (size_t)(first + fr);
      if (rec) {
        int *r = reinterpret_cast<int *>(rec + t); /* mfcc[13], flat: slot k is the record's int k */
        r[s] = v0;
        if (s < 6) r[8 + s] = v1;
      }
      if (bands) {
        uint32_t *bo = bands + t * BL_MEL_BANDS;
#pragma unroll
        for (int q = 0; q < 4; ++q) bo[mel_band(s, q)] = E[q];
      }
      if (energy > 0 && energy >= min_energy) {
        vsum[0] += v0; vsq[0] += (bl_u64)((long long)v0 * v0);
        vsum[1] += v1; vsq[1] += (bl_u64)((long long)v1 * v1);
#pragma unroll
        for (int q = 0; q < 4; ++q) bsum[q] += E[q];
        used += 1;
      }
    }
  }

  /* behind the song's last frame and a workgroup barrier: the eight frames of a wave are added by shuffles, lane s of
   * every wave puts its sums where the record has them ([wave][61] in the exchange buffers, which nothing reads any
   * more), and the workgroup's first lane adds the four waves and writes every field with plain stores */
  __device__ __forceinline__ void finish(void *, int wave, int lane) {
    bl_u64 *part = reinterpret_cast<bl_u64 *>(smem);
    bl_u64 v[9] = {(bl_u64)vsum[0], vsq[0], (bl_u64)vsum[1], vsq[1], bsum[0], bsum[1], bsum[2], bsum[3], used};
#pragma unroll
    for (int off = 32; off >= 8; off >>= 1) {
#pragma unroll
      for (int k = 0; k < 9; ++k) v[k] += __shfl_down(v[k], off);
    }
    if (lane < 8) {
      bl_u64 *p = part + BL_MEL_SUMS * wave;
      const int s = lane;
      p[s] = v[0];        /* mfcc_sum[s] */
      p[13 + s] = v[1];   /* mfcc_sumsq[s] */
      if (s < 5) { p[8 + s] = v[2]; p[21 + s] = v[3]; }
      if (s == 5) { p[26] = v[2]; p[27] = v[3]; } /* flat_sum, flat_sumsq */
#pragma unroll
      for (int q = 0; q < 4; ++q) p[28 + mel_band(s, q)] = v[4 + q];
      if (s == 0) p[60] = v[8];
    }
    __syncthreads();
    if (wave == 0 && lane == 0) {
      bl_u64 *out = reinterpret_cast<bl_u64 *>(song);
      bl_u64 t = 0;
      for (int k = 0; k < BL_MEL_SUMS; ++k) {
        t = part[k];
        for (int w = 1; w < BL_MEL_WAVES; ++w) t += part[BL_MEL_SUMS * w + k];
        if (k < BL_MEL_SUMS - 1) out[k] = t;
      }
      song->frames = n_frames;
      song->used = (int)t;
      song->status = BL_OK;
      song->reserved = 0;
    }
  }
};

/* one workgroup per song; the channel count is uniform per workgroup (as k_timbre) */
__global__ __launch_bounds__(64 * BL_MEL_WAVES, 2) void k_mel(const int16_t *__restrict__ pcm,
                                                             const bl_timbre_song *__restrict__ songs, bl_tables tb,
                                                             const uint4 *__restrict__ image, bl_u64 min_energy,
                                                             bl_amd_song_mel *songs_out, bl_amd_frame_mel *frames_out,
                                                             uint32_t *bands_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const bl_timbre_song ts = songs[blockIdx.x];
  /* the image, 148 x 16 bytes: visible to every wave behind the barrier freq_frames_lavc has after its own tables */
  if (threadIdx.x < BL_MEL_IMAGE_BYTES / 16)
    reinterpret_cast<uint4 *>(smem + BL_FREQ_LDS_BYTES)[threadIdx.x] = image[threadIdx.x];
  bl_dsong sg = {};
  sg.pcm_off = ts.pcm_off;
  sg.channels = ts.channels;
  sg.n_frames = ts.n_frames;
  bl_mel_frames pf;
  pf.rec = frames_out ? frames_out + ts.frame_off : nullptr;
  pf.bands = bands_out ? bands_out + ts.frame_off * BL_MEL_BANDS : nullptr;
  pf.song = songs_out + ts.out_idx;
  pf.min_energy = min_energy;
  pf.n_frames = ts.n_frames;
  pf.image = smem + BL_FREQ_LDS_BYTES;
  pf.smem = smem;
  if (ts.channels == 2) freq_frames_lavc<true, BL_MEL_WAVES, false>(pcm, sg, tb, nullptr, nullptr, nullptr, &pf);
  else freq_frames_lavc<false, BL_MEL_WAVES, false>(pcm, sg, tb, nullptr, nullptr, nullptr, &pf);
}

/* bl_amd_selftest_ilog2: out[i] = L(bl_ilog2_sweep_value(i)) for i < BL_ILOG2_SWEEP; index 0 is no value of the domain */
__global__ __launch_bounds__(256) void k_ilog2_sweep(uint32_t *out) {
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < BL_ILOG2_SWEEP; i += gridDim.x * 256u) {
    const bl_u64 x = bl_ilog2_sweep_value(i);
    out[i] = x ? bl_ilog2_q12(x) : 0u;
  }
}

/* ========================================================================= */
/* launchers (declared in bl_launch.h)                                        */

static std::vector<unsigned char> mel_build_image() {
  std::vector<uint8_t> w((size_t)BL_MEL_BANDS * BL_MEL_BINS);
  int32_t dct[BL_MEL_COEFFS * BL_MEL_BANDS];
  if (bl_mel_build(nullptr, w.data(), dct) != 0) return std::vector<unsigned char>(); /* the bounds would not hold */
  std::vector<unsigned char> img(BL_MEL_IMAGE_BYTES, 0);
  for (int b = 0; b < BL_MEL_BANDS; ++b) {
    const uint8_t *row = w.data() + (size_t)b * BL_MEL_BINS;
    int d0 = 0, n = 0;
    for (int d = 1; d < BL_MEL_BINS; ++d)
      if (row[d]) { d0 = n ? d0 : d; n += 1; }
    unsigned char *bd = img.data() + (size_t)b * BL_MEL_BAND_STRIDE;
    bd[0] = (unsigned char)d0;
    bd[1] = (unsigned char)n;
    for (int j = 0; j < n; ++j) bd[4 + j] = row[d0 + j]; /* contiguous: bl_mel_build checked it */
  }
  int16_t *dl = reinterpret_cast<int16_t *>(img.data() + BL_MEL_DCT_OFF);
  for (int s = 0; s < 8; ++s)
    for (int k = 0; k < BL_MEL_COEFFS; ++k)
      for (int q = 0; q < 4; ++q) dl[(s * BL_MEL_COEFFS + k) * 4 + q] = (int16_t)dct[k * BL_MEL_BANDS + mel_band(s, q)];
  return img;
}

size_t blk_mel_image_bytes(void) { return BL_MEL_IMAGE_BYTES; }

const unsigned char *blk_mel_image_host(void) {
  static const std::vector<unsigned char> img = mel_build_image();
  return img.empty() ? nullptr : img.data();
}

int blk_mel_configure_device(void) {
  BL_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_mel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   BL_MEL_LDS_BYTES));
  return BL_OK;
}

int blk_mel(hipStream_t s, const int16_t *d_pcm, const bl_timbre_song *d_songs, int n_songs, const bl_tables &tb,
            const void *d_image, unsigned long long min_energy, bl_amd_song_mel *d_songs_out,
            bl_amd_frame_mel *d_frames, uint32_t *d_bands) {
  hipLaunchKernelGGL(k_mel, dim3(n_songs), dim3(64 * BL_MEL_WAVES), BL_MEL_LDS_BYTES, s, d_pcm, d_songs, tb,
                     static_cast<const uint4 *>(d_image), min_energy, d_songs_out, d_frames, d_bands);
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}

int blk_ilog2_sweep(hipStream_t s, uint32_t *d_out, int n_cu) {
  hipLaunchKernelGGL(k_ilog2_sweep, dim3(n_cu > 0 ? n_cu : 64), dim3(256), 0, s, d_out);
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}
