/*
 * bl_chroma_kernels.hip — gfx950 kernels and launch layer of chroma and key (bl_amd_chroma_batch_device,
 * include/bliss_amd.h: bl_amd_song_chroma, bl_amd_frame_chroma).  Nothing of the reference's analysis is restated here:
 * "Chromagram / HPCP" is a row of its author's ROADMAP.md.  Every quantity is an exact integer (the definitions are in
 * the header), so neither the split of a song over waves nor the order of the atomics that join them shows in a result.
 *
 * Kernels:
 *   k_chroma_pitch  the constant-Q bank as int8 matrix products (v_mfma_i32_16x16x64_i8): 96 rows (48 pitches x re / im)
 *                   by 16 frames per wave, K = the frame's 4 096 samples; then energies, the fold into twelve classes,
 *                   the frame records and the song's sums (64-bit integer atomics, one per wave and class)
 *   k_chroma_key    one lane per song: the 24 profile scores and the record
 *
 * Formulation.  A column of the product is a FRAME, not a block of 2 048: a sample still meets each of the 96 rows
 * in two frames, the same 768 int8 operations per mono sample as 192 half-rows on blocks would take, and nothing has
 * to be joined across column tiles; the price is that a sample is loaded (and split into bytes) twice.  A sample is
 * s = 256 h + l' + 128 with h = s >> 8 and l' = (s & 255) - 128 as in bl_fir_int.h, so
 *     sum c s = sum c l' + 256 sum c h + 128 sum c:
 * two products per row tile, the constant 128 sum_n c[n] of each row in the initial value of the first.  Stereo uses
 * linearity, not a mixed 17-bit sample with a third digit: the lane takes the left and the right bytes of its frames
 * apart (two v_perm levels) and the four planes l'_L, l'_R, h_L, h_R meet the SAME coefficient registers — four
 * products per row tile and 64 frames against the three a mixed sample would need, but no addition, no third split and
 * one coefficient image for both layouts.  Mono doubles the sum at the end (m = 2 s).
 * Bounds: sum |c| <= 140 000 per row (checked when the image is built), |l'|, |h| <= 128, so the first accumulator
 * stays below 2 * 128 * 140 000 + 2 * 128 * 140 000 < 2^27 and the second below 2^26: int32 never wraps; the rest is
 * int64 (header).
 *
 * Operand layout.  K-step ks (0 .. 63) of a frame is 64 samples; lane group g = lane >> 4 holds, in byte j of its 16,
 * sample ch_kappa(ks, g, j) = 128 (ks >> 1) + 32 g + 16 (ks & 1) + j of the frame: a lane's two K-steps of a block of
 * 128 frames are 32 consecutive frames, 64 (mono) or 128 (stereo) contiguous bytes of PCM.  BOTH operands are laid out
 * by that one rule (the image is built with it on the host), so a product pairs equal samples whatever order the
 * hardware walks K in.  A operand: row 16 rt + (lane & 15) of the bank, row R = 2 p + (0: cr, 1: ci); B operand:
 * column lane & 15 = frame 16 tile + (lane & 15); result register r of lane (col, g): row 16 rt + 4 g + r, that is both
 * parts of pitches 8 rt + 2 g and 8 rt + 2 g + 1, so the energy is formed in the lane.
 *
 * Zero blocks.  The windows are centred and short for high pitches (sum L_p is 57 k of 196 k entries): the image
 * carries, per block of 128 samples, a mask of the row tiles that have a non-zero coefficient there, built from the
 * table; a block no row tile needs is not even loaded.
 */
#include <hip/hip_runtime.h>

#include <vector>

#include "bl_chroma_table.h"
#include "bl_fir_int.h"
#include "bl_launch.h"

typedef unsigned long long bl_u64;
typedef int ch_v4i __attribute__((ext_vector_type(4)));

#define CH_RT 6                    /* row tiles of 16: 96 rows */
#define CH_KS 64                   /* K-steps of 64 samples per frame */
#define CH_KP 32                   /* blocks of 128 samples (two K-steps) per frame */
#define CH_ROWS (2 * BL_CHROMA_PITCHES)
#define CH_OFF_CSUM ((size_t)CH_RT * CH_KS * 64 * 16)        /* int32 [96]: 128 sum_n c[R][n] */
#define CH_OFF_GAIN (CH_OFF_CSUM + sizeof(int) * CH_ROWS)    /* uint32 [48] */
#define CH_OFF_LIVE (CH_OFF_GAIN + sizeof(unsigned) * BL_CHROMA_PITCHES) /* uint32 [32]: bit rt = row tile rt is live */
#define CH_IMAGE_BYTES (CH_OFF_LIVE + sizeof(unsigned) * CH_KP)

__host__ __device__ __forceinline__ int ch_kappa(int ks, int g, int j) {
  return 128 * (ks >> 1) + 32 * g + 16 * (ks & 1) + j;
}

/* 16 mono samples (8 words as loaded) -> the planes of l' and of h, byte e of word q = sample 4 q + e */
__device__ __forceinline__ void ch_planes_mono(const unsigned w[8], ch_v4i &lo, ch_v4i &hi) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    lo[q] = (int)(bl_firi_perm(w[2 * q + 1], w[2 * q], 0x06040200u) ^ 0x80808080u);
    hi[q] = (int)bl_firi_perm(w[2 * q + 1], w[2 * q], 0x07050301u);
  }
}

/* 16 stereo frames (16 words, left in the low half) -> the four planes.  Level one: two frames' low bytes
 * [l0 l1 r0 r1] and high bytes; level two: the left halves and the right halves of two such words. */
__device__ __forceinline__ void ch_planes_stereo(const unsigned w[16], ch_v4i &llo, ch_v4i &rlo, ch_v4i &lhi,
                                                 ch_v4i &rhi) {
  unsigned a[8], b[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    a[i] = bl_firi_perm(w[2 * i + 1], w[2 * i], 0x06020400u);
    b[i] = bl_firi_perm(w[2 * i + 1], w[2 * i], 0x07030501u);
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    llo[q] = (int)(bl_firi_perm(a[2 * q + 1], a[2 * q], 0x05040100u) ^ 0x80808080u);
    rlo[q] = (int)(bl_firi_perm(a[2 * q + 1], a[2 * q], 0x07060302u) ^ 0x80808080u);
    lhi[q] = (int)bl_firi_perm(b[2 * q + 1], b[2 * q], 0x05040100u);
    rhi[q] = (int)bl_firi_perm(b[2 * q + 1], b[2 * q], 0x07060302u);
  }
}

/* One song on the workgroups of its grid row.  A wave owns column tile 4 tg + wave of tile group tg; every wave of a
 * workgroup takes the same number of turns (a wave whose tile lies behind the song skips the products and contributes
 * zeros), so the barriers see whole workgroups.  sE: the wave's [16 columns][48 pitches], sX: its [16][12]. */
template <bool MONO>
__device__ __forceinline__ void ch_song(const int16_t *p, int T, const unsigned char *img, bl_u64 *acc,
                                        bl_amd_frame_chroma *frames, bl_u64 (*sE)[BL_CHROMA_PITCHES], bl_u64 (*sX)[12]) {
  constexpr int NQ = MONO ? 4 : 8;   /* 16-byte vectors of a lane's 32 frames */
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, grp = lane >> 4;
  const int ntile = (T + 15) / 16, ngroup = (ntile + 3) / 4;
  const ch_v4i *A = reinterpret_cast<const ch_v4i *>(img);
  const int *csum = reinterpret_cast<const int *>(img + CH_OFF_CSUM);
  const unsigned *gain = reinterpret_cast<const unsigned *>(img + CH_OFF_GAIN);
  const unsigned *live = reinterpret_cast<const unsigned *>(img + CH_OFF_LIVE);
  bl_u64 run = 0; /* lanes 0 .. 11: the wave's share of chroma[lane] */
  for (int tg = blockIdx.x; tg < ngroup; tg += gridDim.x) {
    const int tile = 4 * tg + wave, t = 16 * tile + col;
    const bool valid = t < T;
    ch_v4i c0[CH_RT], c1[CH_RT];
#pragma unroll
    for (int rt = 0; rt < CH_RT; ++rt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        c0[rt][r] = (MONO ? 1 : 2) * csum[16 * rt + 4 * grp + r];
        c1[rt][r] = 0;
      }
    }
    if (16 * tile < T) {
      /* the lane's 32 frames of block kp start at frame 2048 t + 128 kp + 32 grp of the song: 8 (mono) or 4 (stereo)
       * frames to a 16-byte vector */
      const uint4 *src = reinterpret_cast<const uint4 *>(p) + (size_t)(NQ / 4) * (256 * (size_t)(valid ? t : 0) + 4 * grp);
      for (int kp = 0; kp < CH_KP; ++kp) {
        const unsigned mask = live[kp];
        if (!mask) continue;
        uint4 q[NQ];
#pragma unroll
        for (int i = 0; i < NQ; ++i) q[i] = valid ? src[(size_t)kp * (4 * NQ) + i] : make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          unsigned w[2 * NQ];
#pragma unroll
          for (int i = 0; i < NQ / 2; ++i) {
            const uint4 v = q[h * (NQ / 2) + i];
            w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
          }
          ch_v4i b0, b1 = {0, 0, 0, 0}, b2, b3 = {0, 0, 0, 0};
          if constexpr (MONO) ch_planes_mono(w, b0, b2);
          else ch_planes_stereo(w, b0, b1, b2, b3);
          const ch_v4i *Ak = A + ((size_t)(2 * kp + h) * 64 + lane);
#pragma unroll
          for (int rt = 0; rt < CH_RT; ++rt) {
            if (!((mask >> rt) & 1u)) continue;
            const ch_v4i a = Ak[(size_t)rt * CH_KS * 64];
            c0[rt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b0, c0[rt], 0, 0, 0);
            c1[rt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b2, c1[rt], 0, 0, 0);
            if constexpr (!MONO) {
              c0[rt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b1, c0[rt], 0, 0, 0);
              c1[rt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b3, c1[rt], 0, 0, 0);
            }
          }
        }
      }
    }
    /* energies of the lane's twelve pitches */
#pragma unroll
    for (int rt = 0; rt < CH_RT; ++rt) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int pitch = 8 * rt + 2 * grp + u;
        long long re = (long long)c0[rt][2 * u] + 256ll * (long long)c1[rt][2 * u];
        long long im = (long long)c0[rt][2 * u + 1] + 256ll * (long long)c1[rt][2 * u + 1];
        if (MONO) { re *= 2; im *= 2; }
        const long long a = re >> 15, b = im >> 15;
        const bl_u64 e = (bl_u64)(a * a) + (bl_u64)(b * b);
        sE[col][pitch] = (e * (bl_u64)gain[pitch]) >> 16;
      }
    }
    __syncthreads();
    /* fold: 16 columns x 12 classes on 64 lanes; class k collects the pitches p = k + 3 (mod 12) */
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int i = lane + 64 * j, c = i / 12, k = i % 12, p0 = (k + 3) % 12, tt = 16 * tile + c;
      const bl_u64 X = sE[c][p0] + sE[c][p0 + 12] + sE[c][p0 + 24] + sE[c][p0 + 36];
      const bool ok = tt < T;
      if (ok && frames) frames[tt].x[k] = X;
      sX[c][k] = ok ? X : 0;
    }
    __syncthreads();
    if (lane < 12) {
#pragma unroll
      for (int c = 0; c < 16; ++c) run += sX[c][lane];
    }
  }
  if (lane < 12 && run) atomicAdd(acc + lane, run);
}

__global__ __launch_bounds__(256) void k_chroma_pitch(const int16_t *__restrict__ pcm,
                                                      const bl_chroma_song *__restrict__ songs,
                                                      const unsigned char *__restrict__ img, bl_u64 *acc,
                                                      bl_amd_frame_chroma *frames) {
  __shared__ bl_u64 sE[4][16][BL_CHROMA_PITCHES];
  __shared__ bl_u64 sX[4][16][12];
  const bl_chroma_song sg = songs[blockIdx.y];
  const int wave = threadIdx.x >> 6;
  const int16_t *p = pcm + sg.pcm_off;
  bl_amd_frame_chroma *f = frames ? frames + sg.frame_off : nullptr;
  bl_u64 *a = acc + 12 * (size_t)blockIdx.y;
  if (sg.channels == 1) ch_song<true>(p, sg.frames, img, a, f, sE[wave], sX[wave]);
  else ch_song<false>(p, sg.frames, img, a, f, sE[wave], sX[wave]);
}

/* k_chroma_key: one lane per song.  Every byte of the record is written. */
__global__ __launch_bounds__(64) void k_chroma_key(const bl_chroma_song *__restrict__ songs, const bl_u64 *acc, int n,
                                                   bl_amd_song_chroma *out) {
  const int QM[12] = {10737, -4690, -9, -4315, 3361, 2275, -3604, 6394, -4091, 665, -4465, -2256};
  const int Qm[12] = {10733, -4215, -775, 6842, -4542, -734, -4788, 4262, 1109, -4174, -1512, -2208};
  const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (i >= n) return;
  const int T = songs[i].frames;
  bl_u64 ch[12], mx = 0;
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    ch[k] = T ? acc[12 * (size_t)i + k] : 0;
    mx = ch[k] > mx ? ch[k] : mx;
  }
  long long best = 0, next = 0;
  int key = -1;
  if (mx) {
    const int bits = 64 - __clzll(mx), s = bits > 12 ? bits - 12 : 0;
    long long c[12], score[24];
#pragma unroll
    for (int k = 0; k < 12; ++k) c[k] = (long long)(ch[k] >> s);
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      long long sM = 0, sm = 0;
#pragma unroll
      for (int j = 0; j < 12; ++j) {
        sM += QM[j] * c[(j + k) % 12];
        sm += Qm[j] * c[(j + k) % 12];
      }
      score[k] = sM;
      score[12 + k] = sm;
    }
    key = 0;
    best = score[0];
#pragma unroll
    for (int k = 1; k < 24; ++k)
      if (score[k] > best) { best = score[k]; key = k; }
    bool first = true;
#pragma unroll
    for (int k = 0; k < 24; ++k)
      if (k != key && (first || score[k] > next)) { next = score[k]; first = false; }
  }
  bl_amd_song_chroma *rec = out + i;
#pragma unroll
  for (int k = 0; k < 12; ++k) rec->chroma[k] = ch[k];
  rec->score = best;
  rec->score_next = next;
  rec->frames = T;
  rec->key = key;
  rec->status = T ? BL_OK : BL_UNEXPECTED;
  rec->reserved = 0;
}

/* ========================================================================= */
/* launchers (declared in bl_launch.h)                                        */

size_t blk_chroma_image_bytes(void) { return CH_IMAGE_BYTES; }

static std::vector<unsigned char> ch_build_image() {
  std::vector<int8_t> re((size_t)BL_CHROMA_PITCHES * BL_CHROMA_FRAME), im(re.size());
  uint32_t gain[BL_CHROMA_PITCHES];
  bl_chroma_build(re.data(), im.data(), gain, nullptr);
  std::vector<unsigned char> img(CH_IMAGE_BYTES, 0);
  int csum[CH_ROWS];
  unsigned live[CH_KP] = {0};
  for (int R = 0; R < CH_ROWS; ++R) {
    const int8_t *row = ((R & 1) ? im.data() : re.data()) + (size_t)(R >> 1) * BL_CHROMA_FRAME;
    long long sum = 0, abs_sum = 0;
    for (int n = 0; n < BL_CHROMA_FRAME; ++n) {
      sum += row[n];
      abs_sum += row[n] < 0 ? -row[n] : row[n];
      if (row[n]) live[n / 128] |= 1u << (R / 16);
    }
    if (abs_sum > BL_CHROMA_ABS_SUM_MAX) return std::vector<unsigned char>(); /* the int32 bounds would not hold */
    csum[R] = (int)(128 * sum);
    for (int ks = 0; ks < CH_KS; ++ks)
      for (int g = 0; g < 4; ++g)
        for (int j = 0; j < 16; ++j)
          img[((((size_t)(R / 16) * CH_KS + ks) * 64) + 16 * g + (R % 16)) * 16 + j] =
              (unsigned char)row[ch_kappa(ks, g, j)];
  }
  memcpy(img.data() + CH_OFF_CSUM, csum, sizeof(csum));
  memcpy(img.data() + CH_OFF_GAIN, gain, sizeof(gain));
  memcpy(img.data() + CH_OFF_LIVE, live, sizeof(live));
  return img;
}

const unsigned char *blk_chroma_image_host(void) {
  static const std::vector<unsigned char> img = ch_build_image();
  return img.empty() ? nullptr : img.data();
}

int blk_chroma(hipStream_t s, const int16_t *d_pcm, const bl_chroma_song *d_songs, int n_songs, int max_frames,
               int n_cu, const void *d_image, unsigned long long *d_acc, bl_amd_song_chroma *d_songs_out,
               bl_amd_frame_chroma *d_frames, blk_mark_fn mark, void *mark_user) {
  BL_HIP_CHECK(hipMemsetAsync(d_acc, 0, sizeof(bl_u64) * 12 * (size_t)n_songs, s));
  if (max_frames > 0) {
    Mark m(mark, mark_user, PK_CHROMA_PITCH, s);
    const int groups = ((max_frames + 15) / 16 + 3) / 4;
    hipLaunchKernelGGL(k_chroma_pitch, dim3(grid_x_for(groups, n_songs, 8, n_cu), n_songs), dim3(256), 0, s, d_pcm,
                       d_songs, static_cast<const unsigned char *>(d_image), d_acc, d_frames);
  }
  {
    Mark m(mark, mark_user, PK_CHROMA_KEY, s);
    hipLaunchKernelGGL(k_chroma_key, dim3((n_songs + 63) / 64), dim3(64), 0, s, d_songs, d_acc, n_songs, d_songs_out);
  }
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}
