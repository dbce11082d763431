/*
 * bl_level_kernels.hip — gfx950 kernels and launch layer of the per-song signal levels (bl_amd_levels_batch_device,
 * include/bliss_amd.h: bl_amd_song_levels).  Nothing of the reference's analysis is restated here: the quantities are
 * those its author's ROADMAP.md names as next ("zero-crossing rate", "rough measure of the dB level of songs") and the
 * four samples ref examples/detect-gapless.c:28-33 reads.  Every accumulated quantity is an integer, so the atomics
 * that join the waves of a song do not disturb determinism.
 *
 * Kernels:
 *   k_level_scan   per channel: sum, sum of squares, minimum / maximum (the peak), zero crossings, clipped samples,
 *                  in one streaming pass shaped like k_pcm_scan (bl_stats_kernels.hip)
 *   k_level_ends   lead / trail (a search from both ends, as k_trim), frames, status, head and tail
 *
 * Layout of the arithmetic.  A 32-bit word holds two samples.  Stereo: the low half is channel 0 and the high half
 * channel 1 of one frame.  Mono: two consecutive frames of channel 0.  The pass therefore accumulates per HALF (low,
 * high) whatever the song is, and only the end of the kernel knows channels: stereo takes the halves as the channels,
 * mono adds them into channel 0.  The one thing that differs inside the loop is the predecessor of a sample for the
 * zero crossings: the same half of the previous word (stereo), or the previous half (mono), which is the previous
 * word and this one shifted by 16 bits (v_alignbit_b32).
 *
 * Seams.  The predecessor of the first word of a 16-byte vector is the last word of the vector before it in memory,
 * whoever owns that vector (the next lane, the other load in flight, another block): every lane loads that one word
 * itself, from a line its wave is loading anyway.  Vector 0 has no predecessor frame and takes its own first frame.
 * The up to seven samples behind the last whole vector are taken one per lane by block 0, each with its own
 * predecessor sample.
 *
 * Nothing packed lives longer than one vector.  The 16-bit packed counters (crossings, clips) count the 4 samples a
 * half has in a vector, at most 4, and the 32-bit partial sums hold 4 samples (|sum| <= 2^17) or 2 squares (<= 2^31,
 * read as unsigned); each is added to a 32-bit counter or a 64-bit sum before the next vector.  A lane's 32-bit
 * counters see at most n / 2 <= 2^30 samples per half, the 64-bit sums at most 2^31 * 2^30.  So there is no flush
 * interval to get wrong: it is one vector.
 */
#include <hip/hip_runtime.h>

#include "bl_launch.h"

typedef short bl_s2 __attribute__((ext_vector_type(2)));
typedef unsigned short bl_us2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ bl_s2 as_s2(unsigned w) { bl_s2 v; __builtin_memcpy(&v, &w, 4); return v; }
__device__ __forceinline__ bl_us2 as_us2(unsigned w) { bl_us2 v; __builtin_memcpy(&v, &w, 4); return v; }
__device__ __forceinline__ unsigned as_u32(bl_s2 v) { unsigned w; __builtin_memcpy(&w, &v, 4); return w; }
__device__ __forceinline__ unsigned as_u32(bl_us2 v) { unsigned w; __builtin_memcpy(&w, &v, 4); return w; }

/* per-half accumulators of one lane */
struct lv_acc {
  long long sum[2];
  unsigned long long sq[2];
  bl_s2 mx, mn;        /* packed maximum / minimum of each half: |-32768| does not fit an int16, so both are kept */
  unsigned zc[2], cl[2];
};

/* One 16-byte vector (words q.x .. q.w); before: the word in front of q.x in memory (see "Seams"). */
template <bool MONO>
__device__ __forceinline__ void lv_eat(const uint4 q, unsigned before, lv_acc &a) {
  const unsigned w[4] = {q.x, q.y, q.z, q.w};
  const bl_us2 one = {1, 1};
  const bl_s2 sel_lo = {1, 0}, sel_hi = {0, 1};
  bl_us2 zc = {0, 0}, cl = {0, 0};
  int s_lo = 0, s_hi = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    /* the predecessor of each half: the same half of the previous word, or (mono) the half before it */
    const unsigned pred = MONO ? __builtin_amdgcn_alignbit(w[k], before, 16) : before;
    before = w[k];
    zc += as_us2(w[k] ^ pred) >> 15; /* the sign bits differ; 0 counts as non-negative */
    /* s ^ (s >> 15) is 32767 for s = 32767 and s = -32768 only, and in [0, 32767) otherwise: + 1 reaches bit 15 */
    const bl_s2 s = as_s2(w[k]);
    cl += (as_us2(as_u32(s ^ (s >> 15))) + one) >> 15;
    a.mx = __builtin_elementwise_max(a.mx, s);
    a.mn = __builtin_elementwise_min(a.mn, s);
    s_lo = __builtin_amdgcn_sdot2(s, sel_lo, s_lo, false);
    s_hi = __builtin_amdgcn_sdot2(s, sel_hi, s_hi, false);
  }
  a.sum[0] += s_lo;
  a.sum[1] += s_hi;
  /* squares: two of one half per 32-bit partial (2 * 2^30 = 2^31 read as unsigned), then one v_mad_u64_u32 into the
   * 64-bit sum, as scan_word (bl_scan.h) does */
#pragma unroll
  for (int k = 0; k < 4; k += 2) {
    unsigned r_lo, r_hi;
    asm("v_mad_i32_i16 %0, %1, %1, 0 op_sel:[0,0,0,0]" : "=v"(r_lo) : "v"(w[k]));
    asm("v_mad_i32_i16 %0, %1, %1, %2 op_sel:[0,0,0,0]" : "=v"(r_lo) : "v"(w[k + 1]), "v"(r_lo));
    asm("v_mad_i32_i16 %0, %1, %1, 0 op_sel:[1,1,0,0]" : "=v"(r_hi) : "v"(w[k]));
    asm("v_mad_i32_i16 %0, %1, %1, %2 op_sel:[1,1,0,0]" : "=v"(r_hi) : "v"(w[k + 1]), "v"(r_hi));
    asm("v_mad_u64_u32 %0, vcc, %1, 1, %0" : "+v"(a.sq[0]) : "v"(r_lo) : "vcc");
    asm("v_mad_u64_u32 %0, vcc, %1, 1, %0" : "+v"(a.sq[1]) : "v"(r_hi) : "vcc");
  }
  const unsigned z = as_u32(zc), c = as_u32(cl);
  a.zc[0] += z & 0xFFFFu;
  a.zc[1] += z >> 16;
  a.cl[0] += c & 0xFFFFu;
  a.cl[1] += c >> 16;
}

/* the whole vectors [0, nvec) of one song that this block's lanes own: two loads in flight per lane */
template <bool MONO>
__device__ __forceinline__ void lv_pass(const int16_t *p, unsigned nvec, lv_acc &a) {
  const uint4 *pv = reinterpret_cast<const uint4 *>(p);
  const unsigned *pw = reinterpret_cast<const unsigned *>(p);
  /* vector 0 has no frame in front of it: its first frame stands in, which is no crossing */
  auto word_before = [&](unsigned v, const uint4 q) -> unsigned {
    const unsigned b = pw[v ? 4u * v - 1u : 0u];
    return v ? b : (MONO ? q.x << 16 : q.x);
  };
  const unsigned gstride = gridDim.x * 256u;
  unsigned v = blockIdx.x * 256u + threadIdx.x;
  for (; v + gstride < nvec; v += 2 * gstride) {
    const uint4 q0 = pv[v], q1 = pv[v + gstride];
    const unsigned b0 = word_before(v, q0), b1 = word_before(v + gstride, q1);
    lv_eat<MONO>(q0, b0, a);
    lv_eat<MONO>(q1, b1, a);
  }
  if (v < nvec) {
    const uint4 q = pv[v];
    lv_eat<MONO>(q, word_before(v, q), a);
  }
}

/* record of one song on the device: bl_level_song (bl_launch.h) */
__global__ __launch_bounds__(256) void k_level_scan(const int16_t *__restrict__ pcm,
                                                    const bl_level_song *__restrict__ songs,
                                                    bl_amd_song_levels *levels) {
  const bl_level_song sg = songs[blockIdx.y];
  const int16_t *p = pcm + sg.pcm_off;
  const int ch = sg.channels;
  const unsigned ne = (unsigned)(sg.n / ch) * (unsigned)ch; /* samples that belong to a frame */
  const unsigned nvec = ne >> 3, rest = ne & 7u;
  if (blockIdx.x * 256u >= nvec && !(blockIdx.x == 0 && rest)) return; /* a block with nothing to read */
  lv_acc a;
  a.sum[0] = a.sum[1] = 0;
  a.sq[0] = a.sq[1] = 0;
  a.mx = (bl_s2){-32768, -32768};
  a.mn = (bl_s2){32767, 32767};
  a.zc[0] = a.zc[1] = a.cl[0] = a.cl[1] = 0;
  if (ch == 1) lv_pass<true>(p, nvec, a);
  else lv_pass<false>(p, nvec, a);

  /* halves -> channels */
  long long sum[2] = {a.sum[0], a.sum[1]};
  unsigned long long sq[2] = {a.sq[0], a.sq[1]};
  int hi[2] = {a.mx.x, a.mx.y}, lo[2] = {a.mn.x, a.mn.y};
  unsigned zc[2] = {a.zc[0], a.zc[1]}, cl[2] = {a.cl[0], a.cl[1]};
  if (ch == 1) {
    sum[0] += sum[1]; sq[0] += sq[1]; zc[0] += zc[1]; cl[0] += cl[1];
    hi[0] = max(hi[0], hi[1]); lo[0] = min(lo[0], lo[1]);
    sum[1] = 0; sq[1] = 0; zc[1] = 0; cl[1] = 0; hi[1] = -32768; lo[1] = 32767;
  }
  /* the samples behind the last whole vector, one per lane */
  if (blockIdx.x == 0 && threadIdx.x < rest) {
    const unsigned i = 8u * nvec + threadIdx.x;
    const int s = p[i], c = ch == 1 ? 0 : (int)(i & 1u);
    if (c == 0) {
      sum[0] += s; sq[0] += (unsigned)(s * s); hi[0] = max(hi[0], s); lo[0] = min(lo[0], s);
      cl[0] += (s == 32767 || s == -32768);
      if (i >= (unsigned)ch) zc[0] += (s < 0) != (p[i - ch] < 0);
    } else {
      sum[1] += s; sq[1] += (unsigned)(s * s); hi[1] = max(hi[1], s); lo[1] = min(lo[1], s);
      cl[1] += (s == 32767 || s == -32768);
      if (i >= (unsigned)ch) zc[1] += (s < 0) != (p[i - ch] < 0);
    }
  }
  /* a lane that saw no sample of a channel has hi = -32768, lo = 32767: its peak is 0 */
  int peak[2] = {max(max(hi[0], -lo[0]), 0), max(max(hi[1], -lo[1]), 0)};
  /* wave reduction, then one integer atomic per wave and field */
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      sum[c] += __shfl_down(sum[c], off);
      sq[c] += __shfl_down(sq[c], off);
      peak[c] = max(peak[c], __shfl_down(peak[c], off));
      zc[c] += __shfl_down(zc[c], off);
      cl[c] += __shfl_down(cl[c], off);
    }
  }
  if ((threadIdx.x & 63) == 0) {
    bl_amd_song_levels *lv = levels + blockIdx.y;
    for (int c = 0; c < ch; ++c) {
      atomicAdd(reinterpret_cast<unsigned long long *>(&lv->sum[c]), (unsigned long long)sum[c]);
      atomicAdd(reinterpret_cast<unsigned long long *>(&lv->sum_sq[c]), sq[c]);
      atomicMax(&lv->peak[c], peak[c]);
      atomicAdd(&lv->zero_cross[c], (int)zc[c]);
      atomicAdd(&lv->clipped[c], (int)cl[c]);
    }
  }
}

/* bit i of the result: sample i of the vector is loud, |s| > silence.  As 16-bit unsigned numbers
 * (s + silence) mod 2^16 > 2 * silence says exactly that for 0 <= silence <= 32767: a sample in [-silence, silence]
 * lands in [0, 2 silence], a louder positive one in (2 silence, 65534], a louder negative one wraps to
 * [32768 + silence, 65535]. */
__device__ __forceinline__ bool lv_loud(int s, int silence) {
  return (unsigned)((s + silence) & 0xFFFF) > 2u * (unsigned)silence;
}
__device__ __forceinline__ unsigned lv_loud_mask(const uint4 q, int silence) {
  const unsigned w[4] = {q.x, q.y, q.z, q.w};
  unsigned m = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    m |= (unsigned)lv_loud((int)(w[k] & 0xFFFFu), silence) << (2 * k);
    m |= (unsigned)lv_loud((int)(w[k] >> 16), silence) << (2 * k + 1);
  }
  return m;
}

/* k_level_ends: lead and trail of every song, and the fields that are no sums.  A search, not a pass, as k_trim
 * (bl_stats_kernels.hip): one workgroup per song, wave 0 walks forward and wave 1 backward over the samples that
 * belong to a frame, 1 024 per step, until a vector with a loud sample turns up; only an all-silent song is searched
 * whole.  The frame of sample i is i / channels. */
__global__ __launch_bounds__(128) void k_level_ends(const int16_t *__restrict__ pcm,
                                                    const bl_level_song *__restrict__ songs, int silence,
                                                    bl_amd_song_levels *levels) {
  const bl_level_song sg = songs[blockIdx.x];
  const int16_t *p = pcm + sg.pcm_off;
  const uint4 *pv = reinterpret_cast<const uint4 *>(p);
  const int lane = threadIdx.x & 63, ch = sg.channels;
  const int frames = sg.n / ch, ne = frames * ch, nvec = ne >> 3;
  const bool fwd = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) == 0;
  bl_amd_song_levels *lv = levels + blockIdx.x;
  const uint4 z = make_uint4(0, 0, 0, 0);
  if (fwd) {
    int first = -1; /* first loud sample */
    for (int v0 = 0; v0 < nvec; v0 += 128) {
      const int va = v0 + lane, vb = v0 + 64 + lane;
      const uint4 qa = va < nvec ? pv[va] : z, qb = vb < nvec ? pv[vb] : z;
      const unsigned la = va < nvec ? lv_loud_mask(qa, silence) : 0u, lb = vb < nvec ? lv_loud_mask(qb, silence) : 0u;
      const unsigned long long ma = __ballot(la != 0u), mb = __ballot(lb != 0u);
      if (ma | mb) {
        const int src = ma ? __builtin_ctzll(ma) : __builtin_ctzll(mb);
        const int mine = 8 * (ma ? va : vb) + (int)__builtin_ctz((ma ? la : lb) | 0x100u);
        first = __shfl(mine, src);
        break;
      }
    }
    if (first < 0) /* nothing in the whole vectors: the up to seven samples behind them */
      for (int i = 8 * nvec; i < ne; ++i)
        if (lv_loud(p[i], silence)) { first = i; break; }
    if (lane == 0) {
      lv->lead = first < 0 ? frames : first / ch;
      lv->frames = frames;
      lv->status = BL_OK;
      lv->head[0] = p[0];
      lv->head[1] = p[1];
      lv->tail[0] = p[sg.n - 2];
      lv->tail[1] = p[sg.n - 1];
    }
  } else {
    int last = -1; /* last loud sample */
    for (int i = ne - 1; i >= 8 * nvec; --i)
      if (lv_loud(p[i], silence)) { last = i; break; }
    if (last < 0)
      for (int v1 = nvec; v1 > 0; v1 -= 128) { /* vectors [v1 - 128, v1) */
        const int va = v1 - 1 - lane, vb = v1 - 65 - lane;
        const uint4 qa = va >= 0 ? pv[va] : z, qb = vb >= 0 ? pv[vb] : z;
        const unsigned la = va >= 0 ? lv_loud_mask(qa, silence) : 0u, lb = vb >= 0 ? lv_loud_mask(qb, silence) : 0u;
        const unsigned long long ma = __ballot(la != 0u), mb = __ballot(lb != 0u);
        if (ma | mb) { /* lane 0 holds the highest vector of each half */
          const int src = ma ? __builtin_ctzll(ma) : __builtin_ctzll(mb);
          const int mine = 8 * (ma ? va : vb) + 31 - (int)__builtin_clz((ma ? la : lb) | 1u);
          last = __shfl(mine, src);
          break;
        }
      }
    if (lane == 0) lv->trail = last < 0 ? frames : frames - 1 - last / ch;
  }
}

/* ========================================================================= */
/* launcher (declared in bl_launch.h)                                         */

int blk_levels(hipStream_t s, const int16_t *d_pcm, const bl_level_song *d_songs, int n_songs, int max_n, int silence,
               int n_cu, bl_amd_song_levels *d_levels) {
  /* the sums, the peak and the counts start from zero; k_level_ends writes the other fields of every record */
  BL_HIP_CHECK(hipMemsetAsync(d_levels, 0, sizeof(bl_amd_song_levels) * (size_t)n_songs, s));
  for (int b = 0; b < n_songs; b += BL_LEVEL_GROUP_SONGS) { /* gridDim.y and gridDim.x are 16-bit on the safe side */
    const int cnt = n_songs - b < BL_LEVEL_GROUP_SONGS ? n_songs - b : BL_LEVEL_GROUP_SONGS;
    const int gx = grid_x_for(((long long)max_n / 8 + 255) / 256, cnt, 8, n_cu);
    hipLaunchKernelGGL(k_level_scan, dim3(gx, cnt), dim3(256), 0, s, d_pcm, d_songs + b, d_levels + b);
    hipLaunchKernelGGL(k_level_ends, dim3(cnt), dim3(128), 0, s, d_pcm, d_songs + b, silence, d_levels + b);
  }
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}
