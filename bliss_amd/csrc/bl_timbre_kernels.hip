/*
 * bl_timbre_kernels.hip — gfx950 kernel and launch layer of the per-frame spectral timbre (bl_amd_timbre_batch_device,
 * include/bliss_amd.h: bl_amd_frame_timbre, bl_amd_song_timbre).  The frames, the window, the transform and the power
 * values are the frequency pass's own (freq_frames_lavc, bl_freq_frames.h: one piece of source, compiled here in its
 * per-frame form); what is new is the stage behind the transform.  Must be compiled with -ffp-contract=off.
 *
 * Kernel:
 *   k_timbre   one workgroup of four waves per song.  A wave transforms eight frames per iteration; once their 255
 *              power values each lie in the wave's staging rows it turns every frame into energy, moment, rolloff and
 *              peak (bl_timbre_frames::frames) and keeps the song's sums in registers; the workgroup joins them at the
 *              end (::finish).
 *
 * Everything behind the power values is an integer: Q[d] = floor(16 P[d]) as a uint64, so no result depends on the
 * order of a reduction or the shape of the launch.
 *
 * Lane mapping of the per-frame stage.  Eight lanes per frame (lane = 8 frame + seg), 32 consecutive bins per lane
 * (d = 32 seg + j), read as eight b128 from the frame's staging row.  Rows are BL_FREQ_SROW = 264 floats apart, a
 * lane's segment 32 floats: in a b128 read, whose banks are (address / 4) mod 64, frame f segment s starts at bank
 * 8 f + 32 s (mod 64), so segments s and s + 2 of a frame share their banks and every read is 2-way conflicted — eight
 * reads per wave and iteration, behind the about 80 LDS instructions of the transform.  Derived from the addresses,
 * not measured.
 *   pass 1, in-lane: convert, sum, sum of j Q, first maximum
 *   three DPP steps over the eight lanes (lane ^ 1, lane ^ 2, the other quad): totals, each lane's prefix offset, arg-max
 *   pass 2, in-lane: the running prefix C[d] from the lane's offset, rolloff = 1 + #{d in 1..255 : C[d] < T} with
 *           T = ceil(pct energy / 100), which for integers is 100 C[d] < pct energy; three DPP steps add the counts
 * Lane 8 f (segment 0) then holds the frame's record, stores it and adds it to the wave's sums.
 */
#include <hip/hip_runtime.h>

#include "bl_freq_frames.h"

typedef unsigned long long bl_u64;

#define BL_TIMBRE_WAVES 4 /* waves per workgroup: BL_FREQ_LDS_BYTES is the layout of four */

/* cross-lane move inside every group of eight lanes; CTRL 0xB1 = quad_perm [1,0,3,2] (lane ^ 1), 0x4E = quad_perm
 * [2,3,0,1] (lane ^ 2), 0x141 = row_half_mirror (lane 7 - i: the other quad, which is all a step needs once the
 * quads are uniform) */
template <int CTRL> __device__ __forceinline__ unsigned tb_dpp(unsigned v) {
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
}
template <int CTRL> __device__ __forceinline__ bl_u64 tb_dpp(bl_u64 v) {
  return ((bl_u64)tb_dpp<CTRL>((unsigned)(v >> 32)) << 32) | tb_dpp<CTRL>((unsigned)v);
}

/* One step of the eight-lane reduction.  `upper`: this lane is the higher one of the pair the step joins.
 * sum, mom: totals; off: what lies in front of this lane's segment; (best, at): the first maximum. */
template <int CTRL>
__device__ __forceinline__ void tb_step(bool upper, bl_u64 &sum, bl_u64 &mom, bl_u64 &off, bl_u64 &best, int &at) {
  const bl_u64 osum = tb_dpp<CTRL>(sum), omom = tb_dpp<CTRL>(mom), obest = tb_dpp<CTRL>(best);
  const int oat = (int)tb_dpp<CTRL>((unsigned)at);
  if (upper) off += osum;
  sum += osum;
  mom += omom;
  if (obest > best || (obest == best && oat < at)) { best = obest; at = oat; }
}

/* the per-frame form of freq_frames_lavc's PF: the song's records and the wave's share of its sums */
struct bl_timbre_frames {
  static constexpr bool per_frame = true;
  bl_amd_frame_timbre *rec; /* the song's first frame record, or nullptr */
  bl_amd_song_timbre *song;
  bl_u64 min_energy;
  unsigned pct;
  int n_frames;
  /* this lane's share (lanes 8 f only) */
  bl_u64 csum = 0, csq = 0, rsum = 0, rsq = 0, psum = 0, psq = 0, emax = 0;
  unsigned used = 0;

  /* the wave's frames [first, first + 8) lie in stage[8][BL_FREQ_SROW]; the first n_live of them belong to the song */
  __device__ __forceinline__ void frames(const float *stage, int lane, int first, int n_live) {
    const int fr = lane >> 3, seg = lane & 7;
    const float4 *row = reinterpret_cast<const float4 *>(stage + fr * BL_FREQ_SROW + 32 * seg);
    float4 pv[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) pv[q] = row[q];
    bl_u64 q64[32];
    bl_u64 sum = 0, mom = 0, best = 0;
    int at = 1;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      const float4 v = pv[j >> 2];
      float pw = (j & 3) == 0 ? v.x : (j & 3) == 1 ? v.y : (j & 3) == 2 ? v.z : v.w;
      if (j == 0) pw = seg == 0 ? 0.f : pw; /* bin 0 takes no part */
      /* 16 P is exact (a power of two) and below 2^50: the conversion truncates, which is the floor of a value >= 0 */
      const bl_u64 qv = (bl_u64)(pw * 16.f);
      q64[j] = qv;
      sum += qv;
      mom += qv * (unsigned)j;
      if (qv > best) { best = qv; at = 32 * seg + j; }
    }
    mom += sum * (unsigned)(32 * seg); /* sum of d Q, d = 32 seg + j */
    bl_u64 off = 0;
    tb_step<0xB1>((seg & 1) != 0, sum, mom, off, best, at);
    tb_step<0x4E>((seg & 2) != 0, sum, mom, off, best, at);
    tb_step<0x141>((seg & 4) != 0, sum, mom, off, best, at);
    /* sum = energy, mom = moment, (best, at) = peak in all eight lanes; off = Q[1] + .. + Q[32 seg - 1] */
    const bl_u64 thr = (sum * pct + 99u) / 100u; /* 100 C < pct energy  <=>  C < ceil(pct energy / 100) */
    unsigned below = 0;
    bl_u64 run = off;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      run += q64[j];
      below += run < thr;
    }
    if (seg == 0) below -= 0 < thr; /* the slot of bin 0 (C = 0) is no bin */
    below += tb_dpp<0xB1>(below);
    below += tb_dpp<0x4E>(below);
    below += tb_dpp<0x141>(below);
    if (seg == 0 && fr < n_live) {
      const int rolloff = 1 + (int)below;
      if (rec) {
        bl_amd_frame_timbre *r = rec + (first + fr);
        r->energy = sum;
        r->moment = mom;
        r->rolloff = rolloff;
        r->peak = at;
      }
      emax = sum > emax ? sum : emax;
      if (sum > 0 && sum >= min_energy) {
        const bl_u64 c = ((mom / sum) << 12) + (((mom % sum) << 12) / sum);
        csum += c; csq += c * c;
        rsum += (unsigned)rolloff; rsq += (unsigned)(rolloff * rolloff);
        psum += (unsigned)at; psq += (unsigned)(at * at);
        used += 1;
      }
    }
  }

  /* behind the song's last frame and a workgroup barrier: per-wave sums to LDS (8 x 8 bytes per wave), one plain
   * store per field by the workgroup's first lane */
  __device__ __forceinline__ void finish(void *lds, int wave, int lane) {
    bl_u64 *part = static_cast<bl_u64 *>(lds);
    bl_u64 v[8] = {csum, csq, rsum, rsq, psum, psq, emax, used};
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const bl_u64 o = __shfl_down(v[k], off);
        v[k] = k == 6 ? (o > v[k] ? o : v[k]) : v[k] + o;
      }
    }
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < 8; ++k) part[8 * wave + k] = v[k];
    }
    __syncthreads();
    if (wave == 0 && lane == 0) {
      bl_u64 t[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        t[k] = part[k];
        for (int w = 1; w < BL_TIMBRE_WAVES; ++w) {
          const bl_u64 o = part[8 * w + k];
          t[k] = k == 6 ? (o > t[k] ? o : t[k]) : t[k] + o;
        }
      }
      song->centroid_sum = t[0]; song->centroid_sumsq = t[1];
      song->rolloff_sum = t[2]; song->rolloff_sumsq = t[3];
      song->peak_sum = t[4]; song->peak_sumsq = t[5];
      song->energy_max = t[6];
      song->frames = n_frames;
      song->used = (int)t[7];
      song->status = BL_OK;
      song->reserved = 0;
    }
  }
};

static_assert(8 * 8 * BL_TIMBRE_WAVES <= 256 * 4, "the per-wave sums fit the 1 KB the frequency pass keeps its spectrum in");

/* one workgroup per song; the channel count is uniform per workgroup (as k_freq_frames) */
__global__ __launch_bounds__(64 * BL_TIMBRE_WAVES, 2) void k_timbre(const int16_t *__restrict__ pcm,
                                                                   const bl_timbre_song *__restrict__ songs,
                                                                   bl_tables tb, unsigned pct, bl_u64 min_energy,
                                                                   bl_amd_song_timbre *songs_out,
                                                                   bl_amd_frame_timbre *frames_out) {
  const bl_timbre_song ts = songs[blockIdx.x];
  bl_dsong sg = {};
  sg.pcm_off = ts.pcm_off;
  sg.channels = ts.channels;
  sg.n_frames = ts.n_frames;
  bl_timbre_frames pf;
  pf.rec = frames_out ? frames_out + ts.frame_off : nullptr;
  pf.song = songs_out + ts.out_idx;
  pf.min_energy = min_energy;
  pf.pct = pct;
  pf.n_frames = ts.n_frames;
  if (ts.channels == 2) freq_frames_lavc<true, BL_TIMBRE_WAVES, false>(pcm, sg, tb, nullptr, nullptr, nullptr, &pf);
  else freq_frames_lavc<false, BL_TIMBRE_WAVES, false>(pcm, sg, tb, nullptr, nullptr, nullptr, &pf);
}

/* ========================================================================= */
/* launcher (declared in bl_launch.h)                                         */

int blk_timbre_configure_device(void) {
  BL_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_timbre), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   BL_FREQ_LDS_BYTES));
  return BL_OK;
}

int blk_timbre(hipStream_t s, const int16_t *d_pcm, const bl_timbre_song *d_songs, int n_songs, const bl_tables &tb,
               int pct, unsigned long long min_energy, bl_amd_song_timbre *d_songs_out, bl_amd_frame_timbre *d_frames) {
  hipLaunchKernelGGL(k_timbre, dim3(n_songs), dim3(64 * BL_TIMBRE_WAVES), BL_FREQ_LDS_BYTES, s, d_pcm, d_songs, tb,
                     (unsigned)pct, min_energy, d_songs_out, d_frames);
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}
