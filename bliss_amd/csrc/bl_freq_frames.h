/*
 * bl_freq_frames.h — freq_frames_lavc: the per-frame body shared by the frequency pass (bl_freq_kernels.hip:
 * k_freq_frames, k_freq_scan) and the spectral timbre (bl_timbre_kernels.hip: k_timbre).  Hann window, the 512-point
 * f32 real DFT in libavcodec's order (bl_fft_lavc.h) and the power values of every frame are ONE piece of source; what
 * a kernel does with a wave's eight power spectra once they lie in its staging rows is the only thing that differs
 * (the running spectrum of the frequency pass, or the per-frame integers of the timbre).  Must be compiled with
 * -ffp-contract=off.  Device code only, not installed.
 */
#ifndef BL_FREQ_FRAMES_H_
#define BL_FREQ_FRAMES_H_

#include <hip/hip_runtime.h>

#include "bl_launch.h"
#include "bl_fft_lavc.h"
#include "bl_metric.h" /* bl_wave_sync */
#include "bl_scan.h"

typedef bl_c2<bl_f2> c2p; /* a complex number per frame of the pair */

/* LDS of a workgroup of W waves: 4 W exchange buffers, twiddles + Hann, the running spectrum + relay word, and —
 * k_freq_scan only — the central histogram, LAST (scan_hist_word relies on nothing lying behind it) */
#define BL_FREQ_XCH_BYTES(W) (4 * (W) * BL_FFT_XCH_ELEMS * 16)
#define BL_FREQ_ACC_OFF(W) (BL_FREQ_XCH_BYTES(W) + 2 * 256 * 8 + 512 * 4)
#define BL_FREQ_HIST_OFF(W) (BL_FREQ_ACC_OFF(W) + 256 * 4 + 64)
#define BL_FREQ_LDS_BYTES BL_FREQ_HIST_OFF(4)                                 /* k_freq_frames: 76.9 KB */
#define BL_FREQ_SCAN_WAVES 8
#define BL_FREQ_SCAN_LDS_BYTES (BL_FREQ_HIST_OFF(BL_FREQ_SCAN_WAVES) + 4 * BL_HIST_BINS) /* k_freq_scan: 159.1 KB */
/* row stride of the power staging: 2 rows = 16 banks (mod 32) apart, so the two 16-lane groups
 * that share a 32-lane store group land on disjoint banks */
/* every region of the layout, in order: [exchange buffers][twiddles 2 KB + pad 2 KB][Hann 2 KB][spectrum 1 KB][relay 64 B]
 * [histogram] — each ends where the next begins, the histogram ends where the allocation ends (what the
 * range-test-free ds_add of scan_hist_word relies on), and the kernel's launch passes exactly this size */
#define BL_FREQ_TW_OFF(W) BL_FREQ_XCH_BYTES(W)
#define BL_FREQ_HANN_OFF(W) (BL_FREQ_XCH_BYTES(W) + 2 * 256 * 8)
#define BL_FREQ_RELAY_OFF(W) (BL_FREQ_ACC_OFF(W) + 256 * 4)
static_assert(BL_FREQ_TW_OFF(BL_FREQ_SCAN_WAVES) + LV_TW_SLOTS * 16 * 8 <= BL_FREQ_HANN_OFF(BL_FREQ_SCAN_WAVES) &&
                  BL_FREQ_HANN_OFF(BL_FREQ_SCAN_WAVES) + 512 * 4 == BL_FREQ_ACC_OFF(BL_FREQ_SCAN_WAVES) &&
                  BL_FREQ_ACC_OFF(BL_FREQ_SCAN_WAVES) + 256 * 4 == BL_FREQ_RELAY_OFF(BL_FREQ_SCAN_WAVES) &&
                  BL_FREQ_RELAY_OFF(BL_FREQ_SCAN_WAVES) + 64 == BL_FREQ_HIST_OFF(BL_FREQ_SCAN_WAVES) &&
                  BL_FREQ_HIST_OFF(BL_FREQ_SCAN_WAVES) + 4 * BL_HIST_BINS == BL_FREQ_SCAN_LDS_BYTES &&
                  BL_FREQ_SCAN_LDS_BYTES <= 160 * 1024,
              "k_freq_scan: every LDS region ends where the next begins and the histogram is the LAST one (scan_hist_word)");
#define BL_FREQ_SROW 264

/* cross-lane move of a pair of floats through DPP (two 32-bit moves); CTRL 0x140 = row_mirror,
 * 0x120 + n = row_ror:n inside each 16-lane row */
template <int CTRL> __device__ __forceinline__ bl_f2 bl_dpp_f2(bl_f2 v) {
  const int x = __builtin_amdgcn_update_dpp(0, __float_as_int(v.x), CTRL, 0xF, 0xF, true);
  const int y = __builtin_amdgcn_update_dpp(0, __float_as_int(v.y), CTRL, 0xF, 0xF, true);
  return (bl_f2){__int_as_float(x), __int_as_float(y)};
}
/* the same with a value for the lanes that have no source (they keep `old`) */
template <int CTRL> __device__ __forceinline__ bl_f2 bl_dpp_f2_old(bl_f2 old, bl_f2 v) {
  const int x = __builtin_amdgcn_update_dpp(__float_as_int(old.x), __float_as_int(v.x), CTRL, 0xF, 0xF, false);
  const int y = __builtin_amdgcn_update_dpp(__float_as_int(old.y), __float_as_int(v.y), CTRL, 0xF, 0xF, false);
  return (bl_f2){__int_as_float(x), __int_as_float(y)};
}

/*
 * WAVES waves per workgroup (one workgroup per song).  SCAN: the statistics pass rides along — every PCM word the
 * transform loads also goes into the song's sum, sum of squares and central histogram (k_pcm_scan's arithmetic),
 * so the analysis reads the PCM twice instead of three times.
 *
 * The transform is libavcodec's, node for node (bl_fft_lavc.h; round 6): what the reference's av_rdft_calc computes
 * in the order it computes it, so that every frame's power values — and with them `frequency` — are the oracle's bit
 * for bit (the oracle under that order prints the reference's golden values to the last digit).
 * The input is gathered in split-radix order (lane L register r = element (lv_base(L) + K[r]) mod 256 of the frame:
 * immediate offsets from one per-lane base, every 8-byte element still loaded exactly once, 16 lanes per load inside
 * a 16-element neighbourhood), the leaves (fft16, or fft8 twice) run in that layout, ONE transpose through the
 * group's exchange buffer, then pass(32) with its products exchanged between lanes l and l ^ 8 by DPP, pass(64 .. 256)
 * in registers, rdft.c's post-pass with the partner by DPP (row mirror + shift) and re * re + im * im unfused.
 * Rounds 1-5 ran a fused radix-16 transform here (git 6a8cdc4: freq_frames_body; 558 instead of ~760 packed
 * instructions per wave-iteration, k_freq_scan 8.77 instead of 9.64 ms per 1 024 S180 songs) whose `frequency` agreed
 * with the oracle to a few 1e-6 absolute — inside the reference's own tolerance, not bit for bit.
 *
 * PF: what becomes of the power values.  bl_frames_sum (the frequency pass): the running spectrum and the baton
 * described above.  A class with per_frame = true (bl_timbre_kernels.hip): no running spectrum and no baton — the
 * relay wait, accv and the spectrum store are compiled out; once a wave's eight frames lie in its private staging rows
 * it hands them to pf->frames(stage, lane, first frame, live frames), and after the song's last frame the workgroup
 * calls pf->finish(1 KB of LDS, wave, lane) behind a barrier.
 */
struct bl_frames_sum {
  static constexpr bool per_frame = false;
  __device__ __forceinline__ void frames(const float *, int, int, int) {}
  __device__ __forceinline__ void finish(void *, int, int) {}
};

template <bool STEREO, int WAVES, bool SCAN, class PF = bl_frames_sum>
__device__ __forceinline__ void freq_frames_lavc(const int16_t *__restrict__ pcm, const bl_dsong &sg,
                                                 const bl_tables &tb, float *spectrum, bl_dstats *st,
                                                 unsigned *gh, PF *pf = nullptr) {
  constexpr bool PER_FRAME = PF::per_frame;
  static_assert(!(PER_FRAME && SCAN), "the per-frame form has no statistics riding along");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int FPI = 8 * WAVES; /* frames per workgroup iteration */
  c2p *xch = reinterpret_cast<c2p *>(smem); /* 4 WAVES x 272 */
  c2f *lvtw = reinterpret_cast<c2f *>(smem + BL_FREQ_TW_OFF(WAVES)); /* [LV_TW_SLOTS][16 lanes] */
  float *hann = reinterpret_cast<float *>(smem + BL_FREQ_HANN_OFF(WAVES));
  float *accv = reinterpret_cast<float *>(smem + BL_FREQ_ACC_OFF(WAVES)); /* ps[0..255] so far */
  unsigned *lh = reinterpret_cast<unsigned *>(smem + BL_FREQ_HIST_OFF(WAVES)); /* SCAN: the histogram */
  typedef __attribute__((address_space(3))) volatile int lds_vint;
  lds_vint *relay = (lds_vint *)(smem + BL_FREQ_RELAY_OFF(WAVES));
  const int tid = threadIdx.x, g = tid >> 4, l = tid & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, gl = g & 3;
  const int16_t *p = pcm + sg.pcm_off;
  if (WAVES == 4 || tid < 256) {
    lvtw[tid] = tb.lv_tw[tid];
    hann[tid] = tb.hann[tid];
    hann[tid + 256] = tb.hann[tid + 256];
    if (!PER_FRAME) accv[tid] = 0.f;
  }
  if (SCAN)
    for (int i = tid; i < BL_HIST_BINS; i += 64 * WAVES) lh[i] = 0;
  if (tid == 0) relay[0] = 0;
  __syncthreads();
  unsigned lds_hist = (unsigned)(size_t)(bl_lds_u32 *)lh;
  asm volatile("" : "+v"(lds_hist)); /* lives in a VGPR: as a scalar it is copied in front of every use */
  long long sum = 0;
  unsigned long long sq = 0;

  /* this lane's place in the split-radix order (bl_fft_lavc.h): T8 lanes 1, 5, 7, 9, 13; base element lv_base(l),
   * from which the lanes with base >= 251 wrap for every register but the first */
  const bool t16 = ((lv_t8_lane_mask() >> l) & 1u) == 0u;
  const unsigned long long bases = l < 8 ? lv_bases_packed(0) : lv_bases_packed(1);
  const int base0 = (int)((bases >> (8 * (l & 7))) & 0xFFu);
  const int basep = base0 >= 251 ? base0 - 256 : base0;
  const bool lo8 = l < 8;
  /* gather order of the registers, the same for every lane: lv_k_lo | lv_k_hi(true, .) = what lane 0 (base 0) loads.
   * Element of register r: (base0 + KG(r)) mod 256 = basep + KG(r) for r >= 1 (KG >= 16 > 5 >= -basep), base0 for r = 0 */
#define KG(r) lv_gather_index(0, (r))
  static_assert(lv_t8_lane_mask() == 0x22A2u && lv_bases_packed(0) == 0x06FE0A02FC040800ull &&
                    lv_bases_packed(1) == 0xFB0307FFFD050901ull && KG(0) == 0 && KG(1) == 128 && KG(15) == 176 &&
                    lv_gather_index(3, 1) == ((252 + KG(1)) & 255) && lv_gather_index(12, 0) == 255,
                "bl_fft_lavc.h: lane tables");

  c2p *gx = xch + g * BL_FFT_XCH_ELEMS; /* the transpose buffer of this 16-lane group */
  float *stage = reinterpret_cast<float *>(xch + (g - gl) * BL_FFT_XCH_ELEMS); /* wave-private [8][BL_FREQ_SROW] */
  /* one iteration ahead: 32 unconditional loads per lane (frame indices clamped into the song;
   * a frame past the end is transformed like any other and simply not added), so the HBM
   * latency of iteration it+1 hides behind the transforms of iteration it */
  uint2 pa[16], pb[16];
  constexpr bool stereo = STEREO; /* the channel handling is compiled in; k_freq_frames picks per workgroup */
  /* loads of registers [4 * part, 4 * part + 4) of both frames: the iteration issues its 32 loads in
   * four instalments between the phases of the transform (32 at once fill the vector-memory
   * queue and the wave sits in front of it: 1.6 k cycles per iteration) */
  auto fetch = [&](int f_, int part) {
    const int fa = min(f_, sg.n_frames - 1), fb = min(f_ + 1, sg.n_frames - 1);
    if (stereo) {
      const uint2 *qa = reinterpret_cast<const uint2 *>(p + (size_t)fa * 1024) + basep;
      const uint2 *qb = reinterpret_cast<const uint2 *>(p + (size_t)fb * 1024) + basep;
#pragma unroll
      for (int r = 4 * part; r < 4 * part + 4; ++r) {
        const int e = r == 0 ? base0 - basep : KG(r);
        pa[r] = qa[e]; pb[r] = qb[e];
      }
    } else {
      const unsigned *qa = reinterpret_cast<const unsigned *>(p + (size_t)fa * 512) + basep;
      const unsigned *qb = reinterpret_cast<const unsigned *>(p + (size_t)fb * 512) + basep;
#pragma unroll
      for (int r = 4 * part; r < 4 * part + 4; ++r) {
        const int e = r == 0 ? base0 - basep : KG(r);
        pa[r] = make_uint2(qa[e], 0u);
        pb[r] = make_uint2(qb[e], 0u);
      }
    }
  };
  /* the two mono samples (one complex DFT input) a lane takes from an 8-byte (stereo) or 4-byte
   * (mono) word, for both frames of the pair:
   * stereo, ref :69-75: (float)((L + R) / 2), the integer average truncates towards zero —
   * L + R converts exactly, half of it is exact, v_trunc does what the C division does;
   * mono, ref :76-80: (float)s */
  auto mono2 = [&](const uint2 wa, const uint2 wb, bl_f2 &s0, bl_f2 &s1) {
    const int a0 = (int)(short)(wa.x & 0xFFFFu), a1 = (int)(short)(wa.x >> 16);
    const int b0 = (int)(short)(wb.x & 0xFFFFu), b1 = (int)(short)(wb.x >> 16);
    if (stereo) {
      const int a2 = (int)(short)(wa.y & 0xFFFFu), a3 = (int)(short)(wa.y >> 16);
      const int b2 = (int)(short)(wb.y & 0xFFFFu), b3 = (int)(short)(wb.y >> 16);
      const bl_f2 h0 = (bl_f2){(float)(a0 + a1), (float)(b0 + b1)} * 0.5f;
      const bl_f2 h1 = (bl_f2){(float)(a2 + a3), (float)(b2 + b3)} * 0.5f;
      s0 = (bl_f2){__builtin_truncf(h0.x), __builtin_truncf(h0.y)};
      s1 = (bl_f2){__builtin_truncf(h1.x), __builtin_truncf(h1.y)};
    } else {
      s0 = (bl_f2){(float)a0, (float)b0};
      s1 = (bl_f2){(float)a1, (float)b1};
    }
  };
  auto bc = [](float w) { return (bl_f2){w, w}; };
  /* the lane's twiddles of the in-register passes stay in registers for the whole song; pass(32)'s carries the sign
   * of its half of the pair (lv_pass32_mul) */
  const c2f w32 = lvtw[LV_TW_P32 * 16 + l], w64 = lvtw[LV_TW_P64 * 16 + l];
  const float ws32 = lo8 ? -w32.im : w32.im;
  c2f w128[2], w256[4];
#pragma unroll
  for (int q = 0; q < 2; ++q) w128[q] = lvtw[(LV_TW_P128 + q) * 16 + l];
#pragma unroll
  for (int q = 0; q < 4; ++q) w256[q] = lvtw[(LV_TW_P256 + q) * 16 + l];
  const bl_f2 SH = bc(tb.lv_leafc[0]), C1 = bc(tb.lv_leafc[1]), C3 = bc(tb.lv_leafc[2]);
  const bl_f2 *hann2 = reinterpret_cast<const bl_f2 *>(hann) + basep;
  const int n_iter = (sg.n_frames + FPI - 1) / FPI;
#pragma unroll
  for (int part = 0; part < 4; ++part) fetch(8 * wave + 2 * gl, part);
  for (int it = 0; it < n_iter; ++it) {
    const int f = it * FPI + 8 * wave + 2 * gl;
    /* SCAN: the input stage with the statistics (a third of the iteration's instructions and all of its LDS
     * atomics) runs at priority 3, the leaves at 2, the rest at 0: of the two waves of a SIMD the one
     * that is feeding the LDS wins the VALU.  32.6 vs 33.8 ms per 4 096 songs (round 4); the other orders (later
     * phases first, as in k_env_windows3) made no difference, and k_freq_frames gains nothing from any. */
    if (SCAN) __builtin_amdgcn_s_setprio(3);
    bl_f2 re[16], im[16];
    /* SCAN: the statistics of every word as the transform's input stage consumes it (its registers die here).  The
     * frames of a song's last iteration that lie beyond its end (their loads were clamped onto the last frame) are
     * not counted. */
    int s32 = 0;
    auto word = [&](unsigned w) { scan_word(w, s32, sq, lds_hist, true); };
    const bool full = it + 1 < n_iter; /* wave-uniform */
    const bool va = f < sg.n_frames, vb = f + 1 < sg.n_frames;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      bl_f2 xr, xi;
      if (SCAN) {
        if (full) {
          word(pa[r].x); word(pb[r].x);
          if (stereo) { word(pa[r].y); word(pb[r].y); }
        } else {
          if (va) { word(pa[r].x); if (stereo) word(pa[r].y); }
          if (vb) { word(pb[r].x); if (stereo) word(pb[r].y); }
        }
      }
      mono2(pa[r], pb[r], xr, xi);
      const bl_f2 h = hann2[r == 0 ? base0 - basep : KG(r)]; /* hann[2 m], hann[2 m + 1] of this register's element m */
      re[r] = xr * (bl_f2){h.x, h.x};
      im[r] = xi * (bl_f2){h.y, h.y};
    }
    if (SCAN) sum += s32;
    fetch(f + FPI, 0);
    if (SCAN) __builtin_amdgcn_s_setprio(2);
    lv_leaves<bl_f2>(t16, re, im, SH, C1, C3);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      c2p v; v.re = re[r]; v.im = im[r];
      gx[r * 17 + l] = v;
    }
    bl_wave_sync();
    fetch(f + FPI, 1);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const c2p v = gx[l * 17 + j];
      re[j] = v.re; im[j] = v.im;
    }
    bl_wave_sync();
    fetch(f + FPI, 2);
    if (SCAN) __builtin_amdgcn_s_setprio(0);
    { /* pass(32) @ 0, 64, 96, 128, 192: registers (R, R + 1), lanes l and l ^ 8 */
      auto sel = [&](bl_f2 a, bl_f2 b) { return lo8 ? a : b; };
      constexpr int R32[5] = {0, 4, 6, 8, 12};
#pragma unroll
      for (int b = 0; b < 5; ++b) {
        const int R = R32[b];
        bl_f2 tA, tB;
        lv_pass32_mul<bl_f2>(re[R + 1], im[R + 1], bc(w32.re), bc(ws32), tA, tB);
        const bl_f2 pA = bl_dpp_f2<0x128>(tA), pB = bl_dpp_f2<0x128>(tB); /* row_ror:8 = lane ^ 8 */
        lv_pass32_fin<bl_f2>(re[R], im[R], re[R + 1], im[R + 1], tA, tB, pA, pB, sel);
      }
    }
    lv_pass_inlane<bl_f2, 0, 1>(re, im, bc(w64.re), bc(w64.im));
    lv_pass_inlane<bl_f2, 8, 1>(re, im, bc(w64.re), bc(w64.im));
    lv_pass_inlane<bl_f2, 12, 1>(re, im, bc(w64.re), bc(w64.im));
    lv_pass_inlane<bl_f2, 0, 2>(re, im, bc(w128[0].re), bc(w128[0].im));
    lv_pass_inlane<bl_f2, 1, 2>(re, im, bc(w128[1].re), bc(w128[1].im));
    lv_pass_inlane<bl_f2, 0, 4>(re, im, bc(w256[0].re), bc(w256[0].im));
    lv_pass_inlane<bl_f2, 1, 4>(re, im, bc(w256[1].re), bc(w256[1].im));
    lv_pass_inlane<bl_f2, 2, 4>(re, im, bc(w256[2].re), bc(w256[2].im));
    lv_pass_inlane<bl_f2, 3, 4>(re, im, bc(w256[3].re), bc(w256[3].im));
    fetch(f + FPI, 3);
    /* rdft.c's post-pass: the partner of i = l + 16 j is Z[256 - i], register 15 - j of lane 16 - l (row mirror +
     * shift by one); lane 0 is its own partner and takes its register 16 - j */
    bl_f2 own[8], mir[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bl_f2 zr = j ? re[16 - j] : re[0];
      const bl_f2 zi = j ? im[16 - j] : im[0];
      const bl_f2 pr = bl_dpp_f2_old<0x111>(zr, bl_dpp_f2<0x140>(re[15 - j]));
      const bl_f2 pi = bl_dpp_f2_old<0x111>(zi, bl_dpp_f2<0x140>(im[15 - j]));
      const c2f w = lvtw[(LV_TW_POST + j) * 16 + l];
      lv_post_power<bl_f2>(re[j], im[j], pr, pi, bc(w.re), bc(w.im), bc(0.5f), own[j], mir[j]);
    }
    const bl_f2 mid = lv_mid_power<bl_f2>(re[8], im[8]);
    /* ref :88-93: re*re + im*im of bin d, for d = 1..255 (lane 0's own[0] / mir[0] are bins 0 / 256: never read) */
    float *sa = stage + (2 * gl) * BL_FREQ_SROW, *sb = sa + BL_FREQ_SROW;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      sa[l + 16 * k] = own[k].x; sb[l + 16 * k] = own[k].y;
      sa[256 - l - 16 * k] = mir[k].x; sb[256 - l - 16 * k] = mir[k].y;
    }
    if (l == 0) { sa[128] = mid.x; sb[128] = mid.y; }
    bl_wave_sync();
    /* the baton: frames 8 WAVES it + 8 w .. + 7 join the running spectrum after those of wave w - 1 */
    const int turn = WAVES * it + wave;
    /* frames beyond the song's last one (their loads were clamped onto it) are not added */
    const int n_live = sg.n_frames - (it * FPI + 8 * wave);
    if (PER_FRAME) { /* the wave's own frames, no order to keep between the waves */
      pf->frames(stage, lane, it * FPI + 8 * wave, n_live);
      bl_wave_sync(); /* the staging rows are the next iteration's transpose buffers */
      continue;
    }
    /* this wave's 8 x 4 power values per lane are fetched BEFORE it asks for the baton (they are
     * its own), all 32 reads in flight at once; holding the baton then costs one read of the
     * running spectrum, eight dependent adds and a write.  (Reading them one by one behind the
     * frame-count test made the hold 3.2 k cycles: four waves x 3.2 k was the whole iteration.) */
    float sv[4][8];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int fr = 0; fr < 8; ++fr) sv[q][fr] = stage[fr * BL_FREQ_SROW + lane + 64 * q];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    while (__builtin_amdgcn_readfirstlane(relay[0]) < turn) __builtin_amdgcn_s_sleep(1);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    float acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = accv[lane + 64 * q];
    if (n_live >= 8) { /* every iteration but a song's last: no per-frame test (hipcc makes selects of it) */
#pragma unroll
      for (int fr = 0; fr < 8; ++fr)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          acc[q] += sv[q][fr];
          /* one v_add_f32 each: paired into v_pk_add_f32 the operands need more moves than the
           * pairing saves, and this is the stretch during which the wave holds the baton */
          asm volatile("" : "+v"(acc[q]));
        }
    } else {
#pragma unroll
      for (int fr = 0; fr < 8; ++fr)
        if (fr < n_live) { /* wave-uniform */
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[q] += sv[q][fr];
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) accv[lane + 64 * q] = acc[q];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    bl_wave_sync();
    if (lane == 0) relay[0] = turn + 1;
  }
  if (SCAN) {
    /* the samples behind the last whole frame (fewer than 512 per channel) */
    for (int i = sg.n_frames * 512 * sg.channels + tid; i < sg.n; i += 64 * WAVES) {
      const int sv = (int)p[i];
      sum += sv;
      sq += (unsigned)(sv * sv);
      const unsigned b = (unsigned)(sv + BL_HIST_BINS / 2);
      if (b < BL_HIST_BINS) atomicAdd(&lh[b], 1u);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      sum += __shfl_down(sum, off);
      sq += __shfl_down(sq, off);
    }
    if (lane == 0) {
      atomicAdd(&st->sum, (unsigned long long)sum);
      atomicAdd(&st->sumsq, sq);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); /* the inline-asm adds are invisible to hipcc's counters */
  }
  __syncthreads();
  if (PER_FRAME) {
    pf->finish(accv, wave, lane);
    return;
  }
  if (WAVES == 4 || tid < 256) spectrum[(size_t)blockIdx.x * 256 + tid] = accv[tid];
  if (SCAN)
    for (int i = tid; i < BL_HIST_BINS; i += 64 * WAVES) gh[i] = lh[i]; /* the workgroup owns the song: plain stores */
}

#undef KG

#endif /* BL_FREQ_FRAMES_H_ */
