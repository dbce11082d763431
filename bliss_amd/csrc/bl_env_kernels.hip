/*
 * bl_env_kernels.hip — gfx950 kernels and launch layer of the envelope analysis (bl_envelope_sort): the window
 * energies and the serial tail behind them.  Must be compiled with -ffp-contract=off: the FMAs are the explicit ones
 * of bl_fir.h, bl_fft.h and bl_fft_tan.h.
 *
 * Kernels (reference code each one replaces):
 *   k_env_windows3 normalise, 17-tap FIR (bl_fir.h), 512-pt f64 real DFT, f32-rounded
 *                  energy per window            ref src/tempo_atk_sort.c:109-153
 *   k_env_tail     IIR, box filters, peaks, tempo/attack (bl_tail.h)
 *                                               ref src/tempo_atk_sort.c:184-284
 * Also here: which FIR form runs (bl_amd_set_fir_mode, BL_AMD_FIR_FUSED) and, in a measurement build, which of the
 * kernel's priority tables (bl_amd_measure_env).
 */
#include <hip/hip_runtime.h>
#include <atomic>
#include <algorithm>
#include <stdlib.h>

#include "bl_launch.h"
#include "bl_fft_tan.h"
#include "bl_metric.h" /* bl_wave_sync */
#include "bl_fir.h"
#include "bl_tail.h"

/* ------------------------------------------------------------------------- */
/* k_env_windows3: normalise + FIR + DFT + ordered sum, wave-autonomous        */
/*
 * One workgroup per CU: 7 compute waves + 1 summing wave (2 waves per SIMD, 194-234 VGPRs), no workgroup
 * barrier inside the loop.
 *
 * A compute wave walks a CONTIGUOUS run of rounds of four windows (one window per 16-lane group; the song's
 * rounds are split evenly over the compute waves of its workgroups).  Its private LDS slice holds five blocks
 * of 256 filtered samples as a ring: a round filters the 1 024 new samples (16 outputs per lane, from the 32
 * samples the lane loads itself: no cross-lane shift) into the four places the previous round has released and
 * finds the block it shares with that round where it was left.  Then the four 512-point f64 DFTs: inputs as
 * aligned ds_read_b128, two radix-16 passes over 16 lanes x 16 registers with the re and im transposes through
 * the place of the window's own block, partner values of the real-input split through DPP (row mirror + shift),
 * and the 4 x 257 power terms.  The first round of a run is preceded by a short pass that filters the one block
 * it cannot inherit.
 *
 * FIR mode 2 (the default) forms the filter's sum exactly, on the integers (bl_fir_int.h): in the main loop a block
 * of 256 samples is a 16 x 16 tile of outputs and five int8 matrix products (v_mfma_i32_16x16x64_i8 / x32_i8: the
 * matrix pipe, beside the f64 VALU the rest of the round lives on) of the samples' byte planes with the digit planes
 * of the Toeplitz tap matrix; a lane loads its 8 samples of each of the round's four tiles, ends up with four
 * consecutive outputs per tile and converts (3 integer + 3 f64-rate instructions per output where the fma chain took
 * 17 + a conversion per sample).  The sums are never scaled: the transform is linear, so the song's factor enters
 * squared in the split's constants (bl_fft512_power1_sq, bl_fft_tan.h).  The block in front of a run and the zero-state heads form the same
 * exact sum in f64, so a sample's bits do not depend on where the launch geometry puts the run boundaries.
 *
 * The f32-rounded, strictly ordered sum of ref tempo_atk_sort.c:142-149 is a dependent chain of three
 * instructions per term.  It runs on the eighth wave, IN TWO HALVES ON TWICE THE LANES: a compute wave hands over
 * terms 0..129 of the round it has just finished together with terms 130..256 of the round BEFORE (kept in 16
 * registers for one round); the summing wave adds the first halves on lanes 0-27 and, continuing from the partial
 * sums of its previous step, the second halves on lanes 32-59 — 390 dependent instructions per tile of 28 windows
 * instead of 771, the same additions in the same order.  The energies leave one step later.  Hand-over through
 * LDS sequence words (waves of one workgroup are always co-resident, so the bounded spins cannot deadlock).
 *
 * Who gets the VALU.  A SIMD gives its VALU to the wave with the highest s_setprio value and, among equals, to
 * the OLDEST wave — strictly: 96 % of the issue slots to the older of two busy waves (tools/gen_ubench_issue.py).
 * Two compute waves that share a SIMD and are held in step by the tile hand-over therefore do not share it: the
 * older one runs its round and waits, the younger one then runs alone with every LDS round trip of its own
 * exposed, and the tile waits for it.  PRIO gives every phase of a round a priority (4 bits per phase, phase 0 in
 * the lowest digit); the shipped table 0x222011 runs the second half of a round (transposes, second DFT pass,
 * hand-over, power terms) at 2, normalise + FIR and the FIR -> DFT exchange at 1 and the first DFT pass at 0:
 * whichever wave is further along — the one the tile is waiting for — wins, whatever its age.  278 vs 306 ms per
 * 8 192 S180 songs with identical results for 0x222111 (profiles/r04_env_variants.json);
 * the first pass at 0 another 1.0-1.3 % (three sweeps of five rounds; every table with that digit at 0 and the
 * second half at 2 or 3 did the same).
 */
#define EV_CWAVES 7
#define EV_TILE (4 * EV_CWAVES)             /* windows per tile */
#define EV_TROW 258                          /* terms row stride (doubles): even -> 16-byte rows */

/* cross-lane move of a double through DPP (two 32-bit moves).  CTRL 0x110+m = row_shr:m inside
 * each 16-lane row, 0x140 = row_mirror; lanes without a source read 0 (bound_ctrl) */
template <int CTRL> __device__ __forceinline__ double bl_dpp_f64(double v) {
  const unsigned long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(b & 0xFFFFFFFFull), CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(b >> 32), CTRL, 0xF, 0xF, true);
  return __longlong_as_double(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}

/* the same with a value for the lanes that have no source (they keep `old`) */
template <int CTRL> __device__ __forceinline__ double bl_dpp_f64_old(double old, double v) {
  const unsigned long long b = __double_as_longlong(v), o = __double_as_longlong(old);
  const int lo = __builtin_amdgcn_update_dpp((int)(unsigned)(o & 0xFFFFFFFFull), (int)(unsigned)(b & 0xFFFFFFFFull),
                                             CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp((int)(unsigned)(o >> 32), (int)(unsigned)(b >> 32), CTRL, 0xF, 0xF, false);
  return __longlong_as_double(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}

/* Hand-over fences between waves of one workgroup: everything handed over lives in LDS, so
 * only the LDS counter has to drain.  A workgroup-scope fence also waits for vmcnt(0), i.e.
 * for the summing wave's global stores of the finished energies (and for prefetches in
 * flight) — ~1.5 k cycles of HBM latency on the critical path of every tile. */
__device__ __forceinline__ void ev_lds_release() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}
__device__ __forceinline__ void ev_lds_acquire() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

__device__ __forceinline__ void ev_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

/* A block of 256 filtered samples as 16 rows of eight 16-byte units (two samples each): unit c of row r at 16-byte
 * slot 9 r + 2 c, i.e. even rows on even slots and odd rows on the odd slots between them.  Both sides of the
 * FIR -> DFT exchange are then conflict-free: the eight lanes the LDS serves together write unit i of eight
 * consecutive rows (slots 9 r + 2 i: all different mod 8), and the sixteen lanes it serves together read units 0..7
 * of the two rows 2 m1 and 2 m1 + 1 (slots {0, 2, .. 14} and 9 + {0, 2, .. 14}: all different mod 16).  Rows 18
 * doubles apart (slot 9 r + c, rounds 2-3) served every DFT-input read in two turns: 64 of the 580 LDS cycles of a
 * round, the whole SQ_LDS_BANK_CONFLICT count of the kernel (tools/lds_model.py).  160 slots per block keep the
 * blocks of the four windows a multiple of 16 slots apart. */
#define EV3_BLK 320                          /* doubles per block */
#define EV3_ROW(r) (18 * (r))                /* first double of row r */
#define EV3_UNIT(c) (4 * (c))                /* first double of unit c within its row */
#define EV3_HEADS (5 * EV3_BLK)
#define EV3_SLOTS (EV3_HEADS + 64)           /* + 4 x 16 window heads */
#define EV3_TERMS_OFF (EV_CWAVES * EV3_SLOTS * 8)
#define EV3_TW_OFF (EV3_TERMS_OFF + EV_TILE * EV_TROW * 8)
#define EV3_FLAG_OFF (EV3_TW_OFF + 2 * 256 * 16)
#define EV3_ZERO_OFF (EV3_FLAG_OFF + 128)   /* 16 bytes of zeros: the 65th term pair of a second-half lane */
#define EV3_LDS_BYTES (EV3_ZERO_OFF + 16)

#define EV_PROBE_ROUNDS 16
#define EV_PROBE_SLOTS 12
#ifndef BL_ENV_PRIO
#define BL_ENV_PRIO 0x222011 /* the priority table the product launches */
#endif
/* the priority tables the measurement build instantiates beside it (tools/env_ab.py) */
#define EV_PRIO_TABS(X) X(0x000000) X(0x111111) X(0x322110) X(0x321000) X(0x222110) X(0x222111) X(0x232011) X(0x222112)
/* PROBE (measurement builds): s_memtime stamps of one workgroup's phases into `probe` */
template <int FIR_MODE, int PRIO, bool PROBE>
__global__ __launch_bounds__(64 * (EV_CWAVES + 1)) void k_env_windows3(
    const int16_t *__restrict__ pcm, const bl_dsong *__restrict__ songs,
    const bl_dstats *__restrict__ stats, bl_tables tb, float *energies, double *lc, long long *probe) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double *terms = reinterpret_cast<double *>(smem + EV3_TERMS_OFF); /* [EV_TILE][257] */
  c2d *tw256 = reinterpret_cast<c2d *>(smem + EV3_TW_OFF);
  c2d *tw512 = tw256 + 256;
  typedef __attribute__((address_space(3))) volatile int lds_vint;
  lds_vint *flags = (lds_vint *)(smem + EV3_FLAG_OFF); /* [0..6] published by the compute waves, [8] by the summing wave */

  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), ln = tid & 63, g = ln >> 4, l = ln & 15;
  const bool probing = PROBE && blockIdx.x == 0 && blockIdx.y == 0 && probe != nullptr;
  auto stamp = [&](int round, int slot) {
    if (PROBE) {
      __builtin_amdgcn_sched_barrier(0); /* no arithmetic moves across a stamp */
      if (probing && round < EV_PROBE_ROUNDS && ln == 0)
        probe[(wave * EV_PROBE_ROUNDS + round) * EV_PROBE_SLOTS + slot] = (long long)__builtin_amdgcn_s_memtime();
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  const bl_dsong sg = songs[blockIdx.y];
  const bl_dstats st = stats[blockIdx.y];
  const int16_t *p = pcm + sg.pcm_off;
  /* FIR modes 1 / 2 run bl_fft_tan.h's transform: tw512[0..127] holds (t, c) of W512^k — in mode 2, whose transform
   * runs on the unscaled integer sums, the song's (2 kappa cos, -kappa sin) in the same place (bl_fft512_power1_sq) —
   * and tw256 is not read (the lanes keep their constants in registers); mode 0 keeps bl_fft.h's (see the registers
   * below) */
  if (FIR_MODE == 0 && tid < 256) {
    tw256[tid] = tb.tw256_d[((tid & 15) * (tid >> 4)) & 255];
    tw512[tid] = tb.tw512_d[tid];
  }
  if (FIR_MODE == 1 && tid < 128) tw512[tid] = tb.tw512t[tid];
  if (FIR_MODE == 2 && tid < 128) tw512[tid] = bl_fft_sq_consts<double>(tb.cs512[tid], st.kappa);
  if (tid < 36) flags[tid] = 0; /* the sequence words and the zero pair behind them */
  if (tid < EV_TILE) terms[tid * EV_TROW + 257] = 0.0; /* the pad behind term 256 is read as a term */
  __syncthreads();

  /* rounds of four windows, split evenly over the compute waves of the song's workgroups */
  const int n_rounds = (sg.n_windows + 3) / 4;
  const int n_units = EV_CWAVES * (int)gridDim.x;
  auto run_begin = [&](int u) -> int { return (int)((long long)n_rounds * u / n_units); };
  const int u0 = EV_CWAVES * (int)blockIdx.x;
  int steps = 0;
  for (int c = 0; c < EV_CWAVES; ++c) steps = max(steps, run_begin(u0 + c + 1) - run_begin(u0 + c));
  const int n_used = 256 * (sg.n_windows + 1);
  int seq = 0;

  if (wave == EV_CWAVES) {
    /* ---- summing wave ---- */
    __builtin_amdgcn_s_setprio(3);
    {
      /* Step st (1-based): every compute wave has published st.  Lane i < 28 (row i) adds terms 0..129 of round st
       * starting from 0 and keeps the partial sum; lane 32 + i takes the partial sum lane i made in step st - 1 and
       * continues round st - 1 over terms 130..256, then stores the energy.  The second-half lanes read 127 terms and
       * three zeros — (float)((double)sum + 0.0) is sum — so that every lane runs the same 130 additions.  Step
       * steps + 1 only has second halves (the compute waves publish them after their last round). */
      const int rowi = min(ln & 31, EV_TILE - 1);
      const bool own = ln < 32;
      const int c2 = min(rowi >> 2, EV_CWAVES - 1);
      const int q0 = run_begin(u0 + c2), q1 = run_begin(u0 + c2 + 1);
      const double2 *row = reinterpret_cast<const double2 *>(terms + rowi * EV_TROW);
      const double2 *zero2 = reinterpret_cast<const double2 *>(smem + EV3_ZERO_OFF);
      const double2 *tp = own ? row : row + 65;
      const double2 *tail = own ? row + 64 : zero2;
      float psum = 0.f;
      for (int st = 1; st <= steps + 1; ++st) {
        stamp(st - 1, 0);
        for (;;) {
          const int f = ln < EV_CWAVES ? flags[ln] : st;
          if (__all(f >= st)) break;
          __builtin_amdgcn_s_sleep(1);
        }
        ev_lds_acquire();
        stamp(st - 1, 1);
        const int rr = own ? st : st - 1; /* the round (1-based) this lane works on */
        const int rho = q0 + rr - 1, w = 4 * rho + (ln & 3);
        const bool live = (ln & 31) < EV_TILE && rr >= 1 && rr <= steps && rho < q1 && w < sg.n_windows;
        /* the partial sums of the previous step move from lane i to lane 32 + i */
        const float carried = __shfl(psum, ln & 31);
        float sum = own ? 0.f : carried;
        if (live) {
          /* 65 pairs of terms, fetched 8 pairs at a time, one block ahead of the chain that adds them: lgkmcnt
           * counts to 15, so with more than two blocks of 8 in flight the wait in front of a chain can only be
           * for everything.  The scheduling barriers keep hipcc from sinking the loads back down in front of
           * their uses, which would put one LDS latency per block on the step's critical path. */
          double2 ta[8], tb2[8];
#define EV_LOAD8(T, B) _Pragma("unroll") for (int k = 0; k < 8; ++k) T[k] = tp[8 * (B) + k];
#define EV_SUM8(T)                                                                                      \
  _Pragma("unroll") for (int k = 0; k < 8; ++k) {                                                       \
    sum = (float)((double)sum + T[k].x);                                                                \
    sum = (float)((double)sum + T[k].y);                                                                \
  }
#define EV_SB __builtin_amdgcn_sched_barrier(0);
          EV_LOAD8(ta, 0) EV_LOAD8(tb2, 1) EV_SB
          EV_SUM8(ta) EV_SB EV_LOAD8(ta, 2) EV_SB
          EV_SUM8(tb2) EV_SB EV_LOAD8(tb2, 3) EV_SB
          EV_SUM8(ta) EV_SB EV_LOAD8(ta, 4) EV_SB
          EV_SUM8(tb2) EV_SB EV_LOAD8(tb2, 5) EV_SB
          EV_SUM8(ta) EV_SB EV_LOAD8(ta, 6) EV_SB
          EV_SUM8(tb2) EV_SB EV_LOAD8(tb2, 7)
          const double2 tl = tail[0];
          EV_SB
          EV_SUM8(ta) EV_SB
          EV_SUM8(tb2)
          sum = (float)((double)sum + tl.x);
          sum = (float)((double)sum + tl.y);
#undef EV_LOAD8
#undef EV_SUM8
#undef EV_SB
        }
        /* the rows are read: hand them back before the energies are stored */
        ev_lds_release();
        if (ln == 0) flags[8] = st;
        psum = sum;
        if (live && !own) {
          energies[sg.env_off + w] = sum;
          lc[sg.env_off + w] = bl_tail_compress((double)sum, tb.log101);
        }
        stamp(st - 1, 2);
      }
    }
    return;
  }

  /* ---- compute waves ---- */
  /* phase boundary k (0..5) of a round: the priority of the phase that starts here.  k is a literal at every
   * call: one s_setprio (which is also a scheduling barrier: the phases stay apart in the instruction stream) */
  auto phase = [&](int k) {
    const int pr = (PRIO >> (4 * k)) & 3;
    if (pr == 0) __builtin_amdgcn_s_setprio(0);
    else if (pr == 1) __builtin_amdgcn_s_setprio(1);
    else if (pr == 2) __builtin_amdgcn_s_setprio(2);
    else __builtin_amdgcn_s_setprio(3);
  };
  double *buf = reinterpret_cast<double *>(smem) + wave * EV3_SLOTS;
  const int mean = st.mean;
  const double rcp = st.rcp, rcp_lo = st.rcp_lo;
  /* mode 2 filters the integers k = s - mean themselves, exactly (bl_fir_int.h), and transforms the sums as they are:
   * the scale enters squared, through kappa and the pair constants of the split */
  const double kappa = st.kappa;
  auto nrm = [&](int k) -> double { return FIR_MODE == 2 ? (double)k : bl_norm(k, rcp, rcp_lo); };
  const int r0 = run_begin(u0 + wave), r1 = run_begin(u0 + wave + 1);
  /* FIR modes 1 / 2: the DFT is bl_fft_tan.h's; the lane's 15 pass-1 tangents t(l, k1) and the 21 pass-2 folding factors
   * of lane k1 = l live in registers for the whole run, 72 VGPRs where the 15 complex pass-1 twiddles took 60 (213 -> 212
   * VGPRs in mode 2 then; 234 with the matrix form of the FIR).  Mode 0 keeps bl_fft.h's transform and its 15 complex twiddles: with the tan form its FIR's
   * schedule lost more than the DFT gained (212 instead of 194 VGPRs, 41.48 vs 40.96 ms per 1 024 S180 songs), and its
   * energies stay those of the reference arithmetic's previous builds bit for bit.  (Until round 6 modes 0 / 1 kept 12
   * twiddles and read three per round from LDS — a relic of a 220-VGPR build; the 185-VGPR one had the room: 44.15 ->
   * 41.99 ms per 1 024 S180 songs in mode 0, identical records.  The eight split twiddles W512^(l + 16 k0) as well —
   * 218 VGPRs — made mode 0 10 % SLOWER and mode 2 no faster: profiles/EXPERIMENTS.md.) */
  constexpr bool EV3_TAN = FIR_MODE != 0;
  double t1[16];
  bl_fft16_fold<double> fold;
  c2d w1r[16];
  if (EV3_TAN) {
    const bl_fft_tan_lane<double> *tl = reinterpret_cast<const bl_fft_tan_lane<double> *>(tb.tan_lane) + l;
    t1[0] = 0.0;
#pragma unroll
    for (int k1 = 1; k1 < 16; ++k1) {
      t1[k1] = tl->t1[k1];
      asm volatile("" : "+v"(t1[k1]));
    }
    fold = tl->fold;
#define EV3_PIN(A, N) _Pragma("unroll") for (int i = 0; i < N; ++i) asm volatile("" : "+v"(A[i]));
    EV3_PIN(fold.rb, 4) EV3_PIN(fold.rc, 4) EV3_PIN(fold.rd, 4) EV3_PIN(fold.fb, 4) EV3_PIN(fold.fc, 2) EV3_PIN(fold.g, 3)
#undef EV3_PIN
  } else {
#pragma unroll
    for (int k1 = 1; k1 < 16; ++k1) {
      w1r[k1] = tw256[k1 * 16 + l];
      asm volatile("" : "+v"(w1r[k1].re), "+v"(w1r[k1].im));
    }
  }
  /* FIR mode 2, main loop: the lane's rows of the four digit planes of the tap matrix (output row l, K-group g) and
   * the constant part of every output, split over the initial values of the sums a0, a2, a4 (bl_fir_int.h) */
  typedef int ev_v4i __attribute__((ext_vector_type(4)));
  unsigned cp[4][2];
  ev_v4i ini0, ini2, ini4;
  if (FIR_MODE == 2) {
    bl_firi_tap_planes(l, g, cp);
#pragma unroll
    for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(cp[j][0]), "+v"(cp[j][1]));
    int k0, k2, k4;
    bl_firi_const(mean, &k0, &k2, &k4);
    ini0 = ev_v4i{k0, k0, k0, k0};
    ini2 = ev_v4i{k2, k2, k2, k2};
    ini4 = ev_v4i{k4, k4, k4, k4};
  }
  int base5 = (4 * r0) % 5; /* ring position of block 4 rho, the block shared with the previous round */

  if (r0 < r1) { /* the block the first round cannot inherit: samples [1024 r0, 1024 r0 + 256) */
    const int s0 = 1024 * r0 + 4 * ln; /* this lane's 4 outputs; inputs [s0 - 16, s0 + 4) */
    double r[20];
#pragma unroll
    for (int u = 0; u < 5; ++u) {
      const int i0 = s0 - 16 + 4 * u;
      const bool ok = i0 >= 0 && i0 + 4 <= n_used;
      const uint2 v = *reinterpret_cast<const uint2 *>(p + (ok ? i0 : 0));
      const unsigned w[2] = {ok ? v.x : 0u, ok ? v.y : 0u};
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int lo = (int)(short)(w[k] & 0xFFFFu), hi = (int)(short)(w[k] >> 16);
        r[4 * u + 2 * k] = ok ? nrm(lo - mean) : 0.0;
        r[4 * u + 2 * k + 1] = ok ? nrm(hi - mean) : 0.0;
      }
    }
    double *dst = buf + base5 * EV3_BLK + EV3_ROW(ln >> 2) + EV3_UNIT(2 * (ln & 3));
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#define XW(m) r[i + 16 - (m)]
      dst[EV3_UNIT(i >> 1) + (i & 1)] = BL_FIR_SEL(FIR_MODE, XW);
#undef XW
    }
  }

  /* Modes 0 / 1: lane ln owns outputs 16 ln .. 16 ln + 15 of the round's 1 024 new samples and loads the 32
   * samples they read (four 16-byte loads).  Mode 2: the round's four blocks are four 16 x 16 tiles (output 16 a + b
   * of a block at row b, column a); load t is the lane's part of the sample matrix of tile t, the eight samples
   * 16 (l - 1) + 8 g .. + 7 of the block (column l, K-group g), and the lane ends up with outputs 16 l + 4 g .. + 3
   * of every block.  Both: plus the sample that starts its zero-state output; fetched one round ahead.  Buffer loads: the song is the buffer, the lane's byte offset one register
   * that moves on by 2 048 per round, and what lies beyond the song's last window reads as zero by the
   * hardware's range check — it only reaches windows that are never summed, so any sample will do there.
   * Two VALU instructions per round instead of the 21 that clamped 64-bit addresses took (round 5). */
  uint4 pre[4];
  short preh;
  /* descriptor word 3 = 0x00020000 (DATA_FORMAT 32) and "out of range reads as zero" are the gfx9 / CDNA raw-buffer
   * rules; num_records and the offsets are 32-bit byte counts: a song is at most INT_MAX samples (bl_dsong::n is an
   * int), so 2 * n_used < 2^32 */
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "k_env_windows3: the raw-buffer descriptor and its range check are written for gfx950"
#endif
  const __amdgpu_buffer_rsrc_t prs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<int16_t *>(p), 0, (int)(2u * (unsigned)n_used), 0x00020000);
  /* first input = first output - 16 */
  unsigned voff = 2u * (unsigned)(1024 * r0 + 240 + (FIR_MODE == 2 ? 16 * l + 8 * g : 16 * ln));
  unsigned voffh = 2u * (unsigned)(1024 * r0 + 256 * g + l);
  typedef unsigned ev_v4u __attribute__((__vector_size__(16)));
  auto fetch = [&]() {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const ev_v4u v = __builtin_amdgcn_raw_buffer_load_b128(prs, (int)(voff + (FIR_MODE == 2 ? 512u : 16u) * u), 0, 0);
      pre[u] = make_uint4(v[0], v[1], v[2], v[3]);
    }
    preh = (short)__builtin_amdgcn_raw_buffer_load_b16(prs, (int)voffh, 0, 0);
    voff += 2048u;
    voffh += 2048u;
  };
  fetch();
  double held[8]; /* terms 130..256 (mir[]) of the previous round */
#pragma unroll
  for (int k0 = 0; k0 < 8; ++k0) held[k0] = 0.0;
  /* a publication that carries nothing but the second halves of the round before */
  auto publish_held_only = [&]() {
    while (__builtin_amdgcn_readfirstlane(flags[8]) < seq - 1) __builtin_amdgcn_s_sleep(1);
    ev_lds_acquire();
    double *tg = terms + (4 * wave + g) * EV_TROW;
#pragma unroll
    for (int k0 = 0; k0 < 8; ++k0)
      if (k0 < 7 || l != 15) tg[256 - l - 16 * k0] = held[k0];
    ev_wave_sync(); /* no wait: see the publication at the end of a round */
  };
  for (int s = 0; s < steps; ++s) {
    ++seq;
    const int rho = r0 + s;
    if (rho >= r1) { /* this wave's run is one round shorter than its neighbours': nothing to hand over */
      publish_held_only();
      if (ln == 0) flags[wave] = seq;
      continue;
    }
    stamp(s, 0);
    phase(0);
    double yv[16], yh;
    const int kh = (int)preh - mean;   /* this round's head sample: fetch() below overwrites preh */
    if (FIR_MODE == 2) {
      /* 1 + 2. the FIR as exact int8 matrix products (bl_fir_int.h): per tile the l' and h planes of the lane's eight
       * samples (four byte permutes, two xor) and five products, one per weight 2^0 .. 2^32.  Taps are the A operand
       * (rows = position b in a row of 16), samples the B operand (columns = row a of the block): result register r
       * of the lane is output 16 l + 4 g + r, four consecutive samples.  K = 64 operands are [c_(j+1) | c_j] against
       * [l' | h]; the two end weights have one plane each and use the K = 32 form. */
      ev_v4i acc[4][5];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const unsigned w[4] = {pre[t].x, pre[t].y, pre[t].z, pre[t].w};
        unsigned lp[2], hp[2];
        bl_firi_sample_planes(w, lp, hp);
        const ev_v4i smp = {(int)lp[0], (int)lp[1], (int)hp[0], (int)hp[1]};
        const ev_v4i zero = {0, 0, 0, 0};
#define EV3_W64(A, B) (long)(((unsigned long long)(B) << 32) | (unsigned long long)(A))
#define EV3_TAP2(J) ev_v4i{(int)cp[(J) + 1][0], (int)cp[(J) + 1][1], (int)cp[J][0], (int)cp[J][1]}
        acc[t][0] = __builtin_amdgcn_mfma_i32_16x16x32_i8(EV3_W64(cp[0][0], cp[0][1]), EV3_W64(lp[0], lp[1]), ini0, 0, 0, 0);
        acc[t][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(EV3_TAP2(0), smp, zero, 0, 0, 0);
        acc[t][2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(EV3_TAP2(1), smp, ini2, 0, 0, 0);
        acc[t][3] = __builtin_amdgcn_mfma_i32_16x16x64_i8(EV3_TAP2(2), smp, zero, 0, 0, 0);
        acc[t][4] = __builtin_amdgcn_mfma_i32_16x16x32_i8(EV3_W64(cp[3][0], cp[3][1]), EV3_W64(hp[0], hp[1]), ini4, 0, 0, 0);
#undef EV3_W64
#undef EV3_TAP2
      }
      fetch(); /* next round's samples */
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          yv[4 * t + r] = bl_firi_combine(acc[t][0][r], acc[t][1][r], acc[t][2][r], acc[t][3][r], acc[t][4][r]);
      /* zero-state heads of the four windows: the first 16 outputs of a window start from a zeroed delay line
       * (ref :121); lane (g, l) filters sample l of window g with the taps that exist, tap m being the sample of
       * lane l - m of the same 16-lane row, zero when there is none (DPP row_shr:m).  The taps are gathered as
       * integers (a 32-bit DPP move folds into the add), the nine pair sums converted, and the sum is the f64 form of
       * the same exact Y: a head has the main loop's bits where both have all their samples */
#define KH(m) __builtin_amdgcn_update_dpp(0, kh, 0x110 + (m), 0xF, 0xF, true) /* row_shr:m, 0 when there is no lane */
      const double hp_[9] = {(double)kh /* tap 16 lies before the window: zero */,
                             (double)(KH(1) + KH(15)), (double)(KH(2) + KH(14)), (double)(KH(3) + KH(13)),
                             (double)(KH(4) + KH(12)), (double)(KH(5) + KH(11)), (double)(KH(6) + KH(10)),
                             (double)(KH(7) + KH(9)), (double)KH(8)};
#undef KH
#define XP(m) hp_[m]
      yh = BL_FIR_INT_P(XP);
#undef XP
    } else {
      /* 1. normalise (ref :109-114) the 32 samples into registers */
      double r[32];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const unsigned w[4] = {pre[u].x, pre[u].y, pre[u].z, pre[u].w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int lo = (int)(short)(w[k] & 0xFFFFu), hi = (int)(short)(w[k] >> 16);
          r[8 * u + 2 * k] = nrm(lo - mean);
          r[8 * u + 2 * k + 1] = nrm(hi - mean);
        }
      }
      const double xh = nrm(kh);
      fetch(); /* next round's samples */
      /* 2. FIR (ref :123-138): outputs 16 ln .. 16 ln + 15 of the round's new samples */
#pragma unroll
      for (int i = 0; i < 16; ++i) {
#define XR(m) r[i + 16 - (m)]
        yv[i] = BL_FIR_SEL(FIR_MODE, XR);
#undef XR
      }
      /* zero-state heads of the four windows, as in mode 2 above but on the normalised doubles */
      double hx[17];
      hx[0] = xh;
      hx[1] = bl_dpp_f64<0x111>(xh);  hx[2] = bl_dpp_f64<0x112>(xh);  hx[3] = bl_dpp_f64<0x113>(xh);
      hx[4] = bl_dpp_f64<0x114>(xh);  hx[5] = bl_dpp_f64<0x115>(xh);  hx[6] = bl_dpp_f64<0x116>(xh);
      hx[7] = bl_dpp_f64<0x117>(xh);  hx[8] = bl_dpp_f64<0x118>(xh);  hx[9] = bl_dpp_f64<0x119>(xh);
      hx[10] = bl_dpp_f64<0x11A>(xh); hx[11] = bl_dpp_f64<0x11B>(xh); hx[12] = bl_dpp_f64<0x11C>(xh);
      hx[13] = bl_dpp_f64<0x11D>(xh); hx[14] = bl_dpp_f64<0x11E>(xh); hx[15] = bl_dpp_f64<0x11F>(xh);
      hx[16] = 0.0;
#define XH(m) hx[m]
      yh = BL_FIR_SEL(FIR_MODE, XH);
#undef XH
    }
    /* ring positions: window g reads block g (first half) and block g + 1 (second half); the
     * lanes of group g have just filtered block g + 1 */
    const int xa = base5 + g, xb = xa + 1;
    const int pa = xa >= 5 ? xa - 5 : xa, pb = xb >= 5 ? xb - 5 : xb;
    double *blk_a = buf + pa * EV3_BLK, *blk_b = buf + pb * EV3_BLK;
    stamp(s, 1);
    phase(1);
    ev_wave_sync(); /* previous round's LDS reads (DFT exchanges) are complete */
    if (FIR_MODE == 2) {
      /* tile t is block t + 1 of the round; the lane's four outputs are units 2 g and 2 g + 1 of row l.  Eight
       * consecutive lanes write slots 9 l + 4 g + const: all different mod 8, as in the other modes */
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int xt = base5 + t + 1, pt = xt >= 5 ? xt - 5 : xt;
        double *d = buf + pt * EV3_BLK + EV3_ROW(l) + EV3_UNIT(2 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r) d[EV3_UNIT(r >> 1) + (r & 1)] = yv[4 * t + r];
      }
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) blk_b[EV3_ROW(l) + EV3_UNIT(i >> 1) + (i & 1)] = yv[i];
    }
    buf[EV3_HEADS + ln] = yh;
    ev_wave_sync();
    /* 3. DFT input of window g: lane l holds y[32*m1 + 2*l], y[32*m1 + 2*l + 1] */
    double re[16], im[16];
    {
      const int off = EV3_ROW(l >> 3) + EV3_UNIT(l & 7); /* unit l & 7 of row 2 m1' or 2 m1' + 1 of the block */
      const double *ia = blk_a + off, *ib = blk_b + off;
      const double *i0 = l < 8 ? buf + EV3_HEADS + 16 * g + 2 * l : ia;
      re[0] = i0[0];
      im[0] = i0[1];
#pragma unroll
      for (int m1 = 1; m1 < 8; ++m1) { re[m1] = ia[EV3_ROW(2 * m1)]; im[m1] = ia[EV3_ROW(2 * m1) + 1]; }
#pragma unroll
      for (int m1 = 8; m1 < 16; ++m1) { re[m1] = ib[EV3_ROW(2 * (m1 - 8))]; im[m1] = ib[EV3_ROW(2 * (m1 - 8)) + 1]; }
    }
    ev_wave_sync(); /* window data is in registers; block g's place becomes exchange space */
    stamp(s, 2);
    phase(2);
    if (EV3_TAN) {
      /* pass 1: register bl_pos16(k1) leaves holding its value divided by c(l, k1); pass 2 folds the factors back */
      bl_fft512_pass1_tan(re, im, t1);
    } else {
      bl_fft16(re, im);
#pragma unroll
      for (int k1 = 1; k1 < 16; ++k1) bl_cmul(re[bl_pos16(k1)], im[bl_pos16(k1)], w1r[k1].re, w1r[k1].im);
    }
    stamp(s, 3);
    phase(3);
    double *xg = blk_a; /* [16][18] doubles, re then im */
    const double2 *xrow = reinterpret_cast<const double2 *>(xg + l * 18);
#pragma unroll
    for (int k1 = 0; k1 < 16; ++k1) xg[k1 * 18 + l] = re[bl_pos16(k1)];
    ev_wave_sync();
#pragma unroll
    for (int q = 0; q < 8; ++q) { const double2 v = xrow[q]; re[2 * q] = v.x; re[2 * q + 1] = v.y; }
    ev_wave_sync();
#pragma unroll
    for (int k1 = 0; k1 < 16; ++k1) xg[k1 * 18 + l] = im[bl_pos16(k1)];
    ev_wave_sync();
#pragma unroll
    for (int q = 0; q < 8; ++q) { const double2 v = xrow[q]; im[2 * q] = v.x; im[2 * q + 1] = v.y; }
    ev_wave_sync();
    stamp(s, 4);
    phase(4);
    double *tg = terms + (4 * wave + g) * EV_TROW;
    /* The rows are free once the summing wave has taken tile seq - 1 out of them.  The wait stands here, in front
     * of the second DFT pass and the power terms, not behind them (36.3 ms per 1 024 songs against 37.8 with the pass in
     * front of it and 37.5 with the wait in front of the transposes): the second halves kept from the round before leave their registers first, this round's take
     * their place as they are computed (no copies, 16 registers fewer live), and the stores of the first halves
     * go out between the arithmetic instead of in one burst. */
    stamp(s, 5);
    phase(5);
    /* polled without s_sleep: the LDS round trip paces the loop, and a sleep quantum (64 cycles) behind the summing
     * wave's release is 0.5 % of the kernel (35.8 vs 36.0 ms per 1 024 songs, three rounds; the summing wave's own
     * poll and the other waits keep theirs: without it they measured the same or slower) */
    while (__builtin_amdgcn_readfirstlane(flags[8]) < seq - 1) {}
    ev_lds_acquire();
    stamp(s, 6);
#pragma unroll
    for (int k0 = 0; k0 < 8; ++k0)
      if (k0 < 7 || l != 15) tg[256 - l - 16 * k0] = held[k0]; /* terms 130..256 of the round before */
    if (EV3_TAN) bl_fft16_folded(re, im, fold);
    else bl_fft16(re, im);
    /* the partner of pair k = k1 + 16 k0 is Z[256 - k]: register 15 - k0 of lane (16 - k1) mod 16 —
     * a mirror of the 16-lane row followed by a shift by one, two DPP moves per dword and no LDS
     * round trip; lane 0 is its own partner and takes its register 16 - k0 (k0 = 0: Z[0] itself) */
    double mir7 = 0.0;
#pragma unroll
    for (int k0 = 0; k0 < 8; ++k0) {
      const double sr = re[bl_pos16(15 - k0)], si = im[bl_pos16(15 - k0)];
      const double zr = k0 ? re[bl_pos16(16 - k0)] : re[bl_pos16(0)];
      const double zi = k0 ? im[bl_pos16(16 - k0)] : im[bl_pos16(0)];
      /* row_mirror, then a shift by one inside the row: lane 0 has no source there and keeps
       * `old`, which is what it needs instead — its own register */
      const double pr = bl_dpp_f64_old<0x111>(zr, bl_dpp_f64<0x140>(sr));
      const double pi = bl_dpp_f64_old<0x111>(zi, bl_dpp_f64<0x140>(si));
      double own;
      if (FIR_MODE == 2)
        bl_fft512_power1_sq<double>(re[bl_pos16(k0)], im[bl_pos16(k0)], pr, pi, tw512[l + 16 * k0], kappa, own, held[k0]);
      else if (EV3_TAN)
        bl_fft512_power1_tan<double, false>(re[bl_pos16(k0)], im[bl_pos16(k0)], pr, pi, tw512[l + 16 * k0], own, held[k0]);
      else
        bl_fft512_power1<double, false>(re[bl_pos16(k0)], im[bl_pos16(k0)], pr, pi, tw512[l + 16 * k0], own, held[k0]);
      tg[l + 16 * k0] = own; /* terms 0..127 of this round */
      if (k0 == 7) mir7 = held[7];
    }
    /* |X_128|^2 = |Z_128|^2 has no 1/4 of its own: give back the one the halved input took (mode 2: 4 f^2 = 2 kappa
     * for the scale f its input never took) */
    const double mr = re[bl_pos16(8)], mi = im[bl_pos16(8)];
    const double mid = (FIR_MODE == 2 ? 2.0 * kappa : 4.0) * __builtin_fma(mr, mr, mi * mi);
    if (l == 0) tg[128] = mid;
    if (l == 15) tg[129] = mir7; /* term 129 belongs to the first half */
    /* The LDS executes one wave's instructions in order: the sequence word below lands after the terms above
     * whether this wave waits for them or not, and nothing in the next round needs them: no wait (~1 k cycles
     * of LDS queue per round with no arithmetic to cover them). */
    ev_wave_sync();
    if (ln == 0) flags[wave] = seq;
    stamp(s, 7);
    base5 = base5 == 0 ? 4 : base5 - 1; /* (4 (rho + 1)) mod 5 */
  }
  ++seq; /* the second halves of the last round: one more publication, nothing else in it */
  publish_held_only();
  if (ln == 0) flags[wave] = seq;
}

/* ------------------------------------------------------------------------- */
/* k_env_tail: one lane per song, three waves per 64 songs                    */
/*
 * Parts 2-3 of bl_envelope_sort are serial per song.  The 6th-order recurrence is a chain
 * of 8 dependent f64 operations per step, everything after y_j (onset difference, weighted
 * average, two box filters, peak test) another ~30; one wave issuing all of it in order needs
 * ~340 cycles per step.  Three waves of the workgroup share it as a pipeline over 38-step blocks
 * of 64 songs:
 *   wave 0  the recurrence (bl_tail_iir)                        -> y_j   (yblk, double-buffered)
 *   wave 1  onset weighting, atk, first box filter (bl_tail_ab)  -> o1    (oblk + per-lane counts)
 *   wave 2  second box filter, peak test (bl_tail_c)             -> beat
 * Every wave sits alone on a SIMD and is bound by its own dependent chain; a step costs what the
 * slowest stage costs — the recurrence, ~90 cycles.  The o1 stream is not one value per step at
 * the edges of a song (bl_box19): a block carries up to 48 values per lane and a count.
 */
#define BL_TAIL_OMAX 48 /* 38 + the 10 values box 1 flushes when a song ends */

__global__ __launch_bounds__(192) void k_env_tail(const bl_dsong *__restrict__ songs,
                                                  const double *__restrict__ lc, int n_songs,
                                                  bl_amd_song_result *res, int what) {
  __shared__ double yblk[2][38 * 64];            /* y_j of one block, [step][song] */
  __shared__ double oblk[2][BL_TAIL_OMAX * 64];  /* box-1 outputs of one block, [slot][song] */
  __shared__ int ocnt[2][64];                    /* how many of them per song */
  __shared__ double rings_ab[29 * 64];           /* wave 1: box-1 ring + its 10 `old` cells */
  __shared__ double rings_c[19 * 64];            /* wave 2: box-2 ring */
  __shared__ int flag_mem[4];
  typedef __attribute__((address_space(3))) volatile int lds_vint;
  /* [0]: y blocks produced, [1]: y blocks consumed, [2]: o1 blocks produced, [3]: o1 blocks consumed */
  lds_vint *flags = (lds_vint *)flag_mem;
  /* a handful of latency-bound waves that run beside the wide kernels: let them issue first */
  __builtin_amdgcn_s_setprio(3);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int song = blockIdx.x * 64 + lane;
  const bool valid = song < n_songs;
  bl_dsong sg;
  if (valid) sg = songs[song];
  else { sg.nb_frames = 0; sg.n_windows = 0; sg.env_off = 0; sg.n = 1; sg.duration = 1; }
  const int N = 2 * sg.nb_frames;
  int maxN = N;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) maxN = max(maxN, __shfl_xor(maxN, off));
  if (threadIdx.x < 4) flags[threadIdx.x] = 0;
  __syncthreads();
  const int n_blocks = (maxN + 37) / 38;

  if (wave == 0) {
    /* ---- the recurrence: input pairs (x_j, 0) -> (y_j, y_j+1) ---- */
    bl_tail_iir a;
    a.init();
    /* Every lane reads its own song's compressed envelope, 19 windows (one block) at a time and
     * two blocks ahead, straight into registers: three register sets rotate through "in use",
     * "arriving" and "being requested".  The loads are unconditional from clamped addresses
     * (under an exec mask hipcc waits vmcnt(0) after every few of them) and a window past the
     * song's end is zeroed where it is used.  Earlier forms: one coalesced load per song and a
     * transposition through LDS, fetched on demand (~18 k cycles of HBM latency in front of every
     * third block, more than the recurrence itself) or a tile ahead (the 64 x 3 v_readlane that
     * fetch song i's geometry still cost 9 k cycles per tile). */
    const double *mylc = lc + sg.env_off;
    const int nw = sg.n_windows;
    auto fetch = [&](int kb_, double (&dst)[19]) {
#pragma unroll
      for (int q = 0; q < 19; ++q) dst[q] = mylc[max(min(19 * kb_ + q, nw - 1), 0)];
    };
    auto block = [&](int kb, double (&cur)[19], double (&fut)[19]) {
      if (kb >= n_blocks) return;
      fetch(kb + 2, fut);
      double *yo = yblk[kb & 1] + lane;
      double ye[38];
#pragma unroll
      for (int q = 0; q < 19; ++q) a.pair(19 * kb + q < nw ? cur[q] : 0.0, ye[2 * q], ye[2 * q + 1]);
      /* the buffer is free once the block before the previous one has been consumed */
      while (__builtin_amdgcn_readfirstlane(flags[1]) < kb - 1) __builtin_amdgcn_s_sleep(1);
      ev_lds_acquire();
#pragma unroll
      for (int q = 0; q < 38; ++q) yo[q * 64] = ye[q];
      ev_lds_release();
      bl_wave_sync();
      if (lane == 0) flags[0] = kb + 1;
    };
    double pa[19], pb[19], pc[19];
    fetch(0, pa);
    fetch(1, pb);
    for (int kb = 0; kb < n_blocks; kb += 3) {
      block(kb, pa, pc);
      block(kb + 1, pb, pa);
      block(kb + 2, pc, pb);
    }
    return;
  }

  if (wave == 1) {
    /* ---- y_j -> weighting, atk, box 1 -> o1 ---- */
    bl_tail_ab t;
    t.init(sg.nb_frames, rings_ab + lane, 64);
    for (int kb = 0; kb < n_blocks; ++kb) {
      while (__builtin_amdgcn_readfirstlane(flags[0]) < kb + 1) __builtin_amdgcn_s_sleep(1);
      while (__builtin_amdgcn_readfirstlane(flags[3]) < kb - 1) __builtin_amdgcn_s_sleep(1);
      ev_lds_acquire();
      const double *yin = yblk[kb & 1] + lane;
      const int j = 38 * kb;
      bl_tail_fifo f;
      f.base = oblk[kb & 1] + lane;
      f.stride = 64;
      f.count = 0;
      /* A song in its steady state for the whole block takes the straight-line path; the others —
       * the first 40 steps (the same blocks for every song) and each song's own last dozen — take
       * the step-by-step one.  With equal lengths the branch is wave-uniform; with mixed lengths
       * both sides run (exec-masked) only for the block or two in which a song of the wave ends. */
      if (bl_tail_ab::chunk_ok(j, N)) {
        t.fast_chunk38(yin, 64, f.base, 64);
        f.count = 38;
      } else if (j < N) {
        for (int q = 0; q < 38; ++q) {
          const int jj = j + q;
          if (jj < N) {
            t.step(jj, yin[q * 64], f);
            if (jj == N - 1) t.finish(f);
          }
        }
      }
      ocnt[kb & 1][lane] = f.count;
      ev_lds_release();
      bl_wave_sync();
      if (lane == 0) { flags[1] = kb + 1; flags[2] = kb + 1; }
    }
    if (valid) {
      bl_amd_song_result *r = res + sg.out_idx;
      r->atk_sum = t.atk;
      r->v.attack = bl_tail_attack(t.atk, sg.n);
    }
    return;
  }

  /* ---- o1 -> box 2 -> peaks ---- */
  bl_tail_c c;
  c.init(sg.nb_frames, rings_c + lane, 64);
  for (int kb = 0; kb < n_blocks; ++kb) {
    while (__builtin_amdgcn_readfirstlane(flags[2]) < kb + 1) __builtin_amdgcn_s_sleep(1);
    ev_lds_acquire();
    const double *oin = oblk[kb & 1] + lane;
    const int cnt = ocnt[kb & 1][lane];
    if (cnt == 38 && c.chunk_ok()) {
      c.fast_chunk38(oin, 64);
    } else {
      for (int q = 0; q < BL_TAIL_OMAX; ++q)
        if (q < cnt) c.push(oin[q * 64]);
    }
    if (valid && c.taken == N && cnt > 0) c.finish(); /* the block that delivered the song's last output */
    ev_lds_release();
    bl_wave_sync();
    if (lane == 0) flags[3] = kb + 1;
  }
  if (!valid) return;
  bl_amd_song_result *r = res + sg.out_idx;
  r->beat = c.beat();
  r->v.tempo = bl_tail_tempo(c.beat(), sg.duration);
  (void)what;
}

/* ========================================================================= */
/* launchers (declared in bl_launch.h)                                        */

static long long *g_env_probe = nullptr;
#ifdef BL_AMD_MEASURE

/* measurement builds only: pick a priority table of EV_PRIO_TABS at run time (-1: the compiled default; bits 24..:
 * the PROBE instantiation) and give the stamps a device buffer of 8 x EV_PROBE_ROUNDS x EV_PROBE_SLOTS int64 */
static int g_env_variant = -1;
extern "C" __attribute__((visibility("default"))) int bl_amd_measure_env(int variant, void *d_probe) {
  g_env_variant = variant;
  g_env_probe = static_cast<long long *>(d_probe);
  return BL_OK;
}
#endif

/* Which form of the 17-tap FIR k_env_windows3 runs:
 *   0  the reference's unfused order (BL_FIR) — bit-identical window energies;
 *   1  each product folded into the sum by an fma (BL_FIR_FUSED);
 *   2  the normalisation folded into the filter, on the integers: the exact sum of integer taps times integer
 *      samples, scaled once (bl_fir_int.h) — the default.
 * bl_amd_set_fir_mode() wins over the environment variable BL_AMD_FIR_FUSED, which wins over the
 * compiled default.  Read on every launch, so one process can run all of them (the A/B tools do). */
static std::atomic<int> g_fir_mode{-1};
int blk_fir_mode() {
  int m = g_fir_mode.load(std::memory_order_relaxed);
  if (m < 0) {
    const char *e = getenv("BL_AMD_FIR_FUSED");
    m = e && *e ? atoi(e) : BL_FIR_FUSED_DEFAULT;
  }
  return m < 0 || m > 2 ? BL_FIR_FUSED_DEFAULT : m;
}
extern "C" int bl_amd_fir_mode(void) { return blk_fir_mode(); }
extern "C" int bl_amd_set_fir_mode(int mode) {
  if (mode < -1 || mode > 2) return BL_UNEXPECTED;
  g_fir_mode.store(mode, std::memory_order_relaxed);
  return BL_OK;
}

/* Every instantiation of k_env_windows3 the build can launch, as EV_X(FIR mode, priority table, PROBE), written once:
 * blk_env_configure_device gives each its LDS attribute and blk_env_windows picks among the same list, so a table
 * added to EV_PRIO_TABS cannot be launched without its attribute.  The product has the three FIR modes under
 * BL_ENV_PRIO; a measurement build adds the stamped form of mode 2 and both forms of every table of EV_PRIO_TABS. */
#define EV_X_BOTH(T) EV_X(2, T, false) EV_X(2, T, true)
#ifdef BL_AMD_MEASURE
#define EV_INSTANCES EV_X(0, BL_ENV_PRIO, false) EV_X(1, BL_ENV_PRIO, false) EV_X_BOTH(BL_ENV_PRIO) EV_PRIO_TABS(EV_X_BOTH)
#else
#define EV_INSTANCES EV_X(0, BL_ENV_PRIO, false) EV_X(1, BL_ENV_PRIO, false) EV_X(2, BL_ENV_PRIO, false)
#endif

int blk_env_configure_device(void) {
#define EV_X(M, T, P)                                                                                    \
  BL_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_env_windows3<M, T, P>),              \
                                   hipFuncAttributeMaxDynamicSharedMemorySize, EV3_LDS_BYTES));
  EV_INSTANCES
#undef EV_X
  return BL_OK;
}

/* one 512-thread workgroup per CU; the blocks of a song split its rounds of four windows
 * into contiguous runs, one per compute wave: at least four rounds per run, so that the
 * block a run filters before its first round stays a small part of it */
int blk_env_windows(const blk_analyze_args &a, int fir_mode, int first, int count, int maxn) {
  Mark m(a.mark, a.mark_user, PK_ENV, a.stream);
  const int gx2 = grid_x_for(std::max(1, (2 * (maxn / 512)) / (4 * 4 * EV_CWAVES)), count, 2, a.n_cu);
  const dim3 grid(gx2, count), block(64 * (EV_CWAVES + 1));
  int prio = BL_ENV_PRIO;
  bool probe = false;
#ifdef BL_AMD_MEASURE
  /* bl_amd_measure_env(): A/B of the priority tables (FIR mode 2 only), with or without the phase stamps */
  if (fir_mode == 2 && g_env_variant >= 0) {
    prio = g_env_variant & 0xFFFFFF;
    probe = (g_env_variant >> 24) != 0;
  }
#endif
#define EV_X(M, T, P)                                                                                    \
  if (fir_mode == (M) && prio == (T) && probe == (P)) {                                                  \
    hipLaunchKernelGGL((k_env_windows3<M, T, P>), grid, block, EV3_LDS_BYTES, a.stream, a.pcm,           \
                       a.songs + first, a.stats + first, a.tb, a.energies, a.lc, g_env_probe);           \
    return BL_OK;                                                                                        \
  }
  EV_INSTANCES
#undef EV_X
  return BL_UNEXPECTED; /* a priority table the build does not instantiate */
}

void blk_env_tail(const blk_analyze_args &a, hipStream_t s, int first, int count) {
  Mark m(a.mark, a.mark_user, PK_TAIL, s);
  hipLaunchKernelGGL(k_env_tail, dim3((count + 63) / 64), dim3(192), 0, s, a.songs + first, a.lc, count,
                     a.results, a.what);
}
