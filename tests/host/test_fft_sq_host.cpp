// Host-side test of FIR mode 2's unscaled transform (bliss_amd/csrc/bl_fft_tan.h: bl_fft512_power1_sq, bl_fft_sq_fill,
// bl_fft_sq_consts; bl_fir_int.h: bl_firi_power_scale).  The kernel transforms the exact integer filter sums Y and
// multiplies the power terms by kappa = 2 f^2, f = 1 / (1e7 * 2 V'), where it used to transform Y * RN(f).  The lane
// code runs on the CPU as in test_fft_tan_host.cpp, on windows of integer Y with zero-state heads, and is held to
//   (1) every one of the 257 terms against a long-double DFT of Y * f, in units of sum_k |X_k|^2: the largest error at
//       most 2 x, the mean error at most 1.25 x those of the scaled tan path (bl_fft512_power1_tan) on the same windows
//       in the same run (the margin covers kappa and the two scaled constants, each rounded once more);
//   (2) the f32 ordered sum of the 257 terms (ref tempo_atk_sort.c:142-149) equal to the one formed from the
//       long-double terms in every window;
//   (3) sign and factor: own and mir of bl_fft512_power1_sq equal to bl_fft512_power1_tan<double, false> on the
//       f-scaled input for random (z, p) and all 128 k, to 1e-13 of the pair's energy own + mir (the error of either
//       form is of order eps times that energy, whatever the split between own and mir; a wrong sign or factor
//       moves a term by the order of the energy itself);
//   (4) kappa a normal number within one rounding of 2 f^2 (as far as long double can tell: 0.502 ulp) at the two ends
//       of V' and in between.
// Windows: 10^5 random ones in four loudness classes (full range, a few hundred LSB, full-scale signs, near the rails),
// then 2 000 each of few-LSB, impulses in silence, full-scale square waves, alternating full scale, silence, and
// integers just under 2^45 (the bound of |Y|; no PCM reaches it); V' takes its smallest (variance 1), its largest
// (variance 2^31 - 1) and mid-range values in turn.
// Build: g++ -O2 -std=c++17 -ffp-contract=off.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../bliss_amd/csrc/bl_fft_tan.h"
#include "../../bliss_amd/csrc/bl_fir_int.h"

static unsigned long long g_rng = 0x9E3779B97F4A7C15ull;
static unsigned long long xrand() {
  g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
  return g_rng;
}
static double urand() { return (double)(xrand() >> 11) * 0x1p-53; } /* [0, 1) */

/* long-double radix-2 FFT of the 512 real samples: |X_k|^2, k = 0..256 */
static void ref_power(const double *x, long double *pw) {
  static long double wr[256], wi[256];
  static bool init = false;
  const long double PI = 3.14159265358979323846264338327950288L;
  if (!init) {
    for (int k = 0; k < 256; ++k) { wr[k] = cosl(2 * PI * k / 512); wi[k] = -sinl(2 * PI * k / 512); }
    init = true;
  }
  long double re[512], im[512];
  for (int n = 0; n < 512; ++n) {
    int r = 0;
    for (int b = 0; b < 9; ++b) r |= ((n >> b) & 1) << (8 - b);
    re[r] = x[n]; im[r] = 0;
  }
  for (int len = 2; len <= 512; len <<= 1)
    for (int s = 0; s < 512; s += len)
      for (int j = 0; j < len / 2; ++j) {
        const int w = j * (512 / len);
        const long double ur = re[s + j], ui = im[s + j];
        const long double vr = re[s + j + len / 2] * wr[w] - im[s + j + len / 2] * wi[w];
        const long double vi = re[s + j + len / 2] * wi[w] + im[s + j + len / 2] * wr[w];
        re[s + j] = ur + vr; im[s + j] = ui + vi;
        re[s + j + len / 2] = ur - vr; im[s + j + len / 2] = ui - vi;
      }
  for (int k = 0; k <= 256; ++k) pw[k] = re[k] * re[k] + im[k] * im[k];
}

static bl_fft_tan_lane<double> g_lanes[16];
static bl_c2<double> g_tw512t[128], g_cs512[128];

/* both passes of the lane code, as k_env_windows3 runs them: Z_k of lane l = k & 15 at tr[l][bl_pos16(k >> 4)] */
static void lanes_dft(const double *x, double (&tr)[16][16], double (&ti)[16][16]) {
  double re[16][16], im[16][16];
  for (int n0 = 0; n0 < 16; ++n0)
    for (int m1 = 0; m1 < 16; ++m1) { re[n0][m1] = x[2 * (16 * m1 + n0)]; im[n0][m1] = x[2 * (16 * m1 + n0) + 1]; }
  for (int l = 0; l < 16; ++l) bl_fft512_pass1_tan<double>(re[l], im[l], g_lanes[l].t1);
  for (int k1 = 0; k1 < 16; ++k1)
    for (int n0 = 0; n0 < 16; ++n0) { tr[k1][n0] = re[n0][bl_pos16(k1)]; ti[k1][n0] = im[n0][bl_pos16(k1)]; }
  for (int l = 0; l < 16; ++l) bl_fft16_folded<double>(tr[l], ti[l], g_lanes[l].fold);
}

/* the scaled path: x = Y * fsc, the tan-form split, 4 x the middle term */
static void cur_power(const double *Y, double fsc, double *pw) {
  double x[512], tr[16][16], ti[16][16];
  for (int j = 0; j < 512; ++j) x[j] = Y[j] * fsc;
  lanes_dft(x, tr, ti);
  for (int l = 0; l < 16; ++l)
    for (int k0 = 0; k0 < 8; ++k0) {
      /* partner Z[256 - k]: register 15 - k0 of lane (16 - l) % 16; lane 0 its own register 16 - k0 (k0 = 0: Z[0]) */
      const int pl = l ? 16 - l : 0, pk = l ? 15 - k0 : (k0 ? 16 - k0 : 0);
      bl_fft512_power1_tan<double, false>(tr[l][bl_pos16(k0)], ti[l][bl_pos16(k0)], tr[pl][bl_pos16(pk)],
                                          ti[pl][bl_pos16(pk)], g_tw512t[l + 16 * k0], pw[l + 16 * k0], pw[256 - l - 16 * k0]);
    }
  const double mr = tr[0][bl_pos16(8)], mi = ti[0][bl_pos16(8)];
  pw[128] = 4.0 * bl_fma(mr, mr, mi * mi);
}

/* the unscaled path: x = Y, the split from the squares with the song's constants, 2 kappa x the middle term */
static void new_power(const double *Y, double kappa, double *pw) {
  double tr[16][16], ti[16][16];
  lanes_dft(Y, tr, ti);
  for (int l = 0; l < 16; ++l)
    for (int k0 = 0; k0 < 8; ++k0) {
      const int pl = l ? 16 - l : 0, pk = l ? 15 - k0 : (k0 ? 16 - k0 : 0);
      const bl_c2<double> cs = bl_fft_sq_consts<double>(g_cs512[l + 16 * k0], kappa); /* what the kernel keeps in LDS */
      bl_fft512_power1_sq<double>(tr[l][bl_pos16(k0)], ti[l][bl_pos16(k0)], tr[pl][bl_pos16(pk)], ti[pl][bl_pos16(pk)],
                                  cs, kappa, pw[l + 16 * k0], pw[256 - l - 16 * k0]);
    }
  const double mr = tr[0][bl_pos16(8)], mi = ti[0][bl_pos16(8)];
  pw[128] = (2.0 * kappa) * bl_fma(mr, mr, mi * mi);
}

static float ordered_sum(const double *p) { /* ref tempo_atk_sort.c:142-149: float += double */
  float s = 0;
  for (int k = 0; k <= 256; ++k) s = (float)((double)s + p[k]);
  return s;
}

/* one window of integer filter sums with its zero-state head (the first 16 outputs start from a zeroed delay line) */
static void make_window(int kind, double *Y) {
  if (kind == 9) { /* integers just under 2^45 */
    for (int j = 0; j < 512; ++j) {
      const long long m = (1LL << 45) - 1 - (long long)(xrand() % 4096);
      Y[j] = (double)((xrand() & 1) ? m : -m);
    }
    return;
  }
  static const int means[5] = {-32768, -1, 0, 1, 32767};
  const int mean = kind >= 4 && kind != 8 ? (int)(xrand() % 3) - 1 : means[xrand() % 5];
  const int period = 2 + (int)(xrand() % 300), amp = 1 + (int)(xrand() % 4);
  int k[512];
  for (int i = 0; i < 512; ++i) {
    const int16_t x = (int16_t)xrand();
    int s;
    switch (kind) {
      case 0: s = x; break;                                                /* full range */
      case 1: s = x >> 9; break;                                           /* quiet */
      case 2: s = (x & 1) ? 32767 : -32768; break;                         /* full-scale signs */
      case 3: s = (x >> 15) ? -32768 + (x & 3) : 32767 - (x & 3); break;   /* near the rails */
      case 4: s = (int)floor((urand() - 0.5) * 2 * amp + 0.5); break;      /* a few LSB */
      case 5: s = urand() < 0.004 ? ((x & 1) ? 32767 : -32768) : 0; break; /* impulses in silence */
      case 6: s = ((i / period) & 1) ? 32767 : -32768; break;              /* full-scale square wave */
      case 7: s = (i & 1) ? 32767 : -32768; break;                         /* alternating full scale */
      default: s = mean; break;                                            /* silence: k = 0 */
    }
    k[i] = s - mean;
  }
  for (int j = 0; j < 512; ++j) {
    long long y = 0;
    for (int m = 0; m <= 16; ++m)
      if (j - m >= 0) y += (long long)bl_firi_tap(m) * k[j - m];
    Y[j] = (double)y; /* |y| < 2^45: exact */
  }
}

struct song_scale { double fsc, kappa; long double f; };
static song_scale scale_of(long long variance) { /* k_song_prep */
  const double vprime = (double)variance / 32768.0, v2 = 2.0 * vprime;
  const double rcp = 1.0 / v2, rcp_lo = bl_fma(-rcp, v2, 1.0) / v2;
  song_scale s;
  s.fsc = bl_firi_scale(rcp, rcp_lo);
  s.kappa = bl_firi_power_scale(rcp, rcp_lo);
  s.f = 32768.0L / (2.0e7L * (long double)variance);
  return s;
}

static long g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { if (g_fail++ < 10) { printf(__VA_ARGS__); printf("\n"); } } } while (0)

int main() {
  bl_fft_tan_fill(g_lanes, g_tw512t);
  bl_fft_sq_fill(g_cs512);
  const long long VMIN = 1, VMAX = 2147483647LL;

  /* (4) kappa at the ends of V' and in between */
  for (int i = 0; i < 10002; ++i) {
    const long long var = i == 0 ? VMIN : i == 1 ? VMAX : 1 + (long long)(xrand() % (unsigned long long)VMAX);
    const song_scale s = scale_of(var);
    const long double want = 2.0L * s.f * s.f;
    const double ulp = nextafter(s.kappa, INFINITY) - s.kappa;
    CHECK(std::isnormal(s.kappa), "(4) variance %lld: kappa %.17g is not a normal number", var, s.kappa);
    /* half an ulp, plus what the long-double 2 f^2 is itself off by: three roundings of 2^-64, 0.0015 ulp of a double */
    CHECK(fabsl((long double)s.kappa - want) <= 0.502L * ulp, "(4) variance %lld: kappa %.17g, 2 f^2 %.21Lg", var, s.kappa, want);
  }
  printf("(4) kappa: %.17g at the smallest V', %.17g at the largest\n", scale_of(VMIN).kappa, scale_of(VMAX).kappa);

  /* (3) sign and factor of the pair function */
  {
    double worst = 0;
    for (int trial = 0; trial < 2000; ++trial) {
      const song_scale s = scale_of(trial % 3 == 0 ? VMIN : trial % 3 == 1 ? VMAX : 1 + (long long)(xrand() % (unsigned long long)VMAX));
      const double mag = ldexp(1.0, (int)(xrand() % 54));
      for (int k = 0; k < 128; ++k) {
        const double zr = floor((urand() - 0.5) * mag), zi = floor((urand() - 0.5) * mag);
        const double pr = k ? floor((urand() - 0.5) * mag) : zr, pi = k ? floor((urand() - 0.5) * mag) : zi;
        double o1, m1, o2, m2;
        bl_fft512_power1_sq<double>(zr, zi, pr, pi, bl_fft_sq_consts<double>(g_cs512[k], s.kappa), s.kappa, o1, m1);
        bl_fft512_power1_tan<double, false>(zr * s.fsc, zi * s.fsc, pr * s.fsc, pi * s.fsc, g_tw512t[k], o2, m2);
        const double en = o2 + m2;
        const double e = en > 0 ? fmax(fabs(o1 - o2), fabs(m1 - m2)) / en : fmax(fabs(o1 - o2), fabs(m1 - m2));
        worst = fmax(worst, e);
        CHECK(e <= 1e-13, "(3) k %d: own %.17g / %.17g, mir %.17g / %.17g", k, o1, o2, m1, m2);
      }
    }
    printf("(3) pair function against the scaled tan form: largest difference %.3e of the pair's energy\n", worst);
  }

  /* (1), (2) */
  const int N = 100000 + 6 * 2000;
  static double Y[512], pc[257], pn[257], pd[257];
  static long double pr[257];
  double max_cur = 0, max_new = 0;
  long double sum_cur = 0, sum_new = 0;
  long diff_cur = 0, diff_new = 0, windows = 0, terms = 0;
  for (int w = 0; w < N; ++w) {
    const int kind = w < 100000 ? w % 4 : 4 + (w - 100000) / 2000;
    const int vc = (w / 4) % 3; /* every kind meets every class of V' */
    const long long var = vc == 0 ? VMIN : vc == 1 ? VMAX : 1 + (long long)(xrand() % (unsigned long long)VMAX);
    const song_scale s = scale_of(var);
    make_window(kind, Y);
    ref_power(Y, pr);
    const long double f2 = 4.0L * s.f * s.f; /* the kernel's terms are those of the unhalved signal 2 f Y */
    long double tot = 0;
    for (int k = 0; k <= 256; ++k) { pr[k] *= f2; tot += pr[k]; pd[k] = (double)pr[k]; }
    cur_power(Y, s.fsc, pc);
    new_power(Y, s.kappa, pn);
    const long double unit = tot > 0 ? tot : 1;
    for (int k = 0; k <= 256; ++k) {
      const double ec = (double)(fabsl((long double)pc[k] - pr[k]) / unit), en = (double)(fabsl((long double)pn[k] - pr[k]) / unit);
      max_cur = fmax(max_cur, ec); max_new = fmax(max_new, en);
      sum_cur += ec; sum_new += en;
    }
    terms += 257;
    const float e_ref = ordered_sum(pd), e_cur = ordered_sum(pc), e_new = ordered_sum(pn);
    if (memcmp(&e_ref, &e_new, 4)) {
      if (diff_new < 5) printf("(2) window %d (kind %d, variance %lld): energy %.9g, long double %.9g\n", w, kind, var, e_new, e_ref);
      ++diff_new;
    }
    diff_cur += memcmp(&e_ref, &e_cur, 4) != 0;
    ++windows;
  }
  const double mean_cur = (double)(sum_cur / terms), mean_new = (double)(sum_new / terms);
  printf("(1) %ld windows, %ld terms; error per term in units of sum |X|^2: scaled tan path max %.3e mean %.3e, "
         "unscaled path max %.3e mean %.3e\n", windows, terms, max_cur, mean_cur, max_new, mean_new);
  printf("(2) f32 ordered sums differing from the long-double ones: unscaled path %ld, scaled tan path %ld\n", diff_new, diff_cur);
  const bool ok = g_fail == 0 && diff_new == 0 && max_new <= 2.0 * max_cur && mean_new <= 1.25 * mean_cur;
  printf(ok ? "OK\n" : "FAIL\n");
  return ok ? 0 : 1;
}
