// Host-side test of bliss_amd/csrc/bl_fft_tan.h, the tan-form transform of k_env_windows3: runs the lane code on
// the CPU (16 lanes emulated one after another per pass, the transpose and the split's partner values as the
// kernel moves them) over 10^5 random windows and edge material, and holds it to
//   * |X_k|^2 against a long-double FFT: the largest and the mean error per window, in units of sum_k |X_k|^2,
//     no worse than bl_fft.h's bl_fft16 path on the same windows (within a few per cent: both sit at the f64
//     rounding floor, and which one rounds a given window better is a coin toss);
//   * the f32-rounded ordered sum of the 257 terms (ref tempo_atk_sort.c:142-149) equal to the oracle's in every
//     window.
// Edge kinds: few-LSB, impulses in silence, full-scale square waves, tone + noise, silence, and full-range noise at the
// largest scale the FIR can produce (2^46), which exercises the 2^600 scaling of the one cos = 0 twiddle.
// Build: g++ -O2 -std=c++17 -ffp-contract=off, linked with the oracle's C sources.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../bliss_amd/csrc/bl_fft_tan.h"
#include "../../oracle/bliss_oracle.h"

static unsigned long long g_rng = 0x9E3779B97F4A7C15ull;
static double urand() { /* [0, 1) */
  g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
  return (double)(g_rng >> 11) * 0x1p-53;
}

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

/* bl_fft.h's path (tests/host/test_fft_host.cpp's lanes) */
static void old_power(const double *x, double *pw) {
  static std::vector<bl_c2<double>> tw256(256), tw512(256);
  static bool init = false;
  if (!init) {
    const double pi = 3.14159265358979323846;
    for (int e = 0; e < 256; ++e) {
      const int ex = ((e & 15) * (e >> 4)) & 255;
      tw256[e].re = cos(2 * pi * ex / 256); tw256[e].im = -sin(2 * pi * ex / 256);
      tw512[e].re = cos(2 * pi * e / 512); tw512[e].im = -sin(2 * pi * e / 512);
    }
    init = true;
  }
  bl_c2<double> xch[BL_FFT_XCH_ELEMS], par[BL_FFT_PAR_ELEMS];
  double re[16][16], im[16][16];
  for (int n0 = 0; n0 < 16; ++n0)
    for (int m1 = 0; m1 < 16; ++m1) { re[n0][m1] = x[2 * (16 * m1 + n0)]; im[n0][m1] = x[2 * (16 * m1 + n0) + 1]; }
  for (int l = 0; l < 16; ++l) bl_fft512_phaseA<double>(l, re[l], im[l], tw256.data(), xch);
  for (int l = 0; l < 16; ++l) bl_fft512_phaseB<double>(l, re[l], im[l], xch, par);
  for (int l = 0; l < 16; ++l) {
    double own[8], mir[8], mid;
    bl_fft512_phaseC<double>(l, re[l], im[l], tw512.data(), par, own, mir, mid);
    for (int k0 = 0; k0 < 8; ++k0) { pw[l + 16 * k0] = own[k0]; pw[256 - l - 16 * k0] = mir[k0]; }
    if (l == 0) pw[128] = mid;
  }
}

/* bl_fft_tan.h's path, as k_env_windows3 runs it */
static bl_fft_tan_lane<double> g_lanes[16];
static bl_c2<double> g_tw512t[128];
static void new_power(const double *x, double *pw) {
  double re[16][16], im[16][16];
  for (int n0 = 0; n0 < 16; ++n0)
    for (int m1 = 0; m1 < 16; ++m1) { re[n0][m1] = x[2 * (16 * m1 + n0)]; im[n0][m1] = x[2 * (16 * m1 + n0) + 1]; }
  for (int l = 0; l < 16; ++l) bl_fft512_pass1_tan<double>(re[l], im[l], g_lanes[l].t1);
  double tr[16][16], ti[16][16]; /* the transpose: lane k1 register n0 <- lane n0 register bl_pos16(k1) */
  for (int k1 = 0; k1 < 16; ++k1)
    for (int n0 = 0; n0 < 16; ++n0) { tr[k1][n0] = re[n0][bl_pos16(k1)]; ti[k1][n0] = im[n0][bl_pos16(k1)]; }
  for (int l = 0; l < 16; ++l) bl_fft16_folded<double>(tr[l], ti[l], g_lanes[l].fold);
  for (int l = 0; l < 16; ++l)
    for (int k0 = 0; k0 < 8; ++k0) {
      /* partner Z[256 - k]: register 15 - k0 of lane (16 - l) % 16; lane 0 its own register 16 - k0 (k0 = 0: Z[0]) */
      const int pl = l ? 16 - l : 0, pk = l ? 15 - k0 : (k0 ? 16 - k0 : 0);
      bl_fft512_power1_tan<double>(tr[l][bl_pos16(k0)], ti[l][bl_pos16(k0)], tr[pl][bl_pos16(pk)],
                                   ti[pl][bl_pos16(pk)], g_tw512t[l + 16 * k0], pw[l + 16 * k0], pw[256 - l - 16 * k0]);
    }
  const double mr = tr[0][bl_pos16(8)], mi = ti[0][bl_pos16(8)];
  pw[128] = bl_fma(mr, mr, mi * mi);
}

static float ordered_sum(const double *p) { /* ref tempo_atk_sort.c:142-149: float += double */
  float s = 0;
  for (int k = 0; k <= 256; ++k) s = (float)((double)s + p[k]);
  return s;
}

/* one window of kind `kind`: a 17-tap smoothing of int16-like material, as the envelope's FIR leaves it */
static void make_window(int kind, double *x) {
  static const double taps[17] = {0.002, 0.006, 0.014, 0.029, 0.05, 0.074, 0.097, 0.113, 0.118,
                                  0.113, 0.097, 0.074, 0.05, 0.029, 0.014, 0.006, 0.002};
  double s[528];
  /* kind 6: the largest window the kernel can see.  Mode 2 filters k = s - mean (|k| < 2^16) with taps c_m / (2 V),
   * V = variance / 2^30 >= 2^-30: |taps| <= 2^29, outputs below 2^46.  Element (8, 8) of pass 1 carries them times
   * 2^600 (bl_fft_tan.h); far from the 2^1024 of the format */
  const double norm = kind == 6 ? 0x1p29 : 1.0 / (2.0 * (0.05 + urand()) * 32768.0);
  const int period = 2 + (int)(urand() * 300);
  const int amp = 1 + (int)(urand() * 4);
  for (int i = 0; i < 528; ++i) {
    double v;
    switch (kind) {
      case 0: v = floor((urand() - 0.5) * 65535.0); break;                      /* full-range noise */
      case 1: v = floor((urand() - 0.5) * 2 * amp + 0.5); break;                  /* a few LSB loud */
      case 2: v = (urand() < 0.004) ? (urand() < 0.5 ? 32767.0 : -32768.0) : 0; break; /* impulses in silence */
      case 3: v = ((i / period) & 1) ? 32767.0 : -32768.0; break;                 /* full-scale square wave */
      case 4: v = floor(10000.0 * sin(0.001 * period * i) + (urand() - 0.5) * 64); break; /* tone + noise */
      case 6: v = floor((urand() - 0.5) * 65535.0); break;                      /* the same, loudest scale */
      default: v = 0; break;                                                      /* silence */
    }
    s[i] = v * norm;
  }
  for (int j = 0; j < 512; ++j) {
    /* zero-state head: the first 16 outputs see a zeroed delay line (ref tempo_atk_sort.c:121) */
    double y = 0;
    for (int m = 0; m < 17; ++m) y += taps[m] * (j - m >= 0 ? s[16 + j - m] : 0.0);
    x[j] = y;
  }
}

int main() {
  bl_fft_tan_fill(g_lanes, g_tw512t);
  const int N = 100000 + 7 * 2000;
  double x[512], po[257], pn[257], ore[257], oim[257], op[257];
  long double pr[257];
  double max_old = 0, max_new = 0, sum_old = 0, sum_new = 0;
  long diff_new = 0, diff_old = 0, windows = 0;
  for (int w = 0; w < N; ++w) {
    const int kind = w < 100000 ? (w % 3 == 0 ? 0 : w % 3 == 1 ? 4 : 1) : (w - 100000) / 2000;
    make_window(kind, x);
    ref_power(x, pr);
    old_power(x, po);
    new_power(x, pn);
    long double tot = 0;
    for (int k = 0; k <= 256; ++k) tot += pr[k];
    double eo = 0, en = 0;
    for (int k = 0; k <= 256; ++k) {
      eo = fmax(eo, (double)(fabsl((long double)po[k] - pr[k]) / (tot > 0 ? tot : 1)));
      en = fmax(en, (double)(fabsl((long double)pn[k] - pr[k]) / (tot > 0 ? tot : 1)));
    }
    max_old = fmax(max_old, eo); max_new = fmax(max_new, en);
    sum_old += eo; sum_new += en;
    orc_r2c512_f64(x, ore, oim);
    for (int k = 0; k <= 256; ++k) op[k] = ore[k] * ore[k] + oim[k] * oim[k];
    const float e_orc = ordered_sum(op), e_new = ordered_sum(pn), e_old = ordered_sum(po);
    if (memcmp(&e_orc, &e_new, 4)) {
      if (diff_new < 5) printf("window %d (kind %d): energy %.9g, oracle %.9g\n", w, kind, e_new, e_orc);
      ++diff_new;
    }
    diff_old += memcmp(&e_orc, &e_old, 4) != 0;
    ++windows;
  }
  const double mean_old = sum_old / windows, mean_new = sum_new / windows;
  printf("%ld windows; error per window in units of sum |X|^2: bl_fft16 max %.3e mean %.3e, tan form max %.3e mean %.3e\n",
         windows, max_old, mean_old, max_new, mean_new);
  printf("energies differing from the oracle: tan form %ld, bl_fft16 %ld\n", diff_new, diff_old);
  const bool ok = diff_new == 0 && max_new <= 1.05 * max_old && mean_new <= 1.05 * mean_old && max_new < 1e-15;
  printf(ok ? "OK\n" : "FAIL\n");
  return ok ? 0 : 1;
}
