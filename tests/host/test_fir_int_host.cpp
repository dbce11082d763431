// Host-side test of bliss_amd/csrc/bl_fir_int.h, FIR mode 2 of k_env_windows3 as an exact integer convolution.  The
// int8 matrix form is run as the kernel runs it — per 16 x 16 tile the sample planes and the tap planes of every lane
// from the header's own functions, the five products as byte dot products over the four K-groups, the constant in
// the initial values, the combine — and held to
//   (a) Y equal to the int64 convolution sum_m C_m (s[j - m] - mean), bit for bit, on 10^5 random blocks, blocks of
//       -32768, of 32767, of alternating full scale (periods 1, 2, 17) and of silence, each with
//       mean in {-32768, -1, 0, 1, 32767} (the random blocks take the five in turn);
//   (b) every accumulator a0..a4 and both partial sums of the combine inside int32 (computed in int64 here);
//   (c) the f64 form (BL_FIR_INT: the block in front of a run; BL_FIR_INT_P with the taps that exist: the zero-state
//       heads) giving the identical double y = Y * sc;
//   (d) with bl_fft_tan.h's lane code behind it, as the kernel calls it (halved input, no quarter in the split,
//       4 x the middle term): the window energies of the songs tests/test_gpu_fir_int.py analyses against the
//       oracle's — none more than one f32 ulp apart; the count of moved energies is printed and must stay within the
//       two that GPU test allows (its seeds were chosen so that it is 0);
//   (e) the route the shipped kernel takes since it transforms the sums unscaled: the integers Y themselves through the
//       same lane code and bl_fft512_power1_sq with the song's kappa, 2 kappa for the middle term (as in the kernel and
//       in test_fft_sq_host.cpp), on the same songs; its count is printed beside (d)'s.
// With arguments — pairs of a channel count and a file of raw s16 PCM (native byte order, 44.1 kHz) — the program runs
// (d) and (e) on those files instead and prints, per file, how many energies differ from the oracle's and the largest
// step in f32 ulps; the caller (tests/test_fir_int_host.py) holds the numbers to the project's allowance.
// Build: g++ -O2 -std=c++17 -ffp-contract=off, linked with the oracle's C sources.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../bliss_amd/csrc/bl_fft_tan.h"
#include "../../bliss_amd/csrc/bl_fir_int.h"
#include "../../oracle/bliss_oracle.h"

static unsigned long long g_rng = 0x9E3779B97F4A7C15ull;
static unsigned long long xrand() {
  g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
  return g_rng;
}

static long g_fail = 0;
static long long g_amax[7];
#define CHECK(c, ...) do { if (!(c)) { if (g_fail++ < 10) { printf(__VA_ARGS__); printf("\n"); } } } while (0)

/* the planes' words as the signed bytes the matrix instruction reads */
static void bytes8(const unsigned w[2], signed char *o) {
  for (int q = 0; q < 2; ++q)
    for (int e = 0; e < 4; ++e) o[4 * q + e] = (signed char)(w[q] >> (8 * e));
}
static int dot8(const signed char *a, const signed char *b) {
  int s = 0;
  for (int i = 0; i < 8; ++i) s += (int)a[i] * (int)b[i];
  return s;
}

static unsigned g_cp[16][4][4][2]; /* [row b][K-group][digit plane][word] */
static signed char g_c8[16][4][4][8];

/* one tile: s[0..15] are the 16 samples in front of the block, s[16..271] the block.  Y[j], j = 0..255 */
static void tile_int8(const int16_t *s, int mean, double *Y) {
  signed char L8[16][4][8], H8[16][4][8]; /* [column a][K-group][byte] */
  for (int a = 0; a < 16; ++a)
    for (int kb = 0; kb < 4; ++kb) {
      const int16_t *src = s + 16 + 16 * (a - 1) + bl_firi_kappa(kb, 0, 0);
      unsigned w[4], lp[2], hp[2];
      for (int i = 0; i < 4; ++i) w[i] = (unsigned)(uint16_t)src[2 * i] | ((unsigned)(uint16_t)src[2 * i + 1] << 16);
      bl_firi_sample_planes(w, lp, hp);
      bytes8(lp, L8[a][kb]);
      bytes8(hp, H8[a][kb]);
    }
  int k0, k2, k4;
  bl_firi_const(mean, &k0, &k2, &k4);
  for (int a = 0; a < 16; ++a)
    for (int b = 0; b < 16; ++b) {
      long long acc[5] = {k0, 0, k2, 0, k4};
      for (int kb = 0; kb < 4; ++kb) {
        const signed char(*c)[8] = g_c8[b][kb];
        const signed char *L = L8[a][kb], *H = H8[a][kb];
        acc[0] += dot8(c[0], L);                 /* K = 32: [c0] x [l'] */
        acc[1] += dot8(c[1], L) + dot8(c[0], H); /* K = 64: [c1 | c0] x [l' | h] */
        acc[2] += dot8(c[2], L) + dot8(c[1], H);
        acc[3] += dot8(c[3], L) + dot8(c[2], H);
        acc[4] += dot8(c[3], H);                 /* K = 32: [c3] x [h] */
      }
      const long long lo = acc[0] + acc[1] * 256, mid = acc[2] + acc[3] * 256 + acc[4] * 65536;
      const long long all[7] = {acc[0], acc[1], acc[2], acc[3], acc[4], lo, mid};
      for (int i = 0; i < 7; ++i) {
        const long long m = all[i] < 0 ? -all[i] : all[i];
        if (m > g_amax[i]) g_amax[i] = m;
        CHECK(all[i] >= INT32_MIN && all[i] <= INT32_MAX, "(b) sum %d leaves int32: %lld", i, all[i]);
      }
      Y[16 * a + b] = bl_firi_combine((int)acc[0], (int)acc[1], (int)acc[2], (int)acc[3], (int)acc[4]);
    }
}

static long long conv64(const int16_t *s, int j, int mean, int first) { /* taps whose sample index is >= first */
  long long y = 0;
  for (int m = 0; m <= 16; ++m)
    if (j - m >= first) y += (long long)bl_firi_tap(m) * ((int)s[j - m] - mean);
  return y;
}

static long g_blocks = 0;
static void check_block(const int16_t *s, int mean) {
  ++g_blocks;
  double Y[256];
  tile_int8(s, mean, Y);
  const double sc = 1.0 / (1e7 * (0.01 + (double)(xrand() >> 11) * 0x1p-53 * 40000.0)); /* any scale will do */
  for (int j = 0; j < 256; ++j) {
    const long long ref = conv64(s, 16 + j, mean, 0);
    CHECK(Y[j] == (double)ref && (long long)Y[j] == ref, "(a) block %ld output %d: %.17g, int64 %lld", g_blocks, j, Y[j], ref);
    /* (c) the block in front of a run: all 17 samples, as doubles */
#define XK(m) ((double)((int)s[16 + j - (m)] - mean))
    const double yf = BL_FIR_INT(XK) * sc;
#undef XK
    const double yi = Y[j] * sc;
    CHECK(memcmp(&yf, &yi, 8) == 0, "(c) block %ld output %d: f64 form %.17g, matrix form %.17g", g_blocks, j, yf, yi);
  }
  /* (c) zero-state heads of a window that starts at s[16]: the taps that exist, pair sums as the kernel gathers them */
  for (int l = 0; l < 16; ++l) {
    auto K = [&](int m) -> int { return l - m >= 0 ? (int)s[16 + l - m] - mean : 0; };
    const double hp[9] = {(double)K(0) /* tap 16 lies before the window */, (double)(K(1) + K(15)), (double)(K(2) + K(14)),
                          (double)(K(3) + K(13)), (double)(K(4) + K(12)), (double)(K(5) + K(11)), (double)(K(6) + K(10)),
                          (double)(K(7) + K(9)), (double)K(8)};
#define XP(m) hp[m]
    const double Yh = BL_FIR_INT_P(XP);
#undef XP
    const long long ref = conv64(s, 16 + l, mean, 16);
    CHECK(Yh == (double)ref, "(c) head %d of block %ld: %.17g, int64 %lld", l, g_blocks, Yh, ref);
  }
}

/* ---- (d): whole songs through FIR mode 2 and the tan-form DFT ---- */
static bl_fft_tan_lane<double> g_lanes[16];
static bl_c2<double> g_tw512t[128], g_cs512[128];
static void kernel_power(const double *x, double *pw) { /* x: the halved filter output, as the kernel holds it */
  double re[16][16], im[16][16];
  for (int n0 = 0; n0 < 16; ++n0)
    for (int m1 = 0; m1 < 16; ++m1) { re[n0][m1] = x[2 * (16 * m1 + n0)]; im[n0][m1] = x[2 * (16 * m1 + n0) + 1]; }
  for (int l = 0; l < 16; ++l) bl_fft512_pass1_tan<double>(re[l], im[l], g_lanes[l].t1);
  double tr[16][16], ti[16][16];
  for (int k1 = 0; k1 < 16; ++k1)
    for (int n0 = 0; n0 < 16; ++n0) { tr[k1][n0] = re[n0][bl_pos16(k1)]; ti[k1][n0] = im[n0][bl_pos16(k1)]; }
  for (int l = 0; l < 16; ++l) bl_fft16_folded<double>(tr[l], ti[l], g_lanes[l].fold);
  for (int l = 0; l < 16; ++l)
    for (int k0 = 0; k0 < 8; ++k0) {
      const int pl = l ? 16 - l : 0, pk = l ? 15 - k0 : (k0 ? 16 - k0 : 0);
      bl_fft512_power1_tan<double, false>(tr[l][bl_pos16(k0)], ti[l][bl_pos16(k0)], tr[pl][bl_pos16(pk)],
                                          ti[pl][bl_pos16(pk)], g_tw512t[l + 16 * k0], pw[l + 16 * k0], pw[256 - l - 16 * k0]);
    }
  const double mr = tr[0][bl_pos16(8)], mi = ti[0][bl_pos16(8)];
  pw[128] = 4.0 * bl_fma(mr, mr, mi * mi);
}

/* (e) Y: the unscaled integer sums; the split from the squares with the song's constants, 2 kappa x the middle term */
static void shipped_power(const double *Y, double kappa, double *pw) {
  double re[16][16], im[16][16];
  for (int n0 = 0; n0 < 16; ++n0)
    for (int m1 = 0; m1 < 16; ++m1) { re[n0][m1] = Y[2 * (16 * m1 + n0)]; im[n0][m1] = Y[2 * (16 * m1 + n0) + 1]; }
  for (int l = 0; l < 16; ++l) bl_fft512_pass1_tan<double>(re[l], im[l], g_lanes[l].t1);
  double tr[16][16], ti[16][16];
  for (int k1 = 0; k1 < 16; ++k1)
    for (int n0 = 0; n0 < 16; ++n0) { tr[k1][n0] = re[n0][bl_pos16(k1)]; ti[k1][n0] = im[n0][bl_pos16(k1)]; }
  for (int l = 0; l < 16; ++l) bl_fft16_folded<double>(tr[l], ti[l], g_lanes[l].fold);
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

static long g_windows = 0, g_moved = 0, g_far = 0, g_moved_sq = 0, g_far_sq = 0, g_step = 0, g_step_sq = 0;
static void check_song(const std::vector<int16_t> &pcm, const char *name, int channels = 1) {
  const int n = (int)pcm.size();
  orc_result r;
  memset(&r, 0, sizeof r);
  const int nb_frames = (n - (n % 512)) * 2 / 512, n_windows = nb_frames - 2;
  std::vector<float> en(nb_frames);
  const int secs = n / (44100 * channels);
  orc_envelope(pcm.data(), n, secs > 0 ? secs : 1, &r, en.data());
  const int mean = orc_mean(pcm.data(), n), var = orc_variance(pcm.data(), n, mean);
  /* k_song_prep */
  const double v2 = 2.0 * ((double)var / 32768.0), rcp = 1.0 / v2, rcp_lo = bl_fma(-rcp, v2, 1.0) / v2;
  const double sc = bl_firi_scale(rcp, rcp_lo), kappa = bl_firi_power_scale(rcp, rcp_lo);
  long moved = 0, moved_sq = 0, step = 0, step_sq = 0;
  for (int w = 0; w < n_windows; ++w) {
    double Y[512], x[512], pw[257];
    for (int j = 0; j < 512; ++j) {
      Y[j] = (double)conv64(pcm.data(), 256 * w + j, mean, 256 * w);
      x[j] = Y[j] * sc;
    }
    {
      shipped_power(Y, kappa, pw);
      float e = 0;
      for (int k = 0; k <= 256; ++k) e = (float)((double)e + pw[k]);
      int32_t a, b;
      memcpy(&a, &e, 4); memcpy(&b, &en[w], 4);
      const long d = labs((long)a - (long)b);
      moved_sq += d != 0;
      if (d > step_sq) step_sq = d;
      if (d > 1) { if (g_far_sq++ < 5) printf("(e) %s window %d: %.9g, oracle %.9g\n", name, w, e, en[w]); }
    }
    kernel_power(x, pw);
    float e = 0;
    for (int k = 0; k <= 256; ++k) e = (float)((double)e + pw[k]);
    int32_t a, b;
    memcpy(&a, &e, 4); memcpy(&b, &en[w], 4);
    const long d = labs((long)a - (long)b);
    moved += d != 0;
    if (d > step) step = d;
    if (d > 1) { if (g_far++ < 5) printf("(d) %s window %d: %.9g, oracle %.9g\n", name, w, e, en[w]); }
  }
  printf("(d) %-12s %6d samples, %5d windows, mean %6d: %ld energies moved\n", name, n, n_windows, mean, moved);
  printf("(e) %-12s %d channel(s), %5d windows: shipped route %ld differ, largest step %ld ulp; scaled route %ld differ, "
         "largest step %ld ulp\n", name, channels, n_windows, moved_sq, step_sq, moved, step);
  g_windows += n_windows;
  g_moved += moved;
  g_moved_sq += moved_sq;
  if (step > g_step) g_step = step;
  if (step_sq > g_step_sq) g_step_sq = step_sq;
}

/* (d), (e) on files of raw s16 PCM: argv = pairs of channel count and path */
static int run_files(int argc, char **argv) {
  if (argc < 3 || (argc - 1) % 2) { fprintf(stderr, "usage: %s [CHANNELS FILE]...\n", argv[0]); return 2; }
  for (int i = 1; i + 1 < argc; i += 2) {
    const int ch = atoi(argv[i]);
    FILE *f = fopen(argv[i + 1], "rb");
    if ((ch != 1 && ch != 2) || !f) { fprintf(stderr, "cannot read %s as %s-channel PCM\n", argv[i + 1], argv[i]); return 2; }
    std::vector<int16_t> pcm;
    int16_t buf[4096];
    size_t got;
    while ((got = fread(buf, 2, 4096, f)) > 0) pcm.insert(pcm.end(), buf, buf + got);
    fclose(f);
    if (pcm.size() < 5120) { fprintf(stderr, "%s: fewer than 5120 samples\n", argv[i + 1]); return 2; }
    const char *base = strrchr(argv[i + 1], '/');
    check_song(pcm, base ? base + 1 : argv[i + 1], ch);
  }
  printf("files: %ld windows; shipped route %ld differ, largest step %ld ulp; scaled route %ld differ, largest step %ld ulp\n",
         g_windows, g_moved_sq, g_step_sq, g_moved, g_step);
  return 0;
}

int main(int argc, char **argv) {
  bl_fft_tan_fill(g_lanes, g_tw512t);
  bl_fft_sq_fill(g_cs512);
  if (argc > 1) return run_files(argc, argv);
  for (int b = 0; b < 16; ++b)
    for (int kb = 0; kb < 4; ++kb) {
      bl_firi_tap_planes(b, kb, g_cp[b][kb]);
      for (int j = 0; j < 4; ++j) bytes8(g_cp[b][kb][j], g_c8[b][kb][j]);
    }
  /* the digits give the taps back, four are enough, and the sum is the one the constant uses */
  long long tapsum = 0;
  for (int m = 0; m <= 16; ++m) {
    const int c = bl_firi_tap(m);
    tapsum += c;
    CHECK(c == bl_firi_digit(c, 0) + 256 * bl_firi_digit(c, 1) + 65536 * bl_firi_digit(c, 2) + 16777216 * bl_firi_digit(c, 3),
          "tap %d is not its four digits", m);
    CHECK((m == 8) == (bl_firi_digit(c, 3) != 0), "tap %d: fourth digit", m);
  }
  CHECK(tapsum == BL_FIRI_TAPSUM, "tap sum %lld", tapsum);
  CHECK(bl_firi_tap(-1) == 0 && bl_firi_tap(17) == 0, "taps outside 0..16");

  static const int means[5] = {-32768, -1, 0, 1, 32767};
  int16_t s[272];
  for (int i = 0; i < 100000; ++i) {
    const int kind = i % 4;
    for (int j = 0; j < 272; j += 4) {
      const unsigned long long v = xrand();
      for (int q = 0; q < 4; ++q) {
        const int16_t x = (int16_t)(v >> (16 * q));
        s[j + q] = kind == 0 ? x : kind == 1 ? (int16_t)(x >> 9) : kind == 2 ? (int16_t)((x & 1) ? 32767 : -32768)
                                                                               : (int16_t)((x >> 15) ? -32768 + (x & 3) : 32767 - (x & 3));
      }
    }
    check_block(s, means[i % 5]);
  }
  for (int mi = 0; mi < 5; ++mi) {
    for (int j = 0; j < 272; ++j) s[j] = -32768;
    check_block(s, means[mi]);
    for (int j = 0; j < 272; ++j) s[j] = 32767;
    check_block(s, means[mi]);
    for (int j = 0; j < 272; ++j) s[j] = 0;
    check_block(s, means[mi]);
    static const int periods[3] = {1, 2, 17};
    for (int p = 0; p < 3; ++p)
      for (int ph = 0; ph < 2; ++ph) {
        for (int j = 0; j < 272; ++j) s[j] = (((j / periods[p]) + ph) & 1) ? 32767 : -32768;
        check_block(s, means[mi]);
      }
  }
  printf("%ld blocks; largest |a0..a4|, |lo|, |mid|: %lld %lld %lld %lld %lld %lld %lld (int32: 2147483647)\n", g_blocks,
         g_amax[0], g_amax[1], g_amax[2], g_amax[3], g_amax[4], g_amax[5], g_amax[6]);

  /* (d) the songs of tests/test_gpu_fir_int.py: (seed, channels, samples), 44.1 kHz; then its two built songs */
  static const struct { unsigned seed, ch, n; const char *name; } songs[] = {
      {81001, 2, 176400, "stereo 2 s"}, {81002, 1, 132812, "mono 3 s"}, {81003, 2, 529200, "stereo 6 s"},
      {81004, 1, 5120, "shortest"},     {81005, 2, 265134, "stereo 3 s"}};
  for (const auto &sg : songs) {
    std::vector<int16_t> pcm(sg.n);
    orc_synth_fill(pcm.data(), sg.n, sg.seed, 44100, sg.ch);
    check_song(pcm, sg.name, (int)sg.ch);
  }
  {
    std::vector<int16_t> pcm(88533); /* DC offset: |mean| > 13 571 */
    orc_synth_fill(pcm.data(), (uint32_t)pcm.size(), 81006, 44100, 1);
    for (auto &v : pcm) v = (int16_t)(((int)v >> 1) + 15000); /* numpy's // 2 is the arithmetic shift */
    check_song(pcm, "DC offset");
  }
  {
    std::vector<int16_t> pcm(176400); /* full-scale square wave, a quiet sample now and then */
    for (size_t t = 0; t < pcm.size(); ++t) pcm[t] = (t % 1001 == 0) ? 0 : ((t / 37) % 2 == 0 ? 32767 : -32768);
    check_song(pcm, "square");
  }
  printf("(d) %ld windows, %ld energies moved against the oracle, %ld by more than one ulp\n", g_windows, g_moved, g_far);
  printf("(e) %ld windows, shipped route: %ld energies moved against the oracle, %ld by more than one ulp\n", g_windows,
         g_moved_sq, g_far_sq);
  const bool ok = g_fail == 0 && g_far == 0 && g_moved <= 2;
  printf(ok ? "OK\n" : "FAIL\n");
  return ok ? 0 : 1;
}
