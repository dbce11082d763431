/*
 * bl_api.c — the reference's C API (include/bliss.h) on top of the HIP path.
 *
 * Host code stays in C, as in the reference; every analysis result comes from
 * the kernels in the bl_*_kernels.hip files through the thin launch layer declared in
 * bl_device.h.  There is no CPU implementation of the analysis in this
 * library: without a usable HIP device the analysis entry points print a
 * message and return BL_UNEXPECTED (or the float conversion of it, as the
 * reference does for bl_distance_file, ref src/analyze.c:123-124).
 *
 * Three scalar helpers are plain host arithmetic, as in the reference:
 * bl_distance / bl_cosine_similarity of ONE pair (a 4-float expression; through
 * a 1 x 1 kernel launch and a blocking copy a call cost ~20-30 us, so the
 * reference's 10^8-call loop, SURVEY.md section 6, would have taken the better
 * part of an hour) and bl_rectangular_filter (a serial running sum).  Their
 * all-pairs / streaming forms — bl_amd_distance_matrix_*, the box filters inside
 * the envelope tail — stay on the GPU, and the tests hold the scalar functions
 * against those kernels bit for bit.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bl_chroma_table.h"
#include "bl_mel_table.h"
#include "bl_tpeak_table.h"
#include "bl_device.h"
#include "bliss.h"

/* ref src/helpers.c:15-23 */
void bl_initialize_song(struct bl_song *const song) {
  song->artist = NULL;
  song->title = NULL;
  song->album = NULL;
  song->tracknumber = NULL;
  song->sample_array = NULL;
  song->filename = NULL;
  song->genre = NULL;
}

/* ref src/helpers.c:3-13 */
void bl_free_song(struct bl_song *const song) {
  free(song->artist);
  free(song->title);
  free(song->album);
  free(song->tracknumber);
  free(song->sample_array);
  free(song->filename);
  free(song->genre);
  bl_initialize_song(song);
}

/* ref src/helpers.c:25-28 */
float bl_version(void) {
  printf("Using bliss analyzer version %0.1f.\n", BL_VERSION);
  return (float)BL_VERSION;
}

static int song_usable(struct bl_song const *const song) {
  return song && song->sample_array && song->nSamples >= 5120 &&
         (song->channels == 1 || song->channels == 2);
}

static int run_song(struct bl_song const *const song, int what, bl_amd_song_result *res) {
  if (!song_usable(song)) {
    fprintf(stderr, "bliss_amd: song not analysable (need >= 5120 s16 samples, 1 or 2 channels)\n");
    return BL_UNEXPECTED;
  }
  /* duration only enters the tempo score (ref src/tempo_atk_sort.c:283); a clip shorter
   * than one second (duration 0: division by zero in the reference) is rejected when the
   * envelope analysis is asked for, like in the batch entry points */
  uint64_t duration = song->duration;
  if (!(what & 4) && duration == 0) duration = 1;
  return bld_analyze_one_host((const int16_t *)song->sample_array, song->nSamples, song->channels,
                              duration, what, res);
}

/* ref include/bliss.h:200 / src/amplitude_sort.c:12-80 */
float bl_amplitude_sort(struct bl_song const *const song) {
  bl_amd_song_result r;
  if (run_song(song, 1, &r) != BL_OK) return (float)BL_UNEXPECTED;
  return r.v.amplitude;
}

/* ref include/bliss.h:217 / src/frequency_sort.c:20-140 */
float bl_frequency_sort(struct bl_song const *const song) {
  bl_amd_song_result r;
  if (run_song(song, 2, &r) != BL_OK) return (float)BL_UNEXPECTED;
  return r.v.frequency;
}

/* ref include/bliss.h:184-185 / src/tempo_atk_sort.c:42-296 */
void bl_envelope_sort(struct bl_song const *const song, struct envelope_result_s *result) {
  bl_amd_song_result r;
  if (run_song(song, 4, &r) != BL_OK) {
    result->tempo = (float)BL_UNEXPECTED;
    result->attack = (float)BL_UNEXPECTED;
    return;
  }
  result->tempo = r.v.tempo;
  result->attack = r.v.attack;
}

/* ref include/bliss.h:80-81 / src/analyze.c:33-86 */
int bl_analyze(char const *const filename, struct bl_song *current_song) {
  if (bl_audio_decode(filename, current_song) == BL_OK) {
    bl_amd_song_result r;
    if (run_song(current_song, 7, &r) != BL_OK || r.status != BL_OK) {
      fprintf(stderr, "Couldn't analyse song on the HIP device\n");
      return BL_UNEXPECTED;
    }
    current_song->force_vector = r.v;      /* ref :63-66 */
    current_song->force = r.force;         /* ref :68-72 */
    current_song->calm_or_loud = r.calm_or_loud; /* ref :73-79 */
    return current_song->calm_or_loud;
  }
  fprintf(stderr, "Couldn't decode song\n"); /* ref :83 */
  return BL_UNEXPECTED;
}

/* ref include/bliss.h:116-118 / src/analyze.c:88-103: every operand f32, sums left to
 * right, sqrt correctly rounded (this file is compiled with -ffp-contract=off, like the
 * reference's -std=c99 build: no fused multiply-add).  Same bits as k_pairwise<false>. */
float bl_distance(struct force_vector_s v_song1, struct force_vector_s v_song2) {
  const float d0 = v_song1.tempo - v_song2.tempo;
  const float d1 = v_song1.amplitude - v_song2.amplitude;
  const float d2 = v_song1.frequency - v_song2.frequency;
  const float d3 = v_song1.attack - v_song2.attack;
  float s = d0 * d0;
  s = s + d1 * d1;
  s = s + d2 * d2;
  s = s + d3 * d3;
  return sqrtf(s);
}

/* ref include/bliss.h:151-153 / src/analyze.c:127-143: f32 dot product and squared norms,
 * double sqrt, product and quotient.  Same bits as k_pairwise<true>. */
float bl_cosine_similarity(struct force_vector_s v_song1, struct force_vector_s v_song2) {
  const float a[4] = {v_song1.tempo, v_song1.amplitude, v_song1.frequency, v_song1.attack};
  const float b[4] = {v_song2.tempo, v_song2.amplitude, v_song2.frequency, v_song2.attack};
  float dot = a[0] * b[0], na = a[0] * a[0], nb = b[0] * b[0];
  for (int k = 1; k < 4; ++k) {
    dot = dot + a[k] * b[k];
    na = na + a[k] * a[k];
    nb = nb + b[k] * b[k];
  }
  return (float)((double)dot / (sqrt((double)na) * sqrt((double)nb)));
}

/* ref include/bliss.h:99-103 / src/analyze.c:105-125 */
float bl_distance_file(char const *const filename1, char const *const filename2,
                       struct bl_song *song1, struct bl_song *song2) {
  if ((bl_analyze(filename1, song1) != BL_UNEXPECTED) &&
      (bl_analyze(filename2, song2) != BL_UNEXPECTED))
    return bl_distance(song1->force_vector, song2->force_vector);
  return BL_UNEXPECTED;
}

/* ref include/bliss.h:136-140 / src/analyze.c:145-167 */
float bl_cosine_similarity_file(char const *const filename1, char const *const filename2,
                                struct bl_song *song1, struct bl_song *song2) {
  if ((bl_analyze(filename1, song1) != BL_UNEXPECTED) &&
      (bl_analyze(filename2, song2) != BL_UNEXPECTED))
    return bl_cosine_similarity(song1->force_vector, song2->force_vector);
  return BL_UNEXPECTED;
}

/* ref include/bliss.h:270 / src/helpers.c:30-37 */
int bl_mean(int16_t *sample_array, int nSamples) {
  int mean = 0;
  if (bld_mean_variance_host(sample_array, nSamples, 0, 0, &mean, NULL) != BL_OK) return BL_UNEXPECTED;
  return mean;
}

/* ref include/bliss.h:278 / src/helpers.c:39-49 */
int bl_variance(int16_t *sample_array, int nSamples, int mean) {
  int var = 0;
  if (bld_mean_variance_host(sample_array, nSamples, 1, mean, NULL, &var) != BL_OK) return BL_UNEXPECTED;
  return var;
}

/* ref include/bliss.h:289-290 / src/tempo_atk_sort.c:19-40: running sum of `smooth_width`
 * inputs written at the window centre, the last window ADDED to out[n - half], then every
 * cell divided by the width — cells the loop never writes keep their previous contents / width.
 * The hot path uses the streaming form of the same arithmetic (bl_box19 in bl_tail.h). */
void bl_rectangular_filter(double *sample_array_out, double *sample_array_in, int nSamples,
                           int smooth_width) {
  if (!sample_array_out || !sample_array_in || smooth_width <= 0 || smooth_width > nSamples) {
    fprintf(stderr, "bliss_amd: bl_rectangular_filter: need 0 < smooth_width <= nSamples\n");
    return;
  }
  const double *lag = sample_array_in, *lead = sample_array_in + smooth_width;
  const double *const end = sample_array_in + nSamples;
  double run = 0;
  for (const double *p = lag; p < lead; ++p) run += *p;
  const int half = (int)round(smooth_width / 2.);
  double *centre = sample_array_out + half - 1;
  while (lead < end) { /* slide: drop the oldest input, then take the next one */
    *centre++ = run;
    run -= *lag++;
    run += *lead++;
  }
  /* lag == &in[n - width]: the last window is added to whatever out[n - half] held.  For an odd
   * width that is the cell `centre` has reached; for an even one it is the cell after it (the
   * reference names the index, ref :32-33), so the index is named here too. */
  double *const last = sample_array_out + (nSamples - half);
  for (; lag < end; ++lag) *last += *lag;
  for (int k = 0; k < nSamples; ++k) sample_array_out[k] /= smooth_width;
}

/* ---- signal levels: the host arithmetic over bl_amd_song_levels (include/bliss_amd.h) ---- */

/* One interleaved slot of ref examples/detect-gapless.c:35-54: both samples at least 5 away from zero, and their
 * difference, as an f32 quotient by INT16_MAX whose magnitude is compared as a double, below 0.01.  In integers:
 * |tail - head| <= 327 (327 / 32767 = 0.00998, 328 / 32767 = 0.01001). */
static int gapless_slot(int16_t tail, int16_t head) {
  if (abs((int)tail) < 5 || abs((int)head) < 5) return 0;
  const float diff = fabsf(((float)tail - (float)head) / (float)INT16_MAX);
  return (double)diff < 0.01;
}

/* ref examples/detect-gapless.c:49: gapless if either slot says so */
int bl_amd_gapless_host(const bl_amd_song_levels *h_levels, int n_songs, uint8_t *h_linked) {
  if (!h_levels || n_songs < 1 || (n_songs > 1 && !h_linked)) return BL_UNEXPECTED;
  for (int i = 0; i + 1 < n_songs; ++i)
    h_linked[i] = (uint8_t)(gapless_slot(h_levels[i].tail[0], h_levels[i + 1].head[0]) ||
                            gapless_slot(h_levels[i].tail[1], h_levels[i + 1].head[1]));
  return BL_OK;
}

/* 20 log10(peak / 32768): 0 dB is full scale, silence is -inf */
double bl_amd_levels_peak_db(const bl_amd_song_levels *lv, int channel) {
  if (!lv || channel < 0 || channel > 1) return NAN;
  return 20.0 * log10((double)lv->peak[channel] / 32768.0);
}

/* 10 log10(mean square / 2^30): 0 dB is a song of nothing but -32768 */
double bl_amd_levels_rms_db(const bl_amd_song_levels *lv, int channel) {
  if (!lv || channel < 0 || channel > 1 || lv->frames < 1) return NAN;
  return 10.0 * log10((double)lv->sum_sq[channel] / ((double)lv->frames * 1073741824.0));
}

/* ---- spectral timbre: the host arithmetic over bl_amd_song_timbre (include/bliss_amd.h) ---- */

/* F = (n_samples / channels) / 512, ref src/frequency_sort.c:50 */
int bl_amd_timbre_frames(int n_samples, int channels) {
  if (n_samples < 0 || (channels != 1 && channels != 2)) return -1;
  return (n_samples / channels) / 512;
}

/* mean and population standard deviation of a quantity whose sum and sum of squares over `used` frames are given, in
 * units of `unit`.  used * sumsq - sum^2 is taken exactly (it is below 2^22 * 2^62), so the variance loses nothing to
 * cancellation before it becomes a double. */
static double timbre_mean_std(uint64_t sum, uint64_t sumsq, int used, double unit, double *std_out) {
  if (used < 1) {
    if (std_out) *std_out = NAN;
    return NAN;
  }
  if (std_out) {
    const unsigned __int128 n = (unsigned __int128)(unsigned)used * sumsq, s2 = (unsigned __int128)sum * sum;
    const double var = n > s2 ? (double)(n - s2) / ((double)used * (double)used) : 0.0;
    *std_out = sqrt(var) * unit;
  }
  return (double)sum / (double)used * unit;
}

double bl_amd_timbre_centroid_hz(const bl_amd_song_timbre *st, int rate, double *std_hz) {
  if (!st) { if (std_hz) *std_hz = NAN; return NAN; }
  return timbre_mean_std(st->centroid_sum, st->centroid_sumsq, st->used, (double)rate / 512.0 / 4096.0, std_hz);
}

double bl_amd_timbre_rolloff_hz(const bl_amd_song_timbre *st, int rate, double *std_hz) {
  if (!st) { if (std_hz) *std_hz = NAN; return NAN; }
  return timbre_mean_std(st->rolloff_sum, st->rolloff_sumsq, st->used, (double)rate / 512.0, std_hz);
}

double bl_amd_timbre_peak_hz(const bl_amd_song_timbre *st, int rate, double *std_hz) {
  if (!st) { if (std_hz) *std_hz = NAN; return NAN; }
  return timbre_mean_std(st->peak_sum, st->peak_sumsq, st->used, (double)rate / 512.0, std_hz);
}

/* ---- tempo: the host arithmetic over bl_amd_song_rhythm (include/bliss_amd.h) ---- */

/* H = (n_samples / channels) / 128 */
int bl_amd_rhythm_hops(int n_samples, int channels) {
  if (n_samples < 0 || (channels != 1 && channels != 2)) return -1;
  return (n_samples / channels) / BL_AMD_RHYTHM_HOP;
}

/* The period in hops is the lag moved by the vertex of the parabola through (lag - 1, r_prev), (lag, r_lag),
 * (lag + 1, r_next), where there is one: the three values are below 2^60 and become doubles one by one, to 2^-53
 * each. */
double bl_amd_rhythm_bpm(const bl_amd_song_rhythm *r, int rate) {
  if (!r || rate < 1 || r->lag <= 0) return NAN;
  const double p = (double)r->r_prev, c = (double)r->r_lag, n = (double)r->r_next;
  const double den = p - 2.0 * c + n;
  double delta = 0.0;
  if (den < 0.0 && c >= p && c >= n) delta = 0.5 * (p - n) / den;
  if (delta > 0.5) delta = 0.5;
  if (delta < -0.5) delta = -0.5;
  return 60.0 * (double)rate / ((double)BL_AMD_RHYTHM_HOP * ((double)r->lag + delta));
}

double bl_amd_rhythm_strength(const bl_amd_song_rhythm *r) {
  if (!r) return NAN;
  return r->r0 ? (double)r->r_lag / (double)r->r0 : 0.0;
}

/* ---- beats: the host arithmetic over the flags and bl_amd_song_beats (include/bliss_amd.h) ---- */

int bl_amd_beats_list(const uint8_t *h_flags, int hops, int rate, int32_t *h_hop_out, double *h_sec_out, int cap) {
  if (!h_flags || hops < 0 || rate < 1 || cap < 0) return -1;
  int count = 0;
  for (int h = 0; h < hops; ++h) {
    if (!h_flags[h]) continue;
    if (count < cap) {
      if (h_hop_out) h_hop_out[count] = h;
      if (h_sec_out) h_sec_out[count] = (double)BL_AMD_RHYTHM_HOP * (double)h / (double)rate;
    }
    count += 1;
  }
  return count;
}

double bl_amd_beats_bpm(const bl_amd_song_beats *b, int rate) {
  if (!b || rate < 1 || b->n_beats < 2 || b->last <= b->first) return NAN;
  return 60.0 * (double)rate * (double)(b->n_beats - 1) /
         ((double)BL_AMD_RHYTHM_HOP * (double)(b->last - b->first));
}

/* ---- tempo over time: the host arithmetic of bl_amd_tgram_* (include/bliss_amd.h) ---- */

static int tgram_params_bad(const bl_amd_tgram_params *p) {
  return !p || p->stride < 16 || p->stride > 1024 || p->stride % 16 || p->blocks < 1 || p->blocks > 16 ||
         p->lag_min < 1 || p->lag_min > p->lag_max || p->lag_max > BL_AMD_RHYTHM_LAGS - 2 || p->tol < 0 ||
         p->tol > 1000 || (p->octaves != 0 && p->octaves != 1) || p->reserved[0] || p->reserved[1];
}

/* F = (T - W) / S + 1 with T = H - 511 and W = m S, 0 when T < W */
int bl_amd_tgram_frames(int hops, const bl_amd_tgram_params *p) {
  if (tgram_params_bad(p) || hops < 1 || hops >= (1 << 24)) return -1;
  const int T = hops - (BL_AMD_RHYTHM_LAGS - 1), W = p->blocks * p->stride;
  return T >= W ? (T - W) / p->stride + 1 : 0;
}

/* bl_amd_rhythm_bpm on a frame's four values */
double bl_amd_tgram_bpm(const bl_amd_tgram_frame *f, int rate) {
  if (!f) return NAN;
  bl_amd_song_rhythm r;
  memset(&r, 0, sizeof(r));
  r.r_prev = f->r_prev;
  r.r_lag = f->r_lag;
  r.r_next = f->r_next;
  r.lag = f->lag;
  return bl_amd_rhythm_bpm(&r, rate);
}

/* the centre of the window of frame `frame`: hop frame S + W / 2 */
double bl_amd_tgram_seconds(int frame, const bl_amd_tgram_params *p, int rate) {
  if (frame < 0 || rate < 1 || tgram_params_bad(p)) return NAN;
  const double hop = (double)frame * (double)p->stride + 0.5 * (double)(p->blocks * p->stride);
  return (double)BL_AMD_RHYTHM_HOP * hop / (double)rate;
}

double bl_amd_tgram_steadiness(const bl_amd_song_tgram *t) {
  if (!t) return NAN;
  return t->n_tempo > 0 ? (double)t->n_near / (double)t->n_tempo : 0.0;
}

/* ---- beats that follow the tempo over time: the host arithmetic of bl_amd_tbeats_* (include/bliss_amd.h) ---- */

/* frame f's window is centred on hop f S + m S / 2 and a frame speaks for the S hops around its centre: frame f owns
 * [origin + f S, origin + (f + 1) S) with origin = (m - 1) S / 2 */
int bl_amd_tbeats_params_from_tgram(const bl_amd_tgram_params *tgram, int tight, int fold, bl_amd_tbeats_params *out) {
  if (!out || tgram_params_bad(tgram) || tight < 0 || tight > BL_AMD_BEATS_TIGHT_MAX || (fold != 0 && fold != 1))
    return -1;
  memset(out, 0, sizeof(*out));
  out->seg = tgram->stride;
  out->origin = (tgram->blocks - 1) * tgram->stride / 2;
  out->tight = tight;
  out->fold = fold;
  return 0;
}

double bl_amd_tbeats_edge_bpm(const uint8_t *h_flags, int hops, int rate, int n, int at_end) {
  if (!h_flags || hops < 0 || rate < 1 || n < 2) return NAN;
  int k = 0, a = -1, b = -1; /* the k <= n beats taken so far, from hop a to hop b */
  for (int i = 0; i < hops && k < n; ++i) {
    const int h = at_end ? hops - 1 - i : i;
    if (!h_flags[h]) continue;
    if (k == 0) a = h;
    b = h;
    k += 1;
  }
  if (k < 2) return NAN;
  return 60.0 * (double)rate * (double)(k - 1) / ((double)BL_AMD_RHYTHM_HOP * (double)(at_end ? a - b : b - a));
}

/* ---- loudness: the host arithmetic over bl_amd_loud_params and bl_amd_song_loud (include/bliss_amd.h) ---- */

/* The bilinear design of the two K-weighting sections.  The constants are the analogue prototype that gives
 * BS.1770-4's printed coefficients at 48 000 Hz. */
int bl_amd_loud_kweight(int rate, bl_amd_loud_params *p) {
  if (!p || rate < 8000 || rate > 48000 || rate % 10) return BL_UNEXPECTED;
  const double pi = 3.14159265358979323846;
  double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
  double K = tan(pi * f0 / (double)rate);
  const double Vh = pow(10.0, G / 20.0), Vb = pow(Vh, 0.4996667741545416);
  double a0 = 1.0 + K / Q + K * K;
  p->s1_b[0] = (Vh + Vb * K / Q + K * K) / a0;
  p->s1_b[1] = 2.0 * (K * K - Vh) / a0;
  p->s1_b[2] = (Vh - Vb * K / Q + K * K) / a0;
  p->s1_a[0] = 2.0 * (K * K - 1.0) / a0;
  p->s1_a[1] = (1.0 - K / Q + K * K) / a0;
  f0 = 38.13547087602444;
  Q = 0.5003270373238773;
  K = tan(pi * f0 / (double)rate);
  a0 = 1.0 + K / Q + K * K;
  p->s2_a[0] = 2.0 * (K * K - 1.0) / a0;
  p->s2_a[1] = (1.0 - K / Q + K * K) / a0;
  p->hop = rate / 10;
  p->warm = 4096;
  p->abs_gate = (uint64_t)floor(4.0 * (double)p->hop * 1073741824.0 * pow(10.0, -6.9309));
  return BL_OK;
}

static double loud_limbs(const uint64_t s[2]) { return (double)s[1] * 18446744073709551616.0 + (double)s[0]; }
/* -0.691 + 10 log10(sum / (count hops_per_block hop 2^30)); -inf for nothing */
static double loud_lufs_of(double sum, double count, int hops_per_block, int hop) {
  if (sum <= 0.0 || count <= 0.0) return -INFINITY;
  return -0.691 + 10.0 * log10(sum / (count * (double)hops_per_block * (double)hop * 1073741824.0));
}

double bl_amd_loud_lufs(const bl_amd_song_loud *r, int hop) {
  if (!r || hop < 1) return NAN;
  return loud_lufs_of(loud_limbs(r->gated_sum), (double)r->gated_count, 4, hop);
}

double bl_amd_loud_momentary_max_lufs(const bl_amd_song_loud *r, int hop) {
  if (!r || hop < 1) return NAN;
  return loud_lufs_of((double)r->momentary_max, 1.0, 4, hop);
}

double bl_amd_loud_short_max_lufs(const bl_amd_song_loud *r, int hop) {
  if (!r || hop < 1) return NAN;
  return loud_lufs_of((double)r->st_max, 1.0, 30, hop);
}

double bl_amd_loud_range_lu(const bl_amd_song_loud *r) {
  if (!r) return NAN;
  if (r->st_gated < 1 || !r->lra_lo) return 0.0;
  return 10.0 * log10((double)r->lra_hi / (double)r->lra_lo);
}

double bl_amd_loud_gain_db(const bl_amd_song_loud *r, int hop, double target_lufs) {
  if (!r || hop < 1) return NAN;
  return r->gated_count > 0 ? target_lufs - bl_amd_loud_lufs(r, hop) : 0.0;
}

/* ---- true peak: the table and the host arithmetic over bl_amd_song_tpeak (include/bliss_amd.h) ---- */

void bl_amd_tpeak_table(int32_t out[48]) {
  if (!out) return;
  for (int p = 0; p < BL_TPEAK_PHASES; ++p)
    for (int k = 0; k < BL_TPEAK_TAPS; ++k) out[p * BL_TPEAK_TAPS + k] = BL_TPEAK_G[p][k];
}

/* 20 log10(tpeak / 2^29): 2^29 is a full-scale sample (2^15) through a unit-gain phase (2^14) */
double bl_amd_tpeak_dbtp(const bl_amd_song_tpeak *tp, int channel) {
  if (!tp || channel < 0 || channel > 1) return NAN;
  if (!tp->tpeak[channel]) return -INFINITY;
  return 20.0 * log10((double)tp->tpeak[channel] / 536870912.0);
}

double bl_amd_tpeak_song_dbtp(const bl_amd_song_tpeak *tp) {
  if (!tp) return NAN;
  const double a = bl_amd_tpeak_dbtp(tp, 0), b = bl_amd_tpeak_dbtp(tp, 1);
  return a > b ? a : b;
}

double bl_amd_tpeak_gain_db(const bl_amd_song_loud *loud, int hop, double target_lufs, const bl_amd_song_tpeak *tp,
                            double ceiling_dbtp) {
  const double gain = bl_amd_loud_gain_db(loud, hop, target_lufs);
  if (!tp || gain != gain) return NAN;
  if (!tp->tpeak[0] && !tp->tpeak[1]) return gain; /* digital silence has no peak to hold the gain back */
  const double room = ceiling_dbtp - bl_amd_tpeak_song_dbtp(tp);
  return gain < room ? gain : room;
}

/* ---- fingerprints: the host arithmetic over bl_amd_fprint_match (include/bliss_amd.h) ---- */

int bl_amd_fprint_words(int frames) {
  if (frames < 0) return -1;
  return frames >= BL_AMD_FPRINT_FRAMES ? frames - (BL_AMD_FPRINT_FRAMES - 1) : 0;
}

double bl_amd_fprint_ber(const bl_amd_fprint_match *m) {
  if (!m || m->status != BL_OK || !m->overlap) return NAN;
  return (double)m->errors / (32.0 * (double)m->overlap);
}

double bl_amd_fprint_offset_seconds(const bl_amd_fprint_match *m, int rate) {
  if (!m || m->status != BL_OK || rate < 1) return NAN;
  return (double)m->offset * (double)BL_AMD_CHROMA_HOP / (double)rate;
}

/* ---- song structure: the host arithmetic over bl_amd_song_form (include/bliss_amd.h) ---- */

int bl_amd_form_units(int frames, int pool) {
  if (frames < 0 || pool < 1 || pool > 16) return -1;
  return frames / pool;
}

double bl_amd_form_seconds(int unit, int pool, int rate) {
  if (unit < 0 || pool < 1 || pool > 16 || rate < 1) return NAN;
  return (double)unit * (double)pool * (double)BL_AMD_CHROMA_HOP / (double)rate;
}

double bl_amd_form_score(const bl_amd_song_form *f) {
  if (!f || (f->status & BL_AMD_FORM_NO_THUMB) || !f->thumb_self) return NAN;
  return (double)f->thumb_score / (double)f->thumb_self;
}

/* ---- versions: the host arithmetic over bl_amd_cover_match (include/bliss_amd.h) ---- */

double bl_amd_cover_score(const bl_amd_cover_match *m, int thr) {
  if (!m || m->status != 0) return NAN;
  const double den = (16129.0 - (double)thr) * (double)(m->units_a < m->units_b ? m->units_a : m->units_b);
  if (!(den > 0.0)) return NAN;
  return (double)m->score / den;
}

double bl_amd_cover_seconds(int unit, int pool, int rate) { return bl_amd_form_seconds(unit, pool, rate); }

double bl_amd_cover_tempo_ratio(const bl_amd_cover_match *m) {
  if (!m || m->status != 0 || m->a_end < m->a_start || m->b_end < m->b_start) return NAN;
  return (double)(m->b_end - m->b_start + 1) / (double)(m->a_end - m->a_start + 1);
}

/* ---- chords: the host arithmetic of bl_amd_chords_* (include/bliss_amd.h) ---- */

/* the pitch classes of a triad label (0 .. 23) as a 12-bit set */
static unsigned chords_classes(int label) {
  const int r = label % 12;
  return (1u << r) | (1u << ((r + (label < 12 ? 4 : 3)) % 12)) | (1u << ((r + 7) % 12));
}

int bl_amd_chords_costs(int change, int related, uint16_t *cost_out) {
  if (!cost_out || related < 0 || 2 * (long long)related > change || change > BL_AMD_CHORDS_COST_MAX) return BL_UNEXPECTED;
  for (int a = 0; a < BL_AMD_CHORDS_LABELS; ++a)
    for (int b = 0; b < BL_AMD_CHORDS_LABELS; ++b) {
      int v = change;
      if (a == b) {
        v = 0;
      } else if (a != BL_AMD_CHORDS_NONE && b != BL_AMD_CHORDS_NONE) {
        const unsigned both = chords_classes(a) & chords_classes(b);
        for (int k = 0; k < 12; ++k) v -= ((both >> k) & 1u) ? related : 0;
      }
      cost_out[a * BL_AMD_CHORDS_LABELS + b] = (uint16_t)v;
    }
  return BL_OK;
}

const char *bl_amd_chords_name(int label) {
  static const char *const names[BL_AMD_CHORDS_LABELS] = {
      "C",  "C#",  "D",  "D#",  "E",  "F",  "F#",  "G",  "G#",  "A",  "A#",  "B", "Cm",
      "C#m", "Dm", "D#m", "Em", "Fm", "F#m", "Gm", "G#m", "Am", "A#m", "Bm", "N"};
  return label >= 0 && label < BL_AMD_CHORDS_LABELS ? names[label] : "";
}

int bl_amd_chords_segments(const uint8_t *labels, int units, int32_t *starts_out, uint8_t *chords_out, int cap) {
  if (units < 0 || cap < 0 || (!labels && units > 0)) return -1;
  int runs = 0;
  for (int t = 0; t < units; ++t) {
    if (t > 0 && labels[t] == labels[t - 1]) continue;
    if (runs < cap) {
      if (starts_out) starts_out[runs] = t;
      if (chords_out) chords_out[runs] = labels[t];
    }
    ++runs;
  }
  return runs;
}

/* ---- harmonic mixes: the host arithmetic of bl_amd_hmix_* (include/bliss_amd.h) ---- */

static int hmix_rule_args_ok(int tempo_tol, int flags) {
  const int all = BL_AMD_HMIX_KEY | BL_AMD_HMIX_TEMPO | BL_AMD_HMIX_HALF_DOUBLE;
  return tempo_tol >= 0 && tempo_tol <= 1000 && !(flags & ~all) &&
         (!(flags & BL_AMD_HMIX_HALF_DOUBLE) || (flags & BL_AMD_HMIX_TEMPO));
}

/* the wheel: the same key, a fifth up, a fifth down, and the relative key of the other mode */
int bl_amd_hmix_rule_camelot(bl_amd_hmix_rule *out, int tempo_tol, int flags) {
  if (!out || !hmix_rule_args_ok(tempo_tol, flags)) return BL_UNEXPECTED;
  for (int k = 0; k < 12; ++k) {
    const int up = (k + 7) % 12, down = (k + 5) % 12;
    out->key_ok[k] = (1u << k) | (1u << up) | (1u << down) | (1u << (12 + (k + 9) % 12));
    out->key_ok[12 + k] = (1u << (12 + k)) | (1u << (12 + up)) | (1u << (12 + down)) | (1u << ((k + 3) % 12));
  }
  out->tempo_tol = (uint32_t)tempo_tol;
  out->flags = (uint32_t)flags;
  return BL_OK;
}

int bl_amd_hmix_attrs(const bl_amd_song_rhythm *rhythm, const bl_amd_song_chroma *chroma, int n, int rate,
                      bl_amd_hmix_attr *out) {
  if (!out || n < 1) return BL_UNEXPECTED;
  for (int i = 0; i < n; ++i) {
    const double bpm = rhythm ? bl_amd_rhythm_bpm(&rhythm[i], rate) : NAN;
    long long t = 0;
    if (!isnan(bpm)) {
      const double x = 100.0 * bpm;
      t = x >= 65535.0 ? 65535 : llrint(x);
      if (t < 1) t = 1;
    }
    const int key = chroma ? chroma[i].key : -1;
    out[i].tempo = (uint16_t)t;
    out[i].key = key >= 0 && key <= 23 ? (uint8_t)key : 255;
    out[i].reserved = 0;
  }
  return BL_OK;
}

/* ---- chroma and key: the host side of bl_amd_song_chroma (include/bliss_amd.h) ---- */

/* T = 0 below one frame, else (Fr - 4096) / 2048 + 1 */
int bl_amd_chroma_frames(int n_samples, int channels) {
  if (n_samples < 0 || (channels != 1 && channels != 2)) return -1;
  const int fr = n_samples / channels;
  return fr < BL_AMD_CHROMA_FRAME ? 0 : (fr - BL_AMD_CHROMA_FRAME) / BL_AMD_CHROMA_HOP + 1;
}

int bl_amd_chroma_table(int8_t *re, int8_t *im, uint32_t *gain, int32_t *len) {
  bl_chroma_build(re, im, gain, len);
  return BL_OK;
}

int bl_amd_chroma_key_name(int key, char out[8]) {
  static const char *const kTonic[12] = {"C", "C#", "D", "D#", "E", "F", "F#", "G", "G#", "A", "A#", "B"};
  if (!out) return BL_UNEXPECTED;
  out[0] = 0;
  if (key < 0 || key > 23) return BL_UNEXPECTED;
  strcpy(out, kTonic[key % 12]);
  if (key >= 12) strcat(out, "m");
  return BL_OK;
}

/* ---- mel bands, cepstrum and flatness: the host side of bl_amd_song_mel (include/bliss_amd.h) ---- */

int bl_amd_mel_frames(int n_samples, int channels) { return bl_amd_timbre_frames(n_samples, channels); }

int bl_amd_mel_table(int32_t *edges, uint8_t *weights, int32_t *dct) {
  return bl_mel_build(edges, weights, dct) == 0 ? BL_OK : BL_UNEXPECTED;
}

/* mean and population standard deviation of a signed quantity from its sum and sum of squares over `used` frames, in
 * units of `unit` (timbre_mean_std with a sign): used * sumsq - sum^2 is taken exactly before it becomes a double */
static double mel_mean_std(int64_t sum, uint64_t sumsq, int used, double unit, double *std_out) {
  if (used < 1) {
    if (std_out) *std_out = NAN;
    return NAN;
  }
  if (std_out) {
    const unsigned __int128 a = (unsigned __int128)(sum < 0 ? -(unsigned __int128)sum : (unsigned __int128)sum);
    const unsigned __int128 n = (unsigned __int128)(unsigned)used * sumsq, s2 = a * a;
    const double var = n > s2 ? (double)(n - s2) / ((double)used * (double)used) : 0.0;
    *std_out = sqrt(var) * fabs(unit);
  }
  return (double)sum / (double)used * unit;
}

double bl_amd_mel_mfcc(const bl_amd_song_mel *song, int k, double *std) {
  if (!song || k < 0 || k >= BL_AMD_MEL_COEFFS) { if (std) *std = NAN; return NAN; }
  return mel_mean_std(song->mfcc_sum[k], song->mfcc_sumsq[k], song->used, 1.0 / 4096.0, std);
}

double bl_amd_mel_flatness_db(const bl_amd_song_mel *song, double *std) {
  if (!song) { if (std) *std = NAN; return NAN; }
  /* 10 log10 2 per unit of log2, and flat is 32 * 4096 times the log2 ratio */
  return mel_mean_std(song->flat_sum, song->flat_sumsq, song->used, -3.010299956639812 / (32.0 * 4096.0), std);
}
