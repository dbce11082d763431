/*
 * bl_launch.h — internal seam between the kernel translation units (device code + launch
 * geometry: bl_kernels.hip the launch order of the per-song analysis, whose stages are
 * bl_stats_kernels.hip, bl_freq_kernels.hip and bl_env_kernels.hip; bl_level_kernels.hip the signal
 * levels, bl_timbre_kernels.hip the per-frame spectral timbre, bl_rhythm_kernels.hip the tempo,
 * bl_beat_kernels.hip the beat grid,
 * bl_chroma_kernels.hip chroma and key, bl_mel_kernels.hip mel bands, cepstrum and flatness,
 * bl_matrix_kernels.hip the pairwise matrix,
 * bl_query_kernels.hip the vector queries, bl_desc_kernels.hip the descriptors and their kNN,
 * bl_desc_chain_kernels.hip the playlist chains over descriptors,
 * bl_rs_kernels.hip the rate converter)
 * and the runtime (bl_runtime.hip: contexts, workspaces, streams, the analysis C-ABI of
 * include/bliss_amd.h; bl_query_api.hip: its matrix, playlist and vector-query C-ABI; bl_desc_api.hip: its descriptor C-ABI; bl_multi.hip: the multi-device
 * corpus path).  Also BL_HIP_CHECK, which
 * every .hip file uses.  C++ only, not installed.
 */
#ifndef BL_LAUNCH_H_
#define BL_LAUNCH_H_

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "bl_device.h"
#include "bl_fft.h"

/* a failed HIP call: one line on stderr, the enclosing function returns BL_UNEXPECTED */
#define BL_HIP_CHECK(expr)                                                              \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess) {                                                             \
      fprintf(stderr, "bliss_amd: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_), \
              __FILE__, __LINE__);                                                      \
      return BL_UNEXPECTED;                                                             \
    }                                                                                   \
  } while (0)

/* ---- device-side records ------------------------------------------------- */

struct bl_dsong {
  unsigned long long pcm_off;  /* int16 elements from the arena base */
  unsigned long long duration; /* seconds */
  long long env_off;           /* first slot of this song in the per-window arrays */
  int n, channels;
  int n_frames;  /* (n / channels) / 512              ref frequency_sort.c:50 */
  int nb_frames; /* 2 * floor(n / 512)                ref tempo_atk_sort.c:63-64 */
  int n_windows; /* nb_frames - 2 windows of hop 256  ref tempo_atk_sort.c:66-67,120 */
  int reserved0;
  int out_idx;   /* result slot = position in the caller's order (records are length-sorted) */
  int reserved1;
};

struct bl_dstats {
  unsigned long long sum;   /* two's-complement sum of all samples */
  unsigned long long sumsq; /* sum of squares */
  unsigned first;           /* first index with a non-zero sample */
  int last;                 /* last index with a non-zero sample */
  int mean, variance;
  double vprime; /* variance * 2^-15 */
  double rcp;    /* RN(1 / (2 vprime)) */
  double rcp_lo; /* 1 / (2 vprime) - rcp, see bl_norm */
  int wrap_pass; /* 1: variance must come from k_variance_wrap */
  int status;
  long long wrap_acc; /* accumulator of k_variance_wrap */
  double fsc;         /* 1e-7 / (2 vprime): the scale of FIR mode 2's integer sums (bl_firi_scale) */
  double kappa;       /* 2 (1e-7 / (2 vprime))^2: what FIR mode 2 multiplies the power terms by (bl_firi_power_scale) */
};

typedef bl_c2<double> c2d;
typedef bl_c2<float> c2f;

struct bl_tables {
  const c2d *tw256_d, *tw512_d;
  const float *hann;
  const c2f *lv_tw;   /* bl_fft_lavc.h: [LV_TW_SLOTS][16 lanes] (cos, "sin") pairs of libavcodec's tables */
  float lv_leafc[4];  /* sqrthalf, cos_16[1], cos_16[3] */
  const double *tan_lane; /* bl_fft_tan.h: [16][BL_FFT_TAN_LANE_DOUBLES] per-lane constants of k_env_windows3's DFT */
  const c2d *tw512t;      /* bl_fft_tan.h: (t, c) of W512^k, k = 0..127 */
  const c2d *cs512;       /* bl_fft_tan.h: (cos, sin) of W512^k, k = 0..127 (FIR mode 2 scales them per song) */
  double log101;
};

/* ---- per-kernel timing (bench.py's roofline leg) ---------------------------- */

enum { PK_SCAN, PK_AMP, PK_FREQ, PK_FREQ_FIN, PK_ENV, PK_TAIL, PK_DIST, PK_FREQ_SCAN, PK_RHYTHM_HOPS, PK_RHYTHM_ACF,
       PK_RHYTHM_PICK, PK_CHROMA_PITCH, PK_CHROMA_KEY, PK_DESC_RANGE, PK_DESC_QUANTIZE, PK_DESC_KNN, PK_DESC_MERGE,
       PK_BEATS, PK_COUNT };

/* called by the launchers around a kernel when profiling is on: begin = 1 before the
 * launch, 0 after it, on the stream the kernel is launched on */
typedef void (*blk_mark_fn)(void *user, int kernel_id, hipStream_t stream, int begin);

/* what a launcher puts around a launch: begin at construction, end when the scope closes */
struct Mark {
  blk_mark_fn fn;
  void *user;
  int k;
  hipStream_t s;
  Mark(blk_mark_fn f, void *u, int kk, hipStream_t ss) : fn(f), user(u), k(kk), s(ss) {
    if (fn) fn(user, k, s, 1);
  }
  ~Mark() {
    if (fn) fn(user, k, s, 0);
  }
};

/* grid.x of a (grid.x, songs) launch */
inline int grid_x_for(long long units_max, int n_songs, int blocks_per_cu, int n_cu) {
  /* enough blocks to fill the chip several times over, never more than the
   * longest song has work for */
  long long want = ((long long)n_cu * blocks_per_cu + n_songs - 1) / n_songs;
  if (want < 1) want = 1;
  if (want > units_max) want = units_max;
  if (want < 1) want = 1;
  if (want > 65535) want = 65535;
  return (int)want;
}

/* ---- launchers (all asynchronous on the given stream, current device) ------ */

size_t blk_tables_bytes(void);
void blk_tables_fill_host(unsigned char *h);           /* twiddles + Hann, double math on the host */
bl_tables blk_tables_bind(const void *d_mem);          /* pointers into the device copy */
int blk_configure_device(void);                        /* dynamic-LDS attributes of the analysis stages, once per device */

struct blk_analyze_args {
  const int16_t *pcm;        /* arena base */
  const bl_dsong *songs;     /* device, n_songs records */
  bl_dstats *stats;          /* device scratch */
  unsigned *hist;            /* device scratch, BL_HIST_BINS per song (zeroed by the launcher) */
  float *spectrum;           /* device scratch, 256 per song */
  float *energies;           /* device scratch, one per envelope slot */
  double *lc;                /* device scratch, one per envelope slot */
  bl_amd_song_result *results;
  int n_songs, max_n, what, n_cu;
  int n_head = 0, max_n_rest = 0; /* mixed lengths: the first n_head (longest) songs get their own window launch */
  bl_tables tb;
  hipStream_t stream, side;  /* side == nullptr: envelope tail on `stream` */
  hipEvent_t ev_env, ev_tail;
  hipStream_t side2 = nullptr; /* mixed lengths: the long songs' tail (nullptr: no separate launch for them) */
  hipEvent_t ev_head = nullptr, ev_tail2 = nullptr;
  blk_mark_fn mark;          /* may be nullptr */
  void *mark_user;
};
int blk_analyze(const blk_analyze_args &a);             /* bl_kernels.hip: the launch order of the stages below */
int blk_analyze_parts(int what);                        /* BL_AMD_PART_* bits of the scratch that launch order writes */

/* ---- the stages of blk_analyze, one translation unit each --------------------- */
/* Each launches on a.stream unless it takes a stream, for all a.n_songs songs unless it takes a range. */

/* statistics, amplitude, force (bl_stats_kernels.hip) */
void blk_stats_init(const blk_analyze_args &a);
int blk_pcm_scan(const blk_analyze_args &a);            /* zeroes a.hist first; k_freq_scan stands in for it when fused */
void blk_song_prep(const blk_analyze_args &a);          /* k_trim, k_song_prep, k_variance_wrap(_finish) */
void blk_amp_finish(const blk_analyze_args &a, hipStream_t s);
void blk_force(const blk_analyze_args &a);
/* frequency (bl_freq_kernels.hip) */
int blk_freq_configure_device(void);
bool blk_freq_scan_fused(int what);                     /* do the statistics ride along with the frequency pass? */
void blk_freq_scan(const blk_analyze_args &a);          /* k_freq_scan: frequency pass + statistics */
void blk_freq_frames(const blk_analyze_args &a, hipStream_t s);
void blk_freq_finish(const blk_analyze_args &a, hipStream_t s);
/* envelope (bl_env_kernels.hip) */
int blk_env_configure_device(void);
int blk_fir_mode();                                     /* 0 | 1 | 2: bl_amd_set_fir_mode, BL_AMD_FIR_FUSED, the compiled default */
/* window energies of the songs [first, first + count), the longest of them maxn samples */
int blk_env_windows(const blk_analyze_args &a, int fir_mode, int first, int count, int maxn);
void blk_env_tail(const blk_analyze_args &a, hipStream_t s, int first, int count);
/* bl_mean / bl_variance helpers (bl_stats_kernels.hip): one song described by d_songs[0] */
int blk_scan_one(hipStream_t s, const int16_t *pcm, const bl_dsong *d_songs, bl_dstats *d_stats,
                 unsigned *d_hist, int n, int n_cu);
int blk_variance_wrap_one(hipStream_t s, const int16_t *pcm, const bl_dsong *d_songs,
                          bl_dstats *d_stats, int n, int n_cu);

/* ---- per-song signal levels (bl_level_kernels.hip) ----------------------------- */

struct bl_level_song { /* what the level kernels read of a bl_amd_song_desc; record i belongs to d_levels[i] */
  unsigned long long pcm_off; /* int16 elements from the arena base, a multiple of 8 */
  int n, channels;            /* n >= 2 interleaved samples of 1 | 2 channels */
};
#define BL_LEVEL_GROUP_SONGS 32768 /* songs per launch: gridDim.y of the (blocks, songs) grid */
/* bl_amd_levels_batch_device: zeroes d_levels, then fills every field of its n_songs records; max_n: the longest n */
int blk_levels(hipStream_t s, const int16_t *d_pcm, const bl_level_song *d_songs, int n_songs, int max_n, int silence,
               int n_cu, bl_amd_song_levels *d_levels);

/* ---- per-frame spectral timbre (bl_timbre_kernels.hip) -------------------------- */

struct bl_timbre_song { /* one workgroup's song; the records are sorted longest first */
  unsigned long long pcm_off; /* int16 elements from the arena base, a multiple of 8 */
  long long frame_off;        /* the song's first record in d_frames: the sum of F over the songs before it in the
                                 caller's order */
  int n_frames, channels;     /* F >= 1, 1 | 2 */
  int out_idx;                /* position in the caller's order: its record in d_songs_out */
  int reserved;
};
int blk_timbre_configure_device(void);                 /* dynamic-LDS attribute, once per device */
/* bl_amd_timbre_batch_device: one workgroup per record of d_songs; writes every field of the n_songs song records and,
 * unless d_frames is nullptr, of every frame record */
int blk_timbre(hipStream_t s, const int16_t *d_pcm, const bl_timbre_song *d_songs, int n_songs, const bl_tables &tb,
               int pct, unsigned long long min_energy, bl_amd_song_timbre *d_songs_out, bl_amd_frame_timbre *d_frames);

/* ---- mel bands, cepstrum and flatness (bl_mel_kernels.hip) ------------------------- */

/* the image of bl_mel_table.h the kernel copies into its LDS (the bands' first bin, length and weights, the cosine
 * table in the order the lanes take it): its size, and its bytes as built on the host, once per process (nullptr if
 * the table does not have the properties the kernel's bounds rest on) */
size_t blk_mel_image_bytes(void);
const unsigned char *blk_mel_image_host(void);
int blk_mel_configure_device(void);                    /* dynamic-LDS attribute, once per device */
/* bl_amd_mel_batch_device: one workgroup per record of d_songs (the timbre's records: the frames are the same); writes
 * every field of the n_songs song records and, unless they are nullptr, of every frame record and every frame's 32
 * band levels.  d_image: the device copy of the image. */
int blk_mel(hipStream_t s, const int16_t *d_pcm, const bl_timbre_song *d_songs, int n_songs, const bl_tables &tb,
            const void *d_image, unsigned long long min_energy, bl_amd_song_mel *d_songs_out,
            bl_amd_frame_mel *d_frames, uint32_t *d_bands);
/* bl_amd_selftest_ilog2: d_out[i] = bl_ilog2_q12(bl_ilog2_sweep_value(i)) for i < BL_ILOG2_SWEEP (bl_ilog2.h) */
int blk_ilog2_sweep(hipStream_t s, uint32_t *d_out, int n_cu);

/* ---- per-song tempo (bl_rhythm_kernels.hip) -------------------------------------- */

struct bl_rhythm_song { /* one song of a launch group; the records are sorted longest first */
  unsigned long long pcm_off; /* int16 elements from the arena base, a multiple of 8 (unused from a curve) */
  long long onset_off;        /* the song's first hop in d_onsets_out / the caller's curve: the sum of H over the songs
                                 before it in the caller's order */
  long long hop_off;          /* the song's first hop in the novelty scratch: the sum of H over the songs before it in
                                 its launch group */
  int hops, channels;         /* H >= 1, 1 | 2 */
  int out_idx;                /* position in the caller's order: its record in d_songs_out, its row in d_acf_out */
  int reserved;
};
#define BL_RHYTHM_GROUP_SONGS 32768          /* songs per launch group: gridDim.y of the (blocks, songs) grids */
#define BL_RHYTHM_GROUP_HOPS (1ll << 25)     /* hops per launch group, unless its first song alone has more */
/* bytes of the per-group block d_rows: the songs' onset sums, then (own_rows) their 512 lag products */
size_t blk_rhythm_rows_bytes(int n_songs, bool own_rows);
/* One launch group of bl_amd_rhythm_batch_device (d_curve == nullptr: from d_pcm through the novelty scratch d_n, one
 * uint32 per hop of the group) or of bl_amd_rhythm_from_onsets (d_curve: the caller's onset curve on the device, d_n
 * unused).  d_songs: the group's n_songs records, the first of them the longest (max_hops).  d_rows: at least
 * blk_rhythm_rows_bytes(n_songs, !d_acf_out) bytes, zeroed here.  d_acf_out: nullptr, or the rows of ALL songs of the
 * call in the caller's order, zeroed by the caller of this function.  Writes every field of the group's records in
 * d_songs_out and, unless d_onsets_out is nullptr, the onset curve of every hop of the group. */
int blk_rhythm_group(hipStream_t s, const int16_t *d_pcm, const uint32_t *d_curve, const bl_rhythm_song *d_songs,
                     int n_songs, int max_hops, int lag_min, int lag_max, int n_cu, uint32_t *d_n, void *d_rows,
                     bl_amd_song_rhythm *d_songs_out, uint32_t *d_onsets_out, uint64_t *d_acf_out, blk_mark_fn mark,
                     void *mark_user);
/* bl_amd_selftest_isqrt: d_counts[0..1] += values checked, values whose bl_isqrt64 is not the floor of the root */
int blk_isqrt_sweep(hipStream_t s, unsigned long long *d_counts, int n_cu);

/* ---- per-song beat grid (bl_beat_kernels.hip) -------------------------------------- */

struct bl_beat_song { /* one song of a launch group; the records are sorted longest first */
  long long onset_off; /* the song's first hop in the caller's curve and arrays: the sum of H over the songs before it in
                          the caller's order */
  long long hop_off;   /* the song's first hop in the link scratch: the sum of H over the songs before it in its launch
                          group */
  int hops;            /* 1 <= H < 2^24 */
  int out_idx;         /* position in the caller's order: its record in d_songs_out, its period in d_period */
};
#define BL_BEAT_GROUP_SONGS 32768        /* songs per launch group */
#define BL_BEAT_GROUP_HOPS (1ll << 25)   /* hops per launch group, unless its first song alone has more */
/* One launch group of bl_amd_beats_device: one workgroup per record of d_songs.  The period of a song is the int32 at
 * d_period + out_idx * period_stride.  d_links_out, d_scores_out: nullptr or the arrays of ALL songs of the call;
 * d_link_scratch: used without d_links_out, one uint16 per hop of the group.  Writes every byte of the group's records
 * in d_songs_out and every element of its songs in the arrays. */
int blk_beats_group(hipStream_t s, const uint32_t *d_onsets, const bl_beat_song *d_songs, int n_songs,
                    const void *d_period, int period_stride, int tight, bl_amd_song_beats *d_songs_out,
                    uint8_t *d_flags_out, uint16_t *d_links_out, uint16_t *d_link_scratch, int64_t *d_scores_out,
                    blk_mark_fn mark, void *mark_user);

/* ---- chroma and key (bl_chroma_kernels.hip) ---------------------------------------- */

struct bl_chroma_song { /* record i belongs to d_songs_out[i]: the caller's order */
  unsigned long long pcm_off; /* int16 elements from the arena base, a multiple of 8 */
  long long frame_off;        /* the song's first record in d_frames: the sum of T over the songs before it */
  int frames, channels;       /* T >= 0, 1 | 2 */
};
#define BL_CHROMA_GROUP_SONGS 32768 /* songs per launch: gridDim.y of the (blocks, songs) grid */
/* the image of the bank the pitch kernel reads (coefficients in the order its lanes take them, the rows' constants, the
 * gains, the live blocks): its size, and its bytes as built on the host from bl_chroma_table.h, once per process */
size_t blk_chroma_image_bytes(void);
const unsigned char *blk_chroma_image_host(void);
/* bl_amd_chroma_batch_device on one launch group: d_songs its n_songs records, the longest of them max_frames frames;
 * d_image: the device copy of the image; d_acc: 12 uint64 per song, zeroed here.  Writes every byte of the group's
 * records in d_songs_out and, unless d_frames is nullptr, of every frame record of the group. */
int blk_chroma(hipStream_t s, const int16_t *d_pcm, const bl_chroma_song *d_songs, int n_songs, int max_frames,
               int n_cu, const void *d_image, unsigned long long *d_acc, bl_amd_song_chroma *d_songs_out,
               bl_amd_frame_chroma *d_frames, blk_mark_fn mark, void *mark_user);

/* ---- benchmark corpus and sample narrowing (bl_kernels.hip) -------------------- */

int blk_synth(hipStream_t s, int16_t *pcm, const bl_dsong *d_songs, int n_songs, int max_n,
              int n_cu, unsigned seed_base, unsigned rate);
/* out[i] = (int16)(in[i] >> 16): the same-rate S32 -> S16 narrowing */
int blk_narrow_s32(hipStream_t s, const int32_t *d_in, int16_t *d_out, size_t n, int n_cu);

/* ---- matrix, playlist and self-tests over force vectors (bl_matrix_kernels.hip) -- */

int blk_pairwise(hipStream_t s, const struct force_vector_s *d_vecs, int n, int row_begin,
                 int n_rows, float *d_out, bool cosine, blk_mark_fn mark, void *mark_user);
/* exhaustive self-test of bl_sqrt.h over f32 bit patterns [first, first + count): d_counts[0..2] +=
 * values in the fast domain, mismatches of the fast root, mismatches of the compiler's sqrtf */
int blk_sqrt_sweep(hipStream_t s, unsigned long long first, unsigned long long count,
                   unsigned long long *d_counts, int n_cu);
int blk_cos_sweep(hipStream_t s, unsigned long long seed, int per_thread, unsigned long long *d_counts, int n_cu);
int blk_playlist(hipStream_t s, const struct force_vector_s *d_vecs, int n, int seed_index,
                 int32_t *d_order, float *d_dist);
/* the same from a seed vector that is no row of d_vecs (bl_amd_playlist_vec_device) */
int blk_playlist_vec(hipStream_t s, const struct force_vector_s *d_vecs, int n, struct force_vector_s seed,
                     int32_t *d_order, float *d_dist);
/* out[order[i]] = in[i] for 16-byte force vectors (shard-major -> caller order) */
int blk_scatter_vecs(hipStream_t s, const struct force_vector_s *d_in, const int32_t *d_order,
                     struct force_vector_s *d_out, int n);
/* force vectors of a result array, in result order */
int blk_extract_vecs(hipStream_t s, const bl_amd_song_result *d_res, struct force_vector_s *d_out,
                     int n);

/* ---- vector queries over force vectors (bl_query_kernels.hip) ------------------ */

int blk_query_configure_device(void);                  /* dynamic-LDS attributes, once per device */
/* Column split shared by the queries: waves of `qpw` query rows, splits of at least `min_cols` columns; *cols is a
 * multiple of 64 and *n_split the number of blockIdx.y slices.  Not static so that it can be checked on the host. */
void blk_split_plan(int n, int n_rows, int n_cu, int qpw, int min_cols, int *n_split, int *cols);
#define KNN_SPLIT_MIN_COLS 4096 /* min_cols of both kNN forms (force vectors here, descriptors in bl_desc_kernels.hip) */
/* kNN and radius take the query array beside the library.  d_queries == nullptr: the queries are rows
 * [row_begin, row_begin + n_rows) of d_vecs, and a row is no candidate of its own (bl_amd_knn_device,
 * bl_amd_radius_*_device).  Otherwise they are d_queries[0 .. n_rows), vectors of their own that may alias the library,
 * row_begin must be 0 and no candidate is excluded (bl_amd_cross_*_device).  The split plan is
 * blk_split_plan(n, n_rows, ...) either way.  Query scratch, 256-byte aligned, front to back: the library's cosine prep,
 * the queries' own (cross and cosine only), then a column split's partial results.  The *_scratch_bytes functions
 * take d_queries only to tell the two forms apart. */
/* the k nearest songs of each query; d_scratch: at least blk_knn_scratch_bytes(d_queries, n, n_rows, k, cosine, n_cu) */
size_t blk_knn_scratch_bytes(const struct force_vector_s *d_queries, int n, int n_rows, int k, bool cosine, int n_cu);
int blk_knn(hipStream_t s, const struct force_vector_s *d_queries, const struct force_vector_s *d_vecs, int n,
            int row_begin, int n_rows, int k, bool cosine, int n_cu, void *d_scratch, int32_t *d_index, float *d_value);
/* song-to-song chains (bl_amd_chain_device).  blk_chain_shape: 1 = one workgroup per chain, 2 = column split with one
 * launch per step; force: 0 = the launch layer's rule, 1 / 2 = that shape.  d_scratch: at least
 * blk_chain_scratch_bytes(...) bytes for the same (n, n_chains, cosine, n_cu, force), 256-byte aligned; it is
 * re-initialised by every call. */
int blk_chain_shape(int n, int n_chains, int n_cu, int force);
size_t blk_chain_scratch_bytes(int n, int n_chains, bool cosine, int n_cu, int force);
int blk_chain(hipStream_t s, const struct force_vector_s *d_vecs, int n, const int32_t *d_seeds, int n_chains,
              int length, bool cosine, int n_cu, int force, void *d_scratch, int32_t *d_order, float *d_value);
/* chains under rules (bl_amd_mix_device): exactly one of d_seeds / d_seed_vecs, d_tags used when gap > 0, d_exclude
 * nullptr or n bytes.  Shape, force and scratch as blk_chain's. */
size_t blk_mix_scratch_bytes(int n, int n_chains, bool cosine, int n_cu, int force);
int blk_mix(hipStream_t s, const struct force_vector_s *d_vecs, int n, const int32_t *d_seeds,
            const struct force_vector_s *d_seed_vecs, int n_chains, int length, bool cosine, const int32_t *d_tags,
            int gap, const uint8_t *d_exclude, int n_cu, int force, void *d_scratch, int32_t *d_order, float *d_value);
/* the songs within a radius of each query.  bound: the largest squared sum whose correctly rounded root is <= the
 * radius (distance) or the radius itself (cosine).  d_scratch: at least blk_radius_scratch_bytes(d_queries, n, n_rows,
 * cosine, n_cu) bytes; count and fill both rewrite it, and fill needs nothing of what count left there.  d_offset:
 * n_rows + 1 entries. */
size_t blk_radius_scratch_bytes(const struct force_vector_s *d_queries, int n, int n_rows, bool cosine, int n_cu);
int blk_radius_count(hipStream_t s, const struct force_vector_s *d_queries, const struct force_vector_s *d_vecs, int n,
                     int row_begin, int n_rows, bool cosine, float bound, int n_cu, void *d_scratch,
                     long long *d_offset);
int blk_radius_fill(hipStream_t s, const struct force_vector_s *d_queries, const struct force_vector_s *d_vecs, int n,
                    int row_begin, int n_rows, bool cosine, float bound, int n_cu, void *d_scratch,
                    const long long *d_offset, int32_t *d_index, float *d_value);
/* duplicate groups (bl_amd_groups_device): d_group[i] = the smallest index of i's component; d_scratch: the cosine prep */
size_t blk_groups_scratch_bytes(int n, bool cosine);
int blk_groups(hipStream_t s, const struct force_vector_s *d_vecs, int n, bool cosine, float bound, int n_cu,
               void *d_scratch, int32_t *d_group);

/* ---- library-normalised descriptors (bl_desc_kernels.hip) --------------------- */

struct blk_desc_scale { uint16_t s[BL_AMD_DESC_DIMS]; }; /* the per-column scale, passed to the kernel by value */
/* column-wise range of the finite entries of x[n][d]; d_scratch: at least blk_desc_range_scratch_bytes(n, n_cu) */
size_t blk_desc_range_scratch_bytes(int n, int n_cu);
int blk_desc_range(hipStream_t s, const float *d_x, int n, int d, int n_cu, void *d_scratch, bl_amd_desc_range *d_range,
                   blk_mark_fn mark, void *mark_user);
int blk_desc_quantize(hipStream_t s, const float *d_x, int n, int d, const bl_amd_desc_range *d_range,
                      const blk_desc_scale &scale, bl_amd_desc *d_out, blk_mark_fn mark, void *mark_user);
/* the k nearest descriptors of each query by (d^2, index).  d_queries == nullptr: the queries are rows [row_begin,
 * row_begin + n_rows) of d_lib and a row is no candidate of its own; otherwise d_queries[0 .. n_rows), row_begin 0 and
 * nothing excluded.  The column split is blk_split_plan(n, n_rows, n_cu, 16, KNN_SPLIT_MIN_COLS); d_scratch: at least
 * blk_desc_knn_scratch_bytes(n, n_rows, k, n_cu) bytes, which is 0 exactly when the call is not split. */
size_t blk_desc_knn_scratch_bytes(int n, int n_rows, int k, int n_cu);
int blk_desc_knn(hipStream_t s, const bl_amd_desc *d_queries, const bl_amd_desc *d_lib, int n, int row_begin, int n_rows,
                 int k, int n_cu, void *d_scratch, int32_t *d_index, uint64_t *d_dist2, blk_mark_fn mark,
                 void *mark_user);

/* ---- playlist chains over descriptors (bl_desc_chain_kernels.hip) -------------- */

int blk_desc_chain_configure_device(void);             /* dynamic-LDS attributes, once per device */
/* bl_amd_desc_chain_device: exactly one of d_seeds / d_seed_desc, d_tags used when gap > 0, d_exclude nullptr or n
 * bytes.  blk_desc_chain_shape: 1 = one workgroup per group of 16 chains, 2 = column split with one launch per step;
 * force: 0 = the launch layer's rule, 1 / 2 = that shape.  d_scratch: at least blk_desc_chain_scratch_bytes(...) bytes
 * for the same (n, n_chains, n_cu, force), 256-byte aligned; it is re-initialised by every call. */
int blk_desc_chain_shape(int n, int n_chains, int n_cu, int force);
size_t blk_desc_chain_scratch_bytes(int n, int n_chains, int n_cu, int force);
int blk_desc_chain(hipStream_t s, const bl_amd_desc *d_lib, int n, const int32_t *d_seeds,
                   const bl_amd_desc *d_seed_desc, int n_chains, int length, const int32_t *d_tags, int gap,
                   const uint8_t *d_exclude, int n_cu, int force, void *d_scratch, int32_t *d_order,
                   uint64_t *d_dist2);
/* bl_amd_desc_hmix_device: blk_desc_chain under a rule on consecutive songs, the PAIR variant of the same kernels.
 * rule: checked by the caller (flags, tempo_tol) and passed to the kernels by value; d_attr: n attributes, nullptr
 * allowed when the rule has neither BL_AMD_HMIX_KEY nor BL_AMD_HMIX_TEMPO, and then the call is blk_desc_chain.  The
 * shape is blk_desc_chain_shape's; the workspace is its own figure, since the rule's state takes LDS from the played
 * words of the per-chain shape. */
size_t blk_desc_hmix_scratch_bytes(int n, int n_chains, const bl_amd_hmix_rule &rule, int n_cu, int force);
int blk_desc_hmix(hipStream_t s, const bl_amd_desc *d_lib, const bl_amd_hmix_attr *d_attr, int n,
                  const bl_amd_hmix_rule &rule, const int32_t *d_seeds, const bl_amd_desc *d_seed_desc, int n_chains,
                  int length, const int32_t *d_tags, int gap, const uint8_t *d_exclude, int n_cu, int force,
                  void *d_scratch, int32_t *d_order, uint64_t *d_dist2);

/* ---- device rate converter (bl_rs_kernels.hip) ------------------------------ */

#define BL_RS_MAX_DEVICES 16

struct bl_rs_dsong {
  unsigned long long in_off;  /* elements (int16 or int32) from the input base */
  unsigned long long out_off; /* int16 elements from the output base, even */
  int frames, channels;       /* input frames, 1 | 2 */
  int out_frames, refl;       /* bl_rs_out_frames() */
};

struct bl_rs_geom {
  int phase_count, taps, taps8, alloc, w0, span, tiles_per_wg;
  unsigned long long src_incr, dst_incr;
};

/* geometry + LDS budget of a plan (bl_resample.h); BL_UNEXPECTED when a tile's input span
 * does not fit the LDS (input rates far above 192 kHz) */
int blk_resample_geom(int phase_count, int taps, int alloc, int src_incr, int dst_incr, bl_rs_geom *g,
                      size_t *lds_bytes, int *bank_in_lds);
/* d_bank: phase_count rows of `alloc` 32-bit elements (float, or the Q15 coefficients as int) */
int blk_resample(hipStream_t s, const void *d_in, int in_is_s32, const bl_rs_dsong *d_songs, int n_songs,
                 int max_out_frames, const void *d_bank, const bl_rs_geom &g, size_t lds_bytes,
                 int bank_in_lds, int16_t *d_out);

#endif /* BL_LAUNCH_H_ */
