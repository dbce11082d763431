/*
 * bliss_amd.h — batch / device-resident C-ABI of libbliss_amd.so.
 *
 * The reference has no batch API: its only corpus loop is the sequential
 * `for file: bl_song(file)` of python/examples/make_m3u_playlist.py:51-72 and the
 * per-pair bl_distance of src/analyze.c:88-103.  These entry points are the
 * batched form of exactly that path (bl_analyze's analyzers after decode,
 * ref src/analyze.c:40-80, and bl_distance / bl_cosine_similarity over all
 * pairs) for callers that hold many decoded songs.  Plain pointers and sizes
 * only; `stream` is a hipStream_t passed as void* (NULL = default stream).
 * Pointers named d_* are device pointers, h_* host pointers.
 *
 * All functions return BL_OK (0) or BL_UNEXPECTED (-2); there is no CPU
 * fallback: without a usable HIP device they fail and print to stderr.
 */
#ifndef BLISS_AMD_H_
#define BLISS_AMD_H_

#include <stddef.h>
#include <stdint.h>
#include "bliss.h"

#ifdef __cplusplus
extern "C" {
#endif
/* the library itself is built with -fvisibility=hidden: what these headers declare is its whole export list */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* One decoded song inside a PCM arena: what the analyzers read from
 * struct bl_song (ref include/bliss.h:49-67): sample_array, nSamples,
 * channels, duration. */
typedef struct bl_amd_song_desc {
  uint64_t pcm_offset; /* int16 elements from the arena base; multiple of 8 */
  int32_t n_samples;   /* interleaved sample count (bl_song.nSamples), >= 5120 */
  int32_t channels;    /* 1 or 2 */
  uint64_t duration;   /* whole seconds (bl_song.duration), > 0 */
} bl_amd_song_desc;

/* Per-song output: the force vector plus every integer intermediate the
 * reference computes on the way (bit-exact quantities of SURVEY.md §8a). */
typedef struct bl_amd_song_result {
  struct force_vector_s v; /* tempo, amplitude, frequency, attack */
  float force;             /* ref src/analyze.c:68-72 */
  int32_t calm_or_loud;    /* BL_LOUD / BL_CALM / BL_UNKNOWN, ref :73-79 */
  int32_t status;          /* BL_OK, or BL_UNEXPECTED for an input the
                              reference leaves undefined (all-zero PCM, ...) */
  int32_t start, end;      /* ref src/amplitude_sort.c:26-31 */
  int32_t mean, variance;  /* ref src/helpers.c:30-49 */
  int32_t n_frames;        /* ref src/frequency_sort.c:50 */
  int32_t nb_frames;       /* ref src/tempo_atk_sort.c:63-64 */
  int32_t n_windows;       /* FIR+FFT windows run, ref :120 */
  int32_t beat;            /* ref src/tempo_atk_sort.c:277-280 */
  float hist_integral;     /* ref src/amplitude_sort.c:69-71 */
  float freq_peak;         /* ref src/frequency_sort.c:101 */
  double atk_sum;          /* ref src/tempo_atk_sort.c:246-248 */
} bl_amd_song_result;

/* Select the HIP device the plain entry points below use ON THE CALLING THREAD and create
 * its default context (workspace, internal streams).  The first call of the process also
 * sets the process default, which threads that never called bl_amd_init use (device 0 if
 * nobody did).  One process can drive several GPUs: one thread per device. */
int bl_amd_init(int device);
/* Number of visible HIP devices (0 if none / no runtime). */
int bl_amd_device_count(void);

/* Explicit contexts: one device, an own scratch workspace, own internal streams and pinned
 * staging.  Calls on one context are ordered; different contexts — also on the same device —
 * are independent and may be driven from different host threads concurrently. */
typedef struct bl_amd_ctx bl_amd_ctx;
int bl_amd_ctx_create(int device, bl_amd_ctx **out);
void bl_amd_ctx_destroy(bl_amd_ctx *ctx);
int bl_amd_ctx_device(const bl_amd_ctx *ctx);

/* Analyse n_songs songs whose PCM already sits in device memory.
 * d_pcm: arena base; h_desc: host array of n_songs descriptors (copied before the call
 * returns); d_results: device array of n_songs results, written asynchronously on `stream`.
 * The call only enqueues work (descriptor upload from pinned memory, kernels); it does not
 * wait for the device unless the workspace has to grow or four earlier batches of the
 * context are still in flight.  Scratch comes from the context's growing workspace: batches
 * of one context enqueued on different streams are ordered on the device (each waits for the
 * previous one to finish with the workspace); batches of different contexts overlap. */
int bl_amd_analyze_batch_device(const int16_t *d_pcm, const bl_amd_song_desc *h_desc,
                                int n_songs, bl_amd_song_result *d_results, void *stream);
int bl_amd_ctx_analyze_batch_device(bl_amd_ctx *ctx, const int16_t *d_pcm,
                                    const bl_amd_song_desc *h_desc, int n_songs,
                                    bl_amd_song_result *d_results, void *stream);

/* Same from host memory: stages PCM through pinned buffers with
 * hipMemcpyAsync overlapped against the kernels of the previous wave of
 * songs, then copies the results back.  Blocking. */
/* A wave holds at most BL_AMD_HOST_WAVE_BYTES bytes of PCM (environment, read when a context is created; default 2 GiB). */
int bl_amd_analyze_batch_host(const int16_t *const *h_pcm, const int32_t *n_samples,
                              const int32_t *channels, const uint64_t *duration, int n_songs,
                              bl_amd_song_result *h_results);
int bl_amd_ctx_analyze_batch_host(bl_amd_ctx *ctx, const int16_t *const *h_pcm,
                                  const int32_t *n_samples, const int32_t *channels,
                                  const uint64_t *duration, int n_songs,
                                  bl_amd_song_result *h_results);
/* The reference's corpus loop — `for file: bl_analyze(file, &song)` (ref python/examples/
 * make_m3u_playlist.py:51-72, examples/analyze.c:17) — as one call.  Files are decoded
 * (bl_audio_decode) on n_threads host threads (0 = one per hardware thread, at most 32) that run a
 * bounded number of files ahead; the decoded songs go to the GPU in file order, wave by wave,
 * through the pinned-staging path of bl_amd_analyze_batch_host, so decoding, transfer and
 * analysis overlap.  songs[i] (caller-owned, uninitialised is fine) is filled exactly as
 * bl_analyze(filenames[i], &songs[i]) fills it — release each with bl_free_song; with
 * keep_pcm == 0 the sample_array is freed (and NULL) once the song has been analysed.  With keep_pcm != 0 every decoded
 * sample_array stays allocated until the caller frees it: the library bounds its decoders' read-ahead (3 GiB of PCM
 * not yet analysed), not the total, which is the caller's — a corpus that does not fit in host memory has to be
 * analysed with keep_pcm == 0 or in slices.
 * codes (optional, n_files ints) receives what bl_analyze would have returned for the file:
 * BL_LOUD / BL_CALM / BL_UNKNOWN or BL_UNEXPECTED.  Returns the number of files analysed, or
 * BL_UNEXPECTED if the device path itself failed.  Blocking. */
int bl_amd_analyze_files(const char *const *filenames, int n_files, struct bl_song *songs, int *codes,
                         int n_threads, int keep_pcm);

/* How host buffers reach the device: BL_AMD_HOST_STAGED copies them into the library's pinned
 * double buffers on several host threads (default); BL_AMD_HOST_REGISTERED pins the caller's
 * buffers in place with hipHostRegister for the duration of the call (free() stays valid,
 * SURVEY.md section 8b) and copies each song straight into the arena.  Also settable with
 * the environment variable BL_AMD_HOST_MODE=staged|registered. */
#define BL_AMD_HOST_STAGED 0
#define BL_AMD_HOST_REGISTERED 1
int bl_amd_set_host_transfer(int mode);

/* 32-bit sources (BASELINE configs[4] "s16/s32"): h_pcm[i] holds n_samples[i] interleaved
 * int32 samples; they reach the hot path as s16 through an arithmetic >> 16 — the same-rate
 * S32 -> S16 conversion the reference gets from libswresample (ref src/decode.c:323-346,
 * 388-392; third-party arithmetic, parity unpinned).  The narrowing happens while the songs
 * are staged, so the PCIe link only carries s16. */
int bl_amd_analyze_batch_host_s32(const int32_t *const *h_pcm, const int32_t *n_samples,
                                  const int32_t *channels, const uint64_t *duration, int n_songs,
                                  bl_amd_song_result *h_results);
/* Host batches at another sample rate (a 44.1 or 48 kHz collection decoded by the caller):
 * every song is at `sample_rate` Hz, int16 or (pcm_is_s32) int32 left-justified, n_samples[i]
 * interleaved samples at that rate.  Each wave of songs is converted on the device between its
 * transfer and its analysis (bl_amd_resample_batch_device's arithmetic); the results describe
 * the converted songs (nb_frames etc. at 22 050 Hz stereo).  sample_rate == 22 050 is the plain
 * host batch.  Blocking. */
int bl_amd_analyze_batch_host_rate(const void *const *h_pcm, int pcm_is_s32, const int32_t *n_samples,
                                   const int32_t *channels, const uint64_t *duration, int n_songs,
                                   int sample_rate, bl_amd_song_result *h_results);
/* The same narrowing for a device-resident int32 buffer: d_out[i] = (int16)(d_in[i] >> 16). */
int bl_amd_narrow_s32_device(const int32_t *d_in, int16_t *d_out, size_t n, void *stream);

/* Rate conversion to the analyzers' 22 050 Hz stereo s16 — the arithmetic bl_audio_decode()
 * applies to a file at another rate (a restatement of libswresample's default resampler that
 * reproduces the digests of ref tests/test_decode.c:35-36,55-56), for
 * callers that bring their own decoder.  PARITY: only the path for sources wider than 16 bits is
 * pinned on the reference's digests; the 16-bit (Q15) path — what a 44.1 kHz s16 collection goes
 * through — is parity unpinned (s16 path): no reference vector covers its rounding, and every
 * throughput figure quoted for it is a figure for this restatement.
 * `in`: interleaved frames of 1 or 2 channels at in_rate
 * Hz, int16, or (in_is_s32 = 1) int32 left-justified, or — host form only — (in_is_s32 = 2)
 * float with full scale +-1.  A mono source comes out as two equal
 * channels at gain 1/sqrt(2), as the reference's out layout does.
 *   bl_amd_resample_out_frames: output frames for `frames` of input (0: shorter than the filter);
 *   bl_amd_resample_host: *out is malloc'd (free() it), 2 * *out_frames int16;
 *   bl_amd_resample_batch_device: songs resident in HBM, one call for the batch; song i reads
 *     h_desc[i].frames frames at d_in + in_offset (elements of the input type) and writes
 *     2 * bl_amd_resample_out_frames(frames, in_rate) int16 at d_out + out_offset, which is what
 *     bl_amd_analyze_batch_device takes (pcm_offset = out_offset, n_samples = 2 * out frames).
 *     Asynchronous on `stream`; bit-identical to the host form. */
typedef struct bl_amd_resample_desc {
  uint64_t in_offset;  /* elements from d_in; even for stereo */
  uint64_t out_offset; /* int16 elements from d_out; even (multiple of 8 to feed the analysis) */
  int32_t frames;      /* input frames */
  int32_t channels;    /* 1 or 2 */
} bl_amd_resample_desc;
size_t bl_amd_resample_out_frames(size_t frames, int in_rate);
int bl_amd_resample_host(const void *in, int in_is_s32, size_t frames, int channels, int in_rate,
                         int16_t **out, size_t *out_frames);
int bl_amd_resample_batch_device(const void *d_in, int in_is_s32, const bl_amd_resample_desc *h_desc,
                                 int n_songs, int in_rate, int16_t *d_out, void *stream);
int bl_amd_ctx_resample_batch_device(bl_amd_ctx *ctx, const void *d_in, int in_is_s32,
                                     const bl_amd_resample_desc *h_desc, int n_songs, int in_rate,
                                     int16_t *d_out, void *stream);

/* Batch-of-songs mode across the GPUs of one node (BASELINE configs[2]): the corpus is
 * sharded by song over the ranks listed in `devices` (one host thread and one context per
 * rank: contiguous blocks for equal lengths, longest-first greedy by sample count
 * otherwise), each rank analyses its shard through the host-batch path, the 16-byte force
 * vectors are all-gathered (flags: BL_AMD_MULTI_GATHER_RCCL = ncclAllGather over xGMI,
 * librccl loaded on first use; BL_AMD_MULTI_GATHER_PEER = direct peer copies, which also
 * permits several ranks on one device) and rank r computes rows [r N / W, (r+1) N / W) of
 * the N x N bl_distance matrix in the caller's song order.  h_results: n_songs records in
 * caller order.  h_matrix: NULL, or n_songs * n_songs floats that receive the row blocks.
 * Blocking. */
#define BL_AMD_MULTI_GATHER_RCCL 0
#define BL_AMD_MULTI_GATHER_PEER 1
int bl_amd_analyze_corpus_multi(const int16_t *const *h_pcm, const int32_t *n_samples,
                                const int32_t *channels, const uint64_t *duration, int n_songs,
                                const int *devices, int n_devices, int flags,
                                bl_amd_song_result *h_results, float *h_matrix);

/* The same for a corpus that is already RESIDENT in the GPUs' memory (configs[2] proper: 8 192
 * three-minute songs are 260 GB per GPU — they are decoded, converted or generated into each
 * GPU's HBM in waves, never held in host memory at once).  One bl_amd_shard per rank: the arena
 * on that rank's device and its songs; the corpus order is shard-major (all songs of shard 0,
 * then shard 1, ...).  Every rank analyses its arena where it lies (a host thread and a context
 * per rank), the force vectors are all-gathered as above, and rank r computes the rows of its
 * own songs against all N.  d_results (optional, on the shard's device): the shard's records;
 * d_rows (optional, on the shard's device): n_songs x N floats, the shard's row block, which
 * stays in HBM.  h_results (optional): N records in corpus order.  h_matrix (optional): N x N
 * floats.  Blocking.  The reference's corpus loop this replaces: python/examples/
 * make_m3u_playlist.py:51-72 (analyse every file, then distances from the vectors). */
typedef struct bl_amd_shard {
  int32_t device;                  /* HIP device the arena lives on */
  int32_t n_songs;
  const int16_t *d_pcm;            /* arena base, on `device` */
  const bl_amd_song_desc *h_desc;  /* host array of n_songs descriptors */
  bl_amd_song_result *d_results;   /* NULL, or n_songs records on `device` */
  float *d_rows;                   /* NULL, or n_songs * N floats on `device` */
} bl_amd_shard;
int bl_amd_analyze_corpus_multi_device(const bl_amd_shard *shards, int n_shards, int flags,
                                       bl_amd_song_result *h_results, float *h_matrix);

/* bl_audio_decode() follows the reference in always presenting 22 050 Hz PCM to the
 * analyzers (ref src/decode.c:7-9,317-346): a file at another rate, or wider than 16 bits at
 * another rate, goes through a restatement of libswresample's default converter and comes out
 * as 22 050 Hz stereo s16 (resampled = 1).  allow != 0 (also BL_AMD_ALLOW_NATIVE_RATE=1)
 * switches that off: the file is handed over at its own rate, narrowed to s16 only, and its
 * force vector is not comparable with the reference's. */
void bl_amd_decode_allow_native_rate(int allow);
/* Integrity check of the FLAC decoder behind bl_audio_decode: decodes `filename` and compares
 * the MD5 of the decoded samples at their native width (before the narrowing to s16) with the
 * signature of the unencoded audio in the file's STREAMINFO block.  1 = match, 0 = mismatch,
 * BL_UNEXPECTED = not decodable.  computed / stored (16 bytes each) may be NULL. */
int bl_amd_flac_verify(const char *filename, uint8_t computed[16], uint8_t stored[16]);

/* Rows [row_begin, row_begin + n_rows) of the N x N bl_distance matrix
 * (ref src/analyze.c:96-100 for every pair).  d_out: n_rows * n floats. */
int bl_amd_distance_matrix_device(const struct force_vector_s *d_vecs, int n, int row_begin,
                                  int n_rows, float *d_out, void *stream);
/* Same for bl_cosine_similarity (ref src/analyze.c:135-140). */
int bl_amd_cosine_matrix_device(const struct force_vector_s *d_vecs, int n, int row_begin,
                                int n_rows, float *d_out, void *stream);
/* Host-pointer conveniences (blocking). */
int bl_amd_distance_matrix_host(const struct force_vector_s *h_vecs, int n, float *h_out);
int bl_amd_cosine_matrix_host(const struct force_vector_s *h_vecs, int n, float *h_out);

/* Self-test of the square root inside the bl_distance kernels (bliss_amd/csrc/bl_sqrt.h): runs it
 * over every f32 bit pattern on the device and compares with the correctly rounded root,
 * (float)sqrt((double)s).  counts[0] = values in the domain of the five-instruction form,
 * counts[1] = its mismatches, counts[2] = mismatches of the fallback (the compiler's correctly
 * rounded sqrtf) over all 2^32 patterns.  Both must be 0 (tests/test_gpu_parity.py). */
int bl_amd_selftest_sqrt(uint64_t counts[3]);
/* Same for the cosine matrix's guarded quotient (bl_cos.h): at least `triples` pseudo-random (dot, |a|^2, |b|^2)
 * on the device against the plain expression of ref src/analyze.c:135-140.  counts: [0] triples tried, [1] taken by
 * the fast path, [2] fast results that differ from the plain expression (must be 0), [3] largest difference of
 * the two double quotients in ulp (provable bound < 6, guard 16), [4] triples within 64 ulp of a float rounding boundary,
 * [5] of those, how many an unguarded fast path would have got wrong. */
int bl_amd_selftest_cos(uint64_t counts[6], uint64_t triples);

/* Seeded playlist (ref python/examples/make_m3u_playlist.py:62-72): d_dist[j] =
 * bl_distance(vecs[seed_index], vecs[j]) and d_order = the song indices by increasing
 * distance (stable: ties by index).  NaN distances after every number, in index order: numpy's
 * stable argsort; d_dist keeps the NaN.  d_order: n int32, a permutation of 0..n-1; d_dist: n floats. */
int bl_amd_playlist_device(const struct force_vector_s *d_vecs, int n, int seed_index,
                           int32_t *d_order, float *d_dist, void *stream);
int bl_amd_playlist_host(const struct force_vector_s *h_vecs, int n, int seed_index,
                         int32_t *h_order, float *h_dist /* may be NULL */);

/* The same from a seed that is no song of the library (a track analysed but not added, a mean of songs): the vector
 * is passed by value, as bl_distance takes its vectors.  d_dist[j] = bl_distance(seed, vecs[j]), d_order the stable
 * argsort; a seed equal to a song lists that song like any other, at distance 0.  NaN distances after every number,
 * in index order: numpy's stable argsort (a seed with a NaN component lists the songs 0..n-1). */
int bl_amd_playlist_vec_device(const struct force_vector_s *d_vecs, int n, struct force_vector_s seed,
                               int32_t *d_order, float *d_dist, void *stream);
int bl_amd_playlist_vec_host(const struct force_vector_s *h_vecs, int n, struct force_vector_s seed,
                             int32_t *h_order, float *h_dist /* may be NULL */);

/* k nearest songs of each query, without the N x N matrix.  Rows [row_begin, row_begin + n_rows) of d_vecs
 * are the queries; the candidates are all n songs minus the query itself (its exact duplicates are ordinary
 * candidates).  d_index / d_value: n_rows * k, row-major; slot j of row r = the (j+1)-th nearest song to song
 * row_begin + r and its value, with the bits of bl_distance (BL_AMD_KNN_DISTANCE, nearest = smallest;
 * ref src/analyze.c:96-100) or bl_cosine_similarity (BL_AMD_KNN_COSINE, nearest = largest;
 * ref src/analyze.c:135-140).  Order: the returned f32 value (+0 and -0 equal, NaN after every number), ties by
 * the smaller song index — the stable argsort of the matrix row.  If k > n - 1 the trailing slots hold index -1
 * and a NaN.  1 <= k <= BL_AMD_KNN_MAX_K.  Asynchronous on `stream`; the result does not depend on the row
 * range asked for. */
#define BL_AMD_KNN_DISTANCE 0
#define BL_AMD_KNN_COSINE 1
#define BL_AMD_KNN_MAX_K 128
int bl_amd_knn_device(const struct force_vector_s *d_vecs, int n, int row_begin, int n_rows, int k, int metric,
                      int32_t *d_index, float *d_value, void *stream);
/* All n songs as queries, host pointers, blocking.  h_value may be NULL. */
int bl_amd_knn_host(const struct force_vector_s *h_vecs, int n, int k, int metric, int32_t *h_index,
                    float *h_value);

/* Cross queries: the queries are n_queries >= 1 vectors of their own (freshly analysed tracks, a mean of songs)
 * against the library of n >= 1 songs.  X[q][j] = bl_distance(queries[q], vecs[j]) or
 * bl_cosine_similarity(queries[q], vecs[j]) with the query as the first operand; its bits are what
 * bl_amd_*_matrix_device writes at [n + q][j] for the concatenation vecs || queries.  Three rules hold for every cross
 * query (bl_amd_cross_knn_*, bl_amd_cross_radius_*; the names begin with "cross" so that bl_amd_knn_* and
 * bl_amd_radius_* stay the self forms, all of them):
 *   1. No candidate is ever excluded — the one semantic difference from the self forms above.  A query equal to
 *      library song 7 lists song 7, at distance 0.
 *   2. Queries are independent: the answer for query q depends neither on n_queries nor on the other queries.  Shard
 *      by offsetting the query pointer; there is no row_begin.
 *   3. d_queries needs 16-byte alignment only and may alias any part of d_vecs: both are only read.
 * A rejected call returns BL_UNEXPECTED and writes nothing.  Asynchronous on `stream`; no allocation, copy or
 * synchronisation inside once the context's workspace is large enough; calls of one context are ordered on the
 * device like its batches.
 *   bl_amd_cross_knn_device: d_index / d_value: n_queries * k, row-major; slot j of row q = the (j+1)-th nearest
 *     library song to queries[q] under bl_amd_knn's order (the f32 value, +0 = -0, NaN after every number, ties by the
 *     smaller index) and X[q][that song].  1 <= k <= BL_AMD_KNN_MAX_K.  If k > n the trailing k - n slots hold -1 and
 *     a NaN (the self form pads from n - 1).
 *   bl_amd_cross_knn_host: host pointers, blocking.  h_value may be NULL. */
int bl_amd_cross_knn_device(const struct force_vector_s *d_queries, int n_queries, const struct force_vector_s *d_vecs,
                            int n, int k, int metric, int32_t *d_index, float *d_value, void *stream);
int bl_amd_cross_knn_host(const struct force_vector_s *h_queries, int n_queries, const struct force_vector_s *h_vecs,
                          int n, int k, int metric, int32_t *h_index, float *h_value);

/* Song-to-song chains (continuous play): chain c starts at song d_seeds[c]; slot t + 1 holds the song nearest to the
 * song of slot t among the songs not yet in chain c.  d_order / d_value: n_chains * length, row-major.
 * d_order[c][0] = d_seeds[c].  d_value[c][t] = the matrix entry M[d_order[c][t-1]][d_order[c][t]] by its bits
 * (t = 0: M[seed][seed]), M = bl_distance (BL_AMD_KNN_DISTANCE, nearest = smallest) or bl_cosine_similarity
 * (BL_AMD_KNN_COSINE, nearest = largest).  "Nearest" is bl_amd_knn's order: the f32 value, +0 = -0, NaN after
 * every number, ties by the smaller song index.  Exact duplicates of the current song are ordinary candidates.
 * If length > n the trailing slots hold -1 and a NaN.  A seed outside [0, n) gives a row of -1 / NaN.
 * Chains are independent of each other: the result of a chain does not depend on n_chains or on the other seeds.
 * n, n_chains, length >= 1.  Asynchronous on `stream`; no allocation, copy or synchronisation inside once the
 * context's workspace is large enough.  Calls of one context are ordered on the device like its batches. */
int bl_amd_chain_device(const struct force_vector_s *d_vecs, int n, const int32_t *d_seeds, int n_chains,
                        int length, int metric, int32_t *d_order, float *d_value, void *stream);
int bl_amd_ctx_chain_device(bl_amd_ctx *ctx, const struct force_vector_s *d_vecs, int n, const int32_t *d_seeds,
                            int n_chains, int length, int metric, int32_t *d_order, float *d_value, void *stream);
/* Host pointers, blocking.  Seeds are checked first: one outside [0, n) returns BL_UNEXPECTED and writes nothing.
 * h_value may be NULL. */
int bl_amd_chain_host(const struct force_vector_s *h_vecs, int n, const int32_t *h_seeds, int n_chains,
                      int length, int metric, int32_t *h_order, float *h_value);
/* The launch shape a chain call of (n, n_chains) takes on the calling thread's device: BL_AMD_CHAIN_PER_CHAIN (one
 * workgroup per chain) or BL_AMD_CHAIN_SPLIT (columns split over workgroups, one launch per step); BL_UNEXPECTED
 * without a device.  The result of a call never depends on it.  bl_amd_chain_force_shape pins the shape for the
 * whole process (BL_AMD_CHAIN_AUTO undoes that) and returns the previous setting: for measurements and tests. */
#define BL_AMD_CHAIN_AUTO 0
#define BL_AMD_CHAIN_PER_CHAIN 1
#define BL_AMD_CHAIN_SPLIT 2
int bl_amd_chain_shape(int n, int n_chains);
int bl_amd_chain_force_shape(int shape);

/* Chains under rules (radio-style continuous play).  Everything not said here is bl_amd_chain_device's contract:
 * d_order / d_value of n_chains * length, the metric constants, the order of "nearest", values by the bits of the
 * matrix entry, independent chains, asynchronous on `stream`, nothing written by a rejected call.
 *   Seeds    exactly one of d_seeds and d_seed_vecs is non-NULL.  d_seeds: slot 0 is the seed, value M[seed][seed], even
 *            if the seed is excluded; a seed outside [0, n) gives a row of -1 / NaN.  d_seed_vecs: n_chains vectors,
 *            16-byte aligned, may alias d_vecs; slot 0 is the song nearest to the vector among the songs not excluded
 *            (tags play no part), its value bl_distance(seed, vecs[j]) / bl_cosine_similarity(seed, vecs[j]) by the
 *            bits bl_amd_cross_knn_device lists; a row of -1 / NaN if every song is excluded.
 *   Exclude  d_exclude is NULL or n bytes, one mask for all chains: a song with a non-zero byte is never picked.
 *   Tags     d_tags is NULL or n int32 (artist, album ...); a negative tag means untagged: never blocked, blocks
 *            nothing.  0 <= gap <= BL_AMD_MIX_MAX_GAP; gap == 0 ignores the tags, gap > 0 needs them.
 *   A step   at slot t >= 1 song j is allowed iff it is in none of the slots 0 .. t-1, is not excluded, and tags[j] < 0
 *            or tags[j] differs from the tag of every song in slots max(0, t-gap) .. t-1.  Slot t is the allowed song
 *            nearest to the song of slot t-1, its value that matrix entry.  If no song is allowed the chain ends:
 *            slots t .. length-1 hold -1 and a NaN.
 * With d_seeds, d_exclude == NULL and gap == 0 the result is bl_amd_chain_device's, byte for byte.  The launch shape
 * is bl_amd_chain_shape(n, n_chains), bl_amd_chain_force_shape pins it here too, and the result never depends on it.
 * To continue a chain call again with seed = its last song and d_exclude = everything played so far. */
#define BL_AMD_MIX_MAX_GAP 16
int bl_amd_mix_device(const struct force_vector_s *d_vecs, int n, const int32_t *d_seeds,
                      const struct force_vector_s *d_seed_vecs, int n_chains, int length, int metric,
                      const int32_t *d_tags, int gap, const uint8_t *d_exclude, int32_t *d_order, float *d_value,
                      void *stream);
int bl_amd_ctx_mix_device(bl_amd_ctx *ctx, const struct force_vector_s *d_vecs, int n, const int32_t *d_seeds,
                          const struct force_vector_s *d_seed_vecs, int n_chains, int length, int metric,
                          const int32_t *d_tags, int gap, const uint8_t *d_exclude, int32_t *d_order, float *d_value,
                          void *stream);
/* Host pointers, blocking.  Index seeds are checked first: one outside [0, n) returns BL_UNEXPECTED and writes nothing.
 * h_value may be NULL. */
int bl_amd_mix_host(const struct force_vector_s *h_vecs, int n, const int32_t *h_seeds,
                    const struct force_vector_s *h_seed_vecs, int n_chains, int length, int metric,
                    const int32_t *h_tags, int gap, const uint8_t *h_exclude, int32_t *h_order, float *h_value);

/* Radius queries: the songs within a radius of each query, however many, as compressed sparse row (CSR) lists and
 * without the N x N matrix.  M is the bl_distance matrix (BL_AMD_KNN_DISTANCE; ref src/analyze.c:96-100) or the
 * bl_cosine_similarity matrix (BL_AMD_KNN_COSINE; ref src/analyze.c:135-140), entries by their bits as
 * bl_amd_*_matrix_device writes them.  Song j is within the radius of query i iff j != i and M[i][j] <= radius
 * (distance) or M[i][j] >= radius (cosine): plain f32 compares, so a NaN entry is never within, +0 and -0 are equal,
 * and exact duplicates of the query at other indices are ordinary candidates.  +-inf and negative radii are legal and
 * mean what the compare says; a NaN radius is an argument error.  Rows [row_begin, row_begin + n_rows) of d_vecs are
 * the queries, n >= 1, 0 <= row_begin, n_rows >= 1, row_begin + n_rows <= n; a rejected call returns BL_UNEXPECTED
 * and writes nothing.
 *   bl_amd_radius_count_device: d_offset (n_rows + 1 entries) receives the exclusive prefix sums of the list lengths:
 *     d_offset[0] = 0, d_offset[r + 1] - d_offset[r] = the number of songs within the radius of song row_begin + r,
 *     the last entry the total.  The sums are taken on the device, exactly, in int64.
 *   bl_amd_radius_fill_device: d_offset is what the count call wrote for the same arguments; the songs of row r go to
 *     d_index[d_offset[r] .. d_offset[r + 1]) in ascending song index, and their matrix entries, by their bits, to
 *     the same slots of d_value (may be NULL).  It reads nothing the count call left behind but d_offset.
 * Both are asynchronous on `stream`; no allocation, copy or synchronisation inside once the context's workspace is
 * large enough; calls of one context are ordered on the device like its batches.  The result depends neither on the
 * row range asked for nor on the launch shape taken.
 *   bl_amd_radius_host: all n songs as queries, host pointers, blocking.  h_offset: n + 1 entries; *h_index and
 *     *h_value are malloc'd (free() them; an empty result is a valid block too).  h_value may be NULL.
 *   bl_amd_radius_bound: the exact bound the distance filter runs on: the largest f32 s with
 *     (float)sqrt((double)s) <= radius, so that "bl_distance <= radius" is "squared sum <= bound" (the rounded root
 *     is monotone).  -inf for a negative radius (nothing is within), 0 for +-0, +inf for +inf, the radius for NaN. */
float bl_amd_radius_bound(float radius);
int bl_amd_radius_count_device(const struct force_vector_s *d_vecs, int n, int row_begin, int n_rows, int metric,
                               float radius, int64_t *d_offset, void *stream);
int bl_amd_ctx_radius_count_device(bl_amd_ctx *ctx, const struct force_vector_s *d_vecs, int n, int row_begin,
                                   int n_rows, int metric, float radius, int64_t *d_offset, void *stream);
int bl_amd_radius_fill_device(const struct force_vector_s *d_vecs, int n, int row_begin, int n_rows, int metric,
                              float radius, const int64_t *d_offset, int32_t *d_index, float *d_value, void *stream);
int bl_amd_ctx_radius_fill_device(bl_amd_ctx *ctx, const struct force_vector_s *d_vecs, int n, int row_begin,
                                  int n_rows, int metric, float radius, const int64_t *d_offset, int32_t *d_index,
                                  float *d_value, void *stream);
int bl_amd_radius_host(const struct force_vector_s *h_vecs, int n, int metric, float radius, int64_t *h_offset,
                       int32_t **h_index, float **h_value);

/* Radius queries from vectors outside the library (the cross rules above bl_amd_cross_knn_device): the CSR contract
 * of bl_amd_radius_* with n_queries + 1 offsets.  Song j is within the radius of query q iff X[q][j] <= radius
 * (distance) or X[q][j] >= radius (cosine) — there is no j != i clause, so radius 0 finds the library's copy of a
 * query.  The distance bound is bl_amd_radius_bound; a NaN radius is an argument error, +-inf and negative radii mean
 * what the compare says.  Offsets are int64, summed on the device; indices ascend within a row; d_value may be NULL.
 *   bl_amd_cross_radius_host: host pointers, blocking.  h_offset: n_queries + 1 entries; *h_index and *h_value are
 *     malloc'd (free() them; an empty result is a valid block too).  h_value may be NULL. */
int bl_amd_cross_radius_count_device(const struct force_vector_s *d_queries, int n_queries,
                                     const struct force_vector_s *d_vecs, int n, int metric, float radius,
                                     int64_t *d_offset, void *stream);
int bl_amd_ctx_cross_radius_count_device(bl_amd_ctx *ctx, const struct force_vector_s *d_queries, int n_queries,
                                         const struct force_vector_s *d_vecs, int n, int metric, float radius,
                                         int64_t *d_offset, void *stream);
int bl_amd_cross_radius_fill_device(const struct force_vector_s *d_queries, int n_queries,
                                    const struct force_vector_s *d_vecs, int n, int metric, float radius,
                                    const int64_t *d_offset, int32_t *d_index, float *d_value, void *stream);
int bl_amd_ctx_cross_radius_fill_device(bl_amd_ctx *ctx, const struct force_vector_s *d_queries, int n_queries,
                                        const struct force_vector_s *d_vecs, int n, int metric, float radius,
                                        const int64_t *d_offset, int32_t *d_index, float *d_value, void *stream);
int bl_amd_cross_radius_host(const struct force_vector_s *h_queries, int n_queries, const struct force_vector_s *h_vecs,
                             int n, int metric, float radius, int64_t *h_offset, int32_t **h_index, float **h_value);

/* Duplicate groups: d_group[i] (n int32) = the smallest song index in the weakly connected component of song i in the
 * graph that has an edge i -> j iff j is within the radius of i (as defined above): a pure function of (vecs, metric,
 * radius).  A song with no neighbour is its own group.  The edges are never stored.  Asynchronous on `stream`, no host
 * round trips; a NaN radius is an argument error. */
int bl_amd_groups_device(const struct force_vector_s *d_vecs, int n, int metric, float radius, int32_t *d_group,
                         void *stream);
int bl_amd_ctx_groups_device(bl_amd_ctx *ctx, const struct force_vector_s *d_vecs, int n, int metric, float radius,
                             int32_t *d_group, void *stream);
int bl_amd_groups_host(const struct force_vector_s *h_vecs, int n, int metric, float radius, int32_t *h_group);

/* Signal levels: what a player needs of a song's PCM beyond the four ratings — how loud it is (peak, RMS, DC), how
 * often it crosses zero, how many samples sit at full scale, where the silence at either end stops, and the four
 * samples that say whether it runs into the next track.  None of it is in the reference's API: its author's ROADMAP.md
 * lists "zero-crossing rate" and "rough measure of the dB level of songs" as next, and head / tail are the samples
 * ref examples/detect-gapless.c:28-33 reads.  Every field is an exact integer.
 * F = n_samples / channels (integer division) is the number of frames; channel c of frame t is
 * pcm[t * channels + c].  A sample behind frame F - 1 (the last one of a stereo song with an odd n_samples) only shows
 * up in `tail`.  For a mono song every [1] entry of the per-channel fields is 0.
 *   lead    the number of frames before the first frame in which some channel has |s| > silence
 *   trail   the number of frames after the last such frame; a song with no such frame has lead = trail = F */
typedef struct bl_amd_song_levels { /* 80 bytes */
  int64_t sum[2];        /* sum of the samples of channel c (DC) */
  uint64_t sum_sq[2];    /* sum of their squares; (-32768)^2 = 2^30 counts in full */
  int32_t peak[2];       /* max |s|, 0 .. 32768 */
  int32_t zero_cross[2]; /* frames t in [1, F) with (s[t] < 0) != (s[t-1] < 0); 0 counts as non-negative */
  int32_t clipped[2];    /* samples equal to 32767 or -32768 */
  int32_t lead, trail;   /* see above */
  int32_t frames;        /* F */
  int32_t status;        /* BL_OK */
  int16_t head[2];       /* pcm[0], pcm[1]: interleaved, whatever `channels` is */
  int16_t tail[2];       /* pcm[n_samples - 2], pcm[n_samples - 1] */
} bl_amd_song_levels;
/* bl_amd_levels_batch_device: the levels of n_songs songs whose PCM sits in device memory, one streaming pass.  The
 * descriptors are those of bl_amd_analyze_batch_device with other limits: pcm_offset a multiple of 8, channels 1 or 2,
 * n_samples >= 2 (not the analysers' 5120: levels make sense for any clip), duration ignored; d_pcm 16-byte aligned.
 * 0 <= silence <= 32767, n_songs >= 1.  A rejected call returns BL_UNEXPECTED and writes nothing.  Asynchronous on
 * `stream`; h_desc is copied before the call returns; d_levels (n_songs records) need not be zeroed by the caller.
 * Calls of one context are ordered on the device like its batches.  The record of a song is a pure function of its
 * samples, `channels` and `silence`: it depends neither on the other songs, nor on n_songs, nor on the launch grid,
 * and no sample outside [pcm_offset, pcm_offset + n_samples) is read.
 *   bl_amd_levels_batch_host: the same from host memory, blocking: the songs are uploaded and analysed in waves.
 *   bl_amd_gapless_host: plain host arithmetic, no device.  h_linked[i], i < n_songs - 1, is 1 iff song i runs into
 *     song i + 1 under the rule of ref examples/detect-gapless.c:35-54: for an interleaved slot k in {0, 1} with
 *     |tail_i[k]| >= 5 and |head_{i+1}[k]| >= 5, fabs(((float)tail_i[k] - head_{i+1}[k]) / (float)INT16_MAX) < 0.01
 *     (in integers: |tail - head| <= 327); slot 0 or slot 1 suffices.  n_songs == 1 writes nothing.
 *   bl_amd_levels_peak_db = 20 log10(peak / 32768), bl_amd_levels_rms_db = 10 log10(sum_sq / (frames * 2^30)), in
 *     double from the exact integers: -inf for a zero argument (also channel 1 of a mono song), NaN for a channel
 *     outside [0, 1]. */
int bl_amd_levels_batch_device(const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs, int silence,
                               bl_amd_song_levels *d_levels, void *stream);
int bl_amd_ctx_levels_batch_device(bl_amd_ctx *ctx, const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs,
                                   int silence, bl_amd_song_levels *d_levels, void *stream);
int bl_amd_levels_batch_host(const int16_t *const *h_pcm, const int32_t *n_samples, const int32_t *channels,
                             int n_songs, int silence, bl_amd_song_levels *h_levels);
int bl_amd_gapless_host(const bl_amd_song_levels *h_levels, int n_songs, uint8_t *h_linked);
double bl_amd_levels_peak_db(const bl_amd_song_levels *lv, int channel);
double bl_amd_levels_rms_db(const bl_amd_song_levels *lv, int channel);

/* Spectral timbre: per frame of the frequency analysis, where the power sits (centroid), where it stops (rolloff) and
 * its strongest bin (peak), summarised over the song.  The reference's author lists "spectral centroid" and "spectral
 * rolloff" in ROADMAP.md ("Timbral features"); none of it is in the reference's API.  Every field is an exact integer.
 * Frames are those of ref src/frequency_sort.c:50,67-80: F = (n_samples / channels) / 512, frame t is samples
 * [512 channels t, 512 channels (t + 1)), stereo averaged with C's truncating / 2, Hann-windowed, libavcodec's
 * 512-point f32 transform; P_t[d], d = 1..255, is re*re + im*im (unfused): bit for bit what the frequency pass adds
 * into its spectrum.  Bins 0 and 256 take no part.  Per frame, with Q_t[d] = floor(16 P_t[d]) as a uint64 (power in
 * sixteenths; the sum over d stays below 2^50):
 *   energy   sum of Q_t[d];   moment   sum of d Q_t[d]
 *   rolloff  the smallest d in 1..255 with 100 * (Q_t[1] + .. + Q_t[d]) >= pct * energy (pct = 100: the last
 *            non-zero bin; energy = 0: 1)
 *   peak     the smallest d that maximises Q_t[d] (an all-zero frame: 1)
 *   centroid floor(4096 moment / energy), for energy > 0: in 1/4096 of a bin; one bin is rate / 512 Hz
 * Per song: a frame is USED iff energy > 0 and energy >= min_energy; the sums and sums of squares of centroid, rolloff
 * and peak run over the used frames. */
typedef struct bl_amd_frame_timbre { /* 24 bytes */
  uint64_t energy, moment;
  int32_t rolloff, peak;
} bl_amd_frame_timbre;
typedef struct bl_amd_song_timbre { /* 72 bytes */
  uint64_t centroid_sum, centroid_sumsq;
  uint64_t rolloff_sum, rolloff_sumsq;
  uint64_t peak_sum, peak_sumsq;
  uint64_t energy_max; /* over ALL frames */
  int32_t frames;      /* F */
  int32_t used;
  int32_t status;      /* BL_OK */
  int32_t reserved;    /* 0 */
} bl_amd_song_timbre;
/* bl_amd_timbre_frames: F of a song, plain host arithmetic; -1 for n_samples < 0 or channels outside {1, 2}.
 * bl_amd_timbre_batch_device: the timbre of n_songs songs whose PCM sits in device memory.  The descriptors are those
 * of bl_amd_analyze_batch_device with other limits: pcm_offset a multiple of 8, channels 1 or 2, F >= 1 (not the
 * analysers' 5120 samples), duration ignored; d_pcm 16-byte aligned.  1 <= pct <= 100, n_songs >= 1.  d_songs_out:
 * n_songs records in the caller's order.  d_frames_out may be NULL (n_frame_records is then ignored); otherwise it
 * receives every frame's record, songs concatenated in the caller's order, song i at the sum of F_j over j < i, and
 * n_frame_records must equal the sum of all F_j.  Neither output needs zeroing.  A rejected call returns
 * BL_UNEXPECTED and writes nothing.  Asynchronous on `stream`; h_desc is copied before the call returns.  Calls of
 * one context are ordered on the device like its batches.  A song's records are a pure function of its samples,
 * `channels`, pct and min_energy: they depend neither on the other songs, n_songs, the order, the launch shape nor on
 * whether d_frames_out is NULL, and no sample outside the song's whole frames is read.  Read-only towards
 * bl_amd_last_energies and bl_amd_last_freq_stats.
 *   bl_amd_timbre_batch_host: the same from host memory, blocking: the songs are uploaded and analysed in waves;
 *     h_frames_out may be NULL.
 *   bl_amd_timbre_centroid_hz / _rolloff_hz / _peak_hz: plain host arithmetic in double from the exact integers, no
 *     device.  Each returns the mean over the used frames in Hz (sum / used, the centroid divided by 4096, times
 *     rate / 512) and stores the population standard deviation in *std_hz if that is not NULL; used == 0 gives NaN
 *     for both. */
int bl_amd_timbre_frames(int n_samples, int channels);
int bl_amd_timbre_batch_device(const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs, int pct,
                               uint64_t min_energy, bl_amd_song_timbre *d_songs_out,
                               bl_amd_frame_timbre *d_frames_out, long long n_frame_records, void *stream);
int bl_amd_ctx_timbre_batch_device(bl_amd_ctx *ctx, const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs,
                                   int pct, uint64_t min_energy, bl_amd_song_timbre *d_songs_out,
                                   bl_amd_frame_timbre *d_frames_out, long long n_frame_records, void *stream);
int bl_amd_timbre_batch_host(const int16_t *const *h_pcm, const int32_t *n_samples, const int32_t *channels,
                             int n_songs, int pct, uint64_t min_energy, bl_amd_song_timbre *h_songs_out,
                             bl_amd_frame_timbre *h_frames_out);
double bl_amd_timbre_centroid_hz(const bl_amd_song_timbre *st, int rate, double *std_hz);
double bl_amd_timbre_rolloff_hz(const bl_amd_song_timbre *st, int rate, double *std_hz);
double bl_amd_timbre_peak_hz(const bl_amd_song_timbre *st, int rate, double *std_hz);

/* Tempo: a song's beat period, which — unlike the reference's `tempo` rating — converts to beats per minute, and how
 * much of the onset energy repeats at it.  The reference's author lists "BPM" and "Beat loudness" in ROADMAP.md
 * ("Temporal features"); none of it is in the reference's API.  Every field is an exact integer: all arithmetic below
 * is integer arithmetic and fits 64 bits.
 * F = n_samples / channels frames, H = F / 128 hops (BL_AMD_RHYTHM_HOP frames each), T = H - 511 terms.
 *   1 mix         m[i] = l[i] + r[i] (stereo) or 2 s[i] (mono: a mono song and its dual-mono copy give the same
 *                 bytes); d[0] = 0, d[i] = m[i] - m[i-1]: across hop boundaries, never across the song's start.  No
 *                 sample outside the song's 128 H whole frames is read.
 *   2 energies    over the hop's 128 frames: A_h = sum m[i]^2, B_h = sum d[i]^2
 *   3 amplitudes  a_h = isqrt((A_h + A_{h-1} + A_{h-2} + A_{h-3}) >> 9), b_h the same from B; indices below 0
 *                 contribute 0; isqrt is the exact floor of the square root
 *   4 novelty     n_0 = 0, n_h = max(0, a_h - a_{h-1}) + max(0, b_h - b_{h-1})
 *   5 local mean  q_h = max(0, 16 n_h - sum_{k=-8..7} n_{h+k}) >> 4, n outside [0, H) taken as 0
 *   6 smoothing   o_h = (q_{h-1} + 2 q_h + q_{h+1}) >> 2, q outside [0, H) taken as 0: the onset curve
 *   7 lags        R[tau] = sum_{h=0}^{T-1} o_h o_{h+tau}, tau = 0 .. 511: the same number of terms for every lag
 *   8 pick        over the caller's range 1 <= lag_min <= lag_max <= 510: r_peak = max R[tau], lag_peak the smallest
 *                 tau that attains it.  r_peak == 0: lag = lag_peak = 0.  Otherwise lag is the smallest tau in the range
 *                 with R[tau] >= R[tau-1], R[tau] >= R[tau+1] and 16 R[tau] >= 15 r_peak (the shortest period that is
 *                 a local maximum within 1/16 of the best: a periodic curve scores equally at every multiple of its
 *                 period), or lag_peak if there is none.
 * Bounds: |m| <= 2^16, so m^2 reaches 2^32 (the all -32768 stereo song) and does not fit 32 bits; d^2 < 2^34;
 * A_h <= 2^39, B_h < 2^41, the window sums < 2^43, so a_h <= 2^16, b_h < 2^17 and n, q, o < 2^18; a product is
 * < 2^36 and H < 2^24 (n_samples is an int), so R < 2^60 and 16 R < 2^64. */
#define BL_AMD_RHYTHM_HOP 128
#define BL_AMD_RHYTHM_LAGS 512
typedef struct bl_amd_song_rhythm { /* 72 bytes */
  uint64_t r0, r_prev, r_lag, r_next; /* R[0], R[lag-1], R[lag], R[lag+1]; the last three are 0 when lag == 0 */
  uint64_t r_peak, onset_sum;         /* max over the range; sum of o_h over all H hops */
  uint32_t onset_max;                 /* max of o_h over all H hops */
  int32_t hops, terms;                /* H, T */
  int32_t lag, lag_peak;
  int32_t status;                     /* BL_OK; BL_UNEXPECTED for a song with H < 512 */
} bl_amd_song_rhythm;
/* bl_amd_rhythm_hops: H of a song, plain host arithmetic; -1 for n_samples < 0 or channels outside {1, 2}.
 * bl_amd_rhythm_batch_device: the tempo of n_songs songs whose PCM sits in device memory.  The descriptors are those
 * of bl_amd_analyze_batch_device with other limits: pcm_offset a multiple of 8, channels 1 or 2, H >= 1, duration
 * ignored; d_pcm 16-byte aligned.  1 <= lag_min <= lag_max <= 510, n_songs >= 1.  d_songs_out: n_songs records in the
 * caller's order.  d_onsets_out may be NULL (n_onsets is then ignored); otherwise it receives o_h of every hop, songs
 * concatenated in the caller's order, song i at the sum of H_j over j < i, and n_onsets must equal the sum of all H_j.
 * d_acf_out may be NULL; otherwise it receives R[0 .. 511] of every song, 512 values per song in the caller's order.
 * No output needs zeroing and every byte of every record is written.  A rejected call returns BL_UNEXPECTED and
 * writes nothing.  A song with H < 512 is no error of the call: its record has status = BL_UNEXPECTED, hops = H,
 * terms = 0 and everything else 0, its row of d_acf_out is 0 and its onsets are written.  Asynchronous on `stream`;
 * h_desc is copied before the call returns.  Calls of one context are ordered on the device like its batches.  A
 * song's outputs are a pure function of its samples, `channels`, lag_min and lag_max: they depend neither on the other
 * songs, n_songs, the order, the launch shape nor on which optional outputs are asked for.  Read-only towards
 * bl_amd_last_energies and bl_amd_last_freq_stats.
 *   bl_amd_rhythm_batch_host: the same from host memory, blocking: the songs are uploaded and analysed in waves;
 *     h_onsets_out and h_acf_out may be NULL.
 *   bl_amd_rhythm_from_onsets: stages 7 and 8 alone on onset curves the caller supplies, from host memory, blocking:
 *     h_onsets holds the curves one behind the other, h_hops[i] >= 1 values of song i, each value < 2^18 and
 *     h_hops[i] < 2^24 (else the call is rejected); onset_sum and onset_max are those of the given curve; h_acf_out
 *     may be NULL.
 *   bl_amd_rhythm_bpm: plain host arithmetic in double from the exact integers, no device.  NaN for lag == 0 (or a
 *     NULL record, or rate < 1).  With den = r_prev - 2 r_lag + r_next: delta = 0.5 (r_prev - r_next) / den if
 *     den < 0 and r_lag is at least as large as both neighbours, else 0; clamped to +-0.5;
 *     bpm = 60 rate / (128 (lag + delta)).
 *   bl_amd_rhythm_strength: r_lag / r0, 0 when r0 == 0 (NaN for a NULL record): how much of the curve's energy repeats
 *     at the beat.  It can slightly exceed 1 because the two factors cover different stretches of the curve.
 *   bl_amd_selftest_isqrt: sweeps, on the device, 0 and k^2 - 1, k^2, k^2 + 1 for every k in [1, 2^17] against
 *     r^2 <= x < (r + 1)^2; counts = {checked, wrong}. */
int bl_amd_rhythm_hops(int n_samples, int channels);
int bl_amd_rhythm_batch_device(const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs, int lag_min,
                               int lag_max, bl_amd_song_rhythm *d_songs_out, uint32_t *d_onsets_out,
                               long long n_onsets, uint64_t *d_acf_out, void *stream);
int bl_amd_ctx_rhythm_batch_device(bl_amd_ctx *ctx, const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs,
                                   int lag_min, int lag_max, bl_amd_song_rhythm *d_songs_out, uint32_t *d_onsets_out,
                                   long long n_onsets, uint64_t *d_acf_out, void *stream);
int bl_amd_rhythm_batch_host(const int16_t *const *h_pcm, const int32_t *n_samples, const int32_t *channels,
                             int n_songs, int lag_min, int lag_max, bl_amd_song_rhythm *h_songs_out,
                             uint32_t *h_onsets_out, uint64_t *h_acf_out);
int bl_amd_rhythm_from_onsets(const uint32_t *h_onsets, const int32_t *h_hops, int n_songs, int lag_min, int lag_max,
                              bl_amd_song_rhythm *h_songs_out, uint64_t *h_acf_out);
double bl_amd_rhythm_bpm(const bl_amd_song_rhythm *r, int rate);
double bl_amd_rhythm_strength(const bl_amd_song_rhythm *r);
int bl_amd_selftest_isqrt(uint64_t counts[2]);

/* Beats: where the beats of a song are, the half of the tempo that the lags of stage 7 discard by construction.  A
 * beat-matched crossfade aligns two songs on a beat; the tempo call gives the period, this gives the grid.  It is
 * Ellis's dynamic-programming beat tracker ("Beat Tracking by Dynamic Programming", 2007) over the onset curve o_h of
 * the tempo call, stated in exact integers: all arithmetic below is integer arithmetic and fits a signed 64-bit value.
 * Per song: a curve o[0 .. H-1] with values < 2^18 and 1 <= H < 2^24, a period L in hops, and one `tight` per call,
 * 0 <= tight <= 4096.  Log2q12 is the base-2 logarithm in 1/4096 of the mel block (bl_ilog2_q12).
 *   1 scale       omax = max o_h, W = tight omax (the record's pen_scale); lo = (L + 1) >> 1, hi = 2 L
 *   2 penalty     for d in [lo, hi]: e(d) = |Log2q12(d) - Log2q12(L)|, pen(d) = (W e(d)^2) >> 28.  tight = 16 prices
 *                 one octave off the period at one omax.
 *   3 scores      for t = 0 .. H-1: best(t) = max over d in [lo, min(hi, t)] of C[t-d] - pen(d), ties to the smallest
 *                 d.  If the range is empty or best(t) <= 0: C[t] = o[t], P[t] = 0.  Otherwise C[t] = o[t] + best(t)
 *                 and P[t] = that d.
 *   4 end         t_end = the arg-max of C[t] over t in [max(0, H - L), H - 1], ties to the largest t;
 *                 score = C[t_end].  score == 0: the song has no beats (n_beats = 0, first = last = -1).
 *   5 back-trace  the beats are t_end, t_end - P[t_end], ... down to and including the first hop with P == 0;
 *                 flag[h] = 1 on a beat and 0 elsewhere; first and last are the smallest and largest beat, n_beats
 *                 their number.
 * Bounds: W < 2^30; e <= 4096 for every L in 2 .. 510 and d in [lo, hi], so W e^2 < 2^54 and pen < 2^26;
 * 0 <= C < 2^42 and P <= 1020.
 * A song whose L lies outside [2, 510] is no error of the call (a lag of 0 means "no tempo"): its record has
 * status = BL_UNEXPECTED, hops = H, period = L as given and every other field 0, and its flags, links and scores are 0. */
#define BL_AMD_BEATS_PERIOD_MAX 510
#define BL_AMD_BEATS_TIGHT_MAX 4096
typedef struct bl_amd_song_beats { /* 40 bytes */
  int64_t score;                   /* C[t_end] */
  uint64_t pen_scale;              /* W */
  int32_t hops, period;            /* H, L */
  int32_t n_beats, first, last;
  int32_t status;                  /* BL_OK; BL_UNEXPECTED for a song with L outside [2, 510] */
} bl_amd_song_beats;
/* bl_amd_beats_device: the beat grids of n_songs songs whose onset curves sit in device memory.  The layout of
 * d_onsets, d_flags_out, d_links_out (P) and d_scores_out (C) is that of d_onsets_out of bl_amd_rhythm_batch_device:
 * songs concatenated in the caller's order, song i at the sum of h_hops[j] over j < i.  The int32 period of song i is
 * read on the device at (char *)d_period + i * period_stride: a stride of 4 takes a packed array, a stride of
 * sizeof(bl_amd_song_rhythm) = 72 together with &d_records->lag takes the tempo straight from the records of the
 * tempo call, with no copy and no kernel in between; the stride is a multiple of 4 and >= 4.  d_links_out and
 * d_scores_out may be NULL: P then stays in the context's workspace and C never leaves the chip.  No output needs
 * zeroing and every element of every output is written.  A rejected call returns BL_UNEXPECTED and writes nothing:
 * a NULL required pointer, a pointer misaligned for its element type, n_songs < 1, an h_hops[i] outside [1, 2^24), a
 * bad stride, tight outside [0, 4096].  An onset value >= 2^18 is the caller's error and is not checked on the device.
 * Asynchronous on `stream`; h_hops is copied before the call returns.  A song's outputs are a pure function of its
 * curve, L and tight: they depend neither on the other songs, n_songs, the order nor on which optional outputs are
 * asked for.  One workgroup works on one song, whatever its length: the recurrence is serial in time.
 *   bl_amd_beats_host: the same from host memory, blocking; h_period is a packed int32 array; an onset value >= 2^18
 *     rejects the call; h_links_out and h_scores_out may be NULL.
 *   bl_amd_beats_list: plain host arithmetic, no device.  Returns the number of set flags among h_flags[0 .. hops) and
 *     writes the first min(count, cap) beats as hop indices to h_hop_out and as seconds, 128.0 hop / rate, to
 *     h_sec_out; either may be NULL.  -1 for a NULL h_flags, hops < 0, rate < 1 or cap < 0.
 *   bl_amd_beats_bpm: plain host arithmetic: 60 rate (n_beats - 1) / (128 (last - first)), the tempo of the grid
 *     itself, finer than one hop.  NaN for n_beats < 2, a NULL record or rate < 1.
 * tight has not been tuned against annotated music; on synthetic click curves with jitter every value from 16 to 256
 * followed every click, and the Python binding's default is 128. */
int bl_amd_beats_device(const uint32_t *d_onsets, const int32_t *h_hops, int n_songs, const void *d_period,
                        int period_stride, int tight, bl_amd_song_beats *d_songs_out, uint8_t *d_flags_out,
                        uint16_t *d_links_out, int64_t *d_scores_out, void *stream);
int bl_amd_ctx_beats_device(bl_amd_ctx *ctx, const uint32_t *d_onsets, const int32_t *h_hops, int n_songs,
                            const void *d_period, int period_stride, int tight, bl_amd_song_beats *d_songs_out,
                            uint8_t *d_flags_out, uint16_t *d_links_out, int64_t *d_scores_out, void *stream);
int bl_amd_beats_host(const uint32_t *h_onsets, const int32_t *h_hops, int n_songs, const int32_t *h_period, int tight,
                      bl_amd_song_beats *h_songs_out, uint8_t *h_flags_out, uint16_t *h_links_out,
                      int64_t *h_scores_out);
int bl_amd_beats_list(const uint8_t *h_flags, int hops, int rate, int32_t *h_hop_out, double *h_sec_out, int cap);
double bl_amd_beats_bpm(const bl_amd_song_beats *b, int rate);

/* Tempo over time (the tempogram): the lag products of stage 7 of the tempo call over a sliding window of the onset
 * curve, and the pick of stage 8 on every window.  The tempo call gives one lag per song; this tells whether that lag
 * holds for the whole song and what the tempo is at the song's two ends, where a beat-matched transition joins it to
 * its neighbours.  Every field is an exact integer: all arithmetic below is integer arithmetic and fits an unsigned
 * 64-bit value.
 * Per song: a curve o[0 .. H-1] with values < 2^18 and 1 <= H < 2^24 (the layout of d_onsets_out of
 * bl_amd_rhythm_batch_device), and one bl_amd_tgram_params per call: stride S, a multiple of 16 in [16, 1024];
 * blocks m in [1, 16], the window is W = m S terms; 1 <= lag_min <= lag_max <= 510; tol per mille in [0, 1000];
 * octaves 0 | 1; the reserved words 0.  T = H - 511 as in the tempo call.
 *   1 frames      F = (T - W) / S + 1 by floor division if T >= W, else F = 0.  Frame f owns the terms h in
 *                 [f S, f S + W).
 *   2 lags        R_f[tau] = sum over the frame's terms of o_h o_{h+tau}, tau = 0 .. 511: every lag has the same
 *                 number of terms, and no hop outside [0, H) is read
 *   3 pick        stage 8 of the tempo call, word for word, on R_f: r_peak, lag_peak and lag; both lags are 0 when
 *                 r_peak == 0.  A frame with lag != 0 "has a tempo".
 *   4 frame       bl_amd_tgram_frame; r_prev, r_lag, r_next are 0 when lag == 0
 *   5 near        near(L, M) is true if 1000 |L - M| <= tol M; with `octaves` set also if 1000 |2 L - M| <= tol M or
 *                 1000 |L - 2 M| <= tol 2 M
 *   6 song        bl_amd_song_tgram, over the frames that have a tempo, in frame order: n_tempo their number;
 *                 frame_first, frame_last and their lags lag_first, lag_last (the frames -1 and the lags 0 when
 *                 n_tempo == 0); lag_low, lag_high the smallest and largest lag; lag_median the lower median, the
 *                 element at index (n_tempo - 1) >> 1 of the sorted lags; n_near the number of frames with
 *                 near(lag, lag_median); n_jumps the number of consecutive pairs (earlier, later) with
 *                 !near(later, earlier), where frames without a tempo are skipped and do not break a pair.
 * Bounds: a product is < 2^36 and W <= 2^14, so R < 2^50 and 16 R fits.
 * A song with F == 0 is no error of the call: its record has status = BL_UNEXPECTED, hops = H and every other field 0. */
typedef struct bl_amd_tgram_params { /* 32 bytes */
  int32_t stride, blocks;            /* S, m */
  int32_t lag_min, lag_max;
  int32_t tol, octaves;
  int32_t reserved[2];               /* 0 */
} bl_amd_tgram_params;
typedef struct bl_amd_tgram_frame { /* 40 bytes */
  uint64_t r0, r_prev, r_lag, r_next; /* R_f[0], R_f[lag-1], R_f[lag], R_f[lag+1]; the last three are 0 when lag == 0 */
  int32_t lag, lag_peak;
} bl_amd_tgram_frame;
typedef struct bl_amd_song_tgram { /* 56 bytes */
  int32_t hops, frames;              /* H, F */
  int32_t n_tempo;
  int32_t status;                    /* BL_OK; BL_UNEXPECTED for a song with F == 0 */
  int32_t frame_first, frame_last, lag_first, lag_last;
  int32_t lag_low, lag_high, lag_median;
  int32_t n_near, n_jumps;
  int32_t reserved;                  /* 0 */
} bl_amd_song_tgram;
/* bl_amd_tgram_frames: F of a song of `hops` hops, plain host arithmetic; -1 for NULL or bad parameters or hops outside
 *   [1, 2^24).
 * bl_amd_tgram_device: the tempograms of n_songs songs whose onset curves sit in device memory, songs concatenated in
 *   the caller's order, song i at the sum of h_hops[j] over j < i.  d_songs_out: n_songs records.  d_frames_out: the
 *   frame records, songs concatenated in the same order, song i at the sum of F_j over j < i; n_frames must equal the
 *   sum of all F_j, and d_frames_out may be NULL when that sum is 0.  d_gram_out may be NULL; otherwise it receives
 *   R_f[0 .. 511] of every frame, 512 uint64 per frame in the order of the frame records.  No output needs zeroing and
 *   every byte of every record is written.  A rejected call returns BL_UNEXPECTED and writes nothing: a NULL required
 *   pointer, a misaligned pointer (the curves 4 bytes, the song records 4, the frame records and the rows 8),
 *   n_songs < 1, an h_hops[i] outside [1, 2^24), a wrong n_frames, bad parameters.  These checks come before any
 *   context or device is touched.  An onset value >= 2^18 is the caller's error and is not checked on the device.
 *   Asynchronous on `stream`; h_hops and params are copied before the call returns.  A song's outputs are a pure
 *   function of its curve and the parameters: they depend neither on the other songs, their order, the launch shape
 *   nor on which optional outputs are asked for.  The workspace is kept per context (32 bytes and 24 bytes per song);
 *   bl_amd_ctx_destroy frees it with the context.
 * bl_amd_tgram_host: the same from host memory, blocking; an onset value >= 2^18 rejects the call; h_frames_out may be
 *   NULL when no song has a frame, h_gram_out may be NULL.
 * Host arithmetic, no device:
 *   bl_amd_tgram_bpm: the interpolation of bl_amd_rhythm_bpm on a frame's r_prev, r_lag, r_next and lag.  NaN for
 *     lag == 0, a NULL record or rate < 1.
 *   bl_amd_tgram_seconds: the time of the centre of frame `frame`'s window, 128 (frame S + W / 2) / rate.  NaN for
 *     frame < 0, NULL or bad parameters or rate < 1.
 *   bl_amd_tgram_steadiness: n_near / n_tempo, 0 when n_tempo == 0 (NaN for a NULL record): the share of the frames
 *     whose tempo is the song's median tempo.
 *   bl_amd_tgram_shape: the lengths at which the kernels change path, for tests: the terms of the curve the block
 *     kernel stages at a time (it stages whole blocks of S terms: max(1, tile_terms / S) of them) and the frames of one
 *     run of the block kernel when a song is cut into runs (a call of few songs cuts every song into runs of exactly
 *     this many frames).  Any pointer may be NULL.
 *   bl_amd_tgram_profile_ms: as bl_amd_chords_profile_ms, for "tgram_blocks" and "tgram_songs".
 * tol, S and m have not been tuned on recorded music. */
int bl_amd_tgram_frames(int hops, const bl_amd_tgram_params *params);
int bl_amd_tgram_device(const uint32_t *d_onsets, const int32_t *h_hops, int n_songs, const bl_amd_tgram_params *params,
                        bl_amd_song_tgram *d_songs_out, bl_amd_tgram_frame *d_frames_out, long long n_frames,
                        uint64_t *d_gram_out, void *stream);
int bl_amd_ctx_tgram_device(bl_amd_ctx *ctx, const uint32_t *d_onsets, const int32_t *h_hops, int n_songs,
                            const bl_amd_tgram_params *params, bl_amd_song_tgram *d_songs_out,
                            bl_amd_tgram_frame *d_frames_out, long long n_frames, uint64_t *d_gram_out, void *stream);
int bl_amd_tgram_host(const uint32_t *h_onsets, const int32_t *h_hops, int n_songs, const bl_amd_tgram_params *params,
                      bl_amd_song_tgram *h_songs_out, bl_amd_tgram_frame *h_frames_out, uint64_t *h_gram_out);
double bl_amd_tgram_bpm(const bl_amd_tgram_frame *f, int rate);
double bl_amd_tgram_seconds(int frame, const bl_amd_tgram_params *params, int rate);
double bl_amd_tgram_steadiness(const bl_amd_song_tgram *t);
void bl_amd_tgram_shape(int *tile_terms, int *run_frames);
double bl_amd_tgram_profile_ms(const char *name, int *launches);

/* Beats that follow the tempo over time: the dynamic programme of bl_amd_beats_* with the period a function of the
 * hop.  bl_amd_beats_* tracks at the tempo call's one lag; on a song whose tempo changes its grid is wrong for part of
 * the song, and the ends, which a beat-matched transition joins, are where it is worst.  Here the period comes from
 * per-frame lags such as bl_amd_tgram_frame.lag, read in place.  All arithmetic is integer arithmetic and fits a signed
 * 64-bit value.
 * Per song: a curve o[0 .. H-1] with values < 2^18 and 1 <= H < 2^24, F frame lags lag_f (int32), 0 <= F <= 2^20, and
 * optionally an anchor lag A (int32).  Per call one bl_amd_tbeats_params: seg in [16, 16384], origin in [0, 2^24),
 * tight in [0, 4096], fold 0 | 1, the reserved words 0.
 *   1 valid       frame f is valid if 2 <= lag_f <= 510.  F == 0 or no valid frame: the song has no tempo
 *   2 fill        q_f = lag_f for a valid frame; an invalid frame takes the lag of the valid frame nearest by |f - f'|,
 *                 ties to the earlier frame; n_filled is the number of invalid frames
 *   3 fold        only with `fold` set, an anchor given and 2 <= A <= 510: if 3 q <= 2 A then q' = 2 q, else if
 *                 3 q > 4 A then q' = q >> 1; applied once, and q stays as it was if q' falls outside [2, 510];
 *                 n_folded is the number of frames that changed.  (42 then 88 with A = 42 gives 42 then 44.)
 *   4 track       g(t) = clamp(floor((t - origin) / seg), 0, F - 1) and L(t) = q_g(t); a tempogram of stride S and m
 *                 blocks gives seg = S and origin = (m - 1) S / 2 (bl_amd_tbeats_params_from_tgram).  A run is a
 *                 maximal stretch of hops with equal L(t); n_runs is their number
 *   5 scale       W = tight max o_h over the whole song (pen_scale)
 *   6 scores      stage 3 of bl_amd_beats_* with L = L(t), the period of the hop being scored, not of its source:
 *                 lo = (L(t) + 1) >> 1, hi = 2 L(t), pen(d) = (W e^2) >> 28 with e = |Log2q12(d) - Log2q12(L(t))|;
 *                 best(t) = max over d in [lo, min(hi, t)] of C[t-d] - pen(d), ties to the smallest d; a link is made
 *                 only if best(t) > 0
 *   7 end         t_end = the arg-max of C over [max(0, H - L(H-1)), H - 1], ties to the largest t; score = C[t_end]
 *   8 back-trace  flags, first, last and n_beats as in bl_amd_beats_*; period_first = L(first) and
 *                 period_last = L(last), both 0 when score == 0
 * Bounds: those of bl_amd_beats_*: pen < 2^26, 0 <= C < 2^42, P <= 1020.
 * Property: if every valid frame has the same lag L and no fold applies, flags, links, scores, score, pen_scale,
 * n_beats, first and last equal those of bl_amd_beats_* at L byte for byte.
 * A song without a tempo is no error of the call: its record has status = BL_UNEXPECTED, hops = H, frames = F and every
 * other field 0, and its flags, links, scores and track are 0. */
typedef struct bl_amd_tbeats_params { /* 32 bytes */
  int32_t seg, origin;               /* hops per frame; the hop at which frame 0 would begin */
  int32_t tight, fold;
  int32_t reserved[4];               /* 0 */
} bl_amd_tbeats_params;
typedef struct bl_amd_song_tbeats { /* 64 bytes */
  int64_t score;                    /* C[t_end] */
  uint64_t pen_scale;               /* W */
  int32_t hops, frames;             /* H, F */
  int32_t n_beats, first, last;
  int32_t status;                   /* BL_OK; BL_UNEXPECTED for a song without a tempo */
  int32_t period_first, period_last;
  int32_t n_runs, n_filled, n_folded;
  int32_t reserved;                 /* 0 */
} bl_amd_song_tbeats;
/* bl_amd_tbeats_device: the grids of n_songs songs whose curves and frame lags sit in device memory.  d_onsets,
 *   h_hops, d_flags_out, d_links_out and d_scores_out are those of bl_amd_beats_device.  h_frames[i] = F_i.  The lag of
 *   frame f of song i is the int32 read at (char *)d_lag + (sum of F_j over j < i, plus f) * lag_stride: a stride of 4
 *   takes a packed array, a stride of sizeof(bl_amd_tgram_frame) = 40 together with &d_frames->lag the tempogram's
 *   frame records in place; d_lag may be NULL when every F_i is 0.  d_anchor may be NULL; otherwise the anchor of song
 *   i is the int32 at (char *)d_anchor + i * anchor_stride: a stride of sizeof(bl_amd_song_tgram) = 56 together with
 *   &d_songs->lag_median takes the tempogram's song records.  d_links_out, d_scores_out and d_track_out may be NULL;
 *   d_track_out receives q of every frame after fill and fold, packed int32 in the order of the lags.  No output needs
 *   zeroing and every byte of every output is written.  A rejected call returns BL_UNEXPECTED and writes nothing: a
 *   NULL required pointer, a misaligned pointer (the curves, lags, anchors and track 4 bytes, the records and scores 8,
 *   the links 2), n_songs < 1, an h_hops[i] outside [1, 2^24), an h_frames[i] outside [0, 2^20], a stride below 4 or
 *   no multiple of 4, bad parameters or a reserved word that is not 0.  These checks come before any context or device
 *   is touched.  An onset value >= 2^18 is the caller's error and is not checked on the device.  Asynchronous on
 *   `stream`; h_hops, h_frames and params are copied before the call returns.  A song's outputs are a pure function of
 *   its curve, its lags, its anchor and the parameters: they depend neither on the other songs, their order nor on
 *   which optional outputs are asked for.  The workspace is kept per context (32 bytes and 40 bytes per song, 4 bytes
 *   per frame without d_track_out, 2 bytes per hop of a launch group without d_links_out); bl_amd_ctx_destroy frees it.
 * bl_amd_tbeats_host: the same from host memory, blocking; h_lag is a packed int32 array of all frames, h_anchor a
 *   packed int32 array or NULL; an onset value >= 2^18 rejects the call.
 * Host arithmetic, no device:
 *   bl_amd_tbeats_params_from_tgram: seg = S and origin = (m - 1) S / 2 of a tempogram's parameters, with `tight` and
 *     `fold`; -1 for a NULL pointer, bad tempogram parameters, tight outside [0, 4096] or fold outside 0 | 1, else 0.
 *   bl_amd_tbeats_edge_bpm: the tempo of the grid over its first (at_end == 0) or last k = min(n, count) beats, where
 *     count is the number of set flags among h_flags[0 .. hops): 60 rate (k - 1) / (128 span), span the hops from the
 *     first to the last of those k beats: the in and out tempo a transition needs.  NaN for k < 2, a NULL pointer,
 *     hops < 0 or rate < 1.
 *   bl_amd_beats_list works on these flags as it does on those of bl_amd_beats_*.
 *   bl_amd_tbeats_shape: the lengths at which the kernels change path, for tests: the scores kept on the chip and the
 *     frames the track kernel scans at a time.  Any pointer may be NULL.
 *   bl_amd_tbeats_profile_ms: as bl_amd_chords_profile_ms, for "tbeats_track" and "tbeats".
 * tight, the fold and the tempogram's parameters have not been tuned on recorded music. */
int bl_amd_tbeats_device(const uint32_t *d_onsets, const int32_t *h_hops, const int32_t *h_frames, int n_songs,
                         const void *d_lag, int lag_stride, const void *d_anchor, int anchor_stride,
                         const bl_amd_tbeats_params *params, bl_amd_song_tbeats *d_songs_out, uint8_t *d_flags_out,
                         uint16_t *d_links_out, int64_t *d_scores_out, int32_t *d_track_out, void *stream);
int bl_amd_ctx_tbeats_device(bl_amd_ctx *ctx, const uint32_t *d_onsets, const int32_t *h_hops, const int32_t *h_frames,
                             int n_songs, const void *d_lag, int lag_stride, const void *d_anchor, int anchor_stride,
                             const bl_amd_tbeats_params *params, bl_amd_song_tbeats *d_songs_out, uint8_t *d_flags_out,
                             uint16_t *d_links_out, int64_t *d_scores_out, int32_t *d_track_out, void *stream);
int bl_amd_tbeats_host(const uint32_t *h_onsets, const int32_t *h_hops, const int32_t *h_frames, int n_songs,
                       const int32_t *h_lag, const int32_t *h_anchor, const bl_amd_tbeats_params *params,
                       bl_amd_song_tbeats *h_songs_out, uint8_t *h_flags_out, uint16_t *h_links_out,
                       int64_t *h_scores_out, int32_t *h_track_out);
int bl_amd_tbeats_params_from_tgram(const bl_amd_tgram_params *tgram, int tight, int fold, bl_amd_tbeats_params *out);
double bl_amd_tbeats_edge_bpm(const uint8_t *h_flags, int hops, int rate, int n, int at_end);
void bl_amd_tbeats_shape(int *ring, int *track_tile);
double bl_amd_tbeats_profile_ms(const char *name, int *launches);

/* Loudness: the K-weighted, gated programme loudness of ITU-R BS.1770-4 / EBU R128 and the loudness range of EBU Tech
 * 3342, the figure a player needs to level "B after A" (the reference's author lists "Loudness features" in ROADMAP.md;
 * bl_amd_levels_* gives peak and plain RMS, which is not loudness).  The filter is f64 in a fixed operation order;
 * everything behind it is exact integers.  One parameter record per call (bl_amd_loud_kweight fills it for a rate);
 * per song F = n_samples / channels frames and H = F / hop whole hops; frames behind hop H-1 are never read.
 *   1 chunks      chunk k covers hops [16 k, min(16 k + 16, H)).  Its filter starts from zero state at frame
 *                 max(0, 16 k hop - warm) and runs serially to the chunk's end.  A chunk's output is a pure function of
 *                 those frames: this cut is what makes the recurrence parallel, and it is part of the definition, not
 *                 a launch detail.
 *   2 filter      per channel, x = (double)sample; every product and sum rounded to f64, unfused, in this order, with
 *                 the y[n-1] term last:
 *                   v = ((((b0*x + b1*x1) + b2*x2) - a2*v2) - a1*v1)          (s1_b, s1_a; v1, v2: v of frames n-1, n-2)
 *                   y = ((((v - (v1 + v1)) + v2) - A2*y2) - A1*y1)            (A = s2_a)
 *                 f64 denormals are honoured (the state decays through them under digital silence).
 *   3 hop energy  e = 0, then e = e + y*y in frame order over the hop's frames (warm-up frames contribute nothing);
 *                 Z[c][h] = floor(e) as uint64.  With bl_amd_loud_kweight's coefficients the impulse response's l1
 *                 norm is 3.23 / 3.33 / 3.34 at 22.05 / 44.1 / 48 kHz, so |y| < 2^16.8 and Z < 2^45.7 for hop <= 4800.
 *                 For other coefficients the caller must keep |y| < 2^17 (Z < 2^46.3); nothing checks it.
 *   4 blocks      P_j = sum over c and k < 4 of Z[c][j+k], j = 0 .. H-4: 400 ms blocks at a stride of one hop.  A mono
 *                 song has one channel: as in BS.1770 and ebur128 it is not counted as dual mono.  P < 2^49.3.
 *   5 gates       A = { j : P_j > abs_gate }, N1 = |A| (abs_count), S1 = sum over A of P_j (abs_sum);
 *                 G = { j in A : P_j 10 N1 > S1 } (gated_count, gated_sum).  Strict product comparisons in 128 bits: no
 *                 division on the device.  The sums are carried as two 64-bit limbs {lo, hi}: no sum wraps for any H.
 *   6 short-term  ST_j = sum over c and k < 30 of Z[c][j+k], j = 0 .. H-30; st_max over every j.  For the range the
 *                 starts are j = 0, 10, 20, ...: those with 2 ST > 15 abs_gate number N and sum to S; the survivors
 *                 of ST 100 N > S (-20 LU) number M (st_gated).  Over the survivors in ascending order v[0 .. M-1]:
 *                 lra_lo = v[(10 (M-1) + 50) / 100], lra_hi = v[(95 (M-1) + 50) / 100], the nearest-rank rule of Tech
 *                 3342's reference code; M = 0 gives 0 for both.
 * A song with H < 4 has blocks = 0 and all sums 0; it is no error of the call. */
typedef struct bl_amd_loud_params {
  double s1_b[3], s1_a[2]; /* stage 1 (shelf): b0 b1 b2, a1 a2 */
  double s2_a[2];          /* stage 2 (high-pass): a1 a2; its numerator is 1 -2 1 by construction */
  int32_t hop;             /* frames per hop (100 ms), 1 .. 4800 */
  int32_t warm;            /* warm-up frames in front of a chunk, 0 .. 8192 */
  uint64_t abs_gate;       /* threshold on a 4-hop block sum, < 2^56 */
} bl_amd_loud_params;
#define BL_AMD_LOUD_CHUNK 16 /* hops per chunk */
typedef struct bl_amd_song_loud { /* 88 bytes */
  uint64_t gated_sum[2];          /* sum over G of P_j: lo, hi */
  uint64_t abs_sum[2];            /* S1: lo, hi */
  uint64_t momentary_max, st_max; /* max P_j, max ST_j */
  uint64_t lra_lo, lra_hi;
  int32_t gated_count, abs_count, st_gated;
  int32_t hops, blocks;           /* H, max(0, H - 3) */
  int32_t status;                 /* BL_OK */
} bl_amd_song_loud;
/* bl_amd_loud_batch_device: the loudness of n_songs songs in the PCM arena d_pcm, laid out as for
 * bl_amd_rhythm_batch_device: pcm_offset a multiple of 8, channels 1 | 2, n_samples >= 1, duration ignored.
 * d_hops_out may be NULL (Z then stays in the context's workspace); otherwise it receives Z as uint64[n_hops][2], songs
 * concatenated in the caller's order, channel 1 of a mono song 0, and n_hops must be the sum of H over the songs.
 * Every byte of every record and of d_hops_out is written; nothing needs zeroing.  A rejected call returns
 * BL_UNEXPECTED and writes nothing: a NULL required pointer, a misaligned pointer (d_pcm 16, the outputs 8 bytes),
 * n_songs < 1, a bad song, hop, warm or abs_gate outside the ranges above, a coefficient that is not finite, a wrong
 * n_hops, more than 2^30 chunks in all.  Asynchronous on `stream`; h_desc and params are copied before the call
 * returns.  A song's outputs depend on nothing but its samples, channels and the params.
 *   bl_amd_loud_batch_host: the same from host memory, blocking; h_hops_out may be NULL.
 *   bl_amd_loud_from_hops: stages 4 to 6 alone on hop energies of the caller's in host memory, uint64[sum of
 *     h_hops][2] laid out as d_hops_out, blocking; only params->abs_gate is read.  0 <= h_hops[i] <= 2^27; a value
 *     >= 2^46 rejects the call.
 * Host arithmetic, no device:
 *   bl_amd_loud_kweight: the K-weighting by the usual bilinear design, K = tan(pi f0 / rate): the shelf with
 *     f0 = 1681.974450955533 Hz, G = 3.999843853973347 dB, Q = 0.7071752369554196, Vb = Vh^0.4996667741545416, the
 *     high-pass with f0 = 38.13547087602444 Hz, Q = 0.5003270373238773 (BS.1770-4's printed table at 48 000 Hz);
 *     hop = rate / 10, warm = 4096, abs_gate = floor(4 hop 2^30 10^-6.9309) (-70 LUFS).  BL_UNEXPECTED for a rate
 *     outside 8000 .. 48000 or no multiple of 10: above 48 kHz a warm-up of 4096 frames is no longer enough.
 *   bl_amd_loud_lufs: -0.691 + 10 log10(gated_sum / (gated_count 4 hop 2^30)); -inf when gated_count is 0.
 *   bl_amd_loud_momentary_max_lufs, bl_amd_loud_short_max_lufs: the same of momentary_max / (4 hop 2^30) and
 *     st_max / (30 hop 2^30); -inf for 0.
 *   bl_amd_loud_range_lu: 10 log10(lra_hi / lra_lo); 0 when st_gated is 0.
 *   bl_amd_loud_gain_db: target_lufs - bl_amd_loud_lufs; 0 when gated_count is 0 (silence gets no gain).
 *   Each returns NaN for a NULL record or hop < 1.
 *   bl_amd_loud_profile_ms: the device time in milliseconds that k_loud_filter ("loud_filter") or k_loud_gate
 *     ("loud_gate") took in the calls made while profiling was on (bl_amd_profile) since this function was last
 *     asked for that name, and the number of launches; -1 for another name.  Waits for those kernels.
 * The loudness keeps its workspace per context it has been called on (the records, Z of a call without d_hops_out,
 * 8 bytes per short-term start); bl_amd_ctx_destroy frees it with the context.
 * The true peak that goes with a gain is bl_amd_tpeak_* below. */
int bl_amd_loud_batch_device(const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs,
                             const bl_amd_loud_params *params, bl_amd_song_loud *d_songs_out, uint64_t *d_hops_out,
                             long long n_hops, void *stream);
int bl_amd_ctx_loud_batch_device(bl_amd_ctx *ctx, const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs,
                                 const bl_amd_loud_params *params, bl_amd_song_loud *d_songs_out, uint64_t *d_hops_out,
                                 long long n_hops, void *stream);
int bl_amd_loud_batch_host(const int16_t *const *h_pcm, const int32_t *n_samples, const int32_t *channels, int n_songs,
                           const bl_amd_loud_params *params, bl_amd_song_loud *h_songs_out, uint64_t *h_hops_out);
int bl_amd_loud_from_hops(const uint64_t *h_hop_energy, const int32_t *h_hops, int n_songs,
                          const bl_amd_loud_params *params, bl_amd_song_loud *h_songs_out);
int bl_amd_loud_kweight(int rate, bl_amd_loud_params *params);
double bl_amd_loud_lufs(const bl_amd_song_loud *r, int hop);
double bl_amd_loud_momentary_max_lufs(const bl_amd_song_loud *r, int hop);
double bl_amd_loud_short_max_lufs(const bl_amd_song_loud *r, int hop);
double bl_amd_loud_range_lu(const bl_amd_song_loud *r);
double bl_amd_loud_gain_db(const bl_amd_song_loud *r, int hop, double target_lufs);
double bl_amd_loud_profile_ms(const char *name, int *launches);

/* True peak: how far the RECONSTRUCTED waveform goes above full scale, the figure ReplayGain 2.0 and EBU R128 pair with
 * the loudness, because a gain to a target is safe only when it is known.  The sample peak of bl_amd_levels_* can be
 * 3 dB short of it: a full-scale sine at a quarter of the rate, sampled at 45 degrees, has samples at -3.01 dBFS and a
 * true peak at 0 dBTP.  As in ITU-R BS.1770 the signal is oversampled four times by a fixed interpolator; every
 * quantity is an exact integer.  Per song F = n_samples / channels frames; per channel c, x_c[t] is the sample for
 * 0 <= t < F and 0 elsewhere.  For 0 <= t < F and phase p = 0 .. 3
 *   y_c[4t + p] = sum over j = -5 .. 6 of G[p][j + 5] * x_c[t + j]
 * with the Q14 table G of bliss_amd/csrc/bl_tpeak_table.h (bl_amd_tpeak_table shows it): G[p][j + 5] =
 * floor(2^14 w(m) sinc(m / 4) + 1/2), m = 4 j - p, w(m) = (1 + cos(pi m / 24)) / 2 for |m| < 24 and 0 otherwise: a
 * Hann-windowed sinc of 12 taps per phase.  Phase 0 is the sample times 2^14, so a true peak is never below the sample
 * peak: tpeak[c] >= peak[c] << 14.  The largest row l1 norm is 30 544, so |y| <= 30 544 * 32 768 < 2^30: full scale is
 * 2^29, and the scale reaches 5.4 dB above it.  For a mono song every [1] entry is 0 and at[1] = -1. */
typedef struct bl_amd_song_tpeak { /* 56 bytes */
  int64_t at[2];     /* the smallest i with |y_c[i]| == tpeak[c]; -1 when F == 0 and for channel 1 of a mono song */
  int64_t overs[2];  /* the number of i in [0, 4F) with |y_c[i]| > ceiling * 2^14 */
  uint32_t tpeak[2]; /* max over i in [0, 4F) of |y_c[i]| */
  int32_t peak[2];   /* max |x_c[t]|, 0 .. 32768 */
  int32_t frames;    /* F */
  int32_t status;    /* BL_OK */
} bl_amd_song_tpeak;
/* bl_amd_tpeak_batch_device: the true peak of n_songs songs in the PCM arena d_pcm, laid out as for
 * bl_amd_loud_batch_device: pcm_offset a multiple of 8, channels 1 | 2, n_samples >= 1, duration ignored.
 * 0 <= ceiling <= 65535 (in sample units: 32767 counts the points above full scale) and 1 <= block <= 65536; both are
 * always validated.  d_blocks_out may be NULL (n_blocks is then ignored); otherwise it receives the profile as
 * uint32[n_blocks][2], songs concatenated in the caller's order: block b of a song is max |y_c[i]| over
 * 4 b block <= i < 4 min(F, (b + 1) block), channel 1 of a mono song 0, and n_blocks must be the sum of
 * ceil(F / block) over the songs.  It is a meter's or limiter's input.  Every byte of every record and of d_blocks_out
 * is written; nothing needs zeroing.  A rejected call returns BL_UNEXPECTED and writes nothing: a NULL required
 * pointer, a misaligned pointer (d_pcm 16, the records 8, the blocks 4 bytes), n_songs < 1, a bad song, ceiling or
 * block, a wrong n_blocks.  Asynchronous on `stream`; h_desc is copied before the call returns.  A song's outputs are a
 * pure function of its samples, channels, ceiling and block: they depend neither on the other songs, nor on n_songs,
 * nor on the launch grid, and no sample outside [pcm_offset, pcm_offset + n_samples) is read.
 *   bl_amd_tpeak_batch_host: the same from host memory, blocking; h_blocks_out may be NULL.
 * Host arithmetic, no device:
 *   bl_amd_tpeak_table: G, row-major, 48 values.
 *   bl_amd_tpeak_shape: the frames one lane and one workgroup of the kernel own (16 and 4 096): the lengths at which
 *     its paths change, for tests.
 *   bl_amd_tpeak_dbtp: 20 log10(tpeak[channel] / 2^29) in dBTP; -inf for 0, NaN for a NULL record or a channel outside
 *     [0, 1].  bl_amd_tpeak_song_dbtp: the larger of the two channels.
 *   bl_amd_tpeak_gain_db: min(bl_amd_loud_gain_db(loud, hop, target_lufs), ceiling_dbtp - bl_amd_tpeak_song_dbtp(tp)):
 *     the gain to the target, held back where it would lift the true peak above ceiling_dbtp.  The loudness gain alone
 *     when both tpeak are 0; NaN for a NULL record or hop < 1.
 *   bl_amd_tpeak_profile_ms: as bl_amd_loud_profile_ms, for k_tpeak_scan ("tpeak_scan") and k_tpeak_finish
 *     ("tpeak_finish").
 * The true peak keeps its workspace per context it has been called on (the songs' records and 48 bytes per song);
 * bl_amd_ctx_destroy frees it with the context. */
int bl_amd_tpeak_batch_device(const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs, int ceiling, int block,
                              bl_amd_song_tpeak *d_songs_out, uint32_t *d_blocks_out, long long n_blocks,
                              void *stream);
int bl_amd_ctx_tpeak_batch_device(bl_amd_ctx *ctx, const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs,
                                  int ceiling, int block, bl_amd_song_tpeak *d_songs_out, uint32_t *d_blocks_out,
                                  long long n_blocks, void *stream);
int bl_amd_tpeak_batch_host(const int16_t *const *h_pcm, const int32_t *n_samples, const int32_t *channels, int n_songs,
                            int ceiling, int block, bl_amd_song_tpeak *h_songs_out, uint32_t *h_blocks_out);
void bl_amd_tpeak_table(int32_t out[48]);
void bl_amd_tpeak_shape(int *frames_per_lane, int *frames_per_group);
double bl_amd_tpeak_dbtp(const bl_amd_song_tpeak *tp, int channel);
double bl_amd_tpeak_song_dbtp(const bl_amd_song_tpeak *tp);
double bl_amd_tpeak_gain_db(const bl_amd_song_loud *loud, int hop, double target_lufs, const bl_amd_song_tpeak *tp,
                            double ceiling_dbtp);
double bl_amd_tpeak_profile_ms(const char *name, int *launches);

/* Chroma and key: how a song's energy spreads over the twelve pitch classes, and the major or minor key whose profile
 * fits that spread best ("same or compatible key next", the companion of the tempo).  The reference's author lists
 * "Chromagram / HPCP" in ROADMAP.md ("Tonal features"); none of it is in the reference's API.  The 512-point frames of
 * the frequency pass cannot give it (one bin is 43 Hz, a semitone at A3 13 Hz): this is a constant-Q bank of 48
 * pitches, A3 .. G#7, over frames of 4 096 samples at a hop of 2 048.  Every field is an exact integer: all arithmetic
 * below is integer arithmetic and fits 64 bits.  Nominal rate 22 050 Hz.
 *   0 table     data, built on the host once per process (bl_amd_chroma_table shows it).  Pitch p = 0 .. 47,
 *               f_p = B[p % 12] * 2^(p / 12) with B = {220.0, 233.081881, 246.941651, 261.625565, 277.182631,
 *               293.664768, 311.126984, 329.627557, 349.228231, 369.994423, 391.995436, 415.304698};
 *               L_p = 2 floor(374850.0 / f_p) (3 406 for p = 0, 224 for p = 47), n0 = (4096 - L_p) / 2; for n in
 *               [0, L_p): w = 0.5 - 0.5 cos(2 pi (n + 0.5) / L_p), t = f_p (n - L_p/2 + 0.5) / 22050, t -= floor(t),
 *               cr[p][n0 + n] = floor(127 w cos(2 pi t) + 0.5), ci[p][n0 + n] = floor(127 w sin(2 pi t) + 0.5), both
 *               int8, every other entry 0.  Sine and cosine are fixed polynomials in IEEE double + - * / (not libm's:
 *               within 1e-9 of them), so the table is the same bits wherever it is built.  Gain G[p] =
 *               (65536 L_47^2) / L_p^2 in integers (283 for p = 0, 65 536 for p = 47): a tone of a given amplitude
 *               scores alike at every pitch.  Pitch class k(p) = (p + 9) % 12, C = 0.
 *   1 mix       m[i] = l[i] + r[i] (stereo) or 2 s[i] (mono: a mono song and its dual-mono copy give the same bytes).
 *               Fr = n_samples / channels, T = 0 if Fr < 4096, else (Fr - 4096) / 2048 + 1; frame t covers
 *               m[2048 t .. 2048 t + 4095].  No sample outside those frames is read.
 *   2 sums      Re_t[p] = sum_n cr[p][n] m[2048 t + n], Im_t[p] the same with ci: exact
 *   3 energy    a = Re >> 15, b = Im >> 15 (arithmetic shifts: floor), e = a^2 + b^2, E_t[p] = (e G[p]) >> 16
 *   4 fold      X_t[k] = sum of E_t[p] over the four p with k(p) = k: the chromagram
 *   5 song      chroma[k] = sum_t X_t[k]
 *   6 key       mx = max_k chroma[k].  mx == 0 (or T == 0): key = -1, score = score_next = 0.  Otherwise
 *               s = max(0, bitlength(mx) - 12), c[k] = chroma[k] >> s (< 4096); with the Krumhansl-Kessler profiles,
 *               mean-removed, unit-normalised and scaled by 2^14,
 *                 QM = {10737, -4690, -9, -4315, 3361, 2275, -3604, 6394, -4091, 665, -4465, -2256}   (major)
 *                 Qm = {10733, -4215, -775, 6842, -4542, -734, -4788, 4262, 1109, -4174, -1512, -2208} (minor)
 *               score[k] = sum_j QM[j] c[(j + k) % 12], score[12 + k] the same with Qm, k = 0 .. 11; key is the
 *               smallest index with the largest score (0 .. 11 major with tonic C .. B, 12 .. 23 minor), score that
 *               maximum, score_next the largest of the other 23.
 * Bounds: sum_n |cr[p][n]| <= 140 000 for every p, likewise ci (137 652 and 137 690 at most in the table as built), and
 * |m| <= 2^16, so |Re| < 2^33.1, |a| < 2^18.1, e < 2^37.2, E <= e, X < 2^39.2; T < 2^20 (n_samples is an int), so
 * chroma[k] < 2^59.2; |score| < 12 * 10737 * 4096 < 2^29. */
#define BL_AMD_CHROMA_FRAME 4096
#define BL_AMD_CHROMA_HOP 2048
#define BL_AMD_CHROMA_PITCHES 48
typedef struct bl_amd_frame_chroma { uint64_t x[12]; } bl_amd_frame_chroma; /* 96 bytes: X_t[0 .. 11] */
typedef struct bl_amd_song_chroma {                                         /* 128 bytes */
  uint64_t chroma[12];
  int64_t score, score_next;
  int32_t frames;   /* T */
  int32_t key;      /* -1, 0 .. 23 */
  int32_t status;   /* BL_OK; BL_UNEXPECTED for a song with T == 0: frames 0, key -1, everything else 0 */
  int32_t reserved; /* 0 */
} bl_amd_song_chroma;
/* bl_amd_chroma_frames: T of a song, plain host arithmetic; -1 for n_samples < 0 or channels outside {1, 2}.
 * bl_amd_chroma_batch_device: chroma and key of n_songs songs whose PCM sits in device memory.  The descriptors are
 * those of bl_amd_analyze_batch_device with other limits: pcm_offset a multiple of 8, channels 1 or 2, Fr >= 1,
 * duration ignored; d_pcm 16-byte aligned; n_songs >= 1.  d_songs_out: n_songs records in the caller's order.
 * d_frames_out may be NULL (n_frame_records is then ignored); otherwise it receives every frame's record, songs
 * concatenated in the caller's order, song i at the sum of T_j over j < i, and n_frame_records must equal the sum of all
 * T_j.  No output needs zeroing and every byte of every record is written.  A rejected call returns BL_UNEXPECTED and
 * writes nothing.  A song with T == 0 is no error of the call (see status).  Asynchronous on `stream` (the first call
 * of a context uploads the table before it returns); h_desc is copied before the call returns.  Calls of one context
 * are ordered on the device like its batches.  A song's outputs are a pure function of its samples and `channels`:
 * they depend neither on the other songs, n_songs, the order, the launch shape nor on whether the frames are asked for.
 * Read-only towards bl_amd_last_energies and bl_amd_last_freq_stats.
 *   bl_amd_chroma_batch_host: the same from host memory, blocking: the songs are uploaded and analysed in waves;
 *     h_frames_out may be NULL.
 *   bl_amd_chroma_table: copies the bank to host buffers, no device work: re, im [48][4096] (cr, ci), gain [48] (G),
 *     len [48] (L); any pointer may be NULL.
 *   bl_amd_chroma_key_name: "C", "F#" (major), "A#m" (minor) for key 0 .. 23, BL_OK; "" and BL_UNEXPECTED for any
 *     other key (BL_UNEXPECTED alone for a NULL out). */
int bl_amd_chroma_frames(int n_samples, int channels);
int bl_amd_chroma_batch_device(const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs,
                               bl_amd_song_chroma *d_songs_out, bl_amd_frame_chroma *d_frames_out,
                               long long n_frame_records, void *stream);
int bl_amd_ctx_chroma_batch_device(bl_amd_ctx *ctx, const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs,
                                   bl_amd_song_chroma *d_songs_out, bl_amd_frame_chroma *d_frames_out,
                                   long long n_frame_records, void *stream);
int bl_amd_chroma_batch_host(const int16_t *const *h_pcm, const int32_t *n_samples, const int32_t *channels,
                             int n_songs, bl_amd_song_chroma *h_songs_out, bl_amd_frame_chroma *h_frames_out);
int bl_amd_chroma_table(int8_t *re, int8_t *im, uint32_t *gain, int32_t *len);
int bl_amd_chroma_key_name(int key, char out[8]);

/* Fingerprints and offset matching: whether two files are the same recording, and how far one starts before the other.
 * The duplicate groups of bl_amd_groups_* are candidates (two different songs can share a force vector; a re-encode or
 * two seconds more lead-in move it by an unknown amount); a fingerprint settles them.  It is one 32-bit word per chroma
 * frame, made of comparisons of sums of the chromagram only, so a gain change cancels except through the chroma
 * stage's own flooring.  Every quantity is an exact integer.
 *   words    A song with T chroma frames X_t[0 .. 11] (bl_amd_frame_chroma) has W = max(0, T - 15) words.  Word t is
 *            built from frames t .. t + 15; per pitch class k: S1[k] = sum of X[k] over frames t .. t + 7, S2[k] the
 *            same over t + 8 .. t + 15, A[k] = S1[k] + S2[k].  X < 2^39.2, so every sum below is under 2^45.  All
 *            comparisons are strict: a tie is 0 and a silent window is the word 0.
 *              bit k,      k = 0 .. 11: S2[k] > S1[k]                                       (is the class rising?)
 *              bit 12 + k, k = 0 .. 11: A[k] > A[(k + 1) % 12]                              (spectral slope, wrapping)
 *              bit 24 + k, k = 0 .. 7:  S1[k] + S2[(k + 1) % 12] > S2[k] + S1[(k + 1) % 12] (checkerboard)
 *   match    Word sequences a (Wa words) and b (Wb words), an offset d in [-D, D], D = max_shift: the overlap is the i
 *            with 0 <= i < Wa and 0 <= i + d < Wb, n(d) its size, e(d) = sum over it of popcount(a[i] ^ b[i + d]).
 *            An offset is a candidate when n(d) >= min_overlap (>= 1, so an empty overlap never is).  s(d) =
 *            floor(e(d) 65536 / n(d)) (<= 2^21), r(d) = 2 |d| - (d < 0) (0, -1, +1, -2, .. in that order); the best
 *            offset is the candidate with the smallest 64-bit key s(d) 2^32 + r(d): fewest errors per word, then the
 *            smallest shift, then the negative one.  A positive d means b carries d more words of lead-in than a: a
 *            copy of a with its first 5 hops cut off matches at d = -5.
 * Bounds: T < 2^20, so e < 2^25; D <= BL_AMD_FPRINT_SHIFT_MAX (about 95 s). */
#define BL_AMD_FPRINT_FRAMES 16
#define BL_AMD_FPRINT_SHIFT_MAX 1024
typedef struct bl_amd_fprint_match { /* 24 bytes */
  uint32_t errors;  /* e(d) of the best offset */
  uint32_t overlap; /* n(d) */
  int32_t offset;   /* d */
  uint32_t score;   /* s(d) */
  int32_t status;   /* BL_OK; BL_UNEXPECTED when no offset is a candidate or a pair index lies outside its set: score
                       0xFFFFFFFF, errors, overlap, offset 0 */
  int32_t reserved; /* 0 */
} bl_amd_fprint_match;
/* bl_amd_fprint_words: W of a song with `frames` chroma frames, plain host arithmetic; -1 for frames < 0.
 * bl_amd_fprint_words_device: the words of n_songs songs.  d_frames is what bl_amd_chroma_batch_device wrote: the
 *   songs' frame records concatenated, song i at the sum of T_j over j < i, h_frames[i] = T_i (0 <= T_i < 2^20).  The
 *   words are concatenated the same way, song i at the sum of W_j over j < i, and n_words must equal the sum of all
 *   W_j (it may be 0; d_words_out is needed all the same).  Every word is written; nothing needs zeroing.  A song's
 *   words depend on its own frames only; no frame of another song is read.
 * bl_amd_fprint_words_host: the same from host memory, blocking.
 * bl_amd_fprint_match_device: one record per pair.  Set a is n_a songs' words concatenated (d_words_a, h_count_a[i]
 *   words each, 0 <= count < 2^20), set b likewise; the self form passes one set twice.  d_pairs is n_pairs x 2 int32
 *   on the device: an index into set a, then one into set b; the kernel range-checks them (see status) and reads
 *   nothing through a bad one.  0 <= max_shift <= BL_AMD_FPRINT_SHIFT_MAX, min_overlap >= 1.  d_profile_out may be
 *   NULL; otherwise it receives (e(d), n(d)) as two uint32 for every pair and every d = -D .. D, non-candidates
 *   included: n_pairs (2 D + 1) 2 values, all 0 for a pair with a bad index.  Every byte of every record and of the
 *   profile is written.  A pair's record depends on its two sequences, max_shift and min_overlap only: not on the other
 *   pairs, their order, n_pairs, the launch shape or whether the profile is asked for; no word outside the two
 *   sequences is read.
 * bl_amd_fprint_match_host: the same with everything in host memory, blocking.
 * A rejected call returns BL_UNEXPECTED and writes nothing: a NULL required pointer, a misaligned pointer (the frame
 * records 8, everything else 4 bytes), n_songs, n_a, n_b or n_pairs < 1, a count outside [0, 2^20), a wrong n_words,
 * max_shift or min_overlap out of range.  The device forms are asynchronous on `stream`; the host arrays are copied
 * before the call returns.  The fingerprints keep their workspace per context they have been called on (32 bytes per
 * song of a words call, 16 per song of the two sets of a match); bl_amd_ctx_destroy frees it with the context.
 * Host arithmetic, no device:
 *   bl_amd_fprint_shape: the lengths at which the kernels change path, for tests: the words one workgroup of the words
 *     kernel owns (256); for the match at max_shift (clamped to its range) the words of `a` a lane walks per tile (64),
 *     the words of `a` per tile (64 to 2 048) and the offsets a workgroup takes at a time (a multiple of 4).  Any
 *     pointer may be NULL.  The match has one launch shape.
 *   bl_amd_fprint_ber: errors / (32 overlap), the bit-error rate at the best offset; NaN for a NULL record or a failed
 *     status.
 *   bl_amd_fprint_offset_seconds: offset 2048 / rate; NaN for a NULL record, a failed status or rate < 1.
 *   bl_amd_fprint_profile_ms: as bl_amd_tpeak_profile_ms, for k_fprint_words ("fprint_words") and k_fprint_match
 *     ("fprint_match"). */
int bl_amd_fprint_words(int frames);
int bl_amd_fprint_words_device(const bl_amd_frame_chroma *d_frames, const int32_t *h_frames, int n_songs,
                               uint32_t *d_words_out, long long n_words, void *stream);
int bl_amd_ctx_fprint_words_device(bl_amd_ctx *ctx, const bl_amd_frame_chroma *d_frames, const int32_t *h_frames,
                                   int n_songs, uint32_t *d_words_out, long long n_words, void *stream);
int bl_amd_fprint_words_host(const bl_amd_frame_chroma *h_frame_records, const int32_t *h_frames, int n_songs,
                             uint32_t *h_words_out);
int bl_amd_fprint_match_device(const uint32_t *d_words_a, const int32_t *h_count_a, int n_a, const uint32_t *d_words_b,
                               const int32_t *h_count_b, int n_b, const int32_t *d_pairs, int n_pairs, int max_shift,
                               int min_overlap, bl_amd_fprint_match *d_out, uint32_t *d_profile_out, void *stream);
int bl_amd_ctx_fprint_match_device(bl_amd_ctx *ctx, const uint32_t *d_words_a, const int32_t *h_count_a, int n_a,
                                   const uint32_t *d_words_b, const int32_t *h_count_b, int n_b,
                                   const int32_t *d_pairs, int n_pairs, int max_shift, int min_overlap,
                                   bl_amd_fprint_match *d_out, uint32_t *d_profile_out, void *stream);
int bl_amd_fprint_match_host(const uint32_t *h_words_a, const int32_t *h_count_a, int n_a, const uint32_t *h_words_b,
                             const int32_t *h_count_b, int n_b, const int32_t *h_pairs, int n_pairs, int max_shift,
                             int min_overlap, bl_amd_fprint_match *h_out, uint32_t *h_profile_out);
void bl_amd_fprint_shape(int max_shift, int *words_block, int *strip_words, int *tile_words, int *chunk_offsets);
double bl_amd_fprint_ber(const bl_amd_fprint_match *m);
double bl_amd_fprint_offset_seconds(const bl_amd_fprint_match *m, int rate);
double bl_amd_fprint_profile_ms(const char *name, int *launches);

/* Song structure: where the part that comes back is, and where the sections change.  Tempo, key, loudness and
 * fingerprints describe a whole song or line two songs up; this block looks inside one song.  It reads the chroma frames
 * (the feature the thumbnailing method of Bartsch and Wakefield, "To catch a chorus", 2001, is defined on) and gives
 * the start and lag of the most strongly repeated stretch of a chosen length, as sums along the diagonals of the
 * self-similarity matrix, and a checkerboard novelty curve (Foote) with the section boundaries picked from it.  All
 * quantities are integers.  No result depends on launch shape, reduction order, batch composition, or which optional
 * outputs are requested.
 *   input    As for bl_amd_fprint_words_device: d_frames holds the songs' chroma frame records concatenated, song i at
 *            the sum of T_j over j < i, h_frames[i] = T_i, 0 <= T_i < 2^20; X_t[k] < 2^39.2 by the chroma block's bound.
 *   params   bl_amd_form_params, passed by pointer: pool P in 1 .. 16, seg M in 2 .. 1024, min_lag in 1 ..
 *            BL_AMD_FORM_UNITS_MAX, nov L in 1 .. 64, 0 <= peak_num <= peak_den, 1 <= peak_den <= 256, reserved 0.
 *   units    U = floor(T / P); trailing frames that do not fill a unit are dropped.  For unit u: Y[k] = sum over j < P
 *            of X_{uP+j}[k] (below 2^43.2); m = max over k of Y[k].  m = 0: the unit is silent, q_u = 0.  Otherwise
 *            s = max(0, bitlength(m) - 20), y[k] = Y[k] >> s (below 2^20), r = bl_isqrt64(sum of y[k]^2) (the sum is
 *            below 2^44, r >= 1), q_u[k] = floor(127 y[k] / r), in 0 .. 127.  A unit is 16 bytes: the twelve q as int8
 *            and four zero bytes.  The similarity is S(u, v) = sum over k of q_u[k] q_v[k], 0 <= S <= 16129.
 *   thumb    With minlag = min_lag: lags l run over [minlag, U - M], starts u over [0, U - M - l], and
 *            F(u, l) = sum over j < M of S(u + j, u + l + j), below 2^24.  The song's thumbnail is the pair with the
 *            largest 64-bit key F 2^40 + (2^20 - 1 - l) 2^20 + (2^20 - 1 - u): the most similar pair of stretches, then
 *            the smaller lag, then the earlier start.  If U < M + minlag, or the best F is 0, the song has no
 *            thumbnail: status has BL_AMD_FORM_NO_THUMB and the four thumbnail fields are 0.  thumb_self = sum over
 *            j < M of S(u* + j, u* + j), so that thumb_score / thumb_self is a figure near 0 .. 1.  Optional per-unit
 *            output rep[u] = (R, l), two uint32: R the largest F(u, l) over the valid l, l the smallest lag that
 *            reaches it; (0, 0) where no l is valid or R = 0.
 *   novelty  Weights w_a = L + 1 - a for a = 1 .. L.  For u in [L, U - L]: P_u[k] = sum over a of w_a q_{u-a}[k],
 *            G_u[k] = sum over a of w_a q_{u+a-1}[k], N(u) = sum over k of (P_u[k] - G_u[k])^2: Foote's checkerboard
 *            kernel with a separable triangular taper, which collapses to the squared distance between the tapered sum
 *            of the L units before u and of the L units from u on.  Each component is below 2^19, N < 2^40, a uint64.
 *            N(u) = 0 for u outside that range.  Nmax is the largest value, nov_max_unit the first u that attains it
 *            (0 when Nmax = 0).  Unit u is a boundary when N(u) > 0, N(u) peak_den >= Nmax peak_num, N(v) < N(u) for v
 *            in [u - L, u) and N(v) <= N(u) for v in (u, u + L], both ranges clipped to [0, U): the first unit of a
 *            plateau wins.
 *   limits   BL_AMD_FORM_UNITS_MAX = 8192: 16 bytes x 8 192 = 128 KB, one song's units in one workgroup's LDS.  A song
 *            with more units has status BL_AMD_FORM_TOO_LONG | BL_AMD_FORM_NO_THUMB and every other field 0 but
 *            `units`; its units are written, its rep, novelty and flags are 0.  The call still succeeds for the
 *            others.  Callers pool such songs with a larger P. */
#define BL_AMD_FORM_UNITS_MAX 8192
#define BL_AMD_FORM_NO_THUMB 1
#define BL_AMD_FORM_TOO_LONG 2
typedef struct bl_amd_form_params { /* 28 bytes */
  int32_t pool;     /* P */
  int32_t seg;      /* M */
  int32_t min_lag;  /* minlag */
  int32_t nov;      /* L */
  int32_t peak_num, peak_den;
  int32_t reserved; /* must be 0 */
} bl_amd_form_params;
typedef struct bl_amd_song_form { /* 48 bytes, every byte written for every song */
  int32_t units;        /* U, whatever the status: the song's share of the per-unit outputs */
  int32_t status;       /* 0, or the OR of BL_AMD_FORM_NO_THUMB and BL_AMD_FORM_TOO_LONG */
  int32_t thumb_start;  /* u* */
  int32_t thumb_lag;    /* l* */
  uint32_t thumb_score; /* F(u*, l*) */
  uint32_t thumb_self;
  int32_t boundaries;   /* the number of boundary units */
  int32_t nov_max_unit;
  uint64_t nov_max;     /* Nmax */
  uint64_t reserved;    /* 0 */
} bl_amd_song_form;
/* bl_amd_form_device: one record per song in d_out.  The optional outputs may each be NULL; each is concatenated at the
 *   sum of U_j over j < i and every element is written: d_units_out (16 bytes per unit), d_rep_out (2 x uint32 per
 *   unit), d_nov_out (uint64 per unit), d_flags_out (uint8 per unit, bit 0 = boundary).  n_units is always passed and
 *   must equal the sum of all U_j (it may be 0).  No unit or frame of another song is read.  Asynchronous on `stream`;
 *   the host arrays and the parameters are copied before the call returns.
 * bl_amd_ctx_form_device: the same on an explicit context.  bl_amd_form_host: everything in host memory, blocking.
 * A rejected call returns BL_UNEXPECTED and writes nothing: a NULL required pointer (frames, counts, parameters,
 * records), a misaligned pointer (frame records, novelty and records 8 bytes, units 16, rep 4), n_songs < 1, a count
 * outside [0, 2^20), a wrong n_units, any parameter out of range, a reserved word that is not 0.  The workspace is kept
 * per context (32 bytes per song, and 16 or 8 bytes per unit where the units or the novelty are not asked for);
 * bl_amd_ctx_destroy frees it with the context.
 * Host arithmetic, no device:
 *   bl_amd_form_units: U = floor(frames / pool); -1 for frames < 0 or pool outside 1 .. 16.
 *   bl_amd_form_seconds: unit pool 2048 / rate, the time at which a unit starts; NaN for unit < 0, a bad pool, rate < 1.
 *   bl_amd_form_score: thumb_score / thumb_self; NaN for a NULL record, one without a thumbnail or thumb_self = 0.
 *   bl_amd_form_shape: the lengths at which the kernels change path, for tests: the lags one workgroup of the thumbnail
 *     kernel takes at a time, and the units one workgroup of the units kernel owns.  Either pointer may be NULL.
 *   bl_amd_form_profile_ms: as bl_amd_fprint_profile_ms, for "form_units", "form_thumb" and "form_novelty". */
int bl_amd_form_device(const bl_amd_frame_chroma *d_frames, const int32_t *h_frames, int n_songs,
                       const bl_amd_form_params *params, bl_amd_song_form *d_out, void *d_units_out,
                       uint32_t *d_rep_out, uint64_t *d_nov_out, uint8_t *d_flags_out, long long n_units, void *stream);
int bl_amd_ctx_form_device(bl_amd_ctx *ctx, const bl_amd_frame_chroma *d_frames, const int32_t *h_frames, int n_songs,
                           const bl_amd_form_params *params, bl_amd_song_form *d_out, void *d_units_out,
                           uint32_t *d_rep_out, uint64_t *d_nov_out, uint8_t *d_flags_out, long long n_units,
                           void *stream);
int bl_amd_form_host(const bl_amd_frame_chroma *h_frame_records, const int32_t *h_frames, int n_songs,
                     const bl_amd_form_params *params, bl_amd_song_form *h_out, void *h_units_out, uint32_t *h_rep_out,
                     uint64_t *h_nov_out, uint8_t *h_flags_out);
int bl_amd_form_units(int frames, int pool);
double bl_amd_form_seconds(int unit, int pool, int rate);
double bl_amd_form_score(const bl_amd_song_form *f);
void bl_amd_form_shape(int *chunk_lags, int *units_block);
double bl_amd_form_profile_ms(const char *name, int *launches);

/* Versions: whether two files are the same piece in another recording, which is what none of the calls above can say.
 * A live take, a remaster at another speed, a cover in another key and an edit with a different intro are far apart as
 * fingerprints (on purpose: those compare frame by frame at a fixed offset) and may be far apart as descriptors.  This
 * block aligns the two songs' chroma sequences: a local alignment (Smith-Waterman) over their cross-similarity matrix,
 * after one of them has been rotated to the other's key.  It tolerates a key change, a tempo change and extra or
 * missing material.  Every quantity is an exact integer; no result depends on launch shape, pair order, batch
 * composition, the context, or whether the self or the cross form is used.  The definition separates synthetic chord
 * songs; it has not been tuned on recorded music.
 *   units    Those of the structure call: 16 bytes, the twelve q in 0 .. 127 and four zero bytes, U = floor(T / pool).
 *            bl_amd_cover_units_device writes them and nothing else; its bytes equal d_units_out of bl_amd_form_device
 *            at the same pool.
 *   sets     As for bl_amd_fprint_match_device: set a is n_a songs' units concatenated (d_units_a, h_count_a[i] units
 *            each, 0 <= count < 2^20), set b likewise; the self form passes one set twice.  d_pairs is n_pairs x 2 int32
 *            on the device: an index into a, then one into b; the kernel range-checks both and reads nothing through a
 *            bad one.
 *   params   bl_amd_cover_params, passed by pointer: thr in 1 .. 16128, gap in 0 .. 2^20, transpose in -1 .. 11,
 *            reserved 0.
 *   transp.  g_x[k] = sum over the units of song x of q[k] (below 2^20).  C(r) = sum over k of g_a[k] g_b[(k + r) mod 12]
 *            (below 2^44).  With transpose = -1, r is the smallest r in 0 .. 11 that attains the largest C; otherwise
 *            r = transpose.  A positive r means b sounds r semitones above a.
 *   simil.   S(i, j) = sum over k of q_a,i[k] q_b,j[(k + r) mod 12], in 0 .. 16129; w(i, j) = S(i, j) - thr.
 *   align    For 0 <= i < Ua, 0 <= j < Ub, with H(-1, .) = H(., -1) = 0:
 *              d = H(i-1, j-1) + w(i, j),  u = H(i-1, j) - gap,  l = H(i, j-1) - gap,  H(i, j) = max(0, d, u, l).
 *            H <= 16129 x 8192 < 2^27.
 *   origin   O(i, j) is defined where H(i, j) > 0; the first rule that applies decides.  If d = H(i, j): (i, j) when
 *            H(i-1, j-1) = 0 (the path starts here), otherwise O(i-1, j-1).  Else if u = H(i, j): O(i-1, j).  Otherwise
 *            O(i, j-1).  The diagonal is preferred over up, and up over left.
 *   best     The cell with the largest 64-bit key H 2^26 + (8191 - i) 2^13 + (8191 - j): the largest score, then the
 *            smaller i, then the smaller j.  The aligned stretch is from that cell's origin to the cell, inclusive.
 *   status   0, or an OR of BL_AMD_COVER_NO_MATCH (the best H is 0, which includes an empty song: the units are
 *            written, the transposition where both songs have units, the rest is 0), BL_AMD_COVER_TOO_LONG (a song has
 *            more than BL_AMD_FORM_UNITS_MAX units: the units are written, the rest is 0; the other pairs still
 *            succeed) and BL_AMD_COVER_BAD_INDEX (a pair index outside its set: everything else is 0).
 * Out of scope: trying all twelve transpositions, a traceback of the path, tuning on recorded music. */
#define BL_AMD_COVER_NO_MATCH 1
#define BL_AMD_COVER_TOO_LONG 2
#define BL_AMD_COVER_BAD_INDEX 4
typedef struct bl_amd_cover_params { /* 16 bytes */
  int32_t thr;       /* what a pair of units must reach to count for the alignment */
  int32_t gap;       /* what a step along one song alone costs */
  int32_t transpose; /* -1: found from the profiles; 0 .. 11: given */
  int32_t reserved;  /* must be 0 */
} bl_amd_cover_params;
typedef struct bl_amd_cover_match { /* 40 bytes, every byte written for every pair */
  uint32_t score;    /* H of the best cell */
  int32_t a_start;   /* the origin's i */
  int32_t a_end;     /* the best cell's i */
  int32_t b_start;   /* the origin's j */
  int32_t b_end;     /* the best cell's j */
  int32_t transpose; /* r */
  int32_t units_a;   /* Ua */
  int32_t units_b;   /* Ub */
  int32_t status;
  int32_t reserved;  /* 0 */
} bl_amd_cover_match;
/* bl_amd_cover_units_device: the units of n_songs songs; d_frames, h_frames and the counts' rules are those of
 *   bl_amd_form_device, pool is in 1 .. 16, n_units must equal the sum of all U (it may be 0; d_units_out is needed all
 *   the same, 16-byte aligned).  bl_amd_ctx_cover_units_device: the same on an explicit context.
 *   bl_amd_cover_units_host: from host memory, blocking.
 * bl_amd_cover_match_device: one record per pair.  A pair's record depends on its two sequences and the three
 *   parameters only; no unit outside the two sequences is read.  Asynchronous on `stream`; the host arrays and the
 *   parameters are copied before the call returns.  bl_amd_ctx_cover_match_device: on an explicit context.
 *   bl_amd_cover_match_host: everything in host memory, blocking.
 * A rejected call returns BL_UNEXPECTED and writes nothing: a NULL required pointer, a misaligned pointer (frame records
 * and pairs 8 bytes, units 16, records 4), n_songs, n_a, n_b or n_pairs < 1, a count outside [0, 2^20), a wrong n_units,
 * a parameter out of range, a reserved word that is not 0.  The workspace is kept per context (32 bytes per song of a
 * units call; 16 + 48 bytes per song of the two sets of a match); bl_amd_ctx_destroy frees it with the context.
 * Host arithmetic, no device:
 *   bl_amd_cover_score: score / ((16129 - thr) min(units_a, units_b)), the share of the shorter song that aligns
 *     perfectly; NaN for a NULL record, a status other than 0 or a denominator that is not positive.
 *   bl_amd_cover_seconds: unit pool 2048 / rate, as bl_amd_form_seconds.
 *   bl_amd_cover_tempo_ratio: (b_end - b_start + 1) / (a_end - a_start + 1): how much longer b takes over the aligned
 *     stretch; NaN for a NULL record or a status other than 0.
 *   bl_amd_cover_shape: the lengths at which the alignment changes path, for tests: the columns of b one wavefront owns
 *     at a time and the rows of a it fetches at a time.  Either pointer may be NULL.
 *   bl_amd_cover_profile_ms: as bl_amd_fprint_profile_ms, for "cover_profile" and "cover_align". */
int bl_amd_cover_units_device(const bl_amd_frame_chroma *d_frames, const int32_t *h_frames, int n_songs, int pool,
                              void *d_units_out, long long n_units, void *stream);
int bl_amd_ctx_cover_units_device(bl_amd_ctx *ctx, const bl_amd_frame_chroma *d_frames, const int32_t *h_frames,
                                  int n_songs, int pool, void *d_units_out, long long n_units, void *stream);
int bl_amd_cover_units_host(const bl_amd_frame_chroma *h_frame_records, const int32_t *h_frames, int n_songs, int pool,
                            void *h_units_out);
int bl_amd_cover_match_device(const void *d_units_a, const int32_t *h_count_a, int n_a, const void *d_units_b,
                              const int32_t *h_count_b, int n_b, const int32_t *d_pairs, int n_pairs,
                              const bl_amd_cover_params *params, bl_amd_cover_match *d_out, void *stream);
int bl_amd_ctx_cover_match_device(bl_amd_ctx *ctx, const void *d_units_a, const int32_t *h_count_a, int n_a,
                                  const void *d_units_b, const int32_t *h_count_b, int n_b, const int32_t *d_pairs,
                                  int n_pairs, const bl_amd_cover_params *params, bl_amd_cover_match *d_out,
                                  void *stream);
int bl_amd_cover_match_host(const void *h_units_a, const int32_t *h_count_a, int n_a, const void *h_units_b,
                            const int32_t *h_count_b, int n_b, const int32_t *h_pairs, int n_pairs,
                            const bl_amd_cover_params *params, bl_amd_cover_match *h_out);
double bl_amd_cover_score(const bl_amd_cover_match *m, int thr);
double bl_amd_cover_seconds(int unit, int pool, int rate);
double bl_amd_cover_tempo_ratio(const bl_amd_cover_match *m);
void bl_amd_cover_shape(int *strip_columns, int *row_block);
double bl_amd_cover_profile_ms(const char *name, int *launches);

/* Chords: which chord sounds when, which is what none of the calls above can say.  The key is one label for a whole
 * song and the structure call's boundaries are novelty peaks without a name.  This block labels every unit of a song
 * with one of 24 triads or "no chord": triad templates over the unit's twelve chroma values, decoded by Viterbi with a
 * caller-given table of transition costs, so that a label holds until the evidence against it outweighs a change.
 * Every quantity is an exact integer and ties are part of the definition; no result depends on launch shape, batch
 * composition, the context, or which optional outputs are asked for.  The defaults (none 150, change 60, related 15)
 * label synthetic triad progressions, silence and noise correctly; there is no annotated music here,
 * so they have not been tuned on recorded music.
 *   units    As set a of bl_amd_cover_match_device: d_units is n_songs songs' units concatenated, 16 bytes each (the
 *            twelve q in 0 .. 127 and four zero bytes), 16-byte aligned; h_count[i] = U_i units, 0 <= U_i < 2^20;
 *            n_units is the sum of all U_i and may be 0.  There is no TOO_LONG: nothing of a song has to fit LDS.
 *   labels   0 .. 11 the major triads on C .. B, 12 .. 23 the minor triads (the numbering of bl_amd_song_chroma.key),
 *            24 "no chord" (N).
 *   emission Of unit t, with q its twelve values:
 *              E_t[r]      = q[r] + q[(r + 4) mod 12] + q[(r + 7) mod 12]   (major, r = 0 .. 11)
 *              E_t[12 + r] = q[r] + q[(r + 3) mod 12] + q[(r + 7) mod 12]   (minor)
 *              E_t[24]     = none
 *            in 0 .. 381.  A silent unit goes to N for any none > 0.
 *   costs    cost[a][b], 25 x 25 uint16 in 0 .. 1024: what going from label a to label b costs.  It is used as given,
 *            the diagonal included.
 *   scores   V_0[c] = E_0[c];  for t >= 1: V_t[c] = E_t[c] + max over a of (V_{t-1}[a] - cost[a][c]), and B_t[c] is the
 *            smallest a that attains the maximum.  Taking a = argmax V_{t-1} shows max V_t >= max V_{t-1} - 1024 and the
 *            emission max V_t <= max V_{t-1} + 381, so with t < 2^20: -2^30 < V < 381 x 2^20 < 2^29, |V| < 2^31.
 *   trace    L_{U-1} is the smallest c with the largest V_{U-1}[c], and that value the record's score;
 *            L_{t-1} = B_t[L_t]. */
#define BL_AMD_CHORDS_LABELS 25
#define BL_AMD_CHORDS_NONE 24
#define BL_AMD_CHORDS_EMPTY 1
#define BL_AMD_CHORDS_COST_MAX 1024
#define BL_AMD_CHORDS_EMISSION_MAX 381
typedef struct bl_amd_chords_params { /* 1264 bytes */
  int32_t none;       /* E[24], in 0 .. 381 */
  int32_t reserved;   /* must be 0 */
  uint16_t cost[625]; /* [a][b], row-major, each in 0 .. 1024 */
  uint16_t pad[3];    /* must be 0 */
} bl_amd_chords_params;
typedef struct bl_amd_song_chords { /* 32 bytes, every byte written for every song */
  int32_t units;      /* U */
  int32_t status;     /* 0, or BL_AMD_CHORDS_EMPTY for U = 0 */
  int32_t score;      /* V_{U-1}[L_{U-1}] */
  int32_t changes;    /* the number of t >= 1 with L_t != L_{t-1} */
  int32_t top;        /* the label with the most units, the smaller label of equals; -1 for an empty song */
  int32_t top_units;
  int32_t none_units; /* the units labelled 24 */
  int32_t reserved;   /* 0 */
} bl_amd_song_chords; /* an empty song has every field but status and top equal to 0 */
/* bl_amd_chords_device: one record per song in d_out.  The optional outputs may each be NULL, and every element is
 *   written where given: d_labels_out (uint8 per unit, concatenated at the sum of U_j over j < i) and d_hist_out (25
 *   uint32 per song: the units per label).  A song's record and outputs depend on its own units and the parameters
 *   only; no unit of another song is read.  Asynchronous on `stream`; the host array and the parameters are copied
 *   before the call returns.  bl_amd_ctx_chords_device: the same on an explicit context.  bl_amd_chords_host:
 *   everything in host memory, blocking.
 * A rejected call returns BL_UNEXPECTED and writes nothing: a NULL required pointer (units, counts, parameters,
 * records), a misaligned pointer (units 16 bytes, records and hist 4), n_songs < 1, a count outside [0, 2^20), a wrong
 * n_units, none or a cost out of range, a reserved or pad word that is not 0.  These checks come before any context or
 * device is touched.  The workspace is kept per context (1264 bytes, 32 bytes per song, and the backpointers: 32 bytes
 * per unit, one byte per label, a song's units rounded up to a multiple of 4); bl_amd_ctx_destroy frees it with the
 * context.
 * Host arithmetic, no device:
 *   bl_amd_chords_costs: the table with 0 on the diagonal, `change` to and from N, and between two chords
 *     change - related x (the pitch classes the two triads share: 0, 1 or 2).  BL_UNEXPECTED, and nothing written,
 *     unless cost_out is given and 0 <= 2 related <= change <= 1024.
 *   bl_amd_chords_name: "C" .. "B", "Cm" .. "Bm", "N", and "" for any other label.  The strings are static.
 *   bl_amd_chords_segments: the runs of equal labels among `units` labels.  Returns their number (-1 for NULL labels
 *     with units > 0, units < 0 or cap < 0) and writes the first unit and the label of the first `cap` of them
 *     (either array may be NULL).  A unit's time is bl_amd_form_seconds.
 *   bl_amd_chords_shape: the lengths at which the kernels change path, for tests: the units the forward kernel takes
 *     at a time, the units the back-trace takes at a time, and the songs that share a wavefront of the forward kernel.
 *     Any pointer may be NULL.
 *   bl_amd_chords_profile_ms: as bl_amd_form_profile_ms, for "chords_forward" and "chords_trace".
 * Out of scope: sevenths, inversions and other chord types; beat-synchronous units (a caller pools as usual); learning
 * the costs from annotated music. */
int bl_amd_chords_device(const void *d_units, const int32_t *h_count, int n_songs, long long n_units,
                         const bl_amd_chords_params *params, bl_amd_song_chords *d_out, uint8_t *d_labels_out,
                         uint32_t *d_hist_out, void *stream);
int bl_amd_ctx_chords_device(bl_amd_ctx *ctx, const void *d_units, const int32_t *h_count, int n_songs,
                             long long n_units, const bl_amd_chords_params *params, bl_amd_song_chords *d_out,
                             uint8_t *d_labels_out, uint32_t *d_hist_out, void *stream);
int bl_amd_chords_host(const void *h_units, const int32_t *h_count, int n_songs,
                       const bl_amd_chords_params *params, bl_amd_song_chords *h_out, uint8_t *h_labels_out,
                       uint32_t *h_hist_out);
int bl_amd_chords_costs(int change, int related, uint16_t *cost_out);
const char *bl_amd_chords_name(int label);
int bl_amd_chords_segments(const uint8_t *labels, int units, int32_t *starts_out, uint8_t *chords_out, int cap);
void bl_amd_chords_shape(int *forward_units, int *trace_units, int *songs_per_wave);
double bl_amd_chords_profile_ms(const char *name, int *launches);

/* Mel bands, cepstrum and flatness: the shape of every frame's spectrum.  The centroid and the rolloff of the timbre
 * block say where a frame's power sits and where it stops; the 32 log-mel band levels say how it is spread, the 13
 * cepstral coefficients (MFCC) are the usual compact description of that spread, and the flatness tells noise from
 * tone.  The reference's author lists "MFCC" and "spectral flatness" in ROADMAP.md ("Timbral features"); none of it is
 * in the reference's API.  The band levels of all frames are the log-mel spectrogram a learned model takes as input.
 * Every field is an exact integer, defined by the algorithms below and not by libm.
 * Frames, P_t[d], Q_t[d] = floor(16 P_t[d]) (uint64, d = 1 .. 255, their sum below 2^50) and energy = sum_d Q_t[d] are
 * exactly those of the timbre block above.
 *   edges    34 integers in sixteenths of a bin, equally spaced on the mel scale 2595 log10(1 + f / 700) from bin 1 to
 *            bin 256 of the 512-point transform at 22 050 Hz, rounded to nearest:
 *              16 40 66 95 126 159 196 236 279 326 377 432 493 558 630 707 792 883 983 1091 1209 1337 1477 1628 1793
 *              1972 2166 2378 2608 2858 3130 3425 3747 4096
 *   weights  32 triangular bands.  With x = 16 d and (a, c, z) = (e[b], e[b+1], e[b+2]), in integer floor divisions:
 *              W[b][d] = (64 (x - a)) / (c - a)  for a < x <= c
 *              W[b][d] = (64 (z - x)) / (z - c)  for c < x < z,   0 otherwise.
 *            Every band has 3 to 41 non-zero weights, no bin feeds more than two bands, a column sums to at most 64 and
 *            that of bin 1 (where a DC offset leaks to under the Hann window) to 0; the row sums run from 90 to 1320.
 *   sums     S_t[b] = sum_d W[b][d] Q_t[d], a uint64, at most 64 * 2^50 = 2^56
 *   log      L(x), 1 <= x < 2^64: log2 x in 1/4096, DEFINED by: e = floor(log2 x); m = x << (30 - e) if e <= 30, else
 *            x >> (e - 30), so 2^30 <= m < 2^31; acc = e; twelve times: t = (m m) >> 30, bit = t >> 31, m = t >> bit,
 *            acc = 2 acc + bit; L = acc.  L(1) = 0, L(2) = 4096, L(3) = 6492, L(2^63) = 258048;
 *            0 <= 4096 log2 x - L(x) < 1 + 2^-10, and L is non-decreasing.
 *   levels   E_t[b] = L(S_t[b] + 1): the log-mel frame, 0 <= E < 2^18
 *   cepstrum D[k][b] = floor(16384 cos(pi k (2 b + 1) / 64) + 0.5), k = 0 .. 12, the cosine the portable polynomial of
 *            the chroma bank at (k (2 b + 1) mod 128) / 128 of a turn (bl_amd_mel_table shows the result);
 *            mfcc_t[k] = floor((sum_b D[k][b] E_t[b]) / 2^14), an arithmetic shift of an int64; |mfcc| < 2^23
 *   flatness T = sum_b (S_t[b] + 1) < 2^57, G = sum_b E_t[b], flat_t = 32 L(T) - 160 * 4096 - G: 32 * 4096 times the
 *            log2 of the ratio of the arithmetic to the geometric mean of the 32 values S + 1.  0 for digital silence
 *            and for a flat band spectrum, growing with tonality; slightly negative values occur because L truncates.
 * Per song: a frame is USED iff energy > 0 and energy >= min_energy (the timbre's rule); the sums run over the used
 * frames.  The sums of squares are exact below 2^64, which |value| < 2^23 guarantees for 2^18 used frames (1.7 hours
 * at 22 050 Hz) whatever the signal; beyond that they are taken modulo 2^64. */
#define BL_AMD_MEL_BANDS 32
#define BL_AMD_MEL_COEFFS 13
typedef struct bl_amd_frame_mel { /* 56 bytes */
  int32_t mfcc[13];
  int32_t flat;
} bl_amd_frame_mel;
typedef struct bl_amd_song_mel { /* 496 bytes */
  int64_t mfcc_sum[13];
  uint64_t mfcc_sumsq[13];
  int64_t flat_sum;
  uint64_t flat_sumsq;
  uint64_t band_sum[32]; /* the sums of E_t[b] */
  int32_t frames;        /* F */
  int32_t used;
  int32_t status;        /* BL_OK */
  int32_t reserved;      /* 0 */
} bl_amd_song_mel;
/* bl_amd_mel_frames: F of a song (that of bl_amd_timbre_frames); -1 for n_samples < 0 or channels outside {1, 2}.
 * bl_amd_mel_batch_device: the mel records of n_songs songs whose PCM sits in device memory.  The descriptors are those
 * of bl_amd_analyze_batch_device with the timbre's limits: pcm_offset a multiple of 8, channels 1 or 2, F >= 1,
 * duration ignored; d_pcm 16-byte aligned; n_songs >= 1.  d_songs_out: n_songs records in the caller's order.
 * d_frames_out (one bl_amd_frame_mel per frame) and d_bands_out (32 uint32 per frame: E_t[0 .. 31], the log-mel
 * spectrogram) may each be NULL; either receives every frame, songs concatenated in the caller's order, song i at the
 * sum of F_j over j < i, and if one of them is given n_frame_records must equal the sum of all F_j (it is ignored
 * when both are NULL).  No output needs zeroing.  A rejected call returns BL_UNEXPECTED and writes nothing.
 * Asynchronous on `stream`; h_desc is copied before the call returns.  Calls of one context are ordered on the device
 * like its batches.  A song's records are a pure function of its samples, `channels` and min_energy: they depend
 * neither on the other songs, n_songs, the order, the launch shape nor on which of the frame outputs are asked for,
 * and no sample outside the song's whole frames is read.  Read-only towards bl_amd_last_energies and
 * bl_amd_last_freq_stats.
 *   bl_amd_mel_batch_host: the same from host memory, blocking: the songs are uploaded and analysed in waves;
 *     h_frames_out and h_bands_out may be NULL.
 *   bl_amd_mel_table: copies the tables to host buffers, no device work: edges [34], weights [32][256] (bin 0 is 0),
 *     dct [13][32]; any pointer may be NULL.  BL_UNEXPECTED if the weights lack the properties listed above.
 *   bl_amd_mel_mfcc: plain host arithmetic in double from the exact integers, no device: the mean of coefficient k
 *     over the used frames in log2 units (sum / used / 4096), the population standard deviation in *std if that is not
 *     NULL; NaN for both when used == 0 (or song is NULL, or k outside 0 .. 12).
 *   bl_amd_mel_flatness_db: -mean(flat) / (32 * 4096) * 10 log10 2: the geometric over the arithmetic mean of the band
 *     powers in dB, 0 for a flat spectrum and more negative the more tonal; *std its standard deviation in dB; NaN as
 *     above.
 *   bl_amd_selftest_ilog2: runs L on the device for 2^e - 1, 2^e, 2^e + 1 of every e <= 63 and for a fixed
 *     multiplicative sequence of 2^17 values, and compares with the host's results from the same source; BL_OK iff
 *     all agree.  counts, if not NULL, receives {checked, wrong}. */
int bl_amd_mel_frames(int n_samples, int channels);
int bl_amd_mel_batch_device(const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs, uint64_t min_energy,
                            bl_amd_song_mel *d_songs_out, bl_amd_frame_mel *d_frames_out, uint32_t *d_bands_out,
                            long long n_frame_records, void *stream);
int bl_amd_ctx_mel_batch_device(bl_amd_ctx *ctx, const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs,
                                uint64_t min_energy, bl_amd_song_mel *d_songs_out, bl_amd_frame_mel *d_frames_out,
                                uint32_t *d_bands_out, long long n_frame_records, void *stream);
int bl_amd_mel_batch_host(const int16_t *const *h_pcm, const int32_t *n_samples, const int32_t *channels, int n_songs,
                          uint64_t min_energy, bl_amd_song_mel *h_songs_out, bl_amd_frame_mel *h_frames_out,
                          uint32_t *h_bands_out);
int bl_amd_mel_table(int32_t *edges, uint8_t *weights, int32_t *dct);
double bl_amd_mel_mfcc(const bl_amd_song_mel *song, int k, double *std);
double bl_amd_mel_flatness_db(const bl_amd_song_mel *song, double *std);
int bl_amd_selftest_ilog2(uint64_t counts[2]);

/* Library-normalised descriptors and exact nearest neighbours over them.  The queries above compare force vectors;
 * this layer compares anything: the caller puts up to 32 features per song into a row-major f32 matrix x[n][d]
 * (bliss_amd.descriptor.features builds one from the records of the sections above), every column is mapped onto the
 * same integer range by the library's own minimum and maximum, and the squared Euclidean distance of two descriptors is
 * an exact integer, so a result depends neither on the reduction order, the column split nor the row range.
 *   range     per column c < d: lo[c] / hi[c] the minimum / maximum over the FINITE entries of the column, compared as
 *             numbers, a zero stored as +0; n_finite[c] their count.  A column without a finite entry, and every
 *             column c >= d, has lo = hi = +0 and n_finite = 0.
 *   quantise  given a range (not necessarily the one fitted on these rows) and scale[c] in 0 .. BL_AMD_DESC_SCALE_MAX
 *             (NULL: all at the maximum): for c < d with x, lo and hi finite and hi > lo, in IEEE double, unfused, in
 *             this order
 *               t = ((double)x - (double)lo) / ((double)hi - (double)lo),  u = 2.0 * t - 1.0,  u clamped to [-1, 1],
 *               q = (int16) rint(u * (double)scale[c])        (ties to even)
 *             and q = 0 in every other case (x not finite, a bound not finite, hi <= lo, c >= d).  The scale is the
 *             feature's weight: half the scale, half the pull.  The clamp is what lets a song from outside the library
 *             be quantised with the library's range.  The cap 32512 = 127 * 256 makes the digits h = (q + 128) >> 8,
 *             l = q - 256 h both signed bytes, which the int8 matrix products of the distance rely on.
 *   distance  d2(a, b) = sum_c (a_c - b_c)^2, an integer below 32 * 65024^2 < 2^37.
 *   kNN       per query the k candidates with the smallest (d2, index), ascending, 1 <= k <= BL_AMD_KNN_MAX_K.  The self
 *             form (queries are rows of the library) excludes the query's own row, the cross form excludes nothing.
 *             Slots beyond the number of candidates hold index -1 and d2 = 2^64 - 1.  n < 2^27.
 * Every argument is checked before any device work: a rejected call returns BL_UNEXPECTED and leaves the outputs
 * untouched (n < 1, n >= 2^27 for the kNN, d outside 1 .. 32, k outside 1 .. BL_AMD_KNN_MAX_K, a row range outside the
 * library, a scale above the maximum, a NULL pointer other than h_scale and h_dist2).  The device forms are
 * asynchronous on `stream`; calls of one context are ordered on the device like its batches.
 *   bl_amd_desc_range_device      writes every byte of *d_range (device memory) from d_x[n][d]
 *   bl_amd_desc_quantize_device   d_out[n] from d_x[n][d] and *d_range (device); h_scale: d values on the host or NULL
 *   bl_amd_desc_knn_device        the self form for rows [row_begin, row_begin + n_rows) of d_lib[n]; d_index and
 *                                 d_dist2 are [n_rows][k]
 *   bl_amd_desc_cross_knn_device  the cross form for d_queries[n_queries]; outputs [n_queries][k]
 *   bl_amd_ctx_desc_*             the same on an explicit context
 *   bl_amd_desc_build_host        blocking, host memory: fit != 0 fits *h_range on h_x and writes it, fit == 0 reads it;
 *                                 then quantises h_x into h_out[n]
 *   bl_amd_desc_knn_host          blocking, host memory: h_queries NULL is the self form over all n rows (n_queries is
 *                                 ignored), otherwise the cross form; h_dist2 may be NULL
 *   bl_amd_desc_knn_scratch_bytes the workspace bytes a kNN call of this shape takes on the default context: 0 exactly
 *                                 when the candidates are not split over workgroup columns (diagnostic; 0 as well for
 *                                 arguments the call would reject) */
#define BL_AMD_DESC_DIMS 32
#define BL_AMD_DESC_SCALE_MAX 32512 /* 127 * 256 */
typedef struct bl_amd_desc { int16_t q[BL_AMD_DESC_DIMS]; } bl_amd_desc; /* 64 bytes */
typedef struct bl_amd_desc_range {                                       /* 384 bytes */
  float lo[BL_AMD_DESC_DIMS], hi[BL_AMD_DESC_DIMS];
  uint32_t n_finite[BL_AMD_DESC_DIMS];
} bl_amd_desc_range;
int bl_amd_desc_range_device(const float *d_x, int n, int d, bl_amd_desc_range *d_range, void *stream);
int bl_amd_desc_quantize_device(const float *d_x, int n, int d, const bl_amd_desc_range *d_range,
                                const uint16_t *h_scale, bl_amd_desc *d_out, void *stream);
int bl_amd_desc_knn_device(const bl_amd_desc *d_lib, int n, int row_begin, int n_rows, int k, int32_t *d_index,
                           uint64_t *d_dist2, void *stream);
int bl_amd_desc_cross_knn_device(const bl_amd_desc *d_queries, int n_queries, const bl_amd_desc *d_lib, int n, int k,
                                 int32_t *d_index, uint64_t *d_dist2, void *stream);
int bl_amd_ctx_desc_knn_device(bl_amd_ctx *ctx, const bl_amd_desc *d_lib, int n, int row_begin, int n_rows, int k,
                               int32_t *d_index, uint64_t *d_dist2, void *stream);
int bl_amd_ctx_desc_cross_knn_device(bl_amd_ctx *ctx, const bl_amd_desc *d_queries, int n_queries,
                                     const bl_amd_desc *d_lib, int n, int k, int32_t *d_index, uint64_t *d_dist2,
                                     void *stream);
int bl_amd_desc_build_host(const float *h_x, int n, int d, const uint16_t *h_scale, int fit, bl_amd_desc_range *h_range,
                           bl_amd_desc *h_out);
int bl_amd_desc_knn_host(const bl_amd_desc *h_queries, int n_queries, const bl_amd_desc *h_lib, int n, int k,
                         int32_t *h_index, uint64_t *h_dist2);
size_t bl_amd_desc_knn_scratch_bytes(int n, int n_rows, int k);

/* Playlist chains over descriptors (continuous play in which every feature counts): bl_amd_mix_device's contract with
 * descriptors in place of force vectors and the exact integer d2 of the section above in place of the f32 metric.
 * With no rules (index seeds, d_tags and d_exclude NULL, gap 0) it is the plain chain: slot t + 1 is the song nearest to
 * the song of slot t among those the chain has not played.
 *   Outputs   d_order and d_dist2 are [n_chains][length], row-major.
 *   Nearest   the smallest (d2, index): the descriptor kNN's order.
 *   Needs     1 <= n < 2^27, n_chains >= 1, length >= 1; the entries of every descriptor as the kNN needs them
 *             (|q| <= BL_AMD_DESC_SCALE_MAX, which the quantiser guarantees).
 *   Seeds     exactly one of d_seeds and d_seed_desc is non-NULL.  d_seeds: slot 0 is the seed with d2 = 0, even if the
 *             seed is excluded; a seed outside [0, n) gives a row of -1 / 2^64 - 1 from the device forms, and the host
 *             form checks the seeds first and refuses the call.  d_seed_desc: n_chains descriptors, which may alias
 *             d_lib; slot 0 is the nearest song among those not excluded (tags play no part), its value
 *             d2(seed, lib[pick]), so a seed equal to library song 7 picks song 7 at 0 (or an equal song of a smaller
 *             index); if every song is excluded the row is -1 / 2^64 - 1.
 *   Exclude   d_exclude is NULL or n bytes, one mask for all chains: a song with a non-zero byte is never picked.
 *   Tags      d_tags is NULL or n int32 (artist, album ...); a negative tag means untagged: never blocked, blocks
 *             nothing.  0 <= gap <= BL_AMD_MIX_MAX_GAP; gap == 0 ignores the tags, gap > 0 needs them.
 *   A step    at slot t >= 1 song j is allowed iff it is in none of the slots 0 .. t-1, d_exclude[j] == 0, and
 *             tags[j] < 0 or tags[j] differs from the tag of every song in slots max(0, t-gap) .. t-1.  Slot t is the
 *             allowed song nearest to the song of slot t-1, its value that d2.  If no song is allowed the chain ends:
 *             slots t .. length-1 hold -1 / 2^64 - 1, as do the slots past n when length > n.
 *   Chains    are independent: a chain's row depends neither on n_chains, on the other seeds, nor on the launch shape.
 *   Shape     bl_amd_desc_chain_shape(n, n_chains) is the shape a call takes on the calling thread's device:
 *             BL_AMD_CHAIN_PER_CHAIN (one workgroup per 16 chains) or BL_AMD_CHAIN_SPLIT (columns split over
 *             workgroups, one launch per step); BL_UNEXPECTED without a device or for n, n_chains the call would
 *             reject.  bl_amd_chain_force_shape pins the shape for these calls too; what it does for
 *             bl_amd_chain_* and bl_amd_mix_* is unchanged.
 * A rejected call (a NULL d_lib, d_order or d_dist2, both seeds or neither, n, n_chains, length or gap outside their
 * ranges, gap > 0 without tags) returns BL_UNEXPECTED before any device work and writes nothing.  Asynchronous on
 * `stream`; no allocation, copy or synchronisation inside once the context's workspace is large enough; calls of one
 * context are ordered on the device like its batches.  To continue a chain call again with seed = its last song and
 * d_exclude = everything played so far.
 *   bl_amd_desc_chain_host: host pointers, blocking; h_dist2 may be NULL. */
int bl_amd_desc_chain_device(const bl_amd_desc *d_lib, int n, const int32_t *d_seeds, const bl_amd_desc *d_seed_desc,
                             int n_chains, int length, const int32_t *d_tags, int gap, const uint8_t *d_exclude,
                             int32_t *d_order, uint64_t *d_dist2, void *stream);
int bl_amd_ctx_desc_chain_device(bl_amd_ctx *ctx, const bl_amd_desc *d_lib, int n, const int32_t *d_seeds,
                                 const bl_amd_desc *d_seed_desc, int n_chains, int length, const int32_t *d_tags,
                                 int gap, const uint8_t *d_exclude, int32_t *d_order, uint64_t *d_dist2, void *stream);
int bl_amd_desc_chain_host(const bl_amd_desc *h_lib, int n, const int32_t *h_seeds, const bl_amd_desc *h_seed_desc,
                           int n_chains, int length, const int32_t *h_tags, int gap, const uint8_t *h_exclude,
                           int32_t *h_order, uint64_t *h_dist2);
int bl_amd_desc_chain_shape(int n, int n_chains);

/* Harmonic mixes (beat-matched crossfades, same or compatible key next): bl_amd_desc_chain_*'s contract, seeds, mask,
 * tags and gap, nearest by (d2, index), outputs, sentinels, shapes and ordering on a context, plus one hard rule on
 * consecutive songs, evaluated on a 4-byte attribute per song in exact integer arithmetic.
 *   Attribute d_attr is n of bl_amd_hmix_attr: tempo in 1/100 BPM, 0 = unknown; key 0 .. 23 as bl_amd_song_chroma.key,
 *             any value >= 24 = unknown; reserved is ignored.  bl_amd_hmix_attrs fills them from analysis records.
 *   Rule      flags chooses the tests: BL_AMD_HMIX_KEY applies key_ok, BL_AMD_HMIX_TEMPO applies tempo_tol, and with
 *             BL_AMD_HMIX_TEMPO, BL_AMD_HMIX_HALF_DOUBLE lets half and double time match as well.  Bit b of key_ok[a]:
 *             a song of key b may follow a song of key a; bits 24 .. 31 are ignored.  The table is used as given and
 *             need not be symmetric; no entry is ever indexed by a value >= 24.  tempo_tol is per mille of the
 *             previous song's tempo, 0 .. 1000.  `rule` is host memory, copied before the call returns.
 *   A step    at slot t >= 1 song j is allowed iff bl_amd_desc_chain_device allows it and the pair (p, j) passes, p
 *             the song of slot t-1.  With (a, ka) the tempo and key of p and (b, kb) those of j:
 *               key    (BL_AMD_HMIX_KEY) passes if ka >= 24, or kb >= 24, or bit kb of key_ok[ka] is set;
 *               tempo  (BL_AMD_HMIX_TEMPO) passes if a == 0, or b == 0, or 1000 |b - a| <= tol a; with
 *                      BL_AMD_HMIX_HALF_DOUBLE also if 1000 |2b - a| <= tol a or 1000 |b - 2a| <= 2 tol a.  All of
 *                      these are integers below 2^28, and the tolerance is relative to the previous song, not to the
 *                      candidate.
 *             Slot t is the allowed song nearest to p, its value that d2.  If no song is allowed the chain ends as
 *             bl_amd_desc_chain_device's does; there is no fall-back to a relaxed rule: the caller continues with a
 *             plain chain from the last song (seed = that song, d_exclude = everything played so far).
 *   Slot 0    is exactly bl_amd_desc_chain_device's and under no pair rule.  An index seed takes slot 0 whatever its
 *             attribute, and its attribute then binds slot 1, even when the seed is excluded.  For a descriptor seed
 *             neither tags nor the pair rule play a part in slot 0; the attribute of its pick binds slot 1.
 *   Off       with neither BL_AMD_HMIX_KEY nor BL_AMD_HMIX_TEMPO in flags d_attr may be NULL and the outputs are byte
 *             for byte those of bl_amd_desc_chain_device with the same remaining arguments; the same holds when every
 *             attribute is unknown.
 *   Shape     bl_amd_desc_chain_shape and bl_amd_chain_force_shape govern these calls as they govern
 *             bl_amd_desc_chain_*; the result never depends on the shape.
 * A rejected call (everything bl_amd_desc_chain_device rejects, a NULL rule, flag bits other than the three,
 * BL_AMD_HMIX_HALF_DOUBLE without BL_AMD_HMIX_TEMPO, tempo_tol > 1000, BL_AMD_HMIX_KEY or BL_AMD_HMIX_TEMPO with a NULL
 * d_attr) returns BL_UNEXPECTED before any device work and writes nothing.
 *   bl_amd_desc_hmix_host: host pointers, blocking; h_dist2 may be NULL; the seeds are checked first as
 *   bl_amd_desc_chain_host checks them.
 *   bl_amd_hmix_rule_camelot: host arithmetic, the usual wheel with tempo_tol and flags as given.  After a major key of
 *   tonic k (index k) may follow: major k, major (k+7)%12, major (k+5)%12 and the relative minor 12 + (k+9)%12; after
 *   a minor key 12 + k: minor 12 + k, 12 + (k+7)%12, 12 + (k+5)%12 and the relative major (k+3)%12.  After C: C, G, F,
 *   Am; after Am: Am, Em, Dm, C.  BL_UNEXPECTED, and nothing written, for a NULL out or for a tempo_tol or flags the
 *   calls above would reject.
 *   bl_amd_hmix_attrs: host arithmetic over n >= 1 records.  Either record array may be NULL, and that field is then
 *   unknown for every song.  tempo = llrint(100 * bl_amd_rhythm_bpm(&rhythm[i], rate)) clamped to 1 .. 65535, and 0
 *   where the BPM is NaN; key = the chroma key, 255 for key -1 (or any key outside 0 .. 23); reserved = 0. */
typedef struct bl_amd_hmix_attr { /* 4 bytes per song */
  uint16_t tempo;                 /* 1/100 BPM; 0 = unknown */
  uint8_t key;                    /* 0 .. 23 as bl_amd_song_chroma.key; any value >= 24 = unknown */
  uint8_t reserved;               /* ignored */
} bl_amd_hmix_attr;

#define BL_AMD_HMIX_KEY 1         /* apply key_ok */
#define BL_AMD_HMIX_TEMPO 2       /* apply tempo_tol */
#define BL_AMD_HMIX_HALF_DOUBLE 4 /* with TEMPO: half and double time also match */
typedef struct bl_amd_hmix_rule { /* 104 bytes */
  uint32_t key_ok[24];            /* bit b of key_ok[a]: a song of key b may follow a song of key a */
  uint32_t tempo_tol;             /* per mille of the previous song's tempo, 0 .. 1000 */
  uint32_t flags;
} bl_amd_hmix_rule;
int bl_amd_desc_hmix_device(const bl_amd_desc *d_lib, const bl_amd_hmix_attr *d_attr, int n,
                            const bl_amd_hmix_rule *rule, const int32_t *d_seeds, const bl_amd_desc *d_seed_desc,
                            int n_chains, int length, const int32_t *d_tags, int gap, const uint8_t *d_exclude,
                            int32_t *d_order, uint64_t *d_dist2, void *stream);
int bl_amd_ctx_desc_hmix_device(bl_amd_ctx *ctx, const bl_amd_desc *d_lib, const bl_amd_hmix_attr *d_attr, int n,
                                const bl_amd_hmix_rule *rule, const int32_t *d_seeds, const bl_amd_desc *d_seed_desc,
                                int n_chains, int length, const int32_t *d_tags, int gap, const uint8_t *d_exclude,
                                int32_t *d_order, uint64_t *d_dist2, void *stream);
int bl_amd_desc_hmix_host(const bl_amd_desc *h_lib, const bl_amd_hmix_attr *h_attr, int n, const bl_amd_hmix_rule *rule,
                          const int32_t *h_seeds, const bl_amd_desc *h_seed_desc, int n_chains, int length,
                          const int32_t *h_tags, int gap, const uint8_t *h_exclude, int32_t *h_order,
                          uint64_t *h_dist2);
int bl_amd_hmix_rule_camelot(bl_amd_hmix_rule *out, int tempo_tol, int flags);
int bl_amd_hmix_attrs(const bl_amd_song_rhythm *rhythm, const bl_amd_song_chroma *chroma, int n, int rate,
                      bl_amd_hmix_attr *out);

/* Integer-only synthetic PCM (the benchmark corpus of BASELINE.json),
 * generated in place on the device: song i = seed_base + i, written at
 * h_desc[i].pcm_offset.  Byte-identical to oracle/orc_synth.c. */
int bl_amd_synth_pcm_device(int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs,
                            uint32_t seed_base, uint32_t sample_rate, void *stream);

/* Arithmetic of the envelope kernel's 17-tap FIR (ref src/tempo_atk_sort.c:123-138):
 *   0  the reference's order, every product and sum rounded separately: window energies
 *      bit-identical to the reference arithmetic;
 *   1  the same sum with the products folded in by fused multiply-adds;
 *   2  (default) the normalisation of ref :109-114 folded into the filter, on the integers: the exact integer sum
 *      of integer taps (the reference's literals times 1e7) and samples minus mean, scaled once per output.
 * 1 and 2 differ from 0 by a few 1e-16 of an output's largest partial sum — what a different
 * FFT library behind it already does — and are 9 % / 25 % faster.  Measured on 2.3 billion windows
 * of 38 912 songs: 10 f32 window energies move, by one ulp, no integer and no feature changes;
 * expected `beat` changes per three-minute song 4e-10.  mode -1 = follow the
 * environment variable BL_AMD_FIR_FUSED, else the default.  Process-wide. */
int bl_amd_set_fir_mode(int mode);
int bl_amd_fir_mode(void);

/* Per-kernel device time, measured with hipEvents on the launch stream while
 * profiling is on (bench.py's roofline leg).  name is one of "pcm_scan", "freq_scan",
 * "amp_finish", "freq_frames", "freq_finish", "env_windows", "env_tail",
 * "distance", "rhythm_hops", "rhythm_acf", "rhythm_pick", "chroma_pitch", "chroma_key",
 * "desc_range", "desc_quantize", "desc_knn", "desc_merge", "beats"; returns accumulated milliseconds and the launch count since the
 * last reset, or -1 for an unknown name. */
void bl_amd_profile(int enable);
void bl_amd_profile_reset(void);
double bl_amd_profile_ms(const char *name, int *launches);

/* Diagnostic: per-window envelope energies (the reference's filtered_array,
 * ref src/tempo_atk_sort.c:150) of the most recent batch, songs concatenated with
 * nb_frames slots each (the last two of a song are never written).  Copies up to
 * max_elems floats to h_out; returns the number copied, 0 if none, -1 on error. */
long long bl_amd_last_energies(float *h_out, long long max_elems);

/* Diagnostic: what the frequency and statistics passes left in the default context's workspace for the most recent
 * launch group, read-only and in the CALLER's song order (the workspace itself is in processing order, longest song
 * first in a mixed-length batch).  Returns the number of songs of that group, 0 if nothing has run, -1 on error, and
 * fills, for the songs whose index is below max_songs, whichever of these is not NULL:
 *   h_spectrum  256 floats per song: the ordered f32 sum over the frames of re*re + im*im per bin (ps[] of ref
 *               src/frequency_sort.c:88-93, before the square root).  Bins 1..255 are the reference's; bin 0 is
 *               unspecified (the reference overwrites ps[0] every frame and never reads it, the kernels sum it);
 *   h_sum       the sum of all samples of the song (exact, not the reference's wrapping int32);
 *   h_sumsq     the sum of their squares;
 *   h_hist      4096 counts per song: samples of value s in [-2048, 2048) at index s + 2048, over ALL samples (the
 *               trimmed silence is taken off bin 2048 later, by the amplitude kernel).
 * *parts (may be NULL) receives the BL_AMD_PART_* bits of what that group's launches wrote; anything else is left
 * over from an earlier call or cleared.  bl_analyze and the batch calls write all three; bl_frequency_sort the spectrum
 * alone (it reads no statistics, so no statistics pass runs); bl_amplitude_sort and bl_envelope_sort the sums and the
 * histogram alone, and so do bl_mean / bl_variance, as a group of one song.
 * Waits for the device like bl_amd_last_energies.  A call that is split into several launch groups (BL_AMD_GROUP_SONGS,
 * or the waves of a host batch) leaves only its last group here. */
#define BL_AMD_PART_SPECTRUM 1
#define BL_AMD_PART_SUMS 2
#define BL_AMD_PART_HIST 4
int bl_amd_last_freq_stats(int max_songs, float *h_spectrum, long long *h_sum, unsigned long long *h_sumsq,
                           unsigned *h_hist, int *parts);

/* Diagnostic: the envelope tail (k_env_tail: recurrence, onset weighting, the two box filters, the peak count; ref
 * src/tempo_atk_sort.c:201-284) of the default context on a compressed envelope the CALLER supplies instead of the one
 * the window kernel leaves, as one launch group of n_songs songs.  h_desc: n_samples and duration per song (channels 1,
 * pcm_offset 0; no PCM is read); h_env: nb_frames = 2 * (n_samples / 512) doubles per song, songs concatenated in the
 * caller's order — slot w < nb_frames - 2 is log(1 + mu f_w) / log(1 + mu) of window w, the last two slots of a song are
 * never read; n_env: their total count, anything but the sum of nb_frames is BL_UNEXPECTED.  The group is laid out as
 * a batch call lays it out (longest song first in a mixed-length group) and runs the same launch.  h_results (host,
 * n_songs records, caller's order) gets nb_frames, n_windows, beat, atk_sum, v.tempo, v.attack and status; every other
 * field is zero.  Read-only towards the other diagnostics: what bl_amd_last_energies and bl_amd_last_freq_stats answer
 * is unchanged.  Blocking. */
int bl_amd_tail_from_envelope(const bl_amd_song_desc *h_desc, int n_songs, const double *h_env, long long n_env,
                              bl_amd_song_result *h_results);

/* Releases every default context (workspaces, streams, pinned staging) and the multi-device
 * state.  Explicit contexts are released by bl_amd_ctx_destroy. */
void bl_amd_shutdown(void);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* BLISS_AMD_H_ */
