/*
 * bl_runtime.h — internal: the per-device context behind include/bliss_amd.h, shared by
 * bl_runtime.hip (contexts and the single-device analysis C-ABI), bl_host_batch.hip (songs from host memory: the host
 * batch, bl_amd_analyze_files), bl_feature_api.hip (levels, timbre, tempo, beats, chroma and mel: device and host
 * forms), bl_query_api.hip (the matrix, playlist and vector-query C-ABI),
 * bl_desc_api.hip (descriptors), bl_multi.hip (multi-device corpus path), bl_side_ws.hip (the workspaces beside the
 * context's own, bl_side_ws.h) and the five call paths on top of those: bl_loud_api.hip, bl_tpeak_api.hip,
 * bl_fprint_api.hip, bl_form_api.hip, bl_cover_api.hip.
 * C++ only, not installed.
 */
#ifndef BL_RUNTIME_H_
#define BL_RUNTIME_H_

#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "bl_launch.h"
#include "bl_resample.h"
#include "bl_waves.h"

#define BL_MAX_DEVICES 16
#define BL_GROUP_SONGS_MAX 32768 /* gridDim.y of the (blocks, songs) launch grids */
#define BL_PIN_SLOTS 4
#define BL_RS_OUT_RATE 22050 /* ref src/decode.c:7 SAMPLE_RATE */
#define BL_HOST_WAVE_MAX ((size_t)2 << 30) /* PCM bytes per wave of the host batch: default and upper bound */

struct bl_buf {
  void *p = nullptr;
  size_t cap = 0;
};

struct bl_pin_slot { /* pinned staging of small host->device records */
  void *p = nullptr;
  size_t cap = 0;
  hipEvent_t ev = nullptr;
  bool busy = false;
};

/* One device, one workspace, one set of internal streams.  Calls on one context are
 * ordered (host mutex for the enqueue, an event for the shared workspace on the device);
 * different contexts — on the same device or on different ones — are independent. */
struct bl_amd_ctx {
  std::mutex mu;
  int device = 0;
  int n_cu = 256;
  int group_songs = BL_GROUP_SONGS_MAX;
  size_t host_wave_bytes = BL_HOST_WAVE_MAX;
  hipStream_t side = nullptr; /* envelope tail runs here, beside the frequency pass */
  hipEvent_t ev_env = nullptr, ev_tail = nullptr;
  hipStream_t side2 = nullptr; /* mixed lengths: the tail of the long songs, under the window kernel of the rest */
  hipEvent_t ev_head = nullptr, ev_tail2 = nullptr;
  hipEvent_t ev_ws = nullptr; /* end of the last launch group that used the workspace */
  bool ws_used = false;
  long long last_env_total = 0;
  /* bl_amd_last_freq_stats: the last launch group's first record in `songs`, its song count, the parts it wrote */
  int last_first = 0, last_songs = 0, last_parts = 0;
  bl_tables tb{};
  void *tables_mem = nullptr;
  bl_buf songs, stats, hist, spectrum, energies, lc, results;
  bl_pin_slot ring[BL_PIN_SLOTS];
  int ring_next = 0;
  /* profiling */
  bool prof = false;
  struct Ev { int k; hipEvent_t a, b; };
  std::vector<Ev> events;
  std::vector<Ev> open; /* begun, not yet ended */
  double prof_ms[PK_COUNT] = {0};
  int prof_n[PK_COUNT] = {0};
  /* host-batch staging: two waves in flight */
  void *pinned[2] = {nullptr, nullptr};
  size_t pinned_cap[2] = {0, 0};
  bl_buf arena[2];
  bl_buf arena22[2]; /* converted (22 050 Hz) songs of a wave whose input is at another rate */
  hipStream_t streams[2] = {nullptr, nullptr};
  std::vector<void *> registered[2]; /* host ranges pinned in place for wave k */
  /* multi-device corpus path (bl_multi.hip): this rank's vectors, the gathered blocks, the
   * vectors in output order, the order table and the row block — grown on demand, kept */
  bl_buf mx_my, mx_gath, mx_all, mx_order, mx_rows;
  /* device rate converter: the plan of the last (input rate, sample kind) stays uploaded */
  bl_buf rs_songs, rs_bank;
  int rs_rate = 0, rs_kind = -1, rs_bank_lds = 0;
  bl_rs_geom rs_geom{};
  size_t rs_lds = 0;
  bl_rs_plan rs_plan{}; /* the uploaded plan's geometry, for bl_rs_out_frames; the bank pointers are null */
  /* bl_amd_knn_device: the cosine prep of the vectors and the column splits' partial lists */
  bl_buf knn;
  /* bl_amd_chain_device, bl_amd_mix_device: cosine prep, the column split's per-chain state and played bits (or the
   * per-chain shape's played bits beyond what LDS holds) */
  bl_buf chain;
  /* bl_amd_radius_*_device, bl_amd_groups_device: cosine prep and the per-(row, column split) counts */
  bl_buf radius;
  /* bl_amd_levels_batch_device: the songs' records (bl_level_song) */
  bl_buf level_songs;
  /* bl_amd_timbre_batch_device: the songs' records (bl_timbre_song), longest first */
  bl_buf timbre_songs;
  /* bl_amd_rhythm_batch_device, bl_amd_rhythm_from_onsets: the songs' records (bl_rhythm_song), longest first; one
   * launch group's novelty values (4 bytes per hop) and its onset sums and lag products (blk_rhythm_rows_bytes) */
  bl_buf rhythm_songs, rhythm_n, rhythm_rows;
  /* bl_amd_beats_device, bl_amd_beats_host: the songs' records (bl_beat_song), longest first, and, for a call without
   * a links output, one launch group's links (2 bytes per hop) */
  bl_buf beat_songs, beat_links;
  /* bl_amd_chroma_batch_device: the songs' records (bl_chroma_song), their twelve sums, and the bank's image
   * (blk_chroma_image_host), uploaded by the context's first call */
  bl_buf chroma_songs, chroma_acc, chroma_image;
  bool chroma_image_ready = false;
  /* bl_amd_mel_batch_device: the songs' records (bl_timbre_song), longest first, and the tables' image
   * (blk_mel_image_host), uploaded by the context's first call */
  bl_buf mel_songs, mel_image;
  bool mel_image_ready = false;
  /* bl_amd_desc_*: the range's per-workgroup shares, the partial lists of a kNN's column split, a chain call's
   * per-group state and played words */
  bl_buf desc;
};

/* bl_runtime.hip */
int blr_ensure(bl_buf &b, size_t bytes);
/* thread's default context (device chosen by bl_amd_init, default 0); nullptr + message on failure */
bl_amd_ctx *blr_default_ctx(void);
/* internal stream k (0 or 1) of the context, created on first use; nullptr + message on failure */
hipStream_t blr_stream(bl_amd_ctx *c, int k);
/* what the analysis accepts of song i; BL_UNEXPECTED + message otherwise */
int blr_validate_desc(const bl_amd_song_desc &d, int i);
int blr_analyze_device(bl_amd_ctx *c, const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs,
                       bl_amd_song_result *d_results, hipStream_t stream, int what);
/* enqueue the conversion of n_songs device-resident songs to BL_RS_OUT_RATE on `s` (caller holds c->mu, device current) */
int blr_resample_device(bl_amd_ctx *c, const void *d_in, int in_is_s32, const bl_amd_resample_desc *h_desc,
                        int n_songs, int in_rate, int16_t *d_out, hipStream_t s);

/* pinned slot of at least `bytes` from a ring of BL_PIN_SLOTS whose next slot is `next`; blocks only when BL_PIN_SLOTS
 * calls are still in flight.  A slot's event is made on first use (the context's own ring has them from ctx_init). */
int blr_ring_get(bl_pin_slot *ring, int &next, size_t bytes, bl_pin_slot **out);
/* frees the blocks and the events of a ring of BL_PIN_SLOTS and leaves it empty */
void blr_ring_free(bl_pin_slot *ring);

/* bl_side_ws.hip: frees the side workspaces (bl_side_ws.h) of a context that is being released (ctx_release: the
 * context held, its device current and idle) */
void blr_side_release(bl_amd_ctx *c);

/* bl_host_batch.hip */
/* host-memory batch on one context; pcm_is_s32: h_pcm[i] points at int32 samples that are
 * narrowed with >> 16 while they are staged.  in_rate: 0 / 22 050 = as is; another rate = the songs
 * are converted on the device first (wide sources then travel as int32).  d_res_out (optional) receives the device
 * pointer of the results (valid until the context's next host batch). */
int blr_analyze_host(bl_amd_ctx *c, const void *const *h_pcm, int pcm_is_s32, const int32_t *n_samples,
                     const int32_t *channels, const uint64_t *duration, int n_songs, int in_rate,
                     bl_amd_song_result *h_results, bl_amd_song_result **d_res_out);

/* drops the registrations (hipHostRegister) the host batch made for its wave slot k */
inline void blr_unregister_wave(bl_amd_ctx *c, int k) {
  for (void *p : c->registered[k]) (void)hipHostUnregister(p);
  c->registered[k].clear();
}

/* what the levels, the timbre and the mel call accept of a song, device and host forms alike (bl_amd_timbre_frames:
 * bl_api.c) */
inline bool levels_song_ok(unsigned long long pcm_offset, int n_samples, int channels) {
  return n_samples >= 2 && (channels == 1 || channels == 2) && !(pcm_offset & 7);
}
inline bool timbre_song_ok(unsigned long long pcm_offset, int n_samples, int channels) {
  return bl_amd_timbre_frames(n_samples, channels) >= 1 && !(pcm_offset & 7);
}
/* the same for the tempo (bl_amd_rhythm_hops: bl_api.c), and its lag range */
inline bool rhythm_song_ok(unsigned long long pcm_offset, int n_samples, int channels) {
  return bl_amd_rhythm_hops(n_samples, channels) >= 1 && !(pcm_offset & 7);
}
/* the same for chroma and key: one whole frame of 1 | 2 channels at least (bl_amd_chroma_frames: bl_api.c) */
inline bool chroma_song_ok(unsigned long long pcm_offset, int n_samples, int channels) {
  return bl_amd_chroma_frames(n_samples, channels) >= 0 && n_samples / channels >= 1 && !(pcm_offset & 7);
}
inline bool rhythm_lags_ok(int lag_min, int lag_max) {
  return lag_min >= 1 && lag_min <= lag_max && lag_max <= BL_AMD_RHYTHM_LAGS - 2;
}

/* makes the context's device current for the duration of a call and puts the caller's back:
 * the current device is per-thread state shared with whoever else uses HIP in this thread
 * (torch, the caller's own code) */
struct DevGuard {
  int prev = -1;
  bool changed = false;
  bool ok = true;
  explicit DevGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) { prev = -1; (void)hipGetLastError(); }
    if (prev != dev) {
      ok = hipSetDevice(dev) == hipSuccess;
      changed = ok && prev >= 0;
    }
  }
  ~DevGuard() {
    if (changed) (void)hipSetDevice(prev);
  }
};

/* a call that uses context c's workspace: the context locked and its device current until the call returns */
struct CtxGuard {
  std::lock_guard<std::mutex> lk;
  DevGuard dg;
  explicit CtxGuard(bl_amd_ctx *c) : lk(c->mu), dg(c->device) {}
  bool ok() const { return dg.ok; }
};

/* the context of a call: the calling thread's default one, or the one it was given */
inline bl_amd_ctx *call_ctx(bl_amd_ctx *c, bool dflt) { return dflt ? blr_default_ctx() : c; }

/* The workspace is shared by every call on a context, whatever stream it is enqueued on: a call waits, on the device,
 * for the previous user before anything of it writes a workspace block (ws_wait), and leaves its stream's position
 * behind as the hand-over point after its last launch (ws_pass).  The mutex only orders the enqueues. */
inline int ws_wait(bl_amd_ctx *c, hipStream_t s) {
  if (c->ws_used) BL_HIP_CHECK(hipStreamWaitEvent(s, c->ev_ws, 0));
  return BL_OK;
}
inline int ws_pass(bl_amd_ctx *c, hipStream_t s) {
  BL_HIP_CHECK(hipEventRecord(c->ev_ws, s));
  c->ws_used = true;
  return BL_OK;
}

/* a device block of the *_host entry points, freed when the call returns; zero bytes: no block, p stays nullptr.
 * Every step answers "did it work", so a call is one && chain and any failure is BL_UNEXPECTED. */
struct DevMem {
  void *p = nullptr;
  size_t bytes;
  explicit DevMem(size_t n) : bytes(n) {
    if (n && hipMalloc(&p, n) != hipSuccess) p = nullptr;
  }
  ~DevMem() {
    if (p) (void)hipFree(p);
  }
  DevMem(const DevMem &) = delete;
  DevMem &operator=(const DevMem &) = delete;
  bool ok() const { return p || !bytes; }
  bool up(const void *h) const { return p && hipMemcpy(p, h, bytes, hipMemcpyHostToDevice) == hipSuccess; }
  bool down(void *h, size_t n) const { return ok() && hipMemcpy(h, p, n, hipMemcpyDeviceToHost) == hipSuccess; }
  bool down(void *h) const { return down(h, bytes); }
  template <class T> T *as() const { return static_cast<T *>(p); }
};

/* samples per wave of the *_batch_host forms of levels, timbre, tempo, chroma, mel, loudness and true peak: the songs
 * are uploaded, analysed and fetched 256 MiB of PCM at a time, or the context's host_wave_bytes if that is less (a song
 * longer than that is a wave of its own) */
#define BL_HOST_WAVE_SAMPLES ((size_t)128 << 20)

/* The host songs in waves (bl_wave_plan): songs [b, e) laid out in a device arena, copied there, and
 * `wave(d_arena, desc, b, e)` called on them with desc[i - b] the place of song i.  The arena is freed when `wave`
 * returns, so `wave` fetches what it computed.  The caller has made c->device current and does not hold c->mu: the
 * budget is read under it, and `wave` calls device forms that take it themselves. */
template <class Wave>
int host_waves(bl_amd_ctx *c, const int16_t *const *h_pcm, const int32_t *n_samples, const int32_t *channels,
               int n_songs, Wave wave) {
  size_t budget;
  {
    std::lock_guard<std::mutex> lk(c->mu);
    budget = std::min(BL_HOST_WAVE_SAMPLES, c->host_wave_bytes / 2);
  }
  std::vector<size_t> off;
  std::vector<bl_amd_song_desc> desc;
  for (int b = 0, e; b < n_songs; b = e) {
    size_t total = 0;
    e = bl_wave_plan(n_samples, b, n_songs, budget, off, total);
    desc.resize(off.size());
    for (int i = b; i < e; ++i) {
      bl_amd_song_desc &d = desc[i - b];
      d.pcm_offset = off[i - b];
      d.n_samples = n_samples[i];
      d.channels = channels[i];
      d.duration = 0;
    }
    DevMem arena(sizeof(int16_t) * total);
    if (!arena.ok()) return BL_UNEXPECTED;
    for (int i = b; i < e; ++i)
      BL_HIP_CHECK(hipMemcpy(arena.as<int16_t>() + desc[i - b].pcm_offset, h_pcm[i],
                             sizeof(int16_t) * (size_t)n_samples[i], hipMemcpyHostToDevice));
    if (wave(arena.as<int16_t>(), desc.data(), b, e) != BL_OK) return BL_UNEXPECTED;
  }
  return BL_OK;
}

/* A *_batch_host form from its first check to its last wave.  `args_ok`: what the form asks of its other arguments;
 * `song_ok(0, n_samples, channels)`: what its device form accepts of a song.  The order is behaviour: a call refused
 * for its arguments creates no context.  Then the default context, its device made current, and host_waves. */
template <class SongOk, class Wave>
int host_form(const int16_t *const *h_pcm, const int32_t *n_samples, const int32_t *channels, int n_songs, bool args_ok,
              SongOk song_ok, Wave wave) {
  if (!h_pcm || !n_samples || !channels || n_songs < 1 || !args_ok) return BL_UNEXPECTED;
  for (int i = 0; i < n_songs; ++i)
    if (!h_pcm[i] || !song_ok(0, n_samples[i], channels[i])) return BL_UNEXPECTED;
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return BL_UNEXPECTED;
  DevGuard dg(c->device);
  if (!dg.ok) return BL_UNEXPECTED;
  return host_waves(c, h_pcm, n_samples, channels, n_songs, wave);
}

/* One output of one wave of a *_batch_host form: `count` elements on the device for the caller's host cursor `h`, or
 * no block and dev() == nullptr where the caller passed none.  fetch() copies them to the cursor and moves it behind
 * them, so the next wave's follow. */
template <class T>
struct WaveOut {
  T *&h;
  size_t count;
  DevMem mem;
  WaveOut(T *&cursor, size_t n) : h(cursor), count(n), mem(cursor ? sizeof(T) * n : 0) {}
  bool ok() const { return mem.ok(); }
  T *dev() const { return mem.as<T>(); }
  bool fetch() {
    if (h && !mem.down(h)) return false;
    if (h) h += count;
    return true;
  }
};

/* the metric and the row range of a vector query (bl_amd_knn_*, bl_amd_chain_*, bl_amd_radius_*, bl_amd_groups_*) */
inline bool metric_ok(int metric) { return metric == BL_AMD_KNN_DISTANCE || metric == BL_AMD_KNN_COSINE; }
inline bool rows_ok(int n, int row_begin, int n_rows) {
  return row_begin >= 0 && n_rows > 0 && row_begin < n && n_rows <= n - row_begin;
}

/* one query on context c: `launch(stream, scratch)` runs with the context locked, its device current, the workspace's
 * last user waited for on `stream` and `buf` grown to `bytes`; then the stream's position becomes the hand-over point */
template <class Launch>
int query_call(bl_amd_ctx *c, void *stream, bl_buf &buf, size_t bytes, Launch launch) {
  CtxGuard g(c);
  if (!g.ok()) return BL_UNEXPECTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (ws_wait(c, s) != BL_OK || blr_ensure(buf, bytes) != BL_OK || launch(s, buf.p) != BL_OK) return BL_UNEXPECTED;
  return ws_pass(c, s);
}

/* One call that uploads n per-song records of type T into `block` and launches on them; the caller holds c->mu and has
 * made c->device current.  `fill(T *h)` writes the records into a pinned slot (BL_OK, or BL_UNEXPECTED to refuse the
 * call), `launch(const T *h, T *d)` enqueues the kernels on `s` and grows whatever other workspace they need.
 * The caller's own descriptors are read by `fill` alone, so they are the caller's again when the call returns, and
 * hipMemcpyAsync from pinned memory does not block, so nothing here waits for the device.  The order is the protocol:
 * the wait for the workspace's last user is on `s` before the copy (the record block is workspace); the slot counts as
 * in flight only once its event is recorded behind the copy, so a call that fails before that leaves the slot free
 * and the hand-over untouched; the hand-over point moves behind the last launch. */
template <class T, class Fill, class Launch>
int record_call(bl_amd_ctx *c, hipStream_t s, bl_buf &block, int n, Fill fill, Launch launch) {
  const size_t bytes = sizeof(T) * (size_t)n;
  bl_pin_slot *slot = nullptr;
  if (blr_ring_get(c->ring, c->ring_next, bytes, &slot) != BL_OK) return BL_UNEXPECTED;
  T *h = static_cast<T *>(slot->p);
  if (fill(h) != BL_OK || ws_wait(c, s) != BL_OK || blr_ensure(block, bytes) != BL_OK) return BL_UNEXPECTED;
  T *d = static_cast<T *>(block.p);
  BL_HIP_CHECK(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s));
  BL_HIP_CHECK(hipEventRecord(slot->ev, s));
  slot->busy = true;
  if (launch(h, d) != BL_OK) return BL_UNEXPECTED;
  return ws_pass(c, s);
}

/* bl_amd_chain_force_shape's setting (bl_query_api.hip), which pins the shape of the descriptor chains too */
int blr_chain_force(void);

/* the profiling callback of the launchers (blk_mark_fn); user: the context */
void mark_cb(void *user, int k, hipStream_t s, int begin);

#endif /* BL_RUNTIME_H_ */
