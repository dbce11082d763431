/*
 * bl_host_batch.hip — everything that feeds songs from host memory: the host batch (blr_analyze_host: waves of songs
 * through two pinned buffers or the caller's registered ones, copy/compute overlap on 2 streams, optional device rate
 * conversion), its C-ABI (bl_amd_*analyze_batch_host*, bl_amd_set_host_transfer) and the corpus loop over files
 * (bl_amd_analyze_files).  Host code only; contexts and the analysis' device form are bl_runtime.hip's, the wave rule
 * is bl_waves.h's.  The *_batch_host forms of the per-song features are bl_feature_api.hip's and bl_*_api.hip's.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <thread>

#include "bl_runtime.h"
#include "bl_resample.h"

namespace {

std::atomic<int> g_host_mode{-1}; /* -1: from BL_AMD_HOST_MODE or staged */

#ifndef BL_STAGE_THREADS
#define BL_STAGE_THREADS 8 /* host threads of the staging copy (BL_AMD_STAGE_THREADS overrides) */
#endif

int stage_threads(void) {
  static const int n = [] { /* initialised once, thread-safe (C++11 function-local static) */
    const char *e = getenv("BL_AMD_STAGE_THREADS");
    const int v = e ? atoi(e) : BL_STAGE_THREADS;
    return v < 1 ? 1 : (v > 64 ? 64 : v);
  }();
  return n;
}

int host_mode(void) {
  int m = g_host_mode.load();
  if (m < 0) {
    const char *e = getenv("BL_AMD_HOST_MODE");
    m = (e && !strcmp(e, "registered")) ? BL_AMD_HOST_REGISTERED : BL_AMD_HOST_STAGED;
    g_host_mode.store(m);
  }
  return m;
}

double now(void) {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

/* reject bad descriptors before anything is staged (a negative length would otherwise become a ~2^64-byte copy);
 * geo: the conversion's geometry, nullptr when the songs are analysed as they are */
int check_songs(const void *const *h_pcm, const int32_t *n_samples, const int32_t *channels, const uint64_t *duration,
                int n_songs, const bl_rs_plan *geo) {
  for (int i = 0; i < n_songs; ++i) {
    if (!h_pcm[i]) {
      fprintf(stderr, "bliss_amd: song %d rejected: NULL sample pointer\n", i);
      return BL_UNEXPECTED;
    }
    bl_amd_song_desc d;
    d.pcm_offset = 0; d.n_samples = n_samples[i]; d.channels = channels[i]; d.duration = duration[i];
    if (geo) { /* what the analyzers will see: stereo at 22 050 Hz */
      if (n_samples[i] <= 0 || (channels[i] != 1 && channels[i] != 2) || n_samples[i] % channels[i]) {
        fprintf(stderr, "bliss_amd: song %d rejected (n_samples=%d channels=%d)\n", i, n_samples[i], channels[i]);
        return BL_UNEXPECTED;
      }
      const size_t of = bl_rs_out_frames(geo, (size_t)(n_samples[i] / channels[i]), nullptr);
      d.n_samples = of > (size_t)INT32_MAX / 2 ? -1 : (int32_t)(2 * of);
      d.channels = 2;
    }
    if (blr_validate_desc(d, i) != BL_OK) return BL_UNEXPECTED;
  }
  return BL_OK;
}

/* The two wave slots of one blr_analyze_host call: wave w uses stream, pinned buffer, arenas and registration list
 * w & 1, and done[w & 1] marks the end of its transfer.  close() is what every exit of the call goes through, by hand
 * where its answer matters and from the destructor otherwise: both streams synchronised, both registration lists
 * dropped, the events destroyed. */
struct WaveSlots {
  bl_amd_ctx *c;
  hipEvent_t done[2] = {nullptr, nullptr};
  bool used[2] = {false, false};
  explicit WaveSlots(bl_amd_ctx *ctx) : c(ctx) {}
  WaveSlots(const WaveSlots &) = delete;
  WaveSlots &operator=(const WaveSlots &) = delete;
  ~WaveSlots() { (void)close(); }
  int open() {
    for (int k = 0; k < 2; ++k) {
      if (!blr_stream(c, k)) return BL_UNEXPECTED;
      BL_HIP_CHECK(hipEventCreateWithFlags(&done[k], hipEventDisableTiming));
    }
    return BL_OK;
  }
  /* pinned buffer k is free again once the transfer of wave-2 has finished */
  int reuse(int k) {
    if (!used[k]) return BL_OK;
    BL_HIP_CHECK(hipEventSynchronize(done[k]));
    blr_unregister_wave(c, k);
    return BL_OK;
  }
  int close() {
    int rc = BL_OK;
    for (int k = 0; k < 2; ++k) {
      if (c->streams[k] && hipStreamSynchronize(c->streams[k]) != hipSuccess) rc = BL_UNEXPECTED;
      blr_unregister_wave(c, k);
      if (done[k]) (void)hipEventDestroy(done[k]);
      done[k] = nullptr;
    }
    return rc;
  }
};

/* pin the caller's buffers where they are (hipHostRegister keeps free() valid for the
 * caller) and copy each song straight to its place in the arena */
int stage_registered(bl_amd_ctx *c, int k, const void *const *h_pcm, const int32_t *n_samples,
                     const std::vector<size_t> &off, int16_t *d_arena, hipStream_t s) {
  for (size_t i = 0; i < off.size(); ++i) {
    void *hp = const_cast<void *>(h_pcm[i]);
    const size_t nb = (size_t)n_samples[i] * 2;
    if (hipHostRegister(hp, nb, hipHostRegisterDefault) == hipSuccess) c->registered[k].push_back(hp);
    else (void)hipGetLastError(); /* already registered / unpinnable: the copy still works, staged by the runtime */
    BL_HIP_CHECK(hipMemcpyAsync(d_arena + off[i], hp, nb, hipMemcpyHostToDevice, s));
  }
  return BL_OK;
}

/* one wave through pinned buffer k: `elems` samples of `esz` bytes; wait_ms is what the trace line reports as the
 * host's wait for the buffer */
int stage_pinned(bl_amd_ctx *c, int k, int wave, double wait_ms, const void *const *h_pcm, int pcm_is_s32,
                 const int32_t *n_samples, const std::vector<size_t> &off, size_t elems, size_t esz, void *d_arena,
                 hipStream_t s) {
  const double t_b = now();
  const size_t bytes = elems * esz + 64;
  if (c->pinned_cap[k] < bytes) {
    if (c->pinned[k]) (void)hipHostFree(c->pinned[k]);
    c->pinned[k] = nullptr; c->pinned_cap[k] = 0;
    BL_HIP_CHECK(hipHostMalloc(&c->pinned[k], bytes, hipHostMallocDefault));
    c->pinned_cap[k] = bytes;
  }
  unsigned char *stage = static_cast<unsigned char *>(c->pinned[k]);
  /* staging copy on several host threads: one thread moves ~10 GB/s, the link takes more.
   * 32-bit sources are narrowed here (>> 16), so the link only ever carries s16. */
  const int n_thr = (int)std::min<size_t>((size_t)stage_threads(), std::max<size_t>(1, elems * esz / ((size_t)32 << 20)));
  auto copy_range = [&](int t) {
    for (size_t i = (size_t)t; i < off.size(); i += (size_t)n_thr) {
      const size_t n = (size_t)n_samples[i], padded = (n + 7) & ~(size_t)7;
      if (esz == 4) { /* wide source on its way to the converter: all 32 bits */
        int32_t *dst = reinterpret_cast<int32_t *>(stage) + off[i];
        memcpy(dst, h_pcm[i], n * 4);
        for (size_t z = n; z < padded; ++z) dst[z] = 0;
        continue;
      }
      int16_t *dst = reinterpret_cast<int16_t *>(stage) + off[i];
      if (pcm_is_s32) {
        const int32_t *src = static_cast<const int32_t *>(h_pcm[i]);
        for (size_t j = 0; j < n; ++j) dst[j] = (int16_t)(src[j] >> 16);
      } else {
        memcpy(dst, h_pcm[i], n * 2);
      }
      for (size_t z = n; z < padded; ++z) dst[z] = 0;
    }
  };
  std::vector<std::thread> pool;
  for (int t = 1; t < n_thr; ++t) pool.emplace_back(copy_range, t);
  copy_range(0);
  for (auto &th : pool) th.join();
  if (getenv("BL_AMD_HOST_TRACE"))
    fprintf(stderr, "wave %d: wait %.1f ms, stage copy %.1f ms (%zu MB, %d threads)\n", wave, wait_ms,
            1e3 * (now() - t_b), elems * esz >> 20, n_thr);
  BL_HIP_CHECK(hipMemcpyAsync(d_arena, stage, elems * esz, hipMemcpyHostToDevice, s));
  return BL_OK;
}

/* native-rate arena -> 22 050 Hz arena of the same wave slot, same stream.  `desc` comes in as the staged songs and
 * leaves as the analysis sees them: stereo at 22 050 Hz, each at a multiple of 8 samples of arena22[k] (*d_pcm). */
int convert_wave(bl_amd_ctx *c, int k, const bl_rs_plan &geo, int in_rate, int wide, const void *d_arena,
                 std::vector<bl_amd_song_desc> &desc, hipStream_t s, const int16_t **d_pcm) {
  std::vector<bl_amd_resample_desc> rdesc(desc.size());
  size_t elems22 = 0;
  for (size_t i = 0; i < desc.size(); ++i) {
    const size_t frames = (size_t)(desc[i].n_samples / desc[i].channels);
    const size_t of = bl_rs_out_frames(&geo, frames, nullptr);
    bl_amd_resample_desc &r = rdesc[i];
    r.in_offset = desc[i].pcm_offset; r.out_offset = elems22; r.frames = (int32_t)frames; r.channels = desc[i].channels;
    desc[i].pcm_offset = elems22; desc[i].n_samples = (int32_t)(2 * of); desc[i].channels = 2;
    elems22 += (2 * of + 7) & ~(size_t)7;
  }
  if (blr_ensure(c->arena22[k], elems22 * 2 + 64) != BL_OK) return BL_UNEXPECTED;
  int16_t *d22 = static_cast<int16_t *>(c->arena22[k].p);
  if (blr_resample_device(c, d_arena, wide, rdesc.data(), (int)rdesc.size(), in_rate, d22, s) != BL_OK)
    return BL_UNEXPECTED;
  *d_pcm = d22;
  return BL_OK;
}

} // namespace

/* ---- host-memory batch: pinned staging, copy/compute overlap on 2 streams ---- */
int blr_analyze_host(bl_amd_ctx *c, const void *const *h_pcm, int pcm_is_s32, const int32_t *n_samples,
                     const int32_t *channels, const uint64_t *duration, int n_songs, int in_rate,
                     bl_amd_song_result *h_results, bl_amd_song_result **d_res_out) {
  /* songs at another rate than the analyzers' are converted on the device, wave by wave, between
   * the transfer and the analysis; wide sources then travel as int32 (the converter's float path
   * needs all their bits) */
  const bool convert = in_rate > 0 && in_rate != BL_RS_OUT_RATE;
  bl_rs_plan geo;
  memset(&geo, 0, sizeof geo);
  if (convert && bl_rs_plan_geometry(&geo, BL_RS_OUT_RATE, in_rate)) return BL_UNEXPECTED;
  const size_t esz = (convert && pcm_is_s32) ? 4 : 2; /* bytes per staged sample */
  if (check_songs(h_pcm, n_samples, channels, duration, n_songs, convert ? &geo : nullptr) != BL_OK)
    return BL_UNEXPECTED;
  if (blr_ensure(c->results, sizeof(bl_amd_song_result) * (size_t)n_songs) != BL_OK) return BL_UNEXPECTED;
  bl_amd_song_result *d_res = static_cast<bl_amd_song_result *>(c->results.p);
  if (d_res_out) *d_res_out = d_res; /* whatever happens below */
  const bool in_place = esz == 2 && !pcm_is_s32 && host_mode() == BL_AMD_HOST_REGISTERED;

  /* The scratch workspace is per context, so the waves' kernels follow each other (event chain
   * inside blr_analyze_device); the copies of wave w+1 overlap the kernels of wave w.  The host
   * only ever waits for a wave's TRANSFER (its pinned buffer is free again), never for its
   * kernels: the device arena is reused in stream order.  Waiting for the kernels put the
   * ~20 ms latency of the serial envelope tail between two transfers (44 instead of 55 GB/s). */
  WaveSlots slots(c);
  if (slots.open() != BL_OK) return BL_UNEXPECTED;
  /* waves of songs of at most host_wave_bytes of PCM each (one song may exceed it): by default large enough
   * that the ~20 ms latency of the serial envelope tail (paid once per wave) stays below
   * the wave's transfer time, small enough for two pinned and two device buffers */
  const size_t budget = c->host_wave_bytes / esz;
  std::vector<size_t> off;
  std::vector<bl_amd_song_desc> desc; /* the staged songs (native rate when converting) */
  for (int begin = 0, end, wave = 0; begin < n_songs; begin = end, ++wave) {
    const int k = wave & 1;
    size_t elems = 0;
    end = bl_wave_plan(n_samples, begin, n_songs, budget, off, elems);
    const double t_a = now();
    if (slots.reuse(k) != BL_OK) return BL_UNEXPECTED;
    const double wait_ms = 1e3 * (now() - t_a);
    if (blr_ensure(c->arena[k], elems * esz + 64) != BL_OK) return BL_UNEXPECTED;
    hipStream_t s = c->streams[k];
    int16_t *d_arena = static_cast<int16_t *>(c->arena[k].p);
    if ((in_place ? stage_registered(c, k, h_pcm + begin, n_samples + begin, off, d_arena, s)
                  : stage_pinned(c, k, wave, wait_ms, h_pcm + begin, pcm_is_s32, n_samples + begin, off, elems, esz,
                                 d_arena, s)) != BL_OK)
      return BL_UNEXPECTED;
    BL_HIP_CHECK(hipEventRecord(slots.done[k], s));
    slots.used[k] = true;
    desc.resize(off.size());
    for (size_t i = 0; i < off.size(); ++i) {
      bl_amd_song_desc &d = desc[i];
      d.pcm_offset = off[i]; d.n_samples = n_samples[begin + i]; d.channels = channels[begin + i];
      d.duration = duration[begin + i];
    }
    const int16_t *d_pcm = d_arena;
    if (convert && convert_wave(c, k, geo, in_rate, esz == 4, d_arena, desc, s, &d_pcm) != BL_OK) return BL_UNEXPECTED;
    if (blr_analyze_device(c, d_pcm, desc.data(), (int)desc.size(), d_res + begin, s, 7) != BL_OK) return BL_UNEXPECTED;
  }
  if (slots.close() != BL_OK) return BL_UNEXPECTED;
  if (h_results)
    BL_HIP_CHECK(hipMemcpy(h_results, d_res, sizeof(bl_amd_song_result) * (size_t)n_songs, hipMemcpyDeviceToHost));
  return BL_OK;
}

/* ========================================================================= */
/* C-ABI                                                                      */

extern "C" {

int bl_amd_set_host_transfer(int mode) {
  if (mode != BL_AMD_HOST_STAGED && mode != BL_AMD_HOST_REGISTERED) return BL_UNEXPECTED;
  g_host_mode.store(mode);
  return BL_OK;
}

/* the host batch on the default context (`dflt`) or a given one: blr_analyze_host with the context locked */
static int analyze_host(bl_amd_ctx *c, bool dflt, const void *const *h_pcm, int pcm_is_s32, const int32_t *n_samples,
                        const int32_t *channels, const uint64_t *duration, int n_songs, int in_rate,
                        bl_amd_song_result *h_results) {
  if (n_songs <= 0 || !h_pcm || !n_samples || !channels || !duration || !h_results || !(c = call_ctx(c, dflt)))
    return BL_UNEXPECTED;
  CtxGuard g(c);
  if (!g.ok()) return BL_UNEXPECTED;
  return blr_analyze_host(c, h_pcm, pcm_is_s32, n_samples, channels, duration, n_songs, in_rate, h_results, nullptr);
}

int bl_amd_ctx_analyze_batch_host(bl_amd_ctx *ctx, const int16_t *const *h_pcm, const int32_t *n_samples,
                                  const int32_t *channels, const uint64_t *duration, int n_songs,
                                  bl_amd_song_result *h_results) {
  return analyze_host(ctx, false, reinterpret_cast<const void *const *>(h_pcm), 0, n_samples, channels, duration,
                      n_songs, 0, h_results);
}

int bl_amd_analyze_batch_host(const int16_t *const *h_pcm, const int32_t *n_samples,
                              const int32_t *channels, const uint64_t *duration, int n_songs,
                              bl_amd_song_result *h_results) {
  return analyze_host(nullptr, true, reinterpret_cast<const void *const *>(h_pcm), 0, n_samples, channels, duration,
                      n_songs, 0, h_results);
}

int bl_amd_analyze_batch_host_s32(const int32_t *const *h_pcm, const int32_t *n_samples,
                                  const int32_t *channels, const uint64_t *duration, int n_songs,
                                  bl_amd_song_result *h_results) {
  return analyze_host(nullptr, true, reinterpret_cast<const void *const *>(h_pcm), 1, n_samples, channels, duration,
                      n_songs, 0, h_results);
}

int bl_amd_analyze_batch_host_rate(const void *const *h_pcm, int pcm_is_s32, const int32_t *n_samples,
                                   const int32_t *channels, const uint64_t *duration, int n_songs,
                                   int sample_rate, bl_amd_song_result *h_results) {
  if (sample_rate <= 0) return BL_UNEXPECTED;
  return analyze_host(nullptr, true, h_pcm, pcm_is_s32 != 0, n_samples, channels, duration, n_songs, sample_rate,
                      h_results);
}

/* The corpus loop of ref python/examples/make_m3u_playlist.py:51-72 / examples/analyze.c:17 as one
 * call: `for file: bl_analyze(file, &song)`.  Decoding (bl_audio_decode: FLAC / WAV readers, rate
 * converter) runs on n_threads host threads that stay a bounded number of files ahead; the calling
 * thread takes the decoded songs in file order, wave by wave, through the pinned-staging host path
 * (blr_analyze_host), so that the next wave is being decoded while this one is transferred and
 * analysed.  Every songs[i] ends up exactly as bl_analyze(filenames[i], &songs[i]) leaves it. */
int bl_amd_analyze_files(const char *const *filenames, int n_files, struct bl_song *songs, int *codes,
                         int n_threads, int keep_pcm) {
  if (n_files <= 0 || !filenames || !songs) return BL_UNEXPECTED;
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return BL_UNEXPECTED;
  if (n_threads <= 0) n_threads = (int)std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 32u);
  n_threads = std::min(n_threads, n_files);
  const size_t WAVE_BYTES = (size_t)1 << 30; /* decoded PCM per wave */
  /* The decoders run ahead of the wave being analysed by at most AHEAD_BYTES of decoded PCM (and AHEAD_FILES
   * files): a byte bound, because a file bound alone lets 768 ten-minute songs (40 GB) pile up on the host.
   * The file the consumer is waiting for is always taken, whatever the budget says, so the two cannot deadlock. */
  const size_t AHEAD_BYTES = 3 * WAVE_BYTES; /* bounds the READ-AHEAD only: with keep_pcm the caller keeps every decoded
                                               * sample_array (include/bliss_amd.h), and that total is the caller's */
  const int WAVE_FILES = 512, AHEAD_FILES = 768; /* AHEAD_FILES >= WAVE_FILES: a wave never waits for a file the decoders may not take */

  std::mutex mu;
  std::condition_variable cv;
  std::vector<signed char> state((size_t)n_files, 0); /* 0 pending, 1 decoded, -1 failed */
  int next = 0, limit = std::min(n_files, AHEAD_FILES); /* decoders take indices below `limit` */
  int want = 0;          /* the file the consumer needs next */
  size_t ahead_bytes = 0; /* decoded PCM not yet released by the consumer */
  bool stop = false;
  auto decoder = [&] {
    for (;;) {
      int i;
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return stop || next >= n_files || (next < limit && (ahead_bytes < AHEAD_BYTES || next <= want)); });
        if (stop || next >= n_files) return;
        i = next++;
      }
      /* bl_audio_decode initialises every field of songs[i] itself and fails on a NULL name: the caller's
       * structs may be uninitialised (ref tests/test_analyze.c:27-28), so it must run for every index */
      const int rc = bl_audio_decode(filenames[i], &songs[i]);
      if (rc != BL_OK) fprintf(stderr, "Couldn't decode song\n"); /* ref src/analyze.c:83 */
      {
        std::lock_guard<std::mutex> lk(mu);
        state[(size_t)i] = rc == BL_OK ? 1 : -1;
        if (rc == BL_OK && songs[i].sample_array) ahead_bytes += (size_t)songs[i].nSamples * 2;
      }
      cv.notify_all();
    }
  };
  std::vector<std::thread> pool;
  for (int t = 0; t < n_threads; ++t) pool.emplace_back(decoder);

  int done = 0, ok_count = 0, rc_all = BL_OK;
  std::vector<const void *> pcm;
  std::vector<int32_t> ns, ch;
  std::vector<uint64_t> du;
  std::vector<int> idx;
  std::vector<bl_amd_song_result> res;
  while (done < n_files) {
    /* the next wave: files in order until the byte or file budget is reached; wait for each decode */
    pcm.clear(); ns.clear(); ch.clear(); du.clear(); idx.clear();
    size_t bytes = 0;
    int e = done;
    while (e < n_files && (int)(e - done) < WAVE_FILES && bytes < WAVE_BYTES) {
      {
        std::unique_lock<std::mutex> lk(mu);
        if (state[(size_t)e] == 0) {
          want = e;
          cv.notify_all();
          cv.wait(lk, [&] { return state[(size_t)e] != 0; });
        }
      }
      if (codes) codes[e] = BL_UNEXPECTED;
      if (state[(size_t)e] == 1) {
        const struct bl_song &sg = songs[e];
        /* what run_song() of bl_api.c and validate_desc() accept; anything else is reported per file */
        if (sg.sample_array && sg.nSamples >= 5120 && (sg.channels == 1 || sg.channels == 2) && sg.duration > 0) {
          pcm.push_back(sg.sample_array); ns.push_back(sg.nSamples); ch.push_back(sg.channels);
          du.push_back(sg.duration); idx.push_back(e);
          bytes += (size_t)sg.nSamples * 2;
        } else {
          fprintf(stderr, "bliss_amd: %s not analysable (need >= 5120 s16 samples, 1 or 2 channels, >= 1 s)\n",
                  filenames[e]);
        }
      }
      ++e;
    }
    { /* let the decoders run ahead of the wave that is about to be analysed */
      std::lock_guard<std::mutex> lk(mu);
      limit = std::min(n_files, e + AHEAD_FILES);
    }
    cv.notify_all();
    if (!idx.empty()) {
      res.assign(idx.size(), bl_amd_song_result());
      const int rc = analyze_host(c, false, pcm.data(), 0, ns.data(), ch.data(), du.data(), (int)idx.size(), 0,
                                  res.data());
      if (rc != BL_OK) rc_all = BL_UNEXPECTED;
      for (size_t k = 0; k < idx.size(); ++k) {
        struct bl_song &sg = songs[idx[k]];
        if (rc == BL_OK && res[k].status == BL_OK) {
          sg.force_vector = res[k].v;            /* ref src/analyze.c:63-66 */
          sg.force = res[k].force;               /* ref :68-72 */
          sg.calm_or_loud = res[k].calm_or_loud; /* ref :73-79 */
          if (codes) codes[idx[k]] = res[k].calm_or_loud;
          ++ok_count;
        } else {
          fprintf(stderr, "Couldn't analyse song on the HIP device\n");
        }
      }
    }
    size_t released = 0;
    for (int i = done; i < e; ++i) {
      if (state[(size_t)i] == 1 && songs[i].sample_array) released += (size_t)songs[i].nSamples * 2;
      if (!keep_pcm) {
        free(songs[i].sample_array);
        songs[i].sample_array = NULL;
      }
    }
    {
      std::lock_guard<std::mutex> lk(mu);
      ahead_bytes -= std::min(released, ahead_bytes);
    }
    cv.notify_all();
    done = e;
  }
  {
    std::lock_guard<std::mutex> lk(mu);
    stop = true;
  }
  cv.notify_all();
  for (auto &t : pool) t.join();
  return rc_all == BL_OK ? ok_count : BL_UNEXPECTED;
}

} /* extern "C" */
