/*
 * bl_runtime.hip — contexts, workspaces, streams and the single-device C-ABI of
 * include/bliss_amd.h (the analysis, the rate converter, the synthesis, the self-tests, the diagnostics), but for the
 * matrix, playlists and vector queries (bl_query_api.hip), the per-song features (bl_feature_api.hip: levels, timbre,
 * tempo, beats, chroma, mel; bl_*_api.hip for the newer ones) and the host batch and bl_amd_analyze_files
 * (bl_host_batch.hip).  Host code only (compiled by hipcc for the HIP runtime API); every
 * kernel lives in a bl_*kernels.hip file and is reached through the launchers of bl_launch.h.
 *
 * Contexts.  A bl_amd_ctx owns one device's scratch workspace, internal streams and pinned
 * staging.  The plain entry points (bl_amd_analyze_batch_device, ...) use the calling
 * thread's default context: the device chosen with bl_amd_init() on that thread, else the
 * process default (the first bl_amd_init of the process, else device 0).  One process can
 * therefore drive several GPUs from several threads, and explicit contexts
 * (bl_amd_ctx_create) give independent workspaces on one device.
 *
 * Asynchrony.  bl_amd_analyze_batch_device() only enqueues: descriptors go through a ring of
 * pinned slots (hipMemcpyAsync from pinned memory does not block), launch groups of more than
 * 32 768 songs follow each other on the stream, and the shared workspace is handed from one
 * batch to the next by an event, not by a host synchronisation.  Every entry point that uploads
 * per-song records (analysis, rate conversion, levels, timbre, tempo, beats, chroma, mel, synthesis, bld_mean_variance_host)
 * does so through record_call (bl_runtime.h), the one place that knows this protocol; the vector queries have
 * query_call beside it, which shares the hand-over (ws_wait, ws_pass) with it.  The loudness, the true peak, the
 * fingerprints, the song structure and the version matching keep workspaces of their own beside the context's and have side_call
 * (bl_side_ws.h), the same protocol over those; the pinned rings of both are served by blr_ring_get.
 *
 * Guards.  An entry point that uses the workspace takes a CtxGuard (context lock + device guard);
 * the *_batch_host forms (host_form, bl_runtime.h), the selftests and bl_amd_narrow_s32_device use no workspace
 * themselves and take a DevGuard alone.  Either way a device that cannot be made current ends the call.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <vector>

#include "bl_runtime.h"
#include "bl_ilog2.h"
#include "bl_resample.h"

namespace {

std::mutex g_mu;                       /* guards the default-context table */
bl_amd_ctx *g_default[BL_MAX_DEVICES]; /* lazily created, one per device */
std::atomic<int> g_process_device{-1};
thread_local int tl_device = -1;

void release_buf(bl_buf &b) {
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr;
  b.cap = 0;
}

/* the streams and events a context owns from ctx_init to ctx_release (streams[] of the host batch come on first use) */
hipStream_t bl_amd_ctx::*const kCtxStreams[] = {&bl_amd_ctx::side, &bl_amd_ctx::side2};
hipEvent_t bl_amd_ctx::*const kCtxEvents[] = {&bl_amd_ctx::ev_env, &bl_amd_ctx::ev_tail, &bl_amd_ctx::ev_head,
                                              &bl_amd_ctx::ev_tail2, &bl_amd_ctx::ev_ws};

int ctx_init(bl_amd_ctx *c, int device) {
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0) {
    fprintf(stderr, "bliss_amd: no HIP device available (%s); this library has no CPU path\n",
            e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    return BL_UNEXPECTED;
  }
  if (device < 0 || device >= count || device >= BL_MAX_DEVICES) {
    fprintf(stderr, "bliss_amd: device %d out of range (%d visible)\n", device, count);
    return BL_UNEXPECTED;
  }
  DevGuard dg(device);
  if (!dg.ok) return BL_UNEXPECTED;
  hipDeviceProp_t prop;
  BL_HIP_CHECK(hipGetDeviceProperties(&prop, device));
  c->device = device;
  c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  std::vector<unsigned char> h(blk_tables_bytes());
  blk_tables_fill_host(h.data());
  BL_HIP_CHECK(hipMalloc(&c->tables_mem, h.size()));
  BL_HIP_CHECK(hipMemcpy(c->tables_mem, h.data(), h.size(), hipMemcpyHostToDevice));
  c->tb = blk_tables_bind(c->tables_mem);
  if (blk_configure_device() != BL_OK || blk_query_configure_device() != BL_OK || blk_timbre_configure_device() != BL_OK ||
      blk_mel_configure_device() != BL_OK || blk_desc_chain_configure_device() != BL_OK)
    return BL_UNEXPECTED;
  {
    /* songs per launch group; lowered by the tests to exercise the multi-group path */
    const char *gs = getenv("BL_AMD_GROUP_SONGS");
    int g = gs ? atoi(gs) : BL_GROUP_SONGS_MAX;
    c->group_songs = g < 1 ? 1 : (g > BL_GROUP_SONGS_MAX ? BL_GROUP_SONGS_MAX : g);
    /* PCM bytes per wave of the host batch; lowered by the tests to exercise the multi-wave path */
    const char *wb = getenv("BL_AMD_HOST_WAVE_BYTES");
    const long long w = wb ? atoll(wb) : (long long)BL_HOST_WAVE_MAX;
    c->host_wave_bytes = w < 1 ? 1 : (w > (long long)BL_HOST_WAVE_MAX ? BL_HOST_WAVE_MAX : (size_t)w);
  }
  for (auto m : kCtxStreams) BL_HIP_CHECK(hipStreamCreateWithFlags(&(c->*m), hipStreamNonBlocking));
  for (auto m : kCtxEvents) BL_HIP_CHECK(hipEventCreateWithFlags(&(c->*m), hipEventDisableTiming));
  for (int k = 0; k < BL_PIN_SLOTS; ++k)
    BL_HIP_CHECK(hipEventCreateWithFlags(&c->ring[k].ev, hipEventDisableTiming));
  return BL_OK;
}

void prof_collect(bl_amd_ctx *c) {
  for (auto &e : c->events) {
    float ms = 0;
    if (hipEventSynchronize(e.b) == hipSuccess && hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) {
      c->prof_ms[e.k] += ms;
      c->prof_n[e.k] += 1;
    }
    (void)hipEventDestroy(e.a);
    (void)hipEventDestroy(e.b);
  }
  c->events.clear();
}

void ctx_release(bl_amd_ctx *c) {
  DevGuard dg(c->device);
  if (!dg.ok) return;
  (void)hipDeviceSynchronize();
  prof_collect(c);
  blr_side_release(c);
  bl_buf *bufs[] = {&c->songs,   &c->stats,   &c->hist, &c->spectrum, &c->energies, &c->lc,
                    &c->results, &c->arena[0], &c->arena[1], &c->arena22[0], &c->arena22[1],
                    &c->rs_songs, &c->rs_bank, &c->mx_my, &c->mx_gath, &c->mx_all, &c->mx_order, &c->mx_rows, &c->knn, &c->chain, &c->radius, &c->level_songs, &c->timbre_songs,
                    &c->rhythm_songs, &c->rhythm_n, &c->rhythm_rows, &c->beat_songs, &c->beat_links, &c->chroma_songs, &c->chroma_acc, &c->chroma_image,
                    &c->mel_songs, &c->mel_image, &c->desc};
  for (bl_buf *b : bufs) release_buf(*b);
  for (int k = 0; k < 2; ++k) {
    blr_unregister_wave(c, k);
    if (c->pinned[k]) (void)hipHostFree(c->pinned[k]);
    c->pinned[k] = nullptr;
    c->pinned_cap[k] = 0;
    if (c->streams[k]) (void)hipStreamDestroy(c->streams[k]);
    c->streams[k] = nullptr;
  }
  blr_ring_free(c->ring);
  if (c->tables_mem) (void)hipFree(c->tables_mem);
  c->tables_mem = nullptr;
  for (auto m : kCtxStreams) {
    if (c->*m) (void)hipStreamDestroy(c->*m);
    c->*m = nullptr;
  }
  for (auto m : kCtxEvents) {
    if (c->*m) (void)hipEventDestroy(c->*m);
    c->*m = nullptr;
  }
  c->ws_used = false;
  c->chroma_image_ready = false;
  c->mel_image_ready = false;
  c->rs_rate = 0;
  c->rs_kind = -1;
}

int current_device(void) {
  if (tl_device >= 0) return tl_device;
  const int d = g_process_device.load();
  return d >= 0 ? d : 0;
}

/* host mirror of the per-song geometry (integer work of ref tempo_atk_sort.c:63-67,
 * frequency_sort.c:50) for one launch group, written to `out` (pinned) */
void fill_group(const bl_amd_song_desc *desc, int n_songs, bl_dsong *out, long long &env_total,
                int &max_n) {
  env_total = 0;
  max_n = 0;
  for (int i = 0; i < n_songs; ++i) {
    const bl_amd_song_desc &d = desc[i];
    bl_dsong &s = out[i];
    s.pcm_off = d.pcm_offset;
    s.duration = d.duration;
    s.n = d.n_samples;
    s.channels = d.channels;
    s.n_frames = (d.n_samples / d.channels) / 512;
    s.nb_frames = (d.n_samples - (d.n_samples % 512)) * 2 / 512;
    s.n_windows = s.nb_frames - 2;
    s.env_off = env_total;
    s.reserved0 = 0;
    s.out_idx = i;
    s.reserved1 = 0;
    env_total += s.nb_frames;
    if (d.n_samples > max_n) max_n = d.n_samples;
  }
  /* Mixed-length corpora: process the records longest first.  The 64 songs that share a
   * wave of k_env_tail then have similar lengths (its straight-line steady-state path is
   * wave-uniform), and the long songs do not straggle at the end of the per-song grids.
   * Results go back to the caller's order through out_idx; scratch offsets keep the
   * caller's order too.  Equal lengths: the order is left alone. */
  bool mixed = false;
  for (int i = 1; i < n_songs && !mixed; ++i) mixed = out[i].n != out[0].n;
  if (mixed)
    std::stable_sort(out, out + n_songs, [](const bl_dsong &a, const bl_dsong &b) { return a.n > b.n; });
}

} // namespace

int blr_validate_desc(const bl_amd_song_desc &d, int i) {
  if (d.n_samples < 5120 || (d.channels != 1 && d.channels != 2) || d.duration == 0 ||
      (d.pcm_offset & 7)) {
    fprintf(stderr,
            "bliss_amd: song %d rejected (n_samples=%d channels=%d duration=%llu offset=%llu): "
            "need n_samples >= 5120, channels 1|2, duration > 0, offset %% 8 == 0\n",
            i, d.n_samples, d.channels, (unsigned long long)d.duration,
            (unsigned long long)d.pcm_offset);
    return BL_UNEXPECTED;
  }
  return BL_OK;
}

void mark_cb(void *user, int k, hipStream_t s, int begin) {
  bl_amd_ctx *c = static_cast<bl_amd_ctx *>(user);
  if (!c->prof) return;
  if (begin) {
    bl_amd_ctx::Ev e{k, nullptr, nullptr};
    if (hipEventCreate(&e.a) != hipSuccess || hipEventCreate(&e.b) != hipSuccess) return;
    (void)hipEventRecord(e.a, s);
    c->open.push_back(e);
  } else {
    for (size_t i = c->open.size(); i-- > 0;)
      if (c->open[i].k == k) {
        (void)hipEventRecord(c->open[i].b, s);
        c->events.push_back(c->open[i]);
        c->open.erase(c->open.begin() + (long)i);
        break;
      }
  }
}

int blr_ring_get(bl_pin_slot *ring, int &next, size_t bytes, bl_pin_slot **out) {
  bl_pin_slot &s = ring[next];
  next = (next + 1) % BL_PIN_SLOTS;
  if (s.busy) {
    BL_HIP_CHECK(hipEventSynchronize(s.ev));
    s.busy = false;
  }
  if (!s.ev) BL_HIP_CHECK(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
  if (s.cap < bytes) {
    if (s.p) (void)hipHostFree(s.p);
    s.p = nullptr;
    s.cap = 0;
    const size_t cap = bytes + bytes / 4 + 4096;
    BL_HIP_CHECK(hipHostMalloc(&s.p, cap, hipHostMallocDefault));
    s.cap = cap;
  }
  *out = &s;
  return BL_OK;
}

void blr_ring_free(bl_pin_slot *ring) {
  for (int k = 0; k < BL_PIN_SLOTS; ++k) {
    if (ring[k].p) (void)hipHostFree(ring[k].p);
    if (ring[k].ev) (void)hipEventDestroy(ring[k].ev);
    ring[k] = bl_pin_slot();
  }
}

int blr_ensure(bl_buf &b, size_t bytes) {
  if (bytes <= b.cap) return BL_OK;
  if (b.p) {
    /* growth is rare (capacity is kept); work in flight may still use the old block */
    BL_HIP_CHECK(hipDeviceSynchronize());
    BL_HIP_CHECK(hipFree(b.p));
    b.p = nullptr;
    b.cap = 0;
  }
  size_t cap = bytes + bytes / 8 + 4096;
  BL_HIP_CHECK(hipMalloc(&b.p, cap));
  b.cap = cap;
  return BL_OK;
}

hipStream_t blr_stream(bl_amd_ctx *c, int k) {
  if (!c->streams[k] && hipStreamCreateWithFlags(&c->streams[k], hipStreamNonBlocking) != hipSuccess) {
    fprintf(stderr, "bliss_amd: hipStreamCreateWithFlags failed (%s:%d)\n", __FILE__, __LINE__);
    c->streams[k] = nullptr;
  }
  return c->streams[k];
}

bl_amd_ctx *blr_default_ctx(void) {
  const int dev = current_device();
  if (dev < 0 || dev >= BL_MAX_DEVICES) return nullptr;
  std::lock_guard<std::mutex> lk(g_mu);
  if (!g_default[dev]) {
    bl_amd_ctx *c = new bl_amd_ctx();
    if (ctx_init(c, dev) != BL_OK) {
      ctx_release(c);
      delete c;
      return nullptr;
    }
    g_default[dev] = c;
  }
  return g_default[dev];
}

/* Enqueue the analysis of n_songs device-resident songs on `stream` (caller holds c->mu and
 * has made c->device current).  Nothing here waits for the device. */
int blr_analyze_device(bl_amd_ctx *c, const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs,
                       bl_amd_song_result *d_results, hipStream_t stream, int what) {
  for (int i = 0; i < n_songs; ++i)
    if (blr_validate_desc(h_desc[i], i) != BL_OK) return BL_UNEXPECTED;
  const int G = c->group_songs;
  const int n_groups = (n_songs + G - 1) / G;
  std::vector<long long> env_total(n_groups);
  std::vector<int> max_n(n_groups);
  /* all descriptors of the call in one pinned slot, one asynchronous copy */
  auto fill = [&](bl_dsong *hs) {
    for (int gi = 0; gi < n_groups; ++gi) {
      const int b = gi * G, cnt = std::min(G, n_songs - b);
      fill_group(h_desc + b, cnt, hs + b, env_total[gi], max_n[gi]);
    }
    return BL_OK;
  };
  auto launch = [&](const bl_dsong *hs, bl_dsong *d_songs) {
    const size_t gmax = (size_t)std::min(G, n_songs);
    size_t env_max = 0;
    for (long long t : env_total) env_max = std::max(env_max, (size_t)t);
    if (blr_ensure(c->stats, sizeof(bl_dstats) * gmax) != BL_OK) return BL_UNEXPECTED;
    if (blr_ensure(c->hist, sizeof(unsigned) * BL_HIST_BINS * gmax) != BL_OK) return BL_UNEXPECTED;
    if (blr_ensure(c->spectrum, sizeof(float) * 256 * gmax) != BL_OK) return BL_UNEXPECTED;
    if (blr_ensure(c->energies, sizeof(float) * env_max) != BL_OK) return BL_UNEXPECTED;
    if (blr_ensure(c->lc, sizeof(double) * env_max) != BL_OK) return BL_UNEXPECTED;
    for (int gi = 0; gi < n_groups; ++gi) {
      const int b = gi * G, cnt = std::min(G, n_songs - b);
      blk_analyze_args a;
      a.pcm = d_pcm;
      a.songs = d_songs + b;
      a.stats = static_cast<bl_dstats *>(c->stats.p);
      a.hist = static_cast<unsigned *>(c->hist.p);
      a.spectrum = static_cast<float *>(c->spectrum.p);
      a.energies = static_cast<float *>(c->energies.p);
      a.lc = static_cast<double *>(c->lc.p);
      a.results = d_results + b;
      a.n_songs = cnt;
      a.max_n = max_n[gi];
      /* a mixed-length group (sorted longest first by fill_group): the songs longer than a quarter of the longest
       * go first, in whole waves of the tail kernel, if both parts stay wide enough to fill the chip */
      if (cnt >= 1024 && hs[b].n != hs[b + cnt - 1].n) {
        int k = 0;
        while (k < cnt && hs[b + k].n > max_n[gi] / 4) ++k;
        k = (k + 63) / 64 * 64;
        if (k >= 256 && k <= cnt - 256) {
          a.n_head = k;
          a.max_n_rest = hs[b + k].n;
        }
      }
      a.what = what;
      a.n_cu = c->n_cu;
      a.tb = c->tb;
      a.stream = stream;
#ifdef BL_AMD_MEASURE
      a.side = getenv("BL_AMD_NO_SIDE") ? nullptr : c->side; /* measurement builds only: serialise the tail */
#else
      a.side = c->side;
#endif
      a.ev_env = c->ev_env;
      a.ev_tail = c->ev_tail;
      a.side2 = a.side ? c->side2 : nullptr;
      a.ev_head = c->ev_head;
      a.ev_tail2 = c->ev_tail2;
      a.mark = c->prof ? mark_cb : nullptr;
      a.mark_user = c;
      if (blk_analyze(a) != BL_OK) return BL_UNEXPECTED;
      c->last_env_total = env_total[gi];
      c->last_first = b;
      c->last_songs = cnt;
      c->last_parts = blk_analyze_parts(what);
    }
    return BL_OK;
  };
  return record_call<bl_dsong>(c, stream, c->songs, n_songs, fill, launch);
}

/* ---- device rate conversion (bl_rs_kernels.hip), shared by the C-ABI and the host batch ---- */

/* (re)build and upload the plan of (in_rate, kind); caller holds c->mu, device is current */
static int rs_prepare(bl_amd_ctx *c, int in_rate, int in_is_s32) {
  if (c->rs_rate == in_rate && c->rs_kind == in_is_s32) return BL_OK;
  bl_rs_plan p;
  if (bl_rs_plan_build(&p, BL_RS_OUT_RATE, in_rate, in_is_s32)) {
    fprintf(stderr, "bliss_amd: no conversion plan for %d Hz\n", in_rate);
    return BL_UNEXPECTED;
  }
  bl_rs_geom g;
  size_t lds = 0;
  int bank_lds = 0;
  if (blk_resample_geom(p.phase_count, p.taps, p.alloc, p.src_incr, p.dst_incr, &g, &lds, &bank_lds) != BL_OK) {
    fprintf(stderr, "bliss_amd: %d Hz is beyond the device converter (input span of a tile exceeds the LDS)\n",
            in_rate);
    bl_rs_plan_free(&p);
    return BL_UNEXPECTED;
  }
  /* 32-bit elements on the device: float as is, Q15 widened */
  const size_t elems = (size_t)p.phase_count * (size_t)p.alloc;
  std::vector<int32_t> host(elems);
  if (in_is_s32) memcpy(host.data(), p.fbank, elems * sizeof(float));
  else for (size_t i = 0; i < elems; ++i) host[i] = p.ibank[i];
  bl_rs_plan_free(&p); /* p stays as the geometry, its bank pointers null */
  /* a plan change is rare; kernels of the previous plan may still be reading the old bank */
  BL_HIP_CHECK(hipDeviceSynchronize());
  c->rs_rate = 0;
  c->rs_kind = -1;
  if (blr_ensure(c->rs_bank, elems * 4) != BL_OK) return BL_UNEXPECTED;
  BL_HIP_CHECK(hipMemcpy(c->rs_bank.p, host.data(), elems * 4, hipMemcpyHostToDevice));
  c->rs_geom = g;
  c->rs_lds = lds;
  c->rs_bank_lds = bank_lds;
  c->rs_plan = p;
  c->rs_rate = in_rate;
  c->rs_kind = in_is_s32;
  return BL_OK;
}

/* Enqueue the conversion of n_songs device-resident songs on `s` (caller holds c->mu and has
 * made c->device current). */
int blr_resample_device(bl_amd_ctx *c, const void *d_in, int in_is_s32, const bl_amd_resample_desc *h_desc,
                        int n_songs, int in_rate, int16_t *d_out, hipStream_t s) {
  in_is_s32 = in_is_s32 != 0;
  if (rs_prepare(c, in_rate, in_is_s32) != BL_OK) return BL_UNEXPECTED;
  auto fill = [&](bl_rs_dsong *hs) {
    for (int i = 0; i < n_songs; ++i) {
      const bl_amd_resample_desc &d = h_desc[i];
      size_t refl = 0;
      const size_t of = d.frames > 0 ? bl_rs_out_frames(&c->rs_plan, (size_t)d.frames, &refl) : 0;
      if (of == 0 || of > (size_t)INT32_MAX / 2 || (d.channels != 1 && d.channels != 2) ||
          (d.out_offset & 1) || (d.channels == 2 && (d.in_offset & 1))) {
        fprintf(stderr,
                "bliss_amd: resample: song %d rejected (frames=%d channels=%d in_offset=%llu out_offset=%llu): "
                "need frames > filter length (%d), channels 1|2, even offsets\n",
                i, d.frames, d.channels, (unsigned long long)d.in_offset, (unsigned long long)d.out_offset,
                c->rs_plan.taps);
        return BL_UNEXPECTED;
      }
      hs[i].in_off = d.in_offset;
      hs[i].out_off = d.out_offset;
      hs[i].frames = d.frames;
      hs[i].channels = d.channels;
      hs[i].out_frames = (int)of;
      hs[i].refl = (int)refl;
    }
    return BL_OK;
  };
  auto launch = [&](const bl_rs_dsong *hs, bl_rs_dsong *d_songs) {
    const int G = BL_GROUP_SONGS_MAX;
    for (int b = 0; b < n_songs; b += G) {
      const int cnt = std::min(G, n_songs - b);
      int max_out = 0;
      for (int i = 0; i < cnt; ++i) max_out = std::max(max_out, hs[b + i].out_frames);
      if (blk_resample(s, d_in, in_is_s32, d_songs + b, cnt, max_out, c->rs_bank.p, c->rs_geom, c->rs_lds,
                       c->rs_bank_lds, d_out) != BL_OK)
        return BL_UNEXPECTED;
    }
    return BL_OK;
  };
  return record_call<bl_rs_dsong>(c, s, c->rs_songs, n_songs, fill, launch);
}

/* the device sweeps behind the selftests: `sweep(d, n_cu)` adds to n zeroed counters on the device */
template <class Sweep>
static int selftest(uint64_t *counts, int n, Sweep sweep) {
  unsigned long long h[6];
  bl_amd_ctx *c = counts ? blr_default_ctx() : nullptr;
  if (!c) return BL_UNEXPECTED;
  DevGuard dg(c->device);
  if (!dg.ok) return BL_UNEXPECTED;
  DevMem d(sizeof(unsigned long long) * (size_t)n);
  if (!d.ok() || hipMemset(d.p, 0, d.bytes) != hipSuccess || sweep(d.as<unsigned long long>(), c->n_cu) != BL_OK ||
      !d.down(h))
    return BL_UNEXPECTED;
  for (int k = 0; k < n; ++k) counts[k] = h[k];
  return BL_OK;
}

/* ========================================================================= */
/* C-ABI                                                                      */

extern "C" {

int bl_amd_device_count(void) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess) return 0;
  return count;
}

int bl_amd_init(int device) {
  const int prev = tl_device;
  tl_device = device;
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) {
    tl_device = prev;
    return BL_UNEXPECTED;
  }
  int expect = -1;
  g_process_device.compare_exchange_strong(expect, device);
  return BL_OK;
}

int bld_ready(void) { return blr_default_ctx() ? BL_OK : BL_UNEXPECTED; }

int bl_amd_ctx_create(int device, bl_amd_ctx **out) {
  if (!out) return BL_UNEXPECTED;
  *out = nullptr;
  bl_amd_ctx *c = new bl_amd_ctx();
  if (ctx_init(c, device) != BL_OK) {
    ctx_release(c);
    delete c;
    return BL_UNEXPECTED;
  }
  *out = c;
  return BL_OK;
}

void bl_amd_ctx_destroy(bl_amd_ctx *ctx) {
  if (!ctx) return;
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx_release(ctx);
  }
  delete ctx;
}

int bl_amd_ctx_device(const bl_amd_ctx *ctx) { return ctx ? ctx->device : BL_UNEXPECTED; }

void bl_amd_profile(int enable) {
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return;
  std::lock_guard<std::mutex> lk(c->mu);
  c->prof = enable != 0;
}

void bl_amd_profile_reset(void) {
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return;
  CtxGuard g(c);
  if (!g.ok()) return;
  prof_collect(c);
  for (int k = 0; k < PK_COUNT; ++k) { c->prof_ms[k] = 0; c->prof_n[k] = 0; }
}

double bl_amd_profile_ms(const char *name, int *launches) {
  static const char *const kProfNames[PK_COUNT] = {"pcm_scan",    "amp_finish", "freq_frames", "freq_finish",
                                                   "env_windows", "env_tail",   "distance",    "freq_scan",
                                                   "rhythm_hops", "rhythm_acf", "rhythm_pick",
                                                   "chroma_pitch", "chroma_key",
                                                   "desc_range",  "desc_quantize", "desc_knn", "desc_merge",
                                                   "beats"};
  if (launches) *launches = 0;
  bl_amd_ctx *c = blr_default_ctx();
  if (!c || !name) return -1.0;
  CtxGuard g(c);
  if (!g.ok()) return -1.0;
  prof_collect(c);
  for (int k = 0; k < PK_COUNT; ++k)
    if (!strcmp(name, kProfNames[k])) {
      if (launches) *launches = c->prof_n[k];
      return c->prof_ms[k];
    }
  return -1.0;
}

int bl_amd_ctx_analyze_batch_device(bl_amd_ctx *ctx, const int16_t *d_pcm, const bl_amd_song_desc *h_desc,
                                    int n_songs, bl_amd_song_result *d_results, void *stream) {
  if (!ctx || n_songs <= 0 || !d_pcm || !h_desc || !d_results) return BL_UNEXPECTED;
  CtxGuard g(ctx);
  if (!g.ok()) return BL_UNEXPECTED;
  return blr_analyze_device(ctx, d_pcm, h_desc, n_songs, d_results, static_cast<hipStream_t>(stream), 7);
}

int bl_amd_analyze_batch_device(const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs,
                                bl_amd_song_result *d_results, void *stream) {
  return bl_amd_ctx_analyze_batch_device(blr_default_ctx(), d_pcm, h_desc, n_songs, d_results, stream);
}

/* L on the device against the same source on the host (bl_ilog2.h), over bl_ilog2_sweep_value */
int bl_amd_selftest_ilog2(uint64_t counts[2]) {
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return BL_UNEXPECTED;
  DevGuard dg(c->device);
  if (!dg.ok) return BL_UNEXPECTED;
  DevMem d(sizeof(uint32_t) * (size_t)BL_ILOG2_SWEEP);
  std::vector<uint32_t> h(BL_ILOG2_SWEEP);
  if (!d.ok() || hipMemset(d.p, 0xFF, d.bytes) != hipSuccess || blk_ilog2_sweep(nullptr, d.as<uint32_t>(), c->n_cu) != BL_OK ||
      !d.down(h.data()))
    return BL_UNEXPECTED;
  uint64_t checked = 0, wrong = 0;
  for (uint32_t i = 0; i < BL_ILOG2_SWEEP; ++i) {
    const uint64_t x = bl_ilog2_sweep_value(i);
    if (!x) continue;
    checked += 1;
    wrong += h[i] != bl_ilog2_q12(x);
  }
  if (counts) { counts[0] = checked; counts[1] = wrong; }
  return wrong ? BL_UNEXPECTED : BL_OK;
}

int bl_amd_selftest_isqrt(uint64_t counts[2]) {
  return selftest(counts, 2, [](unsigned long long *d, int n_cu) { return blk_isqrt_sweep(nullptr, d, n_cu); });
}

int bl_amd_synth_pcm_device(int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs,
                            uint32_t seed_base, uint32_t sample_rate, void *stream) {
  if (n_songs <= 0 || !d_pcm || !h_desc) return BL_UNEXPECTED;
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return BL_UNEXPECTED;
  CtxGuard g(c);
  if (!g.ok()) return BL_UNEXPECTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int i = 0; i < n_songs; ++i)
    if (blr_validate_desc(h_desc[i], i) != BL_OK) return BL_UNEXPECTED;
  const int G = BL_GROUP_SONGS_MAX;
  std::vector<int> max_n((n_songs + G - 1) / G);
  /* the descriptor block of the workspace is shared with the analysis */
  return record_call<bl_dsong>(c, s, c->songs, n_songs, [&](bl_dsong *hs) {
    for (int b = 0, gi = 0; b < n_songs; b += G, ++gi) {
      long long env_total;
      fill_group(h_desc + b, std::min(G, n_songs - b), hs + b, env_total, max_n[gi]);
    }
    return BL_OK;
  }, [&](const bl_dsong *, bl_dsong *d_songs) {
    for (int b = 0, gi = 0; b < n_songs; b += G, ++gi)
      if (blk_synth(s, d_pcm, d_songs + b, std::min(G, n_songs - b), max_n[gi], c->n_cu, seed_base + (uint32_t)b,
                    sample_rate) != BL_OK)
        return BL_UNEXPECTED;
    return BL_OK;
  });
}

int bl_amd_selftest_sqrt(uint64_t counts[3]) {
  return selftest(counts, 3, [](unsigned long long *d, int n_cu) {
    return blk_sqrt_sweep(nullptr, 0ull, 1ull << 32, d, n_cu); /* every f32 bit pattern */
  });
}

int bl_amd_selftest_cos(uint64_t counts[6], uint64_t triples) {
  return selftest(counts, 6, [&](unsigned long long *d, int n_cu) {
    const unsigned long long threads = (unsigned long long)n_cu * 8 * 256;
    const int per_thread = (int)std::min<unsigned long long>((triples / 8 + threads - 1) / threads, 1u << 24);
    return blk_cos_sweep(nullptr, 0x5eedc05ull, std::max(per_thread, 1), d, n_cu);
  });
}

int bl_amd_narrow_s32_device(const int32_t *d_in, int16_t *d_out, size_t n, void *stream) {
  if (!d_in || !d_out) return BL_UNEXPECTED;
  if (n == 0) return BL_OK;
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return BL_UNEXPECTED;
  DevGuard dg(c->device);
  if (!dg.ok) return BL_UNEXPECTED;
  return blk_narrow_s32(static_cast<hipStream_t>(stream), d_in, d_out, n, c->n_cu);
}

/* ---- rate conversion (bl_resample.c on the host, bl_rs_kernels.hip on the device) ---- */

size_t bl_amd_resample_out_frames(size_t frames, int in_rate) {
  bl_rs_plan p;
  if (bl_rs_plan_geometry(&p, BL_RS_OUT_RATE, in_rate)) return 0;
  return bl_rs_out_frames(&p, frames, nullptr);
}

int bl_amd_resample_host(const void *in, int in_is_s32, size_t frames, int channels, int in_rate,
                         int16_t **out, size_t *out_frames) {
  if (!out || !out_frames) return BL_UNEXPECTED;
  return bl_resample_to_stereo_s16(in, in_is_s32, frames, channels, in_rate, BL_RS_OUT_RATE, out, out_frames);
}

int bl_amd_ctx_resample_batch_device(bl_amd_ctx *c, const void *d_in, int in_is_s32,
                                     const bl_amd_resample_desc *h_desc, int n_songs, int in_rate,
                                     int16_t *d_out, void *stream) {
  if (!c || !d_in || !d_out || !h_desc || n_songs <= 0 || in_rate <= 0 || (in_is_s32 != 0 && in_is_s32 != 1))
    return BL_UNEXPECTED; /* float sources: host form only */
  CtxGuard g(c);
  if (!g.ok()) return BL_UNEXPECTED;
  return blr_resample_device(c, d_in, in_is_s32, h_desc, n_songs, in_rate, d_out, static_cast<hipStream_t>(stream));
}

int bl_amd_resample_batch_device(const void *d_in, int in_is_s32, const bl_amd_resample_desc *h_desc,
                                 int n_songs, int in_rate, int16_t *d_out, void *stream) {
  return bl_amd_ctx_resample_batch_device(blr_default_ctx(), d_in, in_is_s32, h_desc, n_songs, in_rate,
                                          d_out, stream);
}


/* ---- helpers behind the reference-API shims of bl_api.c ---- */
int bld_analyze_one_host(const int16_t *h_pcm, int n, int channels, uint64_t duration, int what,
                         bl_amd_song_result *res) {
  if (!h_pcm || !res) return BL_UNEXPECTED;
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return BL_UNEXPECTED;
  CtxGuard g(c);
  if (!g.ok()) return BL_UNEXPECTED;
  hipStream_t s = blr_stream(c, 0);
  if (!s) return BL_UNEXPECTED;
  const size_t elems = ((size_t)n + 7) & ~(size_t)7;
  if (blr_ensure(c->arena[0], elems * 2 + 64) != BL_OK) return BL_UNEXPECTED;
  if (blr_ensure(c->results, sizeof(bl_amd_song_result)) != BL_OK) return BL_UNEXPECTED;
  /* the copies below come before blr_analyze_device's own wait, so the previous user is waited for here */
  if (ws_wait(c, s) != BL_OK) return BL_UNEXPECTED;
  BL_HIP_CHECK(hipMemcpyAsync(c->arena[0].p, h_pcm, (size_t)n * 2, hipMemcpyHostToDevice, s));
  BL_HIP_CHECK(hipMemsetAsync(c->results.p, 0, sizeof(bl_amd_song_result), s));
  bl_amd_song_desc d;
  d.pcm_offset = 0; d.n_samples = n; d.channels = channels; d.duration = duration;
  if (blr_analyze_device(c, static_cast<const int16_t *>(c->arena[0].p), &d, 1,
                         static_cast<bl_amd_song_result *>(c->results.p), s, what) != BL_OK)
    return BL_UNEXPECTED;
  BL_HIP_CHECK(hipMemcpyAsync(res, c->results.p, sizeof(bl_amd_song_result), hipMemcpyDeviceToHost, s));
  BL_HIP_CHECK(hipStreamSynchronize(s));
  return BL_OK;
}

int bld_mean_variance_host(const int16_t *h_pcm, int n, int have_mean, int mean_in, int *mean_out,
                           int *variance_out) {
  if (!h_pcm || n <= 0) return BL_UNEXPECTED;
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return BL_UNEXPECTED;
  CtxGuard g(c);
  if (!g.ok()) return BL_UNEXPECTED;
  hipStream_t s = blr_stream(c, 0);
  if (!s) return BL_UNEXPECTED;
  const size_t elems = ((size_t)n + 7) & ~(size_t)7;
  if (blr_ensure(c->arena[0], elems * 2 + 64) != BL_OK) return BL_UNEXPECTED;
  if (blr_ensure(c->stats, sizeof(bl_dstats)) != BL_OK) return BL_UNEXPECTED;
  if (blr_ensure(c->hist, sizeof(unsigned) * BL_HIST_BINS) != BL_OK) return BL_UNEXPECTED;
  /* same workspace as the batches, same hand-over; the song goes up behind the wait for the previous user */
  return record_call<bl_dsong>(c, s, c->songs, 1, [&](bl_dsong *hs) {
    memset(hs, 0, sizeof *hs);
    hs->n = n; hs->channels = 1; hs->duration = 1;
    return BL_OK;
  }, [&](const bl_dsong *, bl_dsong *d_songs) {
    BL_HIP_CHECK(hipMemcpyAsync(c->arena[0].p, h_pcm, (size_t)n * 2, hipMemcpyHostToDevice, s));
    bl_dstats *d_stats = static_cast<bl_dstats *>(c->stats.p);
    const int16_t *d_pcm = static_cast<const int16_t *>(c->arena[0].p);
    if (blk_scan_one(s, d_pcm, d_songs, d_stats, static_cast<unsigned *>(c->hist.p), n, c->n_cu) != BL_OK)
      return BL_UNEXPECTED;
    c->last_first = 0;
    c->last_songs = 1;
    c->last_parts = BL_AMD_PART_SUMS | BL_AMD_PART_HIST;
    bl_dstats st;
    BL_HIP_CHECK(hipMemcpyAsync(&st, d_stats, sizeof st, hipMemcpyDeviceToHost, s));
    BL_HIP_CHECK(hipStreamSynchronize(s));
    /* ref helpers.c:30-37 */
    const int mean = have_mean ? mean_in : (int)(unsigned)(st.sum & 0xFFFFFFFFull) / n;
    if (mean_out) *mean_out = mean;
    if (variance_out) {
      /* always the exact wrapping form (ref helpers.c:39-49) for the stand-alone helper */
      st.mean = mean; st.wrap_pass = 1; st.wrap_acc = 0;
      BL_HIP_CHECK(hipMemcpyAsync(d_stats, &st, sizeof st, hipMemcpyHostToDevice, s));
      if (blk_variance_wrap_one(s, d_pcm, d_songs, d_stats, n, c->n_cu) != BL_OK) return BL_UNEXPECTED;
      BL_HIP_CHECK(hipMemcpyAsync(&st, d_stats, sizeof st, hipMemcpyDeviceToHost, s));
      BL_HIP_CHECK(hipStreamSynchronize(s));
      *variance_out = (int)(st.wrap_acc / n);
    }
    return BL_OK;
  });
}

/* diagnostic: the per-window energies (ref tempo_atk_sort.c:150, filtered_array) of the
 * most recent launch group, songs concatenated, nb_frames slots per song (last two unused) */
long long bl_amd_last_energies(float *h_out, long long max_elems) {
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return -1;
  CtxGuard g(c);
  if (!g.ok()) return -1;
  if (!c->energies.p || c->last_env_total <= 0) return 0;
  const long long n = c->last_env_total < max_elems ? c->last_env_total : max_elems;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpy(h_out, c->energies.p, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess)
    return -1;
  return n;
}

/* diagnostic: the summed spectrum, the raw sums and the raw histogram of the most recent launch group, un-permuted
 * from the workspace's processing order (slot = block index) to the caller's through the records' out_idx */
int bl_amd_last_freq_stats(int max_songs, float *h_spectrum, long long *h_sum, unsigned long long *h_sumsq,
                           unsigned *h_hist, int *parts) {
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return -1;
  CtxGuard g(c);
  if (!g.ok()) return -1;
  const int n = c->last_songs;
  if (parts) *parts = n > 0 ? c->last_parts : 0;
  if (n <= 0) return 0;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  std::vector<bl_dsong> songs((size_t)n);
  if (hipMemcpy(songs.data(), static_cast<const bl_dsong *>(c->songs.p) + c->last_first, sizeof(bl_dsong) * (size_t)n,
                hipMemcpyDeviceToHost) != hipSuccess)
    return -1;
  for (int i = 0; i < n; ++i)
    if (songs[i].out_idx < 0 || songs[i].out_idx >= n) return -1;
  /* one workspace at a time through a staging block, rows scattered to the caller's order */
  auto fetch = [&](const bl_buf &ws, size_t row_bytes, void *out, size_t out_off, size_t out_bytes) -> bool {
    if (!out) return true;
    if (!ws.p || ws.cap < row_bytes * (size_t)n) return false;
    std::vector<unsigned char> tmp(row_bytes * (size_t)n);
    if (hipMemcpy(tmp.data(), ws.p, tmp.size(), hipMemcpyDeviceToHost) != hipSuccess) return false;
    for (int i = 0; i < n; ++i) {
      const int to = songs[i].out_idx;
      if (to < max_songs)
        memcpy(static_cast<unsigned char *>(out) + out_bytes * (size_t)to, tmp.data() + row_bytes * (size_t)i + out_off,
               out_bytes);
    }
    return true;
  };
  if (!fetch(c->spectrum, sizeof(float) * 256, h_spectrum, 0, sizeof(float) * 256) ||
      !fetch(c->stats, sizeof(bl_dstats), h_sum, offsetof(bl_dstats, sum), sizeof(long long)) ||
      !fetch(c->stats, sizeof(bl_dstats), h_sumsq, offsetof(bl_dstats, sumsq), sizeof(unsigned long long)) ||
      !fetch(c->hist, sizeof(unsigned) * BL_HIST_BINS, h_hist, 0, sizeof(unsigned) * BL_HIST_BINS))
    return -1;
  return n;
}

/* diagnostic: k_env_tail on a compressed envelope the caller supplies.  The group is the product's own (fill_group:
 * env_off, n_windows, longest first) and so is the launch (blk_env_tail); of the workspace only `lc` is written —
 * descriptors and records live in blocks of their own, so bl_amd_last_energies and bl_amd_last_freq_stats answer what
 * they answered before. */
int bl_amd_tail_from_envelope(const bl_amd_song_desc *h_desc, int n_songs, const double *h_env, long long n_env,
                              bl_amd_song_result *h_results) {
  if (!h_desc || !h_env || !h_results || n_songs <= 0 || n_songs > BL_GROUP_SONGS_MAX) return BL_UNEXPECTED;
  for (int i = 0; i < n_songs; ++i)
    if (blr_validate_desc(h_desc[i], i) != BL_OK || h_desc[i].channels != 1 || h_desc[i].pcm_offset != 0) return BL_UNEXPECTED;
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return BL_UNEXPECTED;
  CtxGuard g(c);
  if (!g.ok()) return BL_UNEXPECTED;
  std::vector<bl_dsong> hs((size_t)n_songs);
  long long env_total = 0;
  int max_n = 0;
  fill_group(h_desc, n_songs, hs.data(), env_total, max_n);
  if (env_total != n_env) return BL_UNEXPECTED;
  /* whatever used the workspace last has finished before lc is overwritten */
  BL_HIP_CHECK(hipDeviceSynchronize());
  if (blr_ensure(c->lc, sizeof(double) * (size_t)env_total) != BL_OK) return BL_UNEXPECTED;
  DevMem d_songs(sizeof(bl_dsong) * (size_t)n_songs), d_res(sizeof(bl_amd_song_result) * (size_t)n_songs);
  if (!d_songs.up(hs.data()) || !d_res.ok()) return BL_UNEXPECTED;
  BL_HIP_CHECK(hipMemset(d_res.p, 0, d_res.bytes));
  BL_HIP_CHECK(hipMemcpy(c->lc.p, h_env, sizeof(double) * (size_t)env_total, hipMemcpyHostToDevice));
  blk_analyze_args a{};
  a.songs = d_songs.as<bl_dsong>();
  a.lc = static_cast<double *>(c->lc.p);
  a.results = d_res.as<bl_amd_song_result>();
  a.n_songs = n_songs;
  a.max_n = max_n;
  blk_env_tail(a, nullptr, 0, n_songs);
  BL_HIP_CHECK(hipGetLastError());
  BL_HIP_CHECK(hipDeviceSynchronize());
  if (!d_res.down(h_results)) return BL_UNEXPECTED;
  for (int i = 0; i < n_songs; ++i) { /* the geometry the other kernels write into a record */
    bl_amd_song_result &r = h_results[hs[i].out_idx];
    r.nb_frames = hs[i].nb_frames;
    r.n_windows = hs[i].n_windows;
    r.status = BL_OK;
  }
  return BL_OK;
}

void bl_multi_shutdown(void); /* bl_multi.hip */

void bl_amd_shutdown(void) {
  bl_multi_shutdown();
  std::lock_guard<std::mutex> lk(g_mu);
  for (int d = 0; d < BL_MAX_DEVICES; ++d) {
    if (!g_default[d]) continue;
    {
      std::lock_guard<std::mutex> lk2(g_default[d]->mu);
      ctx_release(g_default[d]);
    }
    delete g_default[d];
    g_default[d] = nullptr;
  }
}

} /* extern "C" */
