/*
 * bl_tpeak_api.hip — call path and C-ABI of the true peak (include/bliss_amd.h: bl_amd_tpeak_*); the kernels are
 * bl_tpeak_kernels.hip's, the host arithmetic over the records bl_api.c's.  Host code only.
 *
 * The true peak keeps its workspace beside the context's own, as the loudness does (bl_loud_api.hip), one per context
 * it has been called on: the songs' records, one accumulator per song, a ring of pinned blocks for the records.  The
 * protocol is the loudness's: a call holds the context (CtxGuard), the map from context to workspace has a lock of its
 * own that is held for the look-up only, a pinned block counts as free once the event behind its copy has passed, a
 * call waits on the device for the workspace's previous user before anything of it writes a block, the hand-over point
 * moves behind a call's last launch whatever way the call ends, and ctx_release (bl_runtime.hip) calls
 * blr_tpeak_release, which frees the context's workspace with the context.
 */
#include <string.h>

#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "bl_runtime.h"
#include "bl_tpeak.h"
#include "bl_waves.h"

namespace {

struct tpeak_ws {
  bl_buf songs, acc;
  bl_pin_slot ring[BL_PIN_SLOTS];
  int ring_next = 0;
  hipEvent_t ev_done = nullptr; /* behind the last launch of the last call */
  bool used = false;
  struct Ev { int k; hipEvent_t a, b; };
  std::mutex ev_mu;       /* guards events: a call appends, bl_amd_tpeak_profile_ms collects */
  std::vector<Ev> events; /* kernel timing, while the context's profiling switch is on */
};

std::mutex g_mu; /* guards g_ws itself; a workspace is its context's, under the context's mutex */
std::map<bl_amd_ctx *, std::unique_ptr<tpeak_ws>> g_ws;

/* the workspace of a context whose mutex the caller holds, made on first use */
tpeak_ws *ws_of(bl_amd_ctx *c) {
  std::lock_guard<std::mutex> lk(g_mu);
  std::unique_ptr<tpeak_ws> &w = g_ws[c];
  if (!w) w.reset(new tpeak_ws());
  return w.get();
}

void tpeak_mark(void *user, int k, hipStream_t s, int begin) {
  tpeak_ws *w = static_cast<tpeak_ws *>(user);
  std::lock_guard<std::mutex> lk(w->ev_mu);
  if (begin) {
    tpeak_ws::Ev e{k, nullptr, nullptr};
    if (hipEventCreate(&e.a) != hipSuccess || hipEventCreate(&e.b) != hipSuccess) return;
    (void)hipEventRecord(e.a, s);
    w->events.push_back(e);
  } else if (!w->events.empty() && w->events.back().k == k) {
    (void)hipEventRecord(w->events.back().b, s);
  }
}

/* pinned block of at least `bytes`; blocks only when BL_PIN_SLOTS calls are still in flight */
int ws_pin(tpeak_ws &w, size_t bytes, bl_pin_slot **out) {
  bl_pin_slot &s = w.ring[w.ring_next];
  w.ring_next = (w.ring_next + 1) % BL_PIN_SLOTS;
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

/* moves the workspace's hand-over point behind whatever a call has enqueued, however the call ends */
struct HandOver {
  tpeak_ws &w;
  hipStream_t s;
  bool armed = false;
  HandOver(tpeak_ws &ws, hipStream_t st) : w(ws), s(st) {}
  ~HandOver() {
    if (armed && hipEventRecord(w.ev_done, s) == hipSuccess) w.used = true;
  }
};

int tpeak_device(bl_amd_ctx *c, bool dflt, const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs,
                 int ceiling, int block, bl_amd_song_tpeak *d_songs_out, uint32_t *d_blocks_out, long long n_blocks,
                 void *stream) {
  if (!d_pcm || ((uintptr_t)d_pcm & 15) || !h_desc || !d_songs_out || ((uintptr_t)d_songs_out & 7) ||
      ((uintptr_t)d_blocks_out & 3) || n_songs < 1 || !tpeak_args_ok(ceiling, block))
    return BL_UNEXPECTED;
  long long total = 0, groups = 0; /* the sums of ceil(F / block) and of ceil(F / 4096) over the songs */
  for (int i = 0; i < n_songs; ++i) {
    if (!tpeak_song_ok(h_desc[i].pcm_offset, h_desc[i].n_samples, h_desc[i].channels)) return BL_UNEXPECTED;
    total += tpeak_blocks(h_desc[i].n_samples, h_desc[i].channels, block);
    groups += tpeak_blocks(h_desc[i].n_samples, h_desc[i].channels, BL_TPEAK_GROUP_FRAMES);
  }
  if ((d_blocks_out && n_blocks != total) || groups > (1ll << 30) || !(c = call_ctx(c, dflt))) return BL_UNEXPECTED;
  CtxGuard g(c);
  if (!g.ok()) return BL_UNEXPECTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  tpeak_ws &w = *ws_of(c);
  if (!w.ev_done) BL_HIP_CHECK(hipEventCreateWithFlags(&w.ev_done, hipEventDisableTiming));
  const size_t bytes = sizeof(bl_tpeak_song) * (size_t)n_songs;
  bl_pin_slot *slot = nullptr;
  if (ws_pin(w, bytes, &slot) != BL_OK) return BL_UNEXPECTED;
  bl_tpeak_song *hs = static_cast<bl_tpeak_song *>(slot->p);
  total = groups = 0;
  for (int i = 0; i < n_songs; ++i) {
    hs[i].pcm_off = h_desc[i].pcm_offset;
    hs[i].group_off = groups;
    hs[i].blk_off = total;
    hs[i].frames = h_desc[i].n_samples / h_desc[i].channels;
    hs[i].channels = h_desc[i].channels;
    total += tpeak_blocks(h_desc[i].n_samples, h_desc[i].channels, block);
    groups += tpeak_blocks(h_desc[i].n_samples, h_desc[i].channels, BL_TPEAK_GROUP_FRAMES);
  }
  if (w.used) BL_HIP_CHECK(hipStreamWaitEvent(s, w.ev_done, 0));
  if (blr_ensure(w.songs, bytes) != BL_OK || blr_ensure(w.acc, sizeof(bl_tpeak_acc) * (size_t)n_songs) != BL_OK)
    return BL_UNEXPECTED;
  bl_tpeak_song *d_songs = static_cast<bl_tpeak_song *>(w.songs.p);
  HandOver done(w, s);
  BL_HIP_CHECK(hipMemcpyAsync(d_songs, hs, bytes, hipMemcpyHostToDevice, s));
  done.armed = true;
  BL_HIP_CHECK(hipEventRecord(slot->ev, s));
  slot->busy = true;
  return blk_tpeak(s, d_pcm, d_songs, n_songs, groups, ceiling, block, static_cast<bl_tpeak_acc *>(w.acc.p),
                   d_songs_out, d_blocks_out, total, c->prof ? tpeak_mark : nullptr, &w);
}

} // namespace

/* ctx_release's hook (bl_runtime.hip): the caller holds the context, has made its device current and has waited for
 * the device */
void blr_tpeak_release(bl_amd_ctx *c) {
  std::unique_ptr<tpeak_ws> w;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_ws.find(c);
    if (it == g_ws.end()) return;
    w = std::move(it->second);
    g_ws.erase(it);
  }
  for (bl_buf *b : {&w->songs, &w->acc})
    if (b->p) (void)hipFree(b->p);
  for (bl_pin_slot &s : w->ring) {
    if (s.p) (void)hipHostFree(s.p);
    if (s.ev) (void)hipEventDestroy(s.ev);
  }
  if (w->ev_done) (void)hipEventDestroy(w->ev_done);
  for (auto &e : w->events) {
    (void)hipEventDestroy(e.a);
    (void)hipEventDestroy(e.b);
  }
}

/* ========================================================================= */
/* C-ABI                                                                      */

extern "C" {

int bl_amd_ctx_tpeak_batch_device(bl_amd_ctx *c, const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs,
                                  int ceiling, int block, bl_amd_song_tpeak *d_songs_out, uint32_t *d_blocks_out,
                                  long long n_blocks, void *stream) {
  return tpeak_device(c, false, d_pcm, h_desc, n_songs, ceiling, block, d_songs_out, d_blocks_out, n_blocks, stream);
}

int bl_amd_tpeak_batch_device(const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs, int ceiling, int block,
                              bl_amd_song_tpeak *d_songs_out, uint32_t *d_blocks_out, long long n_blocks,
                              void *stream) {
  return tpeak_device(nullptr, true, d_pcm, h_desc, n_songs, ceiling, block, d_songs_out, d_blocks_out, n_blocks,
                      stream);
}

/* the songs in waves of at most 256 MiB of PCM (bl_wave_plan; a longer song is a wave of its own): each is laid out in
 * a device arena, copied there, measured by the device form and fetched */
int bl_amd_tpeak_batch_host(const int16_t *const *h_pcm, const int32_t *n_samples, const int32_t *channels, int n_songs,
                            int ceiling, int block, bl_amd_song_tpeak *h_songs_out, uint32_t *h_blocks_out) {
  if (!h_pcm || !n_samples || !channels || !h_songs_out || n_songs < 1 || !tpeak_args_ok(ceiling, block))
    return BL_UNEXPECTED;
  for (int i = 0; i < n_songs; ++i)
    if (!h_pcm[i] || !tpeak_song_ok(0, n_samples[i], channels[i])) return BL_UNEXPECTED;
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return BL_UNEXPECTED;
  DevGuard dg(c->device);
  if (!dg.ok) return BL_UNEXPECTED;
  size_t budget;
  {
    std::lock_guard<std::mutex> lk(c->mu);
    budget = std::min((size_t)128 << 20, c->host_wave_bytes / 2);
  }
  std::vector<size_t> off;
  std::vector<bl_amd_song_desc> desc;
  for (int b = 0, e; b < n_songs; b = e) {
    size_t total = 0;
    e = bl_wave_plan(n_samples, b, n_songs, budget, off, total);
    desc.resize(off.size());
    long long blocks = 0;
    for (int i = b; i < e; ++i) {
      desc[i - b].pcm_offset = off[i - b];
      desc[i - b].n_samples = n_samples[i];
      desc[i - b].channels = channels[i];
      desc[i - b].duration = 0;
      blocks += tpeak_blocks(n_samples[i], channels[i], block);
    }
    DevMem arena(sizeof(int16_t) * total), out(sizeof(bl_amd_song_tpeak) * (size_t)(e - b)),
        bout(h_blocks_out ? 8 * (size_t)blocks : 0);
    if (!arena.ok() || !out.ok() || !bout.ok()) return BL_UNEXPECTED;
    for (int i = b; i < e; ++i)
      BL_HIP_CHECK(hipMemcpy(arena.as<int16_t>() + desc[i - b].pcm_offset, h_pcm[i],
                             sizeof(int16_t) * (size_t)n_samples[i], hipMemcpyHostToDevice));
    if (bl_amd_tpeak_batch_device(arena.as<int16_t>(), desc.data(), e - b, ceiling, block,
                                  out.as<bl_amd_song_tpeak>(), bout.as<uint32_t>(), blocks, nullptr) != BL_OK)
      return BL_UNEXPECTED;
    BL_HIP_CHECK(hipStreamSynchronize(nullptr));
    if (!out.down(h_songs_out + b) || (h_blocks_out && blocks && !bout.down(h_blocks_out))) return BL_UNEXPECTED;
    if (h_blocks_out) h_blocks_out += 2 * blocks;
  }
  return BL_OK;
}

/* the kernel's two tiling constants */
void bl_amd_tpeak_shape(int *frames_per_lane, int *frames_per_group) {
  if (frames_per_lane) *frames_per_lane = BL_TPEAK_LANE_FRAMES;
  if (frames_per_group) *frames_per_group = BL_TPEAK_GROUP_FRAMES;
}

/* device time of a true-peak kernel since this was last asked for it: "tpeak_scan" or "tpeak_finish" */
double bl_amd_tpeak_profile_ms(const char *name, int *launches) {
  if (launches) *launches = 0;
  const int k = !name ? -1 : !strcmp(name, "tpeak_scan") ? TK_SCAN : !strcmp(name, "tpeak_finish") ? TK_FINISH : -1;
  if (k < 0) return -1.0;
  std::lock_guard<std::mutex> lk(g_mu); /* a workspace cannot be released while this is held */
  double ms = 0.0;
  int n = 0;
  for (auto &kv : g_ws) {
    tpeak_ws &w = *kv.second;
    std::lock_guard<std::mutex> lk_ev(w.ev_mu);
    if (w.events.empty()) continue;
    DevGuard dg(kv.first->device);
    if (!dg.ok) continue;
    std::vector<tpeak_ws::Ev> keep;
    for (auto &e : w.events) {
      if (e.k != k) {
        keep.push_back(e);
        continue;
      }
      float t = 0.f;
      if (hipEventSynchronize(e.b) == hipSuccess && hipEventElapsedTime(&t, e.a, e.b) == hipSuccess) {
        ms += t;
        n += 1;
      } else {
        (void)hipGetLastError();
      }
      (void)hipEventDestroy(e.a);
      (void)hipEventDestroy(e.b);
    }
    w.events.swap(keep);
  }
  if (launches) *launches = n;
  return ms;
}

} /* extern "C" */
