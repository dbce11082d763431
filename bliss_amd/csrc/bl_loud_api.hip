/*
 * bl_loud_api.hip — call path and C-ABI of the K-weighted gated loudness (include/bliss_amd.h: bl_amd_loud_*); the
 * kernels are bl_loud_kernels.hip's, the host arithmetic bl_api.c's.  Host code only.
 *
 * The loudness keeps its workspace beside the context's own, one per context it has been called on (the records, the
 * hop energies of a call without a hops output, the short-term sums, a ring of pinned blocks for the records), and
 * leaves the layout of bl_amd_ctx alone.  A call holds the context like every other entry point (CtxGuard: its mutex
 * and its device), so calls on one context are ordered and contexts are independent of each other; the map from
 * context to workspace has a lock of its own that is held for the look-up only.  ctx_release (bl_runtime.hip) calls
 * blr_loud_release, which frees the context's workspace with the context.  The protocol is the one of the contexts'
 * record uploads: a pinned block counts as free once the event behind its copy has passed (BL_PIN_SLOTS calls may be
 * in flight before a caller waits), a call waits on the device for the workspace's previous user before anything of
 * it writes a block, the hand-over point moves behind a call's last launch whatever way the call ends, and a block
 * grows only behind a device synchronisation (blr_ensure).
 */
#include <string.h>

#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "bl_loud.h"
#include "bl_runtime.h"
#include "bl_waves.h"

namespace {

struct loud_ws {
  bl_buf songs, z, st;
  bl_pin_slot ring[BL_PIN_SLOTS];
  int ring_next = 0;
  hipEvent_t ev_done = nullptr; /* behind the last launch of the last call */
  bool used = false;
  struct Ev { int k; hipEvent_t a, b; };
  std::mutex ev_mu;       /* guards events: a call appends, bl_amd_loud_profile_ms collects */
  std::vector<Ev> events; /* kernel timing, while the context's profiling switch is on */
};

std::mutex g_mu; /* guards g_ws itself; a workspace is its context's, under the context's mutex */
std::map<bl_amd_ctx *, std::unique_ptr<loud_ws>> g_ws;

/* the workspace of a context whose mutex the caller holds, made on first use */
loud_ws *ws_of(bl_amd_ctx *c) {
  std::lock_guard<std::mutex> lk(g_mu);
  std::unique_ptr<loud_ws> &w = g_ws[c];
  if (!w) w.reset(new loud_ws());
  return w.get();
}

void loud_mark(void *user, int k, hipStream_t s, int begin) {
  loud_ws *w = static_cast<loud_ws *>(user);
  std::lock_guard<std::mutex> lk(w->ev_mu);
  if (begin) {
    loud_ws::Ev e{k, nullptr, nullptr};
    if (hipEventCreate(&e.a) != hipSuccess || hipEventCreate(&e.b) != hipSuccess) return;
    (void)hipEventRecord(e.a, s);
    w->events.push_back(e);
  } else if (!w->events.empty() && w->events.back().k == k) {
    (void)hipEventRecord(w->events.back().b, s);
  }
}

/* pinned block of at least `bytes`; blocks only when BL_PIN_SLOTS calls are still in flight */
int ws_pin(loud_ws &w, size_t bytes, bl_pin_slot **out) {
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
  loud_ws &w;
  hipStream_t s;
  bool armed = false;
  HandOver(loud_ws &ws, hipStream_t st) : w(ws), s(st) {}
  ~HandOver() {
    if (armed && hipEventRecord(w.ev_done, s) == hipSuccess) w.used = true;
  }
};

/* One call on n_songs songs, from PCM (d_z_in == nullptr) or from hop energies on the device; the caller holds the
 * context (CtxGuard).  `song(i, rec)` writes pcm_off, hops and channels of song i in the caller's order.  The records
 * are sorted stereo first: a wave of k_loud_filter whose lanes all have one channel count runs one shape.  Z goes to
 * d_hops_out where there is one and to the workspace otherwise; both kernels see the same pointer, so the records
 * cannot depend on which it is. */
template <class Song>
int loud_call(bl_amd_ctx *c, hipStream_t s, int n_songs, Song song, const int16_t *d_pcm, const uint64_t *d_z_in,
              const bl_amd_loud_params &p, bl_amd_song_loud *d_songs_out, uint64_t *d_hops_out) {
  loud_ws &w = *ws_of(c);
  if (!w.ev_done) BL_HIP_CHECK(hipEventCreateWithFlags(&w.ev_done, hipEventDisableTiming));
  const size_t bytes = sizeof(bl_loud_song) * (size_t)n_songs;
  bl_pin_slot *slot = nullptr;
  if (ws_pin(w, bytes, &slot) != BL_OK) return BL_UNEXPECTED;
  bl_loud_song *hs = static_cast<bl_loud_song *>(slot->p);
  long long hops = 0, starts = 0, chunks = 0;
  for (int i = 0; i < n_songs; ++i) {
    song(i, hs[i]);
    hs[i].hop_off = hops;
    hs[i].st_off = starts;
    hs[i].out_idx = i;
    hs[i].reserved = 0;
    hops += hs[i].hops;
    starts += blk_loud_starts(hs[i].hops);
  }
  std::stable_sort(hs, hs + n_songs, [](const bl_loud_song &a, const bl_loud_song &b) { return a.channels > b.channels; });
  for (int i = 0; i < n_songs; ++i) {
    hs[i].chunk_off = chunks;
    chunks += (hs[i].hops + BL_AMD_LOUD_CHUNK - 1) / BL_AMD_LOUD_CHUNK;
  }
  if (chunks > (1ll << 30)) return BL_UNEXPECTED; /* nothing has been enqueued: the slot stays free */
  if (w.used) BL_HIP_CHECK(hipStreamWaitEvent(s, w.ev_done, 0));
  unsigned long long *z = reinterpret_cast<unsigned long long *>(d_z_in ? const_cast<uint64_t *>(d_z_in) : d_hops_out);
  if (blr_ensure(w.songs, bytes) != BL_OK || blr_ensure(w.st, 8 * (size_t)std::max(starts, 1ll)) != BL_OK ||
      (!z && blr_ensure(w.z, 16 * (size_t)std::max(hops, 1ll)) != BL_OK))
    return BL_UNEXPECTED;
  if (!z) z = static_cast<unsigned long long *>(w.z.p);
  bl_loud_song *d_songs = static_cast<bl_loud_song *>(w.songs.p);
  HandOver done(w, s);
  BL_HIP_CHECK(hipMemcpyAsync(d_songs, hs, bytes, hipMemcpyHostToDevice, s));
  done.armed = true;
  BL_HIP_CHECK(hipEventRecord(slot->ev, s));
  slot->busy = true;
  blk_mark_fn mark = c->prof ? loud_mark : nullptr;
  if (!d_z_in && blk_loud_filter(s, d_pcm, d_songs, n_songs, chunks, p, z, mark, &w) != BL_OK) return BL_UNEXPECTED;
  return blk_loud_gate(s, z, d_songs, n_songs, p.abs_gate, static_cast<unsigned long long *>(w.st.p), d_songs_out, mark,
                       &w);
}

int loud_device(bl_amd_ctx *c, bool dflt, const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs,
                const bl_amd_loud_params *params, bl_amd_song_loud *d_songs_out, uint64_t *d_hops_out, long long n_hops,
                void *stream) {
  if (!d_pcm || ((uintptr_t)d_pcm & 15) || !h_desc || !d_songs_out || ((uintptr_t)d_songs_out & 7) ||
      ((uintptr_t)d_hops_out & 7) || n_songs < 1 || !loud_params_ok(params, false))
    return BL_UNEXPECTED;
  const bl_amd_loud_params p = *params;
  long long total = 0; /* the sum of H over the songs */
  for (int i = 0; i < n_songs; ++i) {
    if (!loud_song_ok(h_desc[i].pcm_offset, h_desc[i].n_samples, h_desc[i].channels)) return BL_UNEXPECTED;
    total += loud_hops(h_desc[i].n_samples, h_desc[i].channels, p.hop);
  }
  if ((d_hops_out && n_hops != total) || !(c = call_ctx(c, dflt))) return BL_UNEXPECTED;
  CtxGuard g(c);
  if (!g.ok()) return BL_UNEXPECTED;
  return loud_call(c, static_cast<hipStream_t>(stream), n_songs, [&](int i, bl_loud_song &r) {
    r.pcm_off = h_desc[i].pcm_offset;
    r.hops = loud_hops(h_desc[i].n_samples, h_desc[i].channels, p.hop);
    r.channels = h_desc[i].channels;
  }, d_pcm, nullptr, p, d_songs_out, d_hops_out);
}

} // namespace

/* ctx_release's hook (bl_runtime.hip): the caller holds the context, has made its device current and has waited for
 * the device */
void blr_loud_release(bl_amd_ctx *c) {
  std::unique_ptr<loud_ws> w;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_ws.find(c);
    if (it == g_ws.end()) return;
    w = std::move(it->second);
    g_ws.erase(it);
  }
  for (bl_buf *b : {&w->songs, &w->z, &w->st})
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

int bl_amd_ctx_loud_batch_device(bl_amd_ctx *c, const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs,
                                 const bl_amd_loud_params *params, bl_amd_song_loud *d_songs_out, uint64_t *d_hops_out,
                                 long long n_hops, void *stream) {
  return loud_device(c, false, d_pcm, h_desc, n_songs, params, d_songs_out, d_hops_out, n_hops, stream);
}

int bl_amd_loud_batch_device(const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs,
                             const bl_amd_loud_params *params, bl_amd_song_loud *d_songs_out, uint64_t *d_hops_out,
                             long long n_hops, void *stream) {
  return loud_device(nullptr, true, d_pcm, h_desc, n_songs, params, d_songs_out, d_hops_out, n_hops, stream);
}

/* stages 4 to 6 on the caller's hop energies: uploaded, through the same gate launch as the device form, fetched */
int bl_amd_loud_from_hops(const uint64_t *h_hop_energy, const int32_t *h_hops, int n_songs,
                          const bl_amd_loud_params *params, bl_amd_song_loud *h_songs_out) {
  if (!h_hops || !h_songs_out || n_songs < 1 || !loud_params_ok(params, true)) return BL_UNEXPECTED;
  long long total = 0;
  for (int i = 0; i < n_songs; ++i) {
    if (h_hops[i] < 0 || h_hops[i] > (1 << 27)) return BL_UNEXPECTED;
    total += h_hops[i];
  }
  if (total && !h_hop_energy) return BL_UNEXPECTED;
  for (long long k = 0; k < 2 * total; ++k)
    if (h_hop_energy[k] >= (1ull << 46)) return BL_UNEXPECTED;
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return BL_UNEXPECTED;
  CtxGuard g(c);
  if (!g.ok()) return BL_UNEXPECTED;
  DevMem zin(16 * (size_t)std::max(total, 1ll)), out(sizeof(bl_amd_song_loud) * (size_t)n_songs);
  if (!zin.ok() || !out.ok()) return BL_UNEXPECTED;
  if (total) BL_HIP_CHECK(hipMemcpy(zin.p, h_hop_energy, 16 * (size_t)total, hipMemcpyHostToDevice));
  if (loud_call(c, nullptr, n_songs, [&](int i, bl_loud_song &r) {
        r.pcm_off = 0;
        r.hops = h_hops[i];
        r.channels = 2;
      }, nullptr, zin.as<uint64_t>(), *params, out.as<bl_amd_song_loud>(), nullptr) != BL_OK)
    return BL_UNEXPECTED;
  BL_HIP_CHECK(hipStreamSynchronize(nullptr));
  return out.down(h_songs_out) ? BL_OK : BL_UNEXPECTED;
}

/* the songs in waves of at most 256 MiB of PCM (bl_wave_plan; a longer song is a wave of its own): each is laid out in
 * a device arena, copied there, measured by the device form and fetched */
int bl_amd_loud_batch_host(const int16_t *const *h_pcm, const int32_t *n_samples, const int32_t *channels, int n_songs,
                           const bl_amd_loud_params *params, bl_amd_song_loud *h_songs_out, uint64_t *h_hops_out) {
  if (!h_pcm || !n_samples || !channels || !h_songs_out || n_songs < 1 || !loud_params_ok(params, false))
    return BL_UNEXPECTED;
  for (int i = 0; i < n_songs; ++i)
    if (!h_pcm[i] || !loud_song_ok(0, n_samples[i], channels[i])) return BL_UNEXPECTED;
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
    long long hops = 0;
    for (int i = b; i < e; ++i) {
      desc[i - b].pcm_offset = off[i - b];
      desc[i - b].n_samples = n_samples[i];
      desc[i - b].channels = channels[i];
      desc[i - b].duration = 0;
      hops += loud_hops(n_samples[i], channels[i], params->hop);
    }
    DevMem arena(sizeof(int16_t) * total), out(sizeof(bl_amd_song_loud) * (size_t)(e - b)),
        zout(h_hops_out ? 16 * (size_t)hops : 0);
    if (!arena.ok() || !out.ok() || !zout.ok()) return BL_UNEXPECTED;
    for (int i = b; i < e; ++i)
      BL_HIP_CHECK(hipMemcpy(arena.as<int16_t>() + desc[i - b].pcm_offset, h_pcm[i],
                             sizeof(int16_t) * (size_t)n_samples[i], hipMemcpyHostToDevice));
    if (bl_amd_loud_batch_device(arena.as<int16_t>(), desc.data(), e - b, params, out.as<bl_amd_song_loud>(),
                                 zout.as<uint64_t>(), hops, nullptr) != BL_OK)
      return BL_UNEXPECTED;
    BL_HIP_CHECK(hipStreamSynchronize(nullptr));
    if (!out.down(h_songs_out + b) || (h_hops_out && hops && !zout.down(h_hops_out))) return BL_UNEXPECTED;
    if (h_hops_out) h_hops_out += 2 * hops;
  }
  return BL_OK;
}

/* device time of a loudness kernel since this was last asked for it: "loud_filter" or "loud_gate" */
double bl_amd_loud_profile_ms(const char *name, int *launches) {
  if (launches) *launches = 0;
  const int k = !name ? -1 : !strcmp(name, "loud_filter") ? LK_FILTER : !strcmp(name, "loud_gate") ? LK_GATE : -1;
  if (k < 0) return -1.0;
  std::lock_guard<std::mutex> lk(g_mu); /* a workspace cannot be released while this is held */
  double ms = 0.0;
  int n = 0;
  for (auto &kv : g_ws) {
    loud_ws &w = *kv.second;
    std::lock_guard<std::mutex> lk_ev(w.ev_mu);
    if (w.events.empty()) continue;
    DevGuard dg(kv.first->device);
    if (!dg.ok) continue;
    std::vector<loud_ws::Ev> keep;
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
