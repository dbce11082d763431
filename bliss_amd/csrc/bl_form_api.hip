/*
 * bl_form_api.hip — call path and C-ABI of the song structure (include/bliss_amd.h: bl_amd_form_*); the kernels are
 * bl_form_kernels.hip's, the host arithmetic over the records bl_api.c's.  Host code only.
 *
 * The structure pass keeps its workspace beside the context's own, as the fingerprints do, one per context it has been
 * called on: the songs' records, a ring of pinned blocks they are staged in, and the units and the novelty of a call
 * that does not ask for them.  The protocol is the fingerprints' (bl_fprint_api.hip): a call holds the context
 * (CtxGuard), the map from context to workspace has a lock of its own that is held for the look-up only, a pinned block
 * counts as free once the event behind its copy has passed, a call waits on the device for the workspace's previous
 * user before it writes the records, the hand-over point moves behind a call's last launch whatever way the call ends,
 * and ctx_release (bl_runtime.hip) calls blr_form_release, which frees the workspace with the context.
 */
#include <string.h>

#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "bl_form.h"
#include "bl_runtime.h"

namespace {

struct form_ws {
  bl_buf recs, units, nov;
  bl_pin_slot ring[BL_PIN_SLOTS];
  int ring_next = 0;
  hipEvent_t ev_done = nullptr; /* behind the last launch of the last call */
  bool used = false;
  struct Ev { int k; hipEvent_t a, b; };
  std::mutex ev_mu;       /* guards events: a call appends, bl_amd_form_profile_ms collects */
  std::vector<Ev> events; /* kernel timing, while the context's profiling switch is on */
};

std::mutex g_mu; /* guards g_ws itself; a workspace is its context's, under the context's mutex */
std::map<bl_amd_ctx *, std::unique_ptr<form_ws>> g_ws;

/* the workspace of a context whose mutex the caller holds, made on first use */
form_ws *ws_of(bl_amd_ctx *c) {
  std::lock_guard<std::mutex> lk(g_mu);
  std::unique_ptr<form_ws> &w = g_ws[c];
  if (!w) w.reset(new form_ws());
  return w.get();
}

void form_mark(void *user, int k, hipStream_t s, int begin) {
  form_ws *w = static_cast<form_ws *>(user);
  std::lock_guard<std::mutex> lk(w->ev_mu);
  if (begin) {
    form_ws::Ev e{k, nullptr, nullptr};
    if (hipEventCreate(&e.a) != hipSuccess || hipEventCreate(&e.b) != hipSuccess) return;
    (void)hipEventRecord(e.a, s);
    w->events.push_back(e);
  } else if (!w->events.empty() && w->events.back().k == k) {
    (void)hipEventRecord(w->events.back().b, s);
  }
}

/* pinned block of at least `bytes`; blocks only when BL_PIN_SLOTS calls are still in flight */
int ws_pin(form_ws &w, size_t bytes, bl_pin_slot **out) {
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
  form_ws &w;
  hipStream_t s;
  bool armed = false;
  HandOver(form_ws &ws, hipStream_t st) : w(ws), s(st) {}
  ~HandOver() {
    if (armed && hipEventRecord(w.ev_done, s) == hipSuccess) w.used = true;
  }
};

/* what a call's counts add up to; false for a bad count */
struct form_totals {
  long long frames = 0, units = 0, groups = 0;
  int max_units = 0; /* the largest U that is not too long */
};
bool totals_of(const int32_t *h_frames, int n_songs, int pool, form_totals *t) {
  for (int i = 0; i < n_songs; ++i) {
    if (!form_count_ok(h_frames[i])) return false;
    const int u = h_frames[i] / pool;
    t->frames += h_frames[i];
    t->units += u;
    t->groups += (u + BL_FORM_BLOCK_UNITS - 1) / BL_FORM_BLOCK_UNITS;
    if (u <= BL_AMD_FORM_UNITS_MAX && u > t->max_units) t->max_units = u;
  }
  return true;
}

bool args_ok(const void *frames, const int32_t *h_frames, int n_songs, const bl_amd_form_params *p, const void *out,
             const void *units, const void *rep, const void *nov, form_totals *t) {
  return frames && !((uintptr_t)frames & 7) && h_frames && p && out && !((uintptr_t)out & 7) &&
         !((uintptr_t)units & 15) && !((uintptr_t)rep & 3) && !((uintptr_t)nov & 7) && n_songs >= 1 &&
         form_params_ok(*p) && totals_of(h_frames, n_songs, p->pool, t) && t->groups <= 0x7FFFFFFFll;
}

int form_device(bl_amd_ctx *c, bool dflt, const bl_amd_frame_chroma *d_frames, const int32_t *h_frames, int n_songs,
                const bl_amd_form_params *params, bl_amd_song_form *d_out, void *d_units_out, uint32_t *d_rep_out,
                uint64_t *d_nov_out, uint8_t *d_flags_out, long long n_units, void *stream) {
  form_totals t;
  if (!args_ok(d_frames, h_frames, n_songs, params, d_out, d_units_out, d_rep_out, d_nov_out, &t) || n_units != t.units)
    return BL_UNEXPECTED;
  const bl_amd_form_params p = *params;
  if (!(c = call_ctx(c, dflt))) return BL_UNEXPECTED;
  CtxGuard g(c);
  if (!g.ok()) return BL_UNEXPECTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  form_ws &w = *ws_of(c);
  if (!w.ev_done) BL_HIP_CHECK(hipEventCreateWithFlags(&w.ev_done, hipEventDisableTiming));
  const size_t bytes = sizeof(bl_form_song) * (size_t)n_songs;
  bl_pin_slot *slot = nullptr;
  if (ws_pin(w, bytes, &slot) != BL_OK) return BL_UNEXPECTED;
  bl_form_song *hs = static_cast<bl_form_song *>(slot->p);
  long long f = 0, u = 0, gr = 0;
  for (int i = 0; i < n_songs; ++i) {
    hs[i].frame_off = f;
    hs[i].unit_off = u;
    hs[i].group_off = gr;
    hs[i].frames = h_frames[i];
    hs[i].units = h_frames[i] / p.pool;
    f += hs[i].frames;
    u += hs[i].units;
    gr += (hs[i].units + BL_FORM_BLOCK_UNITS - 1) / BL_FORM_BLOCK_UNITS;
  }
  if (w.used) BL_HIP_CHECK(hipStreamWaitEvent(s, w.ev_done, 0));
  const size_t n1 = (size_t)(t.units ? t.units : 1); /* a block even where there is no unit */
  if (blr_ensure(w.recs, bytes) != BL_OK || (!d_units_out && blr_ensure(w.units, sizeof(uint4) * n1) != BL_OK) ||
      (!d_nov_out && blr_ensure(w.nov, 8 * n1) != BL_OK))
    return BL_UNEXPECTED;
  HandOver done(w, s);
  BL_HIP_CHECK(hipMemcpyAsync(w.recs.p, slot->p, bytes, hipMemcpyHostToDevice, s));
  done.armed = true;
  BL_HIP_CHECK(hipEventRecord(slot->ev, s));
  slot->busy = true;
  const bl_form_song *d_songs = static_cast<const bl_form_song *>(w.recs.p);
  uint4 *d_units = static_cast<uint4 *>(d_units_out ? d_units_out : w.units.p);
  unsigned long long *d_nov = d_nov_out ? reinterpret_cast<unsigned long long *>(d_nov_out)
                                        : static_cast<unsigned long long *>(w.nov.p);
  blk_mark_fn mark = c->prof ? form_mark : nullptr;
  if (blk_form_units(s, d_frames, d_songs, n_songs, t.groups, p.pool, d_units, mark, &w) != BL_OK ||
      blk_form_thumb(s, d_units, d_songs, n_songs, t.max_units, p.seg, p.min_lag, d_out, d_rep_out, mark, &w) != BL_OK ||
      blk_form_novelty(s, d_units, d_songs, n_songs, p.nov, p.peak_num, p.peak_den, d_out, d_nov, d_flags_out, mark,
                       &w) != BL_OK)
    return BL_UNEXPECTED;
  return BL_OK;
}

} // namespace

/* ctx_release's hook (bl_runtime.hip): the caller holds the context, has made its device current and has waited for
 * the device */
void blr_form_release(bl_amd_ctx *c) {
  std::unique_ptr<form_ws> w;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_ws.find(c);
    if (it == g_ws.end()) return;
    w = std::move(it->second);
    g_ws.erase(it);
  }
  for (bl_buf *b : {&w->recs, &w->units, &w->nov})
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

int bl_amd_ctx_form_device(bl_amd_ctx *c, const bl_amd_frame_chroma *d_frames, const int32_t *h_frames, int n_songs,
                           const bl_amd_form_params *params, bl_amd_song_form *d_out, void *d_units_out,
                           uint32_t *d_rep_out, uint64_t *d_nov_out, uint8_t *d_flags_out, long long n_units,
                           void *stream) {
  return form_device(c, false, d_frames, h_frames, n_songs, params, d_out, d_units_out, d_rep_out, d_nov_out,
                     d_flags_out, n_units, stream);
}

int bl_amd_form_device(const bl_amd_frame_chroma *d_frames, const int32_t *h_frames, int n_songs,
                       const bl_amd_form_params *params, bl_amd_song_form *d_out, void *d_units_out,
                       uint32_t *d_rep_out, uint64_t *d_nov_out, uint8_t *d_flags_out, long long n_units, void *stream) {
  return form_device(nullptr, true, d_frames, h_frames, n_songs, params, d_out, d_units_out, d_rep_out, d_nov_out,
                     d_flags_out, n_units, stream);
}

/* everything is uploaded, computed by the device form and fetched */
int bl_amd_form_host(const bl_amd_frame_chroma *h_frame_records, const int32_t *h_frames, int n_songs,
                     const bl_amd_form_params *params, bl_amd_song_form *h_out, void *h_units_out, uint32_t *h_rep_out,
                     uint64_t *h_nov_out, uint8_t *h_flags_out) {
  form_totals t;
  if (!h_frame_records || !h_frames || !params || !h_out || n_songs < 1 || !form_params_ok(*params) ||
      !totals_of(h_frames, n_songs, params->pool, &t))
    return BL_UNEXPECTED;
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return BL_UNEXPECTED;
  DevGuard dg(c->device);
  if (!dg.ok) return BL_UNEXPECTED;
  /* a block even where there is nothing to copy: the device form wants the frames' pointer */
  const size_t nu = (size_t)t.units;
  DevMem fr(sizeof(bl_amd_frame_chroma) * (size_t)(t.frames ? t.frames : 1)),
      out(sizeof(bl_amd_song_form) * (size_t)n_songs), units(h_units_out ? 16 * (nu ? nu : 1) : 0),
      rep(h_rep_out ? 8 * (nu ? nu : 1) : 0), nov(h_nov_out ? 8 * (nu ? nu : 1) : 0),
      flags(h_flags_out ? (nu ? nu : 1) : 0);
  if (!fr.ok() || !out.ok() || !units.ok() || !rep.ok() || !nov.ok() || !flags.ok()) return BL_UNEXPECTED;
  if (t.frames)
    BL_HIP_CHECK(hipMemcpy(fr.p, h_frame_records, sizeof(bl_amd_frame_chroma) * (size_t)t.frames, hipMemcpyHostToDevice));
  if (bl_amd_form_device(fr.as<bl_amd_frame_chroma>(), h_frames, n_songs, params, out.as<bl_amd_song_form>(), units.p,
                         rep.as<uint32_t>(), nov.as<uint64_t>(), flags.as<uint8_t>(), t.units, nullptr) != BL_OK)
    return BL_UNEXPECTED;
  BL_HIP_CHECK(hipStreamSynchronize(nullptr));
  if (!out.down(h_out)) return BL_UNEXPECTED;
  if (!nu) return BL_OK;
  return (!h_units_out || units.down(h_units_out, 16 * nu)) && (!h_rep_out || rep.down(h_rep_out, 8 * nu)) &&
                 (!h_nov_out || nov.down(h_nov_out, 8 * nu)) && (!h_flags_out || flags.down(h_flags_out, nu))
             ? BL_OK
             : BL_UNEXPECTED;
}

/* the lengths at which the kernels change path */
void bl_amd_form_shape(int *chunk_lags, int *units_block) {
  if (chunk_lags) *chunk_lags = BL_FORM_CHUNK_LAGS;
  if (units_block) *units_block = BL_FORM_BLOCK_UNITS;
}

/* device time of a structure kernel since this was last asked for it: "form_units", "form_thumb" or "form_novelty" */
double bl_amd_form_profile_ms(const char *name, int *launches) {
  if (launches) *launches = 0;
  const int k = !name                            ? -1
                : !strcmp(name, "form_units")    ? FMK_UNITS
                : !strcmp(name, "form_thumb")    ? FMK_THUMB
                : !strcmp(name, "form_novelty")  ? FMK_NOVELTY
                                                 : -1;
  if (k < 0) return -1.0;
  std::lock_guard<std::mutex> lk(g_mu); /* a workspace cannot be released while this is held */
  double ms = 0.0;
  int n = 0;
  for (auto &kv : g_ws) {
    form_ws &w = *kv.second;
    std::lock_guard<std::mutex> lk_ev(w.ev_mu);
    if (w.events.empty()) continue;
    DevGuard dg(kv.first->device);
    if (!dg.ok) continue;
    std::vector<form_ws::Ev> keep;
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
