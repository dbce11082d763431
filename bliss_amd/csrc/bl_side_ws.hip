/*
 * bl_side_ws.hip — the side workspaces' registry, profiling and release (bl_side_ws.h has the protocol and the call
 * path).  Host code only.
 */
#include <map>
#include <memory>

#include "bl_side_ws.h"

namespace {

struct side_registry {
  std::mutex mu; /* guards g_ws itself; a workspace is its context's, under the context's mutex */
  std::map<bl_amd_ctx *, std::unique_ptr<bl_side_ws>> g_ws;
} g_side[SIDE_COUNT];

} // namespace

bl_side_ws *side_ws_of(int kind, bl_amd_ctx *c) {
  side_registry &r = g_side[kind];
  std::lock_guard<std::mutex> lk(r.mu);
  std::unique_ptr<bl_side_ws> &w = r.g_ws[c];
  if (!w) w.reset(new bl_side_ws());
  return w.get();
}

void side_mark(void *user, int k, hipStream_t s, int begin) {
  bl_side_ws *w = static_cast<bl_side_ws *>(user);
  std::lock_guard<std::mutex> lk(w->ev_mu);
  if (begin) {
    bl_side_ws::Ev e{k, nullptr, nullptr};
    if (hipEventCreate(&e.a) != hipSuccess || hipEventCreate(&e.b) != hipSuccess) return;
    (void)hipEventRecord(e.a, s);
    w->events.push_back(e);
  } else if (!w->events.empty() && w->events.back().k == k) {
    (void)hipEventRecord(w->events.back().b, s);
  }
}

double side_profile_ms(int kind, int k, int *launches) {
  side_registry &r = g_side[kind];
  std::lock_guard<std::mutex> lk(r.mu); /* a workspace cannot be released while this is held */
  double ms = 0.0;
  int n = 0;
  for (auto &kv : r.g_ws) {
    bl_side_ws &w = *kv.second;
    std::lock_guard<std::mutex> lk_ev(w.ev_mu);
    if (w.events.empty()) continue;
    DevGuard dg(kv.first->device);
    if (!dg.ok) continue;
    std::vector<bl_side_ws::Ev> keep;
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

/* ctx_release's hook (bl_runtime.hip): the caller holds the context, has made its device current and has waited for
 * the device */
void blr_side_release(bl_amd_ctx *c) {
  for (side_registry &r : g_side) {
    std::unique_ptr<bl_side_ws> w;
    {
      std::lock_guard<std::mutex> lk(r.mu);
      auto it = r.g_ws.find(c);
      if (it == r.g_ws.end()) continue;
      w = std::move(it->second);
      r.g_ws.erase(it);
    }
    if (w->recs.p) (void)hipFree(w->recs.p);
    for (bl_buf &b : w->extra)
      if (b.p) (void)hipFree(b.p);
    blr_ring_free(w->ring);
    if (w->ev_done) (void)hipEventDestroy(w->ev_done);
    for (auto &e : w->events) {
      (void)hipEventDestroy(e.a);
      (void)hipEventDestroy(e.b);
    }
  }
}
