/*
 * bl_side_ws.h — the workspace that the loudness, the true peak, the fingerprints, the song structure, the version
 * matching, the chords, the tempogram and the beats that follow it each keep beside the context's own, and the one call
 * path over it (bl_loud_api.hip, bl_tpeak_api.hip, bl_fprint_api.hip, bl_form_api.hip, bl_cover_api.hip,
 * bl_chords_api.hip, bl_tgram_api.hip, bl_tbeats_api.hip).  Host code only; the bodies that are no templates are bl_side_ws.hip's.
 *
 * A feature (its `kind`) has one workspace per context it has been called on, made by the first call: the records of a
 * call, a few further blocks of the feature's own, a ring of pinned blocks the records are staged in.  The layout of
 * bl_amd_ctx stays as it is, and a feature's calls wait for that feature's previous call alone, never for an analysis
 * call on another stream.  The protocol is the one of the contexts' record uploads (record_call, bl_runtime.h):
 *  - a call holds its context like every other entry point (CtxGuard: its mutex and its device), so calls on one context
 *    are ordered and contexts are independent of each other;
 *  - each kind has a map from context to workspace with a lock of its own, held for the look-up only (and by
 *    side_profile_ms while it collects, so a workspace cannot be released under it);
 *  - a pinned block counts as free once the event behind its copy has passed: BL_PIN_SLOTS calls may be in flight
 *    before a caller waits;
 *  - a call waits on the device for the workspace's previous user before anything of it writes a block;
 *  - the hand-over point moves behind a call's last launch whatever way the call ends, once anything is enqueued;
 *  - a block grows only behind a device synchronisation (blr_ensure);
 *  - ctx_release (bl_runtime.hip) calls blr_side_release, which frees the context's workspaces with the context.
 */
#ifndef BL_SIDE_WS_H_
#define BL_SIDE_WS_H_

#include "bl_runtime.h"

enum { SIDE_LOUD, SIDE_TPEAK, SIDE_FPRINT, SIDE_FORM, SIDE_COVER, SIDE_CHORDS, SIDE_TGRAM, SIDE_TBEATS, SIDE_COUNT };
#define BL_SIDE_EXTRA 2 /* blocks besides the records: loudness, structure, chords and the following beats two, true peak and matching one, fingerprints and tempogram none */

struct bl_side_ws {
  bl_buf recs, extra[BL_SIDE_EXTRA];
  bl_pin_slot ring[BL_PIN_SLOTS];
  int ring_next = 0;
  hipEvent_t ev_done = nullptr; /* behind the last launch of the last call */
  bool used = false;
  struct Ev { int k; hipEvent_t a, b; };
  std::mutex ev_mu;       /* guards events: a call appends, side_profile_ms collects */
  std::vector<Ev> events; /* kernel timing, while the context's profiling switch is on */
};

/* the workspace of a context whose mutex the caller holds, made on first use */
bl_side_ws *side_ws_of(int kind, bl_amd_ctx *c);
/* the profiling callback of the launchers (blk_mark_fn); user: the workspace */
void side_mark(void *user, int k, hipStream_t s, int begin);
/* device time of kernel k of a kind since this was last asked for it, summed over the contexts; *launches may be null */
double side_profile_ms(int kind, int k, int *launches);

/* moves the workspace's hand-over point behind whatever a call has enqueued, however the call ends */
struct HandOver {
  bl_side_ws &w;
  hipStream_t s;
  bool armed = false;
  HandOver(bl_side_ws &ws, hipStream_t st) : w(ws), s(st) {}
  ~HandOver() {
    if (armed && hipEventRecord(w.ev_done, s) == hipSuccess) w.used = true;
  }
};

/* One call of a kind on context c, which the caller holds (CtxGuard).  `fill(void *pinned)` writes `bytes` of records
 * into a pinned block and answers BL_OK, or refuses the call: nothing has been enqueued then, the block stays free and
 * the hand-over point where it was.  The records are copied to w.recs on `s` behind the workspace's previous user, and
 * `launch(s, w, mark, mark_user)` grows the blocks of w.extra it needs (blr_ensure) and enqueues the kernels.  The
 * order is the protocol: the wait is on `s` before the copy, the hand-over is armed right behind the copy, and the
 * block counts as in flight only once its event is recorded. */
template <class Fill, class Launch>
int side_call(int kind, bl_amd_ctx *c, hipStream_t s, size_t bytes, Fill fill, Launch launch) {
  bl_side_ws &w = *side_ws_of(kind, c);
  if (!w.ev_done) BL_HIP_CHECK(hipEventCreateWithFlags(&w.ev_done, hipEventDisableTiming));
  bl_pin_slot *slot = nullptr;
  if (blr_ring_get(w.ring, w.ring_next, bytes, &slot) != BL_OK || fill(slot->p) != BL_OK) return BL_UNEXPECTED;
  if (w.used) BL_HIP_CHECK(hipStreamWaitEvent(s, w.ev_done, 0));
  if (blr_ensure(w.recs, bytes) != BL_OK) return BL_UNEXPECTED;
  HandOver done(w, s);
  BL_HIP_CHECK(hipMemcpyAsync(w.recs.p, slot->p, bytes, hipMemcpyHostToDevice, s));
  done.armed = true;
  BL_HIP_CHECK(hipEventRecord(slot->ev, s));
  slot->busy = true;
  return launch(s, w, c->prof ? side_mark : nullptr, static_cast<void *>(&w));
}

#endif /* BL_SIDE_WS_H_ */
