/*
 * bl_chords_api.hip — call path and C-ABI of the chord sequences (include/bliss_amd.h: bl_amd_chords_*); the kernels
 * are bl_chords_kernels.hip's, the host arithmetic (costs, names, segments) bl_api.c's.  Host code only.
 *
 * The chords keep a side workspace (bl_side_ws.h, which has the protocol): the parameters and the songs' records, which
 * travel in one pinned block, and as extra blocks the backpointers and what the forward kernel leaves the back-trace.
 * A call is one forward launch and one back-trace launch over all its songs: it is not cut into launch groups.
 */
#include <stdlib.h>
#include <string.h>

#include "bl_chords.h"
#include "bl_side_ws.h"

namespace {

enum { X_BP, X_END }; /* bl_side_ws::extra */

static_assert(sizeof(bl_amd_chords_params) % 16 == 0, "the songs' records follow the parameters in one block");

struct chords_totals {
  long long units = 0, rounds = 0;
};
bool totals_of(const int32_t *h_count, int n_songs, chords_totals *t) {
  for (int i = 0; i < n_songs; ++i) {
    if (!chords_count_ok(h_count[i])) return false;
    t->units += h_count[i];
    t->rounds += (h_count[i] + BL_CHORDS_STEP_UNITS - 1) / BL_CHORDS_STEP_UNITS;
  }
  return true;
}

/* songs that share a wavefront of the forward kernel */
int chords_spw() {
#ifdef BL_AMD_MEASURE
  if (const char *e = getenv("BL_AMD_CHORDS_SPW")) return atoi(e) == 1 ? 1 : 2; /* measurement builds only: the A/B */
#endif
  return BL_CHORDS_SPW;
}

int chords_device(bl_amd_ctx *c, bool dflt, const void *d_units, const int32_t *h_count, int n_songs, long long n_units,
                  const bl_amd_chords_params *params, bl_amd_song_chords *d_out, uint8_t *d_labels_out,
                  uint32_t *d_hist_out, void *stream) {
  chords_totals t;
  if (!d_units || ((uintptr_t)d_units & 15) || !h_count || !params || !d_out || ((uintptr_t)d_out & 3) ||
      ((uintptr_t)d_hist_out & 3) || n_songs < 1 || !totals_of(h_count, n_songs, &t) || n_units != t.units ||
      !chords_params_ok(*params))
    return BL_UNEXPECTED;
  if (!(c = call_ctx(c, dflt))) return BL_UNEXPECTED;
  CtxGuard g(c);
  if (!g.ok()) return BL_UNEXPECTED;
  const size_t bytes = sizeof(bl_amd_chords_params) + sizeof(bl_chords_song) * (size_t)n_songs;
  return side_call(SIDE_CHORDS, c, static_cast<hipStream_t>(stream), bytes, [&](void *pinned) {
    memcpy(pinned, params, sizeof(bl_amd_chords_params));
    bl_chords_song *hs = reinterpret_cast<bl_chords_song *>(static_cast<char *>(pinned) + sizeof(bl_amd_chords_params));
    long long u = 0, r = 0;
    for (int i = 0; i < n_songs; ++i) {
      hs[i].unit_off = u;
      hs[i].bp_off = r;
      hs[i].units = h_count[i];
      hs[i].reserved = 0;
      u += h_count[i];
      r += (h_count[i] + BL_CHORDS_STEP_UNITS - 1) / BL_CHORDS_STEP_UNITS;
    }
    return BL_OK;
  }, [&](hipStream_t s, bl_side_ws &w, blk_mark_fn mark, void *user) {
    /* a block even where there is no unit */
    if (blr_ensure(w.extra[X_BP], 4 * BL_CHORDS_BP_WORDS * (size_t)(t.rounds ? t.rounds : 1)) != BL_OK ||
        blr_ensure(w.extra[X_END], sizeof(bl_chords_end) * (size_t)n_songs) != BL_OK)
      return BL_UNEXPECTED;
    const bl_amd_chords_params *d_params = static_cast<const bl_amd_chords_params *>(w.recs.p);
    const bl_chords_song *d_songs = reinterpret_cast<const bl_chords_song *>(d_params + 1);
    uint32_t *d_bp = static_cast<uint32_t *>(w.extra[X_BP].p);
    bl_chords_end *d_end = static_cast<bl_chords_end *>(w.extra[X_END].p);
    if (blk_chords_forward(s, static_cast<const uint4 *>(d_units), d_songs, n_songs, d_params, chords_spw(), d_bp, d_end,
                           mark, user) != BL_OK ||
        blk_chords_trace(s, d_songs, n_songs, d_bp, d_end, d_out, d_labels_out, d_hist_out, mark, user) != BL_OK)
      return BL_UNEXPECTED;
    return BL_OK;
  });
}

} // namespace

/* ========================================================================= */
/* C-ABI                                                                      */

extern "C" {

int bl_amd_ctx_chords_device(bl_amd_ctx *c, const void *d_units, const int32_t *h_count, int n_songs, long long n_units,
                             const bl_amd_chords_params *params, bl_amd_song_chords *d_out, uint8_t *d_labels_out,
                             uint32_t *d_hist_out, void *stream) {
  return chords_device(c, false, d_units, h_count, n_songs, n_units, params, d_out, d_labels_out, d_hist_out, stream);
}

int bl_amd_chords_device(const void *d_units, const int32_t *h_count, int n_songs, long long n_units,
                         const bl_amd_chords_params *params, bl_amd_song_chords *d_out, uint8_t *d_labels_out,
                         uint32_t *d_hist_out, void *stream) {
  return chords_device(nullptr, true, d_units, h_count, n_songs, n_units, params, d_out, d_labels_out, d_hist_out,
                       stream);
}

/* everything is uploaded, decoded by the device form and fetched */
int bl_amd_chords_host(const void *h_units, const int32_t *h_count, int n_songs, const bl_amd_chords_params *params,
                       bl_amd_song_chords *h_out, uint8_t *h_labels_out, uint32_t *h_hist_out) {
  chords_totals t;
  if (!h_units || !h_count || !params || !h_out || n_songs < 1 || !totals_of(h_count, n_songs, &t) ||
      !chords_params_ok(*params))
    return BL_UNEXPECTED;
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return BL_UNEXPECTED;
  DevGuard dg(c->device);
  if (!dg.ok) return BL_UNEXPECTED;
  const size_t nu = (size_t)t.units;
  /* a block even where there is nothing to copy: the device form wants the units' pointer */
  DevMem units(16 * (nu ? nu : 1)), out(sizeof(bl_amd_song_chords) * (size_t)n_songs),
      labels(h_labels_out ? (nu ? nu : 1) : 0), hist(h_hist_out ? 4 * BL_CHORDS_LABELS * (size_t)n_songs : 0);
  if (!units.ok() || !out.ok() || !labels.ok() || !hist.ok()) return BL_UNEXPECTED;
  if (nu) BL_HIP_CHECK(hipMemcpy(units.p, h_units, 16 * nu, hipMemcpyHostToDevice));
  if (bl_amd_chords_device(units.p, h_count, n_songs, t.units, params, out.as<bl_amd_song_chords>(),
                           labels.as<uint8_t>(), hist.as<uint32_t>(), nullptr) != BL_OK)
    return BL_UNEXPECTED;
  BL_HIP_CHECK(hipStreamSynchronize(nullptr));
  if (!out.down(h_out) || (h_hist_out && !hist.down(h_hist_out))) return BL_UNEXPECTED;
  return !h_labels_out || !nu || labels.down(h_labels_out, nu) ? BL_OK : BL_UNEXPECTED;
}

/* the lengths at which the kernels change path */
void bl_amd_chords_shape(int *forward_units, int *trace_units, int *songs_per_wave) {
  if (forward_units) *forward_units = BL_CHORDS_STEP_UNITS;
  if (trace_units) *trace_units = BL_CHORDS_TRACE_UNITS;
  if (songs_per_wave) *songs_per_wave = BL_CHORDS_SPW;
}

/* device time of a chord kernel since this was last asked for it: "chords_forward" or "chords_trace" */
double bl_amd_chords_profile_ms(const char *name, int *launches) {
  if (launches) *launches = 0;
  const int k = !name                              ? -1
                : !strcmp(name, "chords_forward")  ? CHK_FORWARD
                : !strcmp(name, "chords_trace")    ? CHK_TRACE
                                                   : -1;
  if (k < 0) return -1.0;
  return side_profile_ms(SIDE_CHORDS, k, launches);
}

} /* extern "C" */
