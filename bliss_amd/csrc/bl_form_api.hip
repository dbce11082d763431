/*
 * bl_form_api.hip — call path and C-ABI of the song structure (include/bliss_amd.h: bl_amd_form_*); the kernels are
 * bl_form_kernels.hip's, the host arithmetic over the records bl_api.c's.  Host code only.
 *
 * The structure pass keeps a side workspace (bl_side_ws.h, which has the protocol): the songs' records, and as extra
 * blocks the units and the novelty of a call that does not ask for them.
 */
#include <string.h>

#include "bl_form.h"
#include "bl_side_ws.h"

namespace {

enum { X_UNITS, X_NOV }; /* bl_side_ws::extra */

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
  return side_call(SIDE_FORM, c, static_cast<hipStream_t>(stream), sizeof(bl_form_song) * (size_t)n_songs,
                   [&](void *pinned) {
    bl_form_song *hs = static_cast<bl_form_song *>(pinned);
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
    return BL_OK;
  }, [&](hipStream_t s, bl_side_ws &w, blk_mark_fn mark, void *user) {
    const size_t n1 = (size_t)(t.units ? t.units : 1); /* a block even where there is no unit */
    if ((!d_units_out && blr_ensure(w.extra[X_UNITS], sizeof(uint4) * n1) != BL_OK) ||
        (!d_nov_out && blr_ensure(w.extra[X_NOV], 8 * n1) != BL_OK))
      return BL_UNEXPECTED;
    const bl_form_song *d_songs = static_cast<const bl_form_song *>(w.recs.p);
    uint4 *d_units = static_cast<uint4 *>(d_units_out ? d_units_out : w.extra[X_UNITS].p);
    unsigned long long *d_nov = d_nov_out ? reinterpret_cast<unsigned long long *>(d_nov_out)
                                          : static_cast<unsigned long long *>(w.extra[X_NOV].p);
    if (blk_form_units(s, d_frames, d_songs, n_songs, t.groups, p.pool, d_units, mark, user) != BL_OK ||
        blk_form_thumb(s, d_units, d_songs, n_songs, t.max_units, p.seg, p.min_lag, d_out, d_rep_out, mark, user) !=
            BL_OK ||
        blk_form_novelty(s, d_units, d_songs, n_songs, p.nov, p.peak_num, p.peak_den, d_out, d_nov, d_flags_out, mark,
                         user) != BL_OK)
      return BL_UNEXPECTED;
    return BL_OK;
  });
}

} // namespace

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
  return side_profile_ms(SIDE_FORM, k, launches);
}

} /* extern "C" */
