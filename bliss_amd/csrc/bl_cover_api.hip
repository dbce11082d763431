/*
 * bl_cover_api.hip — call path and C-ABI of the cover and version matching (include/bliss_amd.h: bl_amd_cover_*); the
 * kernels are bl_cover_kernels.hip's and, for the units, bl_form_kernels.hip's k_form_units as it is; the host
 * arithmetic over the records is bl_api.c's.  Host code only.
 *
 * The matching keeps a side workspace (bl_side_ws.h, which has the protocol): the songs' records of a units call or the
 * two sets of a match, and as an extra block the profiles g of a match's songs.
 */
#include <string.h>

#include "bl_cover.h"
#include "bl_form.h"
#include "bl_side_ws.h"

namespace {

enum { X_PROF }; /* bl_side_ws::extra */

static_assert((int)CVK_UNITS == (int)FMK_UNITS, "blk_form_units marks with the id the units have here");

/* One call on context c, or on the default one: side_call with the context held */
template <class Fill, class Launch>
int cover_call(bl_amd_ctx *c, bool dflt, void *stream, size_t bytes, Fill fill, Launch launch) {
  if (!(c = call_ctx(c, dflt))) return BL_UNEXPECTED;
  CtxGuard g(c);
  if (!g.ok()) return BL_UNEXPECTED;
  return side_call(SIDE_COVER, c, static_cast<hipStream_t>(stream), bytes, [&](void *pinned) {
    fill(pinned);
    return BL_OK;
  }, launch);
}

/* ---- units ---- */

struct unit_totals {
  long long frames = 0, units = 0, groups = 0;
};
bool unit_totals_of(const int32_t *h_frames, int n_songs, int pool, unit_totals *t) {
  if (pool < 1 || pool > 16) return false;
  for (int i = 0; i < n_songs; ++i) {
    if (!form_count_ok(h_frames[i])) return false;
    const int u = h_frames[i] / pool;
    t->frames += h_frames[i];
    t->units += u;
    t->groups += (u + BL_FORM_BLOCK_UNITS - 1) / BL_FORM_BLOCK_UNITS;
  }
  return true;
}

int units_device(bl_amd_ctx *c, bool dflt, const bl_amd_frame_chroma *d_frames, const int32_t *h_frames, int n_songs,
                 int pool, void *d_units_out, long long n_units, void *stream) {
  unit_totals t;
  if (!d_frames || ((uintptr_t)d_frames & 7) || !h_frames || !d_units_out || ((uintptr_t)d_units_out & 15) ||
      n_songs < 1 || !unit_totals_of(h_frames, n_songs, pool, &t) || n_units != t.units || t.groups > 0x7FFFFFFFll)
    return BL_UNEXPECTED;
  return cover_call(c, dflt, stream, sizeof(bl_form_song) * (size_t)n_songs, [&](void *p) {
    bl_form_song *hs = static_cast<bl_form_song *>(p);
    long long f = 0, u = 0, gr = 0;
    for (int i = 0; i < n_songs; ++i) {
      hs[i].frame_off = f;
      hs[i].unit_off = u;
      hs[i].group_off = gr;
      hs[i].frames = h_frames[i];
      hs[i].units = h_frames[i] / pool;
      f += hs[i].frames;
      u += hs[i].units;
      gr += (hs[i].units + BL_FORM_BLOCK_UNITS - 1) / BL_FORM_BLOCK_UNITS;
    }
  }, [&](hipStream_t s, bl_side_ws &w, blk_mark_fn mark, void *user) {
    return blk_form_units(s, d_frames, static_cast<const bl_form_song *>(w.recs.p), n_songs, t.groups, pool,
                          static_cast<uint4 *>(d_units_out), mark, user);
  });
}

/* ---- match ---- */

bool seq_ok(const void *units, const int32_t *h_count, int n) {
  if (!units || ((uintptr_t)units & 15) || !h_count || n < 1) return false;
  for (int i = 0; i < n; ++i)
    if (!cover_count_ok(h_count[i])) return false;
  return true;
}

void seq_fill(bl_cover_seq *hs, const int32_t *h_count, int n) {
  long long off = 0;
  for (int i = 0; i < n; ++i) {
    hs[i].off = off;
    hs[i].count = h_count[i];
    hs[i].reserved = 0;
    off += h_count[i];
  }
}

long long total_of(const int32_t *h_count, int n) {
  long long t = 0;
  for (int i = 0; i < n; ++i) t += h_count[i];
  return t;
}

int match_device(bl_amd_ctx *c, bool dflt, const void *d_units_a, const int32_t *h_count_a, int n_a,
                 const void *d_units_b, const int32_t *h_count_b, int n_b, const int32_t *d_pairs, int n_pairs,
                 const bl_amd_cover_params *params, bl_amd_cover_match *d_out, void *stream) {
  if (!seq_ok(d_units_a, h_count_a, n_a) || !seq_ok(d_units_b, h_count_b, n_b) || !d_pairs ||
      ((uintptr_t)d_pairs & 7) || !d_out || ((uintptr_t)d_out & 3) || n_pairs < 1 || !params ||
      !cover_params_ok(*params) || (long long)n_a + n_b > 0x7FFFFFFFll)
    return BL_UNEXPECTED;
  const bl_amd_cover_params p = *params;
  int max_a = 0; /* the largest count of set a that is not too long */
  for (int i = 0; i < n_a; ++i)
    if (h_count_a[i] <= BL_COVER_UNITS_MAX && h_count_a[i] > max_a) max_a = h_count_a[i];
  const int n_seq = n_a + n_b;
  /* the self form is the cross form with one set given twice: both are uploaded */
  return cover_call(c, dflt, stream, sizeof(bl_cover_seq) * (size_t)n_seq, [&](void *pinned) {
    seq_fill(static_cast<bl_cover_seq *>(pinned), h_count_a, n_a);
    seq_fill(static_cast<bl_cover_seq *>(pinned) + n_a, h_count_b, n_b);
  }, [&](hipStream_t s, bl_side_ws &w, blk_mark_fn mark, void *user) {
    if (blr_ensure(w.extra[X_PROF], 12 * sizeof(uint32_t) * (size_t)n_seq) != BL_OK) return BL_UNEXPECTED;
    const bl_cover_seq *sq = static_cast<const bl_cover_seq *>(w.recs.p);
    const uint4 *ua = static_cast<const uint4 *>(d_units_a), *ub = static_cast<const uint4 *>(d_units_b);
    uint32_t *prof = static_cast<uint32_t *>(w.extra[X_PROF].p);
    if (blk_cover_profile(s, ua, ub, sq, n_a, n_seq, prof, mark, user) != BL_OK ||
        blk_cover_align(s, ua, ub, sq, n_a, n_b, prof, d_pairs, n_pairs, max_a, p, d_out, mark, user) != BL_OK)
      return BL_UNEXPECTED;
    return BL_OK;
  });
}

} // namespace

/* ========================================================================= */
/* C-ABI                                                                      */

extern "C" {

int bl_amd_ctx_cover_units_device(bl_amd_ctx *c, const bl_amd_frame_chroma *d_frames, const int32_t *h_frames,
                                  int n_songs, int pool, void *d_units_out, long long n_units, void *stream) {
  return units_device(c, false, d_frames, h_frames, n_songs, pool, d_units_out, n_units, stream);
}

int bl_amd_cover_units_device(const bl_amd_frame_chroma *d_frames, const int32_t *h_frames, int n_songs, int pool,
                              void *d_units_out, long long n_units, void *stream) {
  return units_device(nullptr, true, d_frames, h_frames, n_songs, pool, d_units_out, n_units, stream);
}

int bl_amd_cover_units_host(const bl_amd_frame_chroma *h_frame_records, const int32_t *h_frames, int n_songs, int pool,
                            void *h_units_out) {
  unit_totals t;
  if (!h_frame_records || !h_frames || !h_units_out || n_songs < 1 || !unit_totals_of(h_frames, n_songs, pool, &t))
    return BL_UNEXPECTED;
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return BL_UNEXPECTED;
  DevGuard dg(c->device);
  if (!dg.ok) return BL_UNEXPECTED;
  /* a block even where there is nothing to copy: the device form wants both pointers */
  DevMem fr(sizeof(bl_amd_frame_chroma) * (size_t)(t.frames ? t.frames : 1)), out(16 * (size_t)(t.units ? t.units : 1));
  if (!fr.ok() || !out.ok()) return BL_UNEXPECTED;
  if (t.frames)
    BL_HIP_CHECK(hipMemcpy(fr.p, h_frame_records, sizeof(bl_amd_frame_chroma) * (size_t)t.frames, hipMemcpyHostToDevice));
  if (bl_amd_cover_units_device(fr.as<bl_amd_frame_chroma>(), h_frames, n_songs, pool, out.p, t.units, nullptr) != BL_OK)
    return BL_UNEXPECTED;
  BL_HIP_CHECK(hipStreamSynchronize(nullptr));
  return !t.units || out.down(h_units_out, 16 * (size_t)t.units) ? BL_OK : BL_UNEXPECTED;
}

int bl_amd_ctx_cover_match_device(bl_amd_ctx *c, const void *d_units_a, const int32_t *h_count_a, int n_a,
                                  const void *d_units_b, const int32_t *h_count_b, int n_b, const int32_t *d_pairs,
                                  int n_pairs, const bl_amd_cover_params *params, bl_amd_cover_match *d_out,
                                  void *stream) {
  return match_device(c, false, d_units_a, h_count_a, n_a, d_units_b, h_count_b, n_b, d_pairs, n_pairs, params, d_out,
                      stream);
}

int bl_amd_cover_match_device(const void *d_units_a, const int32_t *h_count_a, int n_a, const void *d_units_b,
                              const int32_t *h_count_b, int n_b, const int32_t *d_pairs, int n_pairs,
                              const bl_amd_cover_params *params, bl_amd_cover_match *d_out, void *stream) {
  return match_device(nullptr, true, d_units_a, h_count_a, n_a, d_units_b, h_count_b, n_b, d_pairs, n_pairs, params,
                      d_out, stream);
}

/* everything is uploaded, matched by the device form and fetched; a set given twice is uploaded once */
int bl_amd_cover_match_host(const void *h_units_a, const int32_t *h_count_a, int n_a, const void *h_units_b,
                            const int32_t *h_count_b, int n_b, const int32_t *h_pairs, int n_pairs,
                            const bl_amd_cover_params *params, bl_amd_cover_match *h_out) {
  if (!h_units_a || !h_count_a || n_a < 1 || !h_units_b || !h_count_b || n_b < 1 || !h_pairs || !h_out ||
      n_pairs < 1 || !params || !cover_params_ok(*params))
    return BL_UNEXPECTED;
  for (int i = 0; i < n_a; ++i)
    if (!cover_count_ok(h_count_a[i])) return BL_UNEXPECTED;
  for (int i = 0; i < n_b; ++i)
    if (!cover_count_ok(h_count_b[i])) return BL_UNEXPECTED;
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return BL_UNEXPECTED;
  DevGuard dg(c->device);
  if (!dg.ok) return BL_UNEXPECTED;
  const bool self = h_units_a == h_units_b;
  long long ta = total_of(h_count_a, n_a);
  const long long tb = total_of(h_count_b, n_b);
  if (self && tb > ta) ta = tb; /* one block holds the units either count list speaks of */
  DevMem a(16 * (size_t)(ta ? ta : 1)), b(self ? 0 : 16 * (size_t)(tb ? tb : 1)), pairs(8 * (size_t)n_pairs),
      out(sizeof(bl_amd_cover_match) * (size_t)n_pairs);
  if (!a.ok() || !b.ok() || !pairs.ok() || !out.ok() || !pairs.up(h_pairs)) return BL_UNEXPECTED;
  if (ta) BL_HIP_CHECK(hipMemcpy(a.p, h_units_a, 16 * (size_t)ta, hipMemcpyHostToDevice));
  if (!self && tb) BL_HIP_CHECK(hipMemcpy(b.p, h_units_b, 16 * (size_t)tb, hipMemcpyHostToDevice));
  if (bl_amd_cover_match_device(a.p, h_count_a, n_a, self ? a.p : b.p, h_count_b, n_b, pairs.as<int32_t>(), n_pairs,
                                params, out.as<bl_amd_cover_match>(), nullptr) != BL_OK)
    return BL_UNEXPECTED;
  BL_HIP_CHECK(hipStreamSynchronize(nullptr));
  return out.down(h_out) ? BL_OK : BL_UNEXPECTED;
}

/* the lengths at which the alignment changes path */
void bl_amd_cover_shape(int *strip_columns, int *row_block) {
  if (strip_columns) *strip_columns = BL_COVER_STRIP;
  if (row_block) *row_block = BL_COVER_ROWS;
}

/* device time of a matching kernel since this was last asked for it: "cover_profile" or "cover_align" */
double bl_amd_cover_profile_ms(const char *name, int *launches) {
  if (launches) *launches = 0;
  const int k = !name                             ? -1
                : !strcmp(name, "cover_profile")  ? CVK_PROFILE
                : !strcmp(name, "cover_align")    ? CVK_ALIGN
                                                  : -1;
  if (k < 0) return -1.0;
  return side_profile_ms(SIDE_COVER, k, launches);
}

} /* extern "C" */
