/*
 * bl_fprint_api.hip — call path and C-ABI of the audio fingerprints (include/bliss_amd.h: bl_amd_fprint_*); the kernels
 * are bl_fprint_kernels.hip's, the host arithmetic over the records bl_api.c's.  Host code only.
 *
 * The fingerprints keep a side workspace (bl_side_ws.h, which has the protocol): the records of a call alone, the songs
 * of a words call or the two sets of a match.
 */
#include <string.h>

#include "bl_fprint.h"
#include "bl_side_ws.h"

namespace {

/* One call on context c, or on the default one: side_call with the context held; `fill` writes `bytes` of records and
 * `launch(s, device records, mark, mark user)` enqueues the kernels */
template <class Fill, class Launch>
int fprint_call(bl_amd_ctx *c, bool dflt, void *stream, size_t bytes, Fill fill, Launch launch) {
  if (!(c = call_ctx(c, dflt))) return BL_UNEXPECTED;
  CtxGuard g(c);
  if (!g.ok()) return BL_UNEXPECTED;
  return side_call(SIDE_FPRINT, c, static_cast<hipStream_t>(stream), bytes, [&](void *pinned) {
    fill(pinned);
    return BL_OK;
  }, [&](hipStream_t s, bl_side_ws &w, blk_mark_fn mark, void *user) { return launch(s, w.recs.p, mark, user); });
}

/* the sum of W over the songs and of ceil(W / 256); false for a bad count */
bool words_totals(const int32_t *h_frames, int n_songs, long long *words, long long *groups) {
  *words = *groups = 0;
  for (int i = 0; i < n_songs; ++i) {
    if (!fprint_count_ok(h_frames[i])) return false;
    const int w = fprint_words_of(h_frames[i]);
    *words += w;
    *groups += (w + BL_FPRINT_BLOCK_WORDS - 1) / BL_FPRINT_BLOCK_WORDS;
  }
  return true;
}

int words_device(bl_amd_ctx *c, bool dflt, const bl_amd_frame_chroma *d_frames, const int32_t *h_frames, int n_songs,
                 uint32_t *d_words_out, long long n_words, void *stream) {
  long long words, groups;
  if (!d_frames || ((uintptr_t)d_frames & 7) || !h_frames || !d_words_out || ((uintptr_t)d_words_out & 3) ||
      n_songs < 1 || !words_totals(h_frames, n_songs, &words, &groups) || n_words != words || groups > 0x7FFFFFFFll)
    return BL_UNEXPECTED;
  return fprint_call(c, dflt, stream, sizeof(bl_fprint_song) * (size_t)n_songs, [&](void *p) {
    bl_fprint_song *hs = static_cast<bl_fprint_song *>(p);
    long long f = 0, w = 0, g = 0;
    for (int i = 0; i < n_songs; ++i) {
      hs[i].frame_off = f;
      hs[i].word_off = w;
      hs[i].group_off = g;
      hs[i].frames = h_frames[i];
      hs[i].words = fprint_words_of(h_frames[i]);
      f += hs[i].frames;
      w += hs[i].words;
      g += (hs[i].words + BL_FPRINT_BLOCK_WORDS - 1) / BL_FPRINT_BLOCK_WORDS;
    }
  }, [&](hipStream_t s, void *d_recs, blk_mark_fn mark, void *user) {
    return blk_fprint_words(s, d_frames, static_cast<const bl_fprint_song *>(d_recs), n_songs, groups, d_words_out,
                            mark, user);
  });
}

bool seq_ok(const uint32_t *words, const int32_t *h_count, int n) {
  if (!words || ((uintptr_t)words & 3) || !h_count || n < 1) return false;
  for (int i = 0; i < n; ++i)
    if (!fprint_count_ok(h_count[i])) return false;
  return true;
}

void seq_fill(bl_fprint_seq *hs, const int32_t *h_count, int n) {
  long long off = 0;
  for (int i = 0; i < n; ++i) {
    hs[i].off = off;
    hs[i].count = h_count[i];
    hs[i].reserved = 0;
    off += h_count[i];
  }
}

bool match_args_ok(int n_pairs, int max_shift, int min_overlap) {
  return n_pairs >= 1 && max_shift >= 0 && max_shift <= BL_AMD_FPRINT_SHIFT_MAX && min_overlap >= 1;
}

int match_device(bl_amd_ctx *c, bool dflt, const uint32_t *d_words_a, const int32_t *h_count_a, int n_a,
                 const uint32_t *d_words_b, const int32_t *h_count_b, int n_b, const int32_t *d_pairs, int n_pairs,
                 int max_shift, int min_overlap, bl_amd_fprint_match *d_out, uint32_t *d_profile_out, void *stream) {
  if (!seq_ok(d_words_a, h_count_a, n_a) || !seq_ok(d_words_b, h_count_b, n_b) || !d_pairs ||
      ((uintptr_t)d_pairs & 3) || !d_out || ((uintptr_t)d_out & 3) || ((uintptr_t)d_profile_out & 3) ||
      !match_args_ok(n_pairs, max_shift, min_overlap))
    return BL_UNEXPECTED;
  /* the self form is the cross form with one set given twice: both are uploaded */
  return fprint_call(c, dflt, stream, sizeof(bl_fprint_seq) * ((size_t)n_a + (size_t)n_b), [&](void *p) {
    seq_fill(static_cast<bl_fprint_seq *>(p), h_count_a, n_a);
    seq_fill(static_cast<bl_fprint_seq *>(p) + n_a, h_count_b, n_b);
  }, [&](hipStream_t s, void *d_recs, blk_mark_fn mark, void *user) {
    const bl_fprint_seq *sq = static_cast<const bl_fprint_seq *>(d_recs);
    return blk_fprint_match(s, d_words_a, sq, n_a, d_words_b, sq + n_a, n_b, d_pairs, n_pairs, max_shift, min_overlap,
                            d_out, d_profile_out, mark, user);
  });
}

long long total_of(const int32_t *h_count, int n) {
  long long t = 0;
  for (int i = 0; i < n; ++i) t += h_count[i];
  return t;
}

} // namespace

/* ========================================================================= */
/* C-ABI                                                                      */

extern "C" {

int bl_amd_ctx_fprint_words_device(bl_amd_ctx *c, const bl_amd_frame_chroma *d_frames, const int32_t *h_frames,
                                   int n_songs, uint32_t *d_words_out, long long n_words, void *stream) {
  return words_device(c, false, d_frames, h_frames, n_songs, d_words_out, n_words, stream);
}

int bl_amd_fprint_words_device(const bl_amd_frame_chroma *d_frames, const int32_t *h_frames, int n_songs,
                               uint32_t *d_words_out, long long n_words, void *stream) {
  return words_device(nullptr, true, d_frames, h_frames, n_songs, d_words_out, n_words, stream);
}

int bl_amd_fprint_words_host(const bl_amd_frame_chroma *h_frame_records, const int32_t *h_frames, int n_songs,
                             uint32_t *h_words_out) {
  long long words, groups;
  if (!h_frame_records || !h_frames || !h_words_out || n_songs < 1 ||
      !words_totals(h_frames, n_songs, &words, &groups))
    return BL_UNEXPECTED;
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return BL_UNEXPECTED;
  DevGuard dg(c->device);
  if (!dg.ok) return BL_UNEXPECTED;
  const long long frames = total_of(h_frames, n_songs);
  /* a block even where there is nothing to copy: the device form wants both pointers */
  DevMem fr(sizeof(bl_amd_frame_chroma) * (size_t)(frames ? frames : 1)), out(4 * (size_t)(words ? words : 1));
  if (!fr.ok() || !out.ok()) return BL_UNEXPECTED;
  if (frames)
    BL_HIP_CHECK(hipMemcpy(fr.p, h_frame_records, sizeof(bl_amd_frame_chroma) * (size_t)frames, hipMemcpyHostToDevice));
  if (bl_amd_fprint_words_device(fr.as<bl_amd_frame_chroma>(), h_frames, n_songs, out.as<uint32_t>(), words,
                                 nullptr) != BL_OK)
    return BL_UNEXPECTED;
  BL_HIP_CHECK(hipStreamSynchronize(nullptr));
  return !words || out.down(h_words_out, 4 * (size_t)words) ? BL_OK : BL_UNEXPECTED;
}

int bl_amd_ctx_fprint_match_device(bl_amd_ctx *c, const uint32_t *d_words_a, const int32_t *h_count_a, int n_a,
                                   const uint32_t *d_words_b, const int32_t *h_count_b, int n_b,
                                   const int32_t *d_pairs, int n_pairs, int max_shift, int min_overlap,
                                   bl_amd_fprint_match *d_out, uint32_t *d_profile_out, void *stream) {
  return match_device(c, false, d_words_a, h_count_a, n_a, d_words_b, h_count_b, n_b, d_pairs, n_pairs, max_shift,
                      min_overlap, d_out, d_profile_out, stream);
}

int bl_amd_fprint_match_device(const uint32_t *d_words_a, const int32_t *h_count_a, int n_a, const uint32_t *d_words_b,
                               const int32_t *h_count_b, int n_b, const int32_t *d_pairs, int n_pairs, int max_shift,
                               int min_overlap, bl_amd_fprint_match *d_out, uint32_t *d_profile_out, void *stream) {
  return match_device(nullptr, true, d_words_a, h_count_a, n_a, d_words_b, h_count_b, n_b, d_pairs, n_pairs, max_shift,
                      min_overlap, d_out, d_profile_out, stream);
}

/* everything is uploaded, matched by the device form and fetched; a set given twice is uploaded once */
int bl_amd_fprint_match_host(const uint32_t *h_words_a, const int32_t *h_count_a, int n_a, const uint32_t *h_words_b,
                             const int32_t *h_count_b, int n_b, const int32_t *h_pairs, int n_pairs, int max_shift,
                             int min_overlap, bl_amd_fprint_match *h_out, uint32_t *h_profile_out) {
  if (!seq_ok(h_words_a, h_count_a, n_a) || !seq_ok(h_words_b, h_count_b, n_b) || !h_pairs || !h_out ||
      !match_args_ok(n_pairs, max_shift, min_overlap))
    return BL_UNEXPECTED;
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return BL_UNEXPECTED;
  DevGuard dg(c->device);
  if (!dg.ok) return BL_UNEXPECTED;
  const bool self = h_words_a == h_words_b;
  long long ta = total_of(h_count_a, n_a);
  const long long tb = total_of(h_count_b, n_b);
  if (self && tb > ta) ta = tb; /* one block holds the words either count list speaks of */
  const size_t prof = h_profile_out ? 8 * (size_t)n_pairs * (size_t)(2 * max_shift + 1) : 0;
  DevMem a(4 * (size_t)(ta ? ta : 1)), b(self ? 0 : 4 * (size_t)(tb ? tb : 1)), pairs(8 * (size_t)n_pairs),
      out(sizeof(bl_amd_fprint_match) * (size_t)n_pairs), pout(prof);
  if (!a.ok() || !b.ok() || !pairs.ok() || !out.ok() || !pout.ok() || !pairs.up(h_pairs)) return BL_UNEXPECTED;
  if (ta) BL_HIP_CHECK(hipMemcpy(a.p, h_words_a, 4 * (size_t)ta, hipMemcpyHostToDevice));
  if (!self && tb) BL_HIP_CHECK(hipMemcpy(b.p, h_words_b, 4 * (size_t)tb, hipMemcpyHostToDevice));
  if (bl_amd_fprint_match_device(a.as<uint32_t>(), h_count_a, n_a, self ? a.as<uint32_t>() : b.as<uint32_t>(),
                                 h_count_b, n_b, pairs.as<int32_t>(), n_pairs, max_shift, min_overlap,
                                 out.as<bl_amd_fprint_match>(), pout.as<uint32_t>(), nullptr) != BL_OK)
    return BL_UNEXPECTED;
  BL_HIP_CHECK(hipStreamSynchronize(nullptr));
  return out.down(h_out) && (!prof || pout.down(h_profile_out)) ? BL_OK : BL_UNEXPECTED;
}

/* the lengths at which the kernels change path */
void bl_amd_fprint_shape(int max_shift, int *words_block, int *strip_words, int *tile_words, int *chunk_offsets) {
  if (max_shift < 0) max_shift = 0;
  if (max_shift > BL_AMD_FPRINT_SHIFT_MAX) max_shift = BL_AMD_FPRINT_SHIFT_MAX;
  const bl_fprint_geom g = fprint_geom(max_shift);
  if (words_block) *words_block = BL_FPRINT_BLOCK_WORDS;
  if (strip_words) *strip_words = BL_FPRINT_STRIP_WORDS;
  if (tile_words) *tile_words = BL_FPRINT_STRIP_WORDS * g.strips;
  if (chunk_offsets) *chunk_offsets = BL_FPRINT_UNIT * g.groups;
}

/* device time of a fingerprint kernel since this was last asked for it: "fprint_words" or "fprint_match" */
double bl_amd_fprint_profile_ms(const char *name, int *launches) {
  if (launches) *launches = 0;
  const int k = !name ? -1 : !strcmp(name, "fprint_words") ? FK_WORDS : !strcmp(name, "fprint_match") ? FK_MATCH : -1;
  if (k < 0) return -1.0;
  return side_profile_ms(SIDE_FPRINT, k, launches);
}

} /* extern "C" */
