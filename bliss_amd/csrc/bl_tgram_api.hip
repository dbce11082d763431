/*
 * bl_tgram_api.hip — call path and C-ABI of the tempo over time (include/bliss_amd.h: bl_amd_tgram_*); the kernels are
 * bl_tgram_kernels.hip's, the host arithmetic (frames, bpm, seconds, steadiness) bl_api.c's.  Host code only.
 *
 * The tempogram keeps a side workspace (bl_side_ws.h, which has the protocol): the parameters and the songs' records,
 * which travel in one pinned block, and no further block: the block rows never leave the chip.  A call is one launch
 * of the block kernel per 32 768 songs and one of the song kernel.
 */
#include <string.h>

#include "bl_side_ws.h"
#include "bl_tgram.h"

namespace {

static_assert(sizeof(bl_amd_tgram_params) % 16 == 0, "the songs' records follow the parameters in one block");
static_assert(sizeof(bl_amd_tgram_params) == 32 && sizeof(bl_amd_tgram_frame) == 40 && sizeof(bl_amd_song_tgram) == 56,
              "the header's sizes");

struct tgram_totals {
  long long hops = 0, frames = 0;
  int max_frames = 0;
};
/* what both forms reject before anything is enqueued; h_onsets: the curves where they are in host memory */
bool totals_of(const int32_t *h_hops, int n_songs, const bl_amd_tgram_params *params, const uint32_t *h_onsets,
               tgram_totals *t) {
  if (!h_hops || !params || n_songs < 1 || !tgram_params_ok(*params)) return false;
  for (int i = 0; i < n_songs; ++i) {
    if (!tgram_hops_ok(h_hops[i])) return false;
    const int f = bl_amd_tgram_frames(h_hops[i], params);
    t->hops += h_hops[i];
    t->frames += f;
    if (f > t->max_frames) t->max_frames = f;
  }
  for (long long k = 0; h_onsets && k < t->hops; ++k)
    if (h_onsets[k] >= (1u << 18)) return false;
  return true;
}

/* one call on curves on the device; the caller holds the context and has checked the arguments */
int tgram_call(bl_amd_ctx *c, hipStream_t stream, const uint32_t *d_onsets, const int32_t *h_hops, int n_songs,
               const bl_amd_tgram_params *params, const tgram_totals &t, bl_amd_song_tgram *d_songs_out,
               bl_amd_tgram_frame *d_frames_out, uint64_t *d_gram_out) {
  const bl_amd_tgram_params p = *params;
  const size_t bytes = sizeof(bl_amd_tgram_params) + sizeof(bl_tgram_song) * (size_t)n_songs;
  return side_call(SIDE_TGRAM, c, stream, bytes, [&](void *pinned) {
    memcpy(pinned, &p, sizeof(p));
    bl_tgram_song *hs = reinterpret_cast<bl_tgram_song *>(static_cast<char *>(pinned) + sizeof(p));
    long long h = 0, f = 0;
    for (int i = 0; i < n_songs; ++i) {
      hs[i].onset_off = h;
      hs[i].frame_off = f;
      hs[i].hops = h_hops[i];
      hs[i].frames = bl_amd_tgram_frames(h_hops[i], &p);
      h += hs[i].hops;
      f += hs[i].frames;
    }
    return BL_OK;
  }, [&](hipStream_t s, bl_side_ws &w, blk_mark_fn mark, void *user) {
    const bl_amd_tgram_params *d_params = static_cast<const bl_amd_tgram_params *>(w.recs.p);
    const bl_tgram_song *d_songs = reinterpret_cast<const bl_tgram_song *>(d_params + 1);
    if (blk_tgram_blocks(s, d_onsets, d_songs, n_songs, t.max_frames, p, d_params, c->n_cu, d_frames_out, d_gram_out,
                         mark, user) != BL_OK ||
        blk_tgram_songs(s, d_songs, n_songs, d_params, d_frames_out, d_songs_out, mark, user) != BL_OK)
      return BL_UNEXPECTED;
    return BL_OK;
  });
}

int tgram_device(bl_amd_ctx *c, bool dflt, const uint32_t *d_onsets, const int32_t *h_hops, int n_songs,
                 const bl_amd_tgram_params *params, bl_amd_song_tgram *d_songs_out, bl_amd_tgram_frame *d_frames_out,
                 long long n_frames, uint64_t *d_gram_out, void *stream) {
  tgram_totals t;
  if (!d_onsets || ((uintptr_t)d_onsets & 3) || !d_songs_out || ((uintptr_t)d_songs_out & 3) ||
      ((uintptr_t)d_frames_out & 7) || ((uintptr_t)d_gram_out & 7) || !totals_of(h_hops, n_songs, params, nullptr, &t) ||
      n_frames != t.frames || (t.frames > 0 && !d_frames_out))
    return BL_UNEXPECTED;
  if (!(c = call_ctx(c, dflt))) return BL_UNEXPECTED;
  CtxGuard g(c);
  if (!g.ok()) return BL_UNEXPECTED;
  return tgram_call(c, static_cast<hipStream_t>(stream), d_onsets, h_hops, n_songs, params, t, d_songs_out, d_frames_out,
                    d_gram_out);
}

} // namespace

/* ========================================================================= */
/* C-ABI                                                                      */

extern "C" {

int bl_amd_ctx_tgram_device(bl_amd_ctx *c, const uint32_t *d_onsets, const int32_t *h_hops, int n_songs,
                            const bl_amd_tgram_params *params, bl_amd_song_tgram *d_songs_out,
                            bl_amd_tgram_frame *d_frames_out, long long n_frames, uint64_t *d_gram_out, void *stream) {
  return tgram_device(c, false, d_onsets, h_hops, n_songs, params, d_songs_out, d_frames_out, n_frames, d_gram_out,
                      stream);
}

int bl_amd_tgram_device(const uint32_t *d_onsets, const int32_t *h_hops, int n_songs, const bl_amd_tgram_params *params,
                        bl_amd_song_tgram *d_songs_out, bl_amd_tgram_frame *d_frames_out, long long n_frames,
                        uint64_t *d_gram_out, void *stream) {
  return tgram_device(nullptr, true, d_onsets, h_hops, n_songs, params, d_songs_out, d_frames_out, n_frames, d_gram_out,
                      stream);
}

/* the caller's curves: uploaded, through the same launches as the device form, fetched */
int bl_amd_tgram_host(const uint32_t *h_onsets, const int32_t *h_hops, int n_songs, const bl_amd_tgram_params *params,
                      bl_amd_song_tgram *h_songs_out, bl_amd_tgram_frame *h_frames_out, uint64_t *h_gram_out) {
  tgram_totals t;
  if (!h_onsets || !h_songs_out || !totals_of(h_hops, n_songs, params, h_onsets, &t) || (t.frames > 0 && !h_frames_out))
    return BL_UNEXPECTED;
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return BL_UNEXPECTED;
  CtxGuard g(c);
  if (!g.ok()) return BL_UNEXPECTED;
  const size_t nf = (size_t)t.frames;
  DevMem curve(sizeof(uint32_t) * (size_t)t.hops), out(sizeof(bl_amd_song_tgram) * (size_t)n_songs),
      frames(sizeof(bl_amd_tgram_frame) * nf), gram(h_gram_out ? sizeof(uint64_t) * BL_AMD_RHYTHM_LAGS * nf : 0);
  if (!curve.ok() || !out.ok() || !frames.ok() || !gram.ok() || !curve.up(h_onsets)) return BL_UNEXPECTED;
  if (tgram_call(c, nullptr, curve.as<uint32_t>(), h_hops, n_songs, params, t, out.as<bl_amd_song_tgram>(),
                 frames.as<bl_amd_tgram_frame>(), gram.as<uint64_t>()) != BL_OK)
    return BL_UNEXPECTED;
  BL_HIP_CHECK(hipStreamSynchronize(nullptr));
  return out.down(h_songs_out) && (!nf || (frames.down(h_frames_out) && (!h_gram_out || gram.down(h_gram_out))))
             ? BL_OK
             : BL_UNEXPECTED;
}

/* the lengths at which the kernels change path */
void bl_amd_tgram_shape(int *tile_terms, int *run_frames) {
  if (tile_terms) *tile_terms = BL_TGRAM_TILE;
  if (run_frames) *run_frames = BL_TGRAM_RUN_FRAMES;
}

/* device time of a tempogram kernel since this was last asked for it: "tgram_blocks" or "tgram_songs" */
double bl_amd_tgram_profile_ms(const char *name, int *launches) {
  if (launches) *launches = 0;
  const int k = !name                           ? -1
                : !strcmp(name, "tgram_blocks") ? TGK_BLOCKS
                : !strcmp(name, "tgram_songs")  ? TGK_SONGS
                                                : -1;
  if (k < 0) return -1.0;
  return side_profile_ms(SIDE_TGRAM, k, launches);
}

} /* extern "C" */
