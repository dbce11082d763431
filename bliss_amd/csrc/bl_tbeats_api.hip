/*
 * bl_tbeats_api.hip — call path and C-ABI of the beat grid that follows the tempo over time (include/bliss_amd.h:
 * bl_amd_tbeats_*); the kernels are bl_tbeats_kernels.hip's, the host arithmetic (params_from_tgram, edge_bpm)
 * bl_api.c's.  Host code only.
 *
 * The call keeps a side workspace (bl_side_ws.h, which has the protocol): the parameters and the songs' records, which
 * travel in one pinned block, and two further blocks: the track where the caller asks for none (4 bytes per frame of
 * the call) and one launch group's links where the caller asks for none (2 bytes per hop).  As the beats call does, the
 * records are sorted longest first and cut into launch groups (bl_groups.h) that follow each other on the stream and
 * share the link scratch.  A call is one launch of the track kernel and one of the grid kernel per group.
 */
#include <string.h>

#include "bl_groups.h"
#include "bl_side_ws.h"
#include "bl_tbeats.h"

namespace {

enum { X_TRACK, X_LINKS };
static_assert(X_LINKS < BL_SIDE_EXTRA, "the workspace's further blocks");
static_assert(sizeof(bl_amd_tbeats_params) == 32 && sizeof(bl_amd_song_tbeats) == 64, "the header's sizes");
static_assert(sizeof(bl_amd_tbeats_params) % 16 == 0 && sizeof(bl_tbeats_song) % 8 == 0,
              "the songs' records follow the parameters in one block");

struct tbeats_totals {
  long long hops = 0, frames = 0;
};
/* what both forms reject before anything is enqueued; h_onsets: the curves where they are in host memory */
bool totals_of(const int32_t *h_hops, const int32_t *h_frames, int n_songs, const bl_amd_tbeats_params *params,
               const uint32_t *h_onsets, tbeats_totals *t) {
  if (!h_hops || !h_frames || !params || n_songs < 1 || !tbeats_params_ok(*params)) return false;
  for (int i = 0; i < n_songs; ++i) {
    if (!tbeats_hops_ok(h_hops[i]) || !tbeats_frames_ok(h_frames[i])) return false;
    t->hops += h_hops[i];
    t->frames += h_frames[i];
  }
  for (long long k = 0; h_onsets && k < t->hops; ++k)
    if (h_onsets[k] >= (1u << 18)) return false;
  return true;
}
bool stride_ok(int stride) { return stride >= 4 && !(stride & 3); }

/* one call on curves and lags on the device; the caller holds the context and has checked the arguments */
int tbeats_call(bl_amd_ctx *c, hipStream_t stream, const uint32_t *d_onsets, const int32_t *h_hops,
                const int32_t *h_frames, int n_songs, const void *d_lag, int lag_stride, const void *d_anchor,
                int anchor_stride, const bl_amd_tbeats_params *params, const tbeats_totals &t,
                bl_amd_song_tbeats *d_songs_out, uint8_t *d_flags_out, uint16_t *d_links_out, int64_t *d_scores_out,
                int32_t *d_track_out) {
  const bl_amd_tbeats_params p = *params;
  const size_t bytes = sizeof(bl_amd_tbeats_params) + sizeof(bl_tbeats_song) * (size_t)n_songs;
  std::vector<int> cuts; /* the first record of every launch group, and n_songs */
  long long max_hops = 0;
  return side_call(SIDE_TBEATS, c, stream, bytes, [&](void *pinned) {
    memcpy(pinned, &p, sizeof(p));
    bl_tbeats_song *hs = reinterpret_cast<bl_tbeats_song *>(static_cast<char *>(pinned) + sizeof(p));
    long long h = 0, f = 0;
    for (int i = 0; i < n_songs; ++i) {
      hs[i].onset_off = h;
      hs[i].frame_off = f;
      hs[i].hop_off = 0;
      hs[i].hops = h_hops[i];
      hs[i].frames = h_frames[i];
      hs[i].out_idx = i;
      hs[i].pad = 0;
      h += h_hops[i];
      f += h_frames[i];
    }
    bl_groups_plan(hs, n_songs, std::min(c->group_songs, BL_TBEATS_GROUP_SONGS), BL_TBEATS_GROUP_HOPS);
    long long hops;
    for (int b = 0; b < n_songs; b = bl_group_end(hs, b, n_songs, hops), max_hops = std::max(max_hops, hops))
      cuts.push_back(b);
    cuts.push_back(n_songs);
    return BL_OK;
  }, [&](hipStream_t s, bl_side_ws &w, blk_mark_fn mark, void *user) {
    /* a block even where there is no frame */
    if ((!d_track_out && blr_ensure(w.extra[X_TRACK], sizeof(int32_t) * (size_t)std::max(t.frames, 1ll)) != BL_OK) ||
        (!d_links_out && blr_ensure(w.extra[X_LINKS], sizeof(uint16_t) * (size_t)max_hops) != BL_OK))
      return BL_UNEXPECTED;
    const bl_amd_tbeats_params *d_params = static_cast<const bl_amd_tbeats_params *>(w.recs.p);
    const bl_tbeats_song *d_songs = reinterpret_cast<const bl_tbeats_song *>(d_params + 1);
    int32_t *d_track = d_track_out ? d_track_out : static_cast<int32_t *>(w.extra[X_TRACK].p);
    if (blk_tbeats_track(s, d_songs, n_songs, d_lag, lag_stride, d_anchor, anchor_stride, d_params, d_track, d_songs_out,
                         mark, user) != BL_OK)
      return BL_UNEXPECTED;
    for (size_t g = 0; g + 1 < cuts.size(); ++g)
      if (blk_tbeats_group(s, d_onsets, d_songs + cuts[g], cuts[g + 1] - cuts[g], d_params, d_track, d_songs_out,
                           d_flags_out, d_links_out, static_cast<uint16_t *>(w.extra[X_LINKS].p), d_scores_out, mark,
                           user) != BL_OK)
        return BL_UNEXPECTED;
    return BL_OK;
  });
}

int tbeats_device(bl_amd_ctx *c, bool dflt, const uint32_t *d_onsets, const int32_t *h_hops, const int32_t *h_frames,
                  int n_songs, const void *d_lag, int lag_stride, const void *d_anchor, int anchor_stride,
                  const bl_amd_tbeats_params *params, bl_amd_song_tbeats *d_songs_out, uint8_t *d_flags_out,
                  uint16_t *d_links_out, int64_t *d_scores_out, int32_t *d_track_out, void *stream) {
  tbeats_totals t;
  if (!d_onsets || ((uintptr_t)d_onsets & 3) || !stride_ok(lag_stride) || ((uintptr_t)d_lag & 3) ||
      (d_anchor && (!stride_ok(anchor_stride) || ((uintptr_t)d_anchor & 3))) || !d_songs_out ||
      ((uintptr_t)d_songs_out & 7) || !d_flags_out || ((uintptr_t)d_links_out & 1) || ((uintptr_t)d_scores_out & 7) ||
      ((uintptr_t)d_track_out & 3) || !totals_of(h_hops, h_frames, n_songs, params, nullptr, &t) ||
      (t.frames > 0 && !d_lag))
    return BL_UNEXPECTED;
  if (!(c = call_ctx(c, dflt))) return BL_UNEXPECTED;
  CtxGuard g(c);
  if (!g.ok()) return BL_UNEXPECTED;
  return tbeats_call(c, static_cast<hipStream_t>(stream), d_onsets, h_hops, h_frames, n_songs, d_lag, lag_stride,
                     d_anchor, anchor_stride, params, t, d_songs_out, d_flags_out, d_links_out, d_scores_out, d_track_out);
}

} // namespace

/* ========================================================================= */
/* C-ABI                                                                      */

extern "C" {

int bl_amd_ctx_tbeats_device(bl_amd_ctx *c, const uint32_t *d_onsets, const int32_t *h_hops, const int32_t *h_frames,
                             int n_songs, const void *d_lag, int lag_stride, const void *d_anchor, int anchor_stride,
                             const bl_amd_tbeats_params *params, bl_amd_song_tbeats *d_songs_out, uint8_t *d_flags_out,
                             uint16_t *d_links_out, int64_t *d_scores_out, int32_t *d_track_out, void *stream) {
  return tbeats_device(c, false, d_onsets, h_hops, h_frames, n_songs, d_lag, lag_stride, d_anchor, anchor_stride, params,
                       d_songs_out, d_flags_out, d_links_out, d_scores_out, d_track_out, stream);
}

int bl_amd_tbeats_device(const uint32_t *d_onsets, const int32_t *h_hops, const int32_t *h_frames, int n_songs,
                         const void *d_lag, int lag_stride, const void *d_anchor, int anchor_stride,
                         const bl_amd_tbeats_params *params, bl_amd_song_tbeats *d_songs_out, uint8_t *d_flags_out,
                         uint16_t *d_links_out, int64_t *d_scores_out, int32_t *d_track_out, void *stream) {
  return tbeats_device(nullptr, true, d_onsets, h_hops, h_frames, n_songs, d_lag, lag_stride, d_anchor, anchor_stride,
                       params, d_songs_out, d_flags_out, d_links_out, d_scores_out, d_track_out, stream);
}

/* the caller's curves, lags (packed) and anchors (packed, or NULL): uploaded, through the same launches as the device
 * form, fetched */
int bl_amd_tbeats_host(const uint32_t *h_onsets, const int32_t *h_hops, const int32_t *h_frames, int n_songs,
                       const int32_t *h_lag, const int32_t *h_anchor, const bl_amd_tbeats_params *params,
                       bl_amd_song_tbeats *h_songs_out, uint8_t *h_flags_out, uint16_t *h_links_out,
                       int64_t *h_scores_out, int32_t *h_track_out) {
  tbeats_totals t;
  if (!h_onsets || !h_songs_out || !h_flags_out || !totals_of(h_hops, h_frames, n_songs, params, h_onsets, &t) ||
      (t.frames > 0 && !h_lag))
    return BL_UNEXPECTED;
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return BL_UNEXPECTED;
  CtxGuard g(c);
  if (!g.ok()) return BL_UNEXPECTED;
  const size_t nh = (size_t)t.hops, nf = (size_t)t.frames;
  DevMem curve(sizeof(uint32_t) * nh), lag(sizeof(int32_t) * nf), anchor(h_anchor ? sizeof(int32_t) * (size_t)n_songs : 0),
      out(sizeof(bl_amd_song_tbeats) * (size_t)n_songs), flags(nh), links(h_links_out ? sizeof(uint16_t) * nh : 0),
      scores(h_scores_out ? sizeof(int64_t) * nh : 0), track(h_track_out ? sizeof(int32_t) * nf : 0);
  if (!curve.ok() || !lag.ok() || !anchor.ok() || !out.ok() || !flags.ok() || !links.ok() || !scores.ok() ||
      !track.ok() || !curve.up(h_onsets) || (nf && !lag.up(h_lag)) || (h_anchor && !anchor.up(h_anchor)))
    return BL_UNEXPECTED;
  if (tbeats_call(c, nullptr, curve.as<uint32_t>(), h_hops, h_frames, n_songs, lag.p, 4, h_anchor ? anchor.p : nullptr, 4,
                  params, t, out.as<bl_amd_song_tbeats>(), flags.as<uint8_t>(), links.as<uint16_t>(),
                  scores.as<int64_t>(), track.as<int32_t>()) != BL_OK)
    return BL_UNEXPECTED;
  BL_HIP_CHECK(hipStreamSynchronize(nullptr));
  return out.down(h_songs_out) && flags.down(h_flags_out) && (!h_links_out || links.down(h_links_out)) &&
                 (!h_scores_out || scores.down(h_scores_out)) && (!h_track_out || !nf || track.down(h_track_out))
             ? BL_OK
             : BL_UNEXPECTED;
}

/* the lengths at which the kernels change path */
void bl_amd_tbeats_shape(int *ring, int *track_tile) {
  if (ring) *ring = BL_TBEATS_RING;
  if (track_tile) *track_tile = BL_TBEATS_TRACK_TILE;
}

/* device time of a kernel of this call since this was last asked for it: "tbeats_track" or "tbeats" */
double bl_amd_tbeats_profile_ms(const char *name, int *launches) {
  if (launches) *launches = 0;
  const int k = !name                           ? -1
                : !strcmp(name, "tbeats_track") ? TBK_TRACK
                : !strcmp(name, "tbeats")       ? TBK_BEATS
                                                : -1;
  if (k < 0) return -1.0;
  return side_profile_ms(SIDE_TBEATS, k, launches);
}

} /* extern "C" */
