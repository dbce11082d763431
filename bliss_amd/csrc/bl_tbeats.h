/*
 * bl_tbeats.h — internal seam between the kernels of the beat grid that follows the tempo over time
 * (bl_tbeats_kernels.hip) and their call path and C-ABI (bl_tbeats_api.hip).  Like the tempogram, the call keeps to
 * itself: its own records, workspace and kernel timing.  C++ only, not installed.
 */
#ifndef BL_TBEATS_H_
#define BL_TBEATS_H_

#include "bl_launch.h"

#define BL_TBEATS_RING 2048       /* scores k_tbeats keeps in LDS, C[t] at t mod 2048 */
#define BL_TBEATS_TRACK_TILE 256  /* frames k_tbeats_track scans at a time: one per lane */
#define BL_TBEATS_GROUP_SONGS 32768       /* songs per launch group */
#define BL_TBEATS_GROUP_HOPS (1ll << 25)  /* hops per launch group, unless its first song alone has more */

struct bl_tbeats_song { /* one song of a launch group; the records are sorted longest first (bl_groups.h) */
  long long onset_off; /* its first hop in the caller's curve and arrays: the sum of H before it in the caller's order */
  long long frame_off; /* its first frame in the caller's lags and track: the sum of F before it in the caller's order */
  long long hop_off;   /* its first hop in the link scratch: the sum of H before it in its launch group */
  int hops, frames;    /* 1 <= H < 2^24, 0 <= F <= 2^20 */
  int out_idx;         /* position in the caller's order: its record in d_songs_out, its anchor in d_anchor */
  int pad;
};

inline bool tbeats_hops_ok(int h) { return h >= 1 && h < (1 << 24); }
inline bool tbeats_frames_ok(int f) { return f >= 0 && f <= (1 << 20); }
inline bool tbeats_params_ok(const bl_amd_tbeats_params &p) {
  return p.seg >= 16 && p.seg <= 16384 && p.origin >= 0 && p.origin < (1 << 24) && p.tight >= 0 &&
         p.tight <= BL_AMD_BEATS_TIGHT_MAX && (p.fold == 0 || p.fold == 1) && p.reserved[0] == 0 && p.reserved[1] == 0 &&
         p.reserved[2] == 0 && p.reserved[3] == 0;
}

/* the kernel ids the launchers hand to their mark function */
enum { TBK_TRACK, TBK_BEATS, TBK_COUNT };

/* Stages 1 to 3, one workgroup per record of d_songs: writes q of every frame of its songs to d_track (the caller's
 * output or scratch, in the layout of the lags) and status, frames, n_filled, n_folded and reserved of their records.
 * d_anchor may be nullptr. */
int blk_tbeats_track(hipStream_t s, const bl_tbeats_song *d_songs, int n_songs, const void *d_lag, int lag_stride,
                     const void *d_anchor, int anchor_stride, const bl_amd_tbeats_params *d_params, int32_t *d_track,
                     bl_amd_song_tbeats *d_songs_out, blk_mark_fn mark, void *mark_user);
/* Stages 4 to 8 of one launch group, one workgroup per record of d_songs, over what blk_tbeats_track left.
 * d_links_out, d_scores_out: nullptr or the arrays of ALL songs of the call; d_link_scratch: used without d_links_out,
 * one uint16 per hop of the group.  Writes the remaining fields of the group's records and every element of its songs
 * in the arrays. */
int blk_tbeats_group(hipStream_t s, const uint32_t *d_onsets, const bl_tbeats_song *d_songs, int n_songs,
                     const bl_amd_tbeats_params *d_params, const int32_t *d_track, bl_amd_song_tbeats *d_songs_out,
                     uint8_t *d_flags_out, uint16_t *d_links_out, uint16_t *d_link_scratch, int64_t *d_scores_out,
                     blk_mark_fn mark, void *mark_user);

#endif /* BL_TBEATS_H_ */
