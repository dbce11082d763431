/*
 * bl_form.h — internal seam between the song-structure kernels (bl_form_kernels.hip) and their call path and C-ABI
 * (bl_form_api.hip).  Like the fingerprints, the structure pass keeps to itself: its own records, workspace and kernel
 * timing.  C++ only, not installed.
 */
#ifndef BL_FORM_H_
#define BL_FORM_H_

#include "bl_launch.h"

#define BL_FORM_COUNT_MAX (1 << 20) /* frames of one song stay below this (T < 2^20) */
#define BL_FORM_BLOCK_UNITS 256     /* units, and lanes, of one workgroup of k_form_units */
#define BL_FORM_LANES 256           /* lanes of one workgroup of k_form_thumb and k_form_novelty */
#define BL_FORM_CHUNK_LAGS BL_FORM_LANES /* lags a workgroup of k_form_thumb takes at a time: one per lane */

struct bl_form_song { /* record i is song i in the caller's order */
  long long frame_off; /* the song's first frame record: the sum of T over the songs before it */
  long long unit_off;  /* the song's first unit: the sum of U over the songs before it */
  long long group_off; /* the song's first workgroup of k_form_units: the sum of ceil(U / 256) over the songs before */
  int frames, units;   /* T, U = floor(T / P) */
};

inline bool form_count_ok(int n) { return n >= 0 && n < BL_FORM_COUNT_MAX; }
inline bool form_params_ok(const bl_amd_form_params &p) {
  return p.pool >= 1 && p.pool <= 16 && p.seg >= 2 && p.seg <= 1024 && p.min_lag >= 1 &&
         p.min_lag <= BL_AMD_FORM_UNITS_MAX && p.nov >= 1 && p.nov <= 64 && p.peak_den >= 1 && p.peak_den <= 256 &&
         p.peak_num >= 0 && p.peak_num <= p.peak_den && p.reserved == 0;
}

enum { FMK_UNITS, FMK_THUMB, FMK_NOVELTY, FMK_COUNT }; /* the kernel ids the launchers hand to their mark function */

/* d_songs: the n_songs records; n_groups: the sum of ceil(U / 256) over them (may be 0).  Writes every unit. */
int blk_form_units(hipStream_t s, const bl_amd_frame_chroma *d_frames, const bl_form_song *d_songs, int n_songs,
                   long long n_groups, int pool, uint4 *d_units, blk_mark_fn mark, void *mark_user);
/* one workgroup per song; max_units: the largest U of the call that is not above BL_AMD_FORM_UNITS_MAX.  Writes units,
 * status and the four thumbnail fields of every record and, unless d_rep is nullptr, every element of it. */
int blk_form_thumb(hipStream_t s, const uint4 *d_units, const bl_form_song *d_songs, int n_songs, int max_units, int seg,
                   int min_lag, bl_amd_song_form *d_out, uint32_t *d_rep, blk_mark_fn mark, void *mark_user);
/* one workgroup per song; writes the remaining fields of every record, every element of d_nov (never nullptr: the
 * caller's output or scratch) and, unless d_flags is nullptr, of it */
int blk_form_novelty(hipStream_t s, const uint4 *d_units, const bl_form_song *d_songs, int n_songs, int nov,
                     int peak_num, int peak_den, bl_amd_song_form *d_out, unsigned long long *d_nov, uint8_t *d_flags,
                     blk_mark_fn mark, void *mark_user);

#endif /* BL_FORM_H_ */
