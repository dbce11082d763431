/*
 * bl_tgram.h — internal seam between the tempogram kernels (bl_tgram_kernels.hip) and their call path and C-ABI
 * (bl_tgram_api.hip).  Like the chords, the tempogram keeps to itself: its own records, workspace and kernel timing.
 * C++ only, not installed.
 */
#ifndef BL_TGRAM_H_
#define BL_TGRAM_H_

#include "bl_launch.h"

#define BL_TGRAM_TILE 1024     /* terms of the curve the block kernel stages at a time: max(1, 1024 / S) whole blocks */
#define BL_TGRAM_RUN_FRAMES 64 /* the fewest frames of one run of the block kernel, where a song is cut into runs */
#define BL_TGRAM_GRID_SONGS 32768 /* songs of one launch: grid.y */

struct bl_tgram_song { /* one song of a call */
  long long onset_off; /* its first hop: the sum of H before it */
  long long frame_off; /* its first frame record: the sum of F before it */
  int hops, frames;
};

inline bool tgram_hops_ok(int h) { return h >= 1 && h < (1 << 24); }
inline bool tgram_params_ok(const bl_amd_tgram_params &p) {
  return p.stride >= 16 && p.stride <= 1024 && p.stride % 16 == 0 && p.blocks >= 1 && p.blocks <= 16 && p.lag_min >= 1 &&
         p.lag_min <= p.lag_max && p.lag_max <= BL_AMD_RHYTHM_LAGS - 2 && p.tol >= 0 && p.tol <= 1000 &&
         (p.octaves == 0 || p.octaves == 1) && p.reserved[0] == 0 && p.reserved[1] == 0;
}

/* the kernel ids the launchers hand to their mark function */
enum { TGK_BLOCKS, TGK_SONGS, TGK_COUNT };

/* The block rows, the frames' rows and the pick: writes every frame record of every song and, unless d_gram_out is
 * nullptr, every frame's 512 lag products.  max_frames: the largest F of the call (nothing is launched for 0);
 * h_params: the caller's checked parameters, for the launch shape alone. */
int blk_tgram_blocks(hipStream_t s, const uint32_t *d_onsets, const bl_tgram_song *d_songs, int n_songs, int max_frames,
                     const bl_amd_tgram_params &h_params, const bl_amd_tgram_params *d_params, int n_cu,
                     bl_amd_tgram_frame *d_frames_out, uint64_t *d_gram_out, blk_mark_fn mark, void *mark_user);
/* one wavefront per song over the frame records: writes every byte of the n_songs records */
int blk_tgram_songs(hipStream_t s, const bl_tgram_song *d_songs, int n_songs, const bl_amd_tgram_params *d_params,
                    const bl_amd_tgram_frame *d_frames, bl_amd_song_tgram *d_out, blk_mark_fn mark, void *mark_user);

#endif /* BL_TGRAM_H_ */
