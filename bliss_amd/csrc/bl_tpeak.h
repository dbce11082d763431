/*
 * bl_tpeak.h — internal seam between the true-peak kernels (bl_tpeak_kernels.hip) and their call path and C-ABI
 * (bl_tpeak_api.hip).  Like the loudness, the true peak keeps to itself: its own records, workspace and kernel timing.
 * C++ only, not installed.
 */
#ifndef BL_TPEAK_H_
#define BL_TPEAK_H_

#include "bl_launch.h"

#define BL_TPEAK_LANE_FRAMES 16                           /* consecutive frames one lane owns */
#define BL_TPEAK_GROUP_LANES 256                          /* lanes of a workgroup */
#define BL_TPEAK_GROUP_FRAMES (BL_TPEAK_LANE_FRAMES * BL_TPEAK_GROUP_LANES) /* frames one workgroup owns: 4096 */

struct bl_tpeak_song { /* record i belongs to d_songs_out[i]: the caller's order */
  unsigned long long pcm_off; /* int16 elements from the arena base, a multiple of 8 */
  long long group_off;        /* the song's first workgroup of k_tpeak_scan: the sum of ceil(F / 4096) over the songs
                                 before it */
  long long blk_off;          /* the song's first block in d_blocks_out: the sum of ceil(F / block) over the songs before
                                 it */
  int frames, channels;       /* F >= 0, 1 | 2 */
};

struct bl_tpeak_acc { /* what the lanes of a song join into; zeroed by the launcher */
  unsigned long long key[2];   /* max of (|y| << 33) | (2^33 - 1 - i) per channel: the largest |y| at its smallest i */
  unsigned long long overs[2];
  int peak[2];
  int reserved[2];
};

enum { TK_SCAN, TK_FINISH, TK_COUNT }; /* the kernel ids the launcher hands to its mark function */

/* One call: d_songs its n_songs records, n_groups the sum of ceil(F / 4096) over them (may be 0); d_acc: n_songs
 * accumulators, zeroed here; d_blocks: nullptr, or n_blocks * 2 values, zeroed here.  Writes every byte of the n_songs
 * records in d_songs_out. */
int blk_tpeak(hipStream_t s, const int16_t *d_pcm, const bl_tpeak_song *d_songs, int n_songs, long long n_groups,
              int ceiling, int block, bl_tpeak_acc *d_acc, bl_amd_song_tpeak *d_songs_out, uint32_t *d_blocks,
              long long n_blocks, blk_mark_fn mark, void *mark_user);

/* what the forms accept of a song and of the two parameters */
inline bool tpeak_song_ok(unsigned long long pcm_offset, int n_samples, int channels) {
  return n_samples >= 1 && (channels == 1 || channels == 2) && !(pcm_offset & 7);
}
inline bool tpeak_args_ok(int ceiling, int block) {
  return ceiling >= 0 && ceiling <= 65535 && block >= 1 && block <= 65536;
}
inline long long tpeak_blocks(int n_samples, int channels, int block) {
  return ((long long)(n_samples / channels) + block - 1) / block;
}

#endif /* BL_TPEAK_H_ */
