/*
 * bl_fprint.h — internal seam between the fingerprint kernels (bl_fprint_kernels.hip) and their call path and C-ABI
 * (bl_fprint_api.hip).  Like the loudness and the true peak, the fingerprints keep to themselves: their own records,
 * workspace and kernel timing.  C++ only, not installed.
 */
#ifndef BL_FPRINT_H_
#define BL_FPRINT_H_

#include "bl_launch.h"

#define BL_FPRINT_COUNT_MAX (1 << 20) /* frames or words of one song stay below this (T < 2^20) */

/* ---- words ---- */
#define BL_FPRINT_BLOCK_WORDS 256 /* words, and lanes, of one workgroup of k_fprint_words */

struct bl_fprint_song { /* record i is song i in the caller's order */
  long long frame_off; /* the song's first frame record: the sum of T over the songs before it */
  long long word_off;  /* the song's first word: the sum of W over the songs before it */
  long long group_off; /* the song's first workgroup: the sum of ceil(W / 256) over the songs before it */
  int frames, words;   /* T, W = max(0, T - 15) */
};

inline int fprint_words_of(int frames) { return frames > 15 ? frames - 15 : 0; }
inline bool fprint_count_ok(int n) { return n >= 0 && n < BL_FPRINT_COUNT_MAX; }

/* ---- match ---- */
#define BL_FPRINT_LANES 256      /* lanes of one workgroup of k_fprint_match */
#define BL_FPRINT_UNIT 4         /* a lane owns 4 consecutive offsets and walks `a` 4 words at a time */
#define BL_FPRINT_STRIP_WORDS 64 /* consecutive words of `a` one lane walks per tile */
#define BL_FPRINT_STRIPS_MAX 32  /* strips per tile at most: a tile of `a` is at most 2 048 words */

struct bl_fprint_seq { /* one song of a set */
  long long off; /* its first word: the sum of the counts before it */
  int count, reserved;
};

/* how a workgroup of k_fprint_match spreads over the 2 D + 1 offsets: they are cut into groups of 4, the groups into
 * `chunks` equal runs of `groups` each, which the workgroup takes one after the other; its 256 lanes are `strips` rows
 * of `groups` lanes, and row r walks words [64 r, 64 r + 64) of every tile of 64 * strips words of `a` */
struct bl_fprint_geom {
  int chunks, groups, strips;
};
inline bl_fprint_geom fprint_geom(int max_shift) {
  const int ng = (2 * max_shift + 1 + BL_FPRINT_UNIT - 1) / BL_FPRINT_UNIT;
  bl_fprint_geom g;
  g.chunks = (ng + BL_FPRINT_LANES - 1) / BL_FPRINT_LANES;
  g.groups = (ng + g.chunks - 1) / g.chunks;
  g.strips = BL_FPRINT_LANES / g.groups;
  if (g.strips > BL_FPRINT_STRIPS_MAX) g.strips = BL_FPRINT_STRIPS_MAX;
  return g;
}

enum { FK_WORDS, FK_MATCH, FK_COUNT }; /* the kernel ids the launchers hand to their mark function */

/* d_songs: the n_songs records, n_groups the sum of ceil(W / 256) over them (may be 0).  Writes every word. */
int blk_fprint_words(hipStream_t s, const bl_amd_frame_chroma *d_frames, const bl_fprint_song *d_songs, int n_songs,
                     long long n_groups, uint32_t *d_words, blk_mark_fn mark, void *mark_user);
/* one workgroup per pair; writes every byte of the n_pairs records and, unless d_profile is nullptr, all
 * n_pairs * (2 max_shift + 1) * 2 values of the profile */
int blk_fprint_match(hipStream_t s, const uint32_t *d_words_a, const bl_fprint_seq *d_seq_a, int n_a,
                     const uint32_t *d_words_b, const bl_fprint_seq *d_seq_b, int n_b, const int32_t *d_pairs,
                     int n_pairs, int max_shift, int min_overlap, bl_amd_fprint_match *d_out, uint32_t *d_profile,
                     blk_mark_fn mark, void *mark_user);

#endif /* BL_FPRINT_H_ */
