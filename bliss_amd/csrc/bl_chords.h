/*
 * bl_chords.h — internal seam between the chord kernels (bl_chords_kernels.hip) and their call path and C-ABI
 * (bl_chords_api.hip).  Like the structure pass and the version matching, the chords keep to themselves: their own
 * records, workspace and kernel timing.  C++ only, not installed.
 */
#ifndef BL_CHORDS_H_
#define BL_CHORDS_H_

#include "bl_launch.h"

#define BL_CHORDS_COUNT_MAX (1 << 20) /* units of one song stay below this */
#define BL_CHORDS_LABELS BL_AMD_CHORDS_LABELS
#define BL_CHORDS_STEP_UNITS 4   /* units of one round of the forward kernel: one backpointer word per label */
#define BL_CHORDS_TRACE_UNITS 256 /* units whose backpointers the back-trace holds in LDS at a time */
#define BL_CHORDS_SPW 1          /* songs that share a wavefront of the forward kernel: 1 | 2; 1 measured faster */
#define BL_CHORDS_BP_WORDS 32    /* uint32 of one round's backpointers: word c holds B_t[c] of its four units */

struct bl_chords_song { /* one song of a call */
  long long unit_off; /* its first unit: the sum of the counts before it */
  long long bp_off;   /* its first round in the backpointer block: the sum of ceil(U / 4) over the songs before it */
  int units, reserved;
};

struct bl_chords_end { /* what the forward kernel leaves the back-trace of a song with units */
  int score, last;     /* V_{U-1}[L_{U-1}] and L_{U-1} */
};

inline bool chords_count_ok(int n) { return n >= 0 && n < BL_CHORDS_COUNT_MAX; }
inline bool chords_params_ok(const bl_amd_chords_params &p) {
  if (p.none < 0 || p.none > BL_AMD_CHORDS_EMISSION_MAX || p.reserved != 0 || p.pad[0] || p.pad[1] || p.pad[2])
    return false;
  for (int i = 0; i < BL_CHORDS_LABELS * BL_CHORDS_LABELS; ++i)
    if (p.cost[i] > BL_AMD_CHORDS_COST_MAX) return false;
  return true;
}

/* the kernel ids the launchers hand to their mark function */
enum { CHK_FORWARD, CHK_TRACE, CHK_COUNT };

/* spw songs per wavefront (1 | 2), one wavefront per workgroup.  Writes the backpointers of every unit t >= 1 of every
 * song (d_bp: BL_CHORDS_BP_WORDS uint32 per round of four units) and d_end of every song with units. */
int blk_chords_forward(hipStream_t s, const uint4 *d_units, const bl_chords_song *d_songs, int n_songs,
                       const bl_amd_chords_params *d_params, int spw, uint32_t *d_bp, bl_chords_end *d_end,
                       blk_mark_fn mark, void *mark_user);
/* one wavefront per song, over what blk_chords_forward left.  Writes every byte of the n_songs records and, unless they
 * are nullptr, every song's labels and its 25 counts. */
int blk_chords_trace(hipStream_t s, const bl_chords_song *d_songs, int n_songs, const uint32_t *d_bp,
                     const bl_chords_end *d_end, bl_amd_song_chords *d_out, uint8_t *d_labels_out, uint32_t *d_hist_out,
                     blk_mark_fn mark, void *mark_user);

#endif /* BL_CHORDS_H_ */
