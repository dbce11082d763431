/*
 * bl_cover.h — internal seam between the cover and version matching kernels (bl_cover_kernels.hip) and their call path
 * and C-ABI (bl_cover_api.hip).  Like the fingerprints and the structure pass, the matching keeps to itself: its own
 * records, workspace and kernel timing.  The units are the structure pass's (bl_form.h: blk_form_units, launched as it
 * is).  C++ only, not installed.
 */
#ifndef BL_COVER_H_
#define BL_COVER_H_

#include "bl_launch.h"

#define BL_COVER_COUNT_MAX (1 << 20)           /* units of one song stay below this */
#define BL_COVER_UNITS_MAX BL_AMD_FORM_UNITS_MAX /* units of a song the alignment takes */
#define BL_COVER_LANES 64                      /* lanes of one workgroup of both kernels: one wavefront */
#define BL_COVER_STRIP 64                      /* columns of b one wavefront owns at a time: one per lane */
#define BL_COVER_ROWS 64                       /* rows of a whose units and strip edge are fetched at a time */
#define BL_COVER_THR_MAX 16128
#define BL_COVER_GAP_MAX (1 << 20)

struct bl_cover_seq { /* one song of a set */
  long long off; /* its first unit: the sum of the counts before it */
  int count, reserved;
};

inline bool cover_count_ok(int n) { return n >= 0 && n < BL_COVER_COUNT_MAX; }
inline bool cover_params_ok(const bl_amd_cover_params &p) {
  return p.thr >= 1 && p.thr <= BL_COVER_THR_MAX && p.gap >= 0 && p.gap <= BL_COVER_GAP_MAX && p.transpose >= -1 &&
         p.transpose <= 11 && p.reserved == 0;
}

/* the kernel ids the launchers hand to their mark function; CVK_UNITS is FMK_UNITS, what blk_form_units marks with */
enum { CVK_UNITS, CVK_PROFILE, CVK_ALIGN, CVK_COUNT };

/* one wavefront per song of the n_seq records (both sets, a first); writes all twelve g of every song, zeros for a song
 * above BL_COVER_UNITS_MAX.  d_units_a / d_units_b: the sets' units; records [0, n_a) address the first. */
int blk_cover_profile(hipStream_t s, const uint4 *d_units_a, const uint4 *d_units_b, const bl_cover_seq *d_seq, int n_a,
                      int n_seq, uint32_t *d_prof, blk_mark_fn mark, void *mark_user);
/* one wavefront per pair; max_units_a: the largest count of set a that is not above BL_COVER_UNITS_MAX.  d_prof is what
 * blk_cover_profile wrote for the same records.  Writes every byte of the n_pairs records. */
int blk_cover_align(hipStream_t s, const uint4 *d_units_a, const uint4 *d_units_b, const bl_cover_seq *d_seq, int n_a,
                    int n_b, const uint32_t *d_prof, const int32_t *d_pairs, int n_pairs, int max_units_a,
                    const bl_amd_cover_params &p, bl_amd_cover_match *d_out, blk_mark_fn mark, void *mark_user);

#endif /* BL_COVER_H_ */
