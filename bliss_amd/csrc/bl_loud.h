/*
 * bl_loud.h — internal seam between the loudness kernels (bl_loud_kernels.hip) and their call path and C-ABI
 * (bl_loud_api.hip).  The loudness keeps to itself: it has its own records, workspace and kernel timing, and nothing of
 * the contexts' workspace (bl_runtime.h) or of the other launchers (bl_launch.h) knows about it.  C++ only, not
 * installed.
 */
#ifndef BL_LOUD_H_
#define BL_LOUD_H_

#include "bl_launch.h"

struct bl_loud_song { /* the records are sorted stereo first, so that the lanes of a wave mostly run one shape */
  unsigned long long pcm_off; /* int16 elements from the arena base, a multiple of 8 (unused from hop energies) */
  long long hop_off;          /* the song's first hop in Z and d_hops_out: the sum of H over the songs before it in the
                                 caller's order */
  long long chunk_off;        /* the song's first lane of k_loud_filter: the sum of ceil(H / 16) over the records before
                                 it in the sorted order */
  long long st_off;           /* the song's first short-term start in the scratch: the sum of blk_loud_starts(H) over
                                 the songs before it in the caller's order */
  int hops, channels;         /* H >= 0, 1 | 2 */
  int out_idx;                /* position in the caller's order: its record in d_songs_out */
  int reserved;
};

enum { LK_FILTER, LK_GATE, LK_COUNT }; /* the kernel ids the launchers hand to their mark function */

/* short-term starts j = 0, 10, 20, ... <= H - 30 of a song of H hops */
__host__ __device__ inline long long blk_loud_starts(long long hops) { return hops >= 30 ? (hops - 30) / 10 + 1 : 0; }
/* stages 1 to 3: one lane per chunk of d_songs[0 .. n_songs), n_chunks in all (may be 0); writes Z of every hop */
int blk_loud_filter(hipStream_t s, const int16_t *d_pcm, const bl_loud_song *d_songs, int n_songs, long long n_chunks,
                    const bl_amd_loud_params &p, unsigned long long *d_z, blk_mark_fn mark, void *mark_user);
/* stages 4 to 6: one workgroup per song over Z; d_st: blk_loud_starts(H) values per song; writes every byte of the
 * n_songs records */
int blk_loud_gate(hipStream_t s, const unsigned long long *d_z, const bl_loud_song *d_songs, int n_songs,
                  unsigned long long abs_gate, unsigned long long *d_st, bl_amd_song_loud *d_songs_out,
                  blk_mark_fn mark, void *mark_user);

/* what the forms accept of a song and of the parameter record (from_hops: only abs_gate is read) */
inline bool loud_song_ok(unsigned long long pcm_offset, int n_samples, int channels) {
  return n_samples >= 1 && (channels == 1 || channels == 2) && !(pcm_offset & 7);
}
inline bool loud_params_ok(const bl_amd_loud_params *p, bool from_hops) {
  if (!p || p->abs_gate >= (1ull << 56)) return false;
  if (from_hops) return true;
  const double coef[] = {p->s1_b[0], p->s1_b[1], p->s1_b[2], p->s1_a[0], p->s1_a[1], p->s2_a[0], p->s2_a[1]};
  for (double x : coef)
    if (!(x - x == 0.0)) return false; /* an infinity or a NaN */
  return p->hop >= 1 && p->hop <= 4800 && p->warm >= 0 && p->warm <= 8192;
}
inline int loud_hops(int n_samples, int channels, int hop) { return n_samples / channels / hop; }

#endif /* BL_LOUD_H_ */
