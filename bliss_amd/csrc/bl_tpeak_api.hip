/*
 * bl_tpeak_api.hip — call path and C-ABI of the true peak (include/bliss_amd.h: bl_amd_tpeak_*); the kernels are
 * bl_tpeak_kernels.hip's, the host arithmetic over the records bl_api.c's.  Host code only.
 *
 * The true peak keeps a side workspace (bl_side_ws.h, which has the protocol): the songs' records, and as extra block
 * one accumulator per song.
 */
#include <string.h>

#include "bl_side_ws.h"
#include "bl_tpeak.h"

namespace {

int tpeak_device(bl_amd_ctx *c, bool dflt, const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs,
                 int ceiling, int block, bl_amd_song_tpeak *d_songs_out, uint32_t *d_blocks_out, long long n_blocks,
                 void *stream) {
  if (!d_pcm || ((uintptr_t)d_pcm & 15) || !h_desc || !d_songs_out || ((uintptr_t)d_songs_out & 7) ||
      ((uintptr_t)d_blocks_out & 3) || n_songs < 1 || !tpeak_args_ok(ceiling, block))
    return BL_UNEXPECTED;
  long long total = 0, groups = 0; /* the sums of ceil(F / block) and of ceil(F / 4096) over the songs */
  for (int i = 0; i < n_songs; ++i) {
    if (!tpeak_song_ok(h_desc[i].pcm_offset, h_desc[i].n_samples, h_desc[i].channels)) return BL_UNEXPECTED;
    total += tpeak_blocks(h_desc[i].n_samples, h_desc[i].channels, block);
    groups += tpeak_blocks(h_desc[i].n_samples, h_desc[i].channels, BL_TPEAK_GROUP_FRAMES);
  }
  if ((d_blocks_out && n_blocks != total) || groups > (1ll << 30) || !(c = call_ctx(c, dflt))) return BL_UNEXPECTED;
  CtxGuard g(c);
  if (!g.ok()) return BL_UNEXPECTED;
  return side_call(SIDE_TPEAK, c, static_cast<hipStream_t>(stream), sizeof(bl_tpeak_song) * (size_t)n_songs,
                   [&](void *pinned) {
    bl_tpeak_song *hs = static_cast<bl_tpeak_song *>(pinned);
    long long blk = 0, grp = 0;
    for (int i = 0; i < n_songs; ++i) {
      hs[i].pcm_off = h_desc[i].pcm_offset;
      hs[i].group_off = grp;
      hs[i].blk_off = blk;
      hs[i].frames = h_desc[i].n_samples / h_desc[i].channels;
      hs[i].channels = h_desc[i].channels;
      blk += tpeak_blocks(h_desc[i].n_samples, h_desc[i].channels, block);
      grp += tpeak_blocks(h_desc[i].n_samples, h_desc[i].channels, BL_TPEAK_GROUP_FRAMES);
    }
    return BL_OK;
  }, [&](hipStream_t s, bl_side_ws &w, blk_mark_fn mark, void *user) {
    if (blr_ensure(w.extra[0], sizeof(bl_tpeak_acc) * (size_t)n_songs) != BL_OK) return BL_UNEXPECTED;
    return blk_tpeak(s, d_pcm, static_cast<bl_tpeak_song *>(w.recs.p), n_songs, groups, ceiling, block,
                     static_cast<bl_tpeak_acc *>(w.extra[0].p), d_songs_out, d_blocks_out, total, mark, user);
  });
}

} // namespace

/* ========================================================================= */
/* C-ABI                                                                      */

extern "C" {

int bl_amd_ctx_tpeak_batch_device(bl_amd_ctx *c, const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs,
                                  int ceiling, int block, bl_amd_song_tpeak *d_songs_out, uint32_t *d_blocks_out,
                                  long long n_blocks, void *stream) {
  return tpeak_device(c, false, d_pcm, h_desc, n_songs, ceiling, block, d_songs_out, d_blocks_out, n_blocks, stream);
}

int bl_amd_tpeak_batch_device(const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs, int ceiling, int block,
                              bl_amd_song_tpeak *d_songs_out, uint32_t *d_blocks_out, long long n_blocks,
                              void *stream) {
  return tpeak_device(nullptr, true, d_pcm, h_desc, n_songs, ceiling, block, d_songs_out, d_blocks_out, n_blocks,
                      stream);
}

/* the songs in waves (host_form, bl_runtime.h): each is measured by the device form and fetched */
int bl_amd_tpeak_batch_host(const int16_t *const *h_pcm, const int32_t *n_samples, const int32_t *channels, int n_songs,
                            int ceiling, int block, bl_amd_song_tpeak *h_songs_out, uint32_t *h_blocks_out) {
  return host_form(h_pcm, n_samples, channels, n_songs, h_songs_out && tpeak_args_ok(ceiling, block), tpeak_song_ok,
                   [&](const int16_t *d_pcm, const bl_amd_song_desc *desc, int b, int e) {
                     long long blocks = 0;
                     for (int i = b; i < e; ++i) blocks += tpeak_blocks(n_samples[i], channels[i], block);
                     WaveOut<bl_amd_song_tpeak> out(h_songs_out, e - b);
                     WaveOut<uint32_t> bout(h_blocks_out, 2 * blocks); /* a block is a pair: 8 bytes */
                     if (!out.ok() || !bout.ok() ||
                         bl_amd_tpeak_batch_device(d_pcm, desc, e - b, ceiling, block, out.dev(), bout.dev(), blocks,
                                                   nullptr) != BL_OK)
                       return BL_UNEXPECTED;
                     BL_HIP_CHECK(hipStreamSynchronize(nullptr));
                     return out.fetch() && (!blocks || bout.fetch()) ? BL_OK : BL_UNEXPECTED;
                   });
}

/* the kernel's two tiling constants */
void bl_amd_tpeak_shape(int *frames_per_lane, int *frames_per_group) {
  if (frames_per_lane) *frames_per_lane = BL_TPEAK_LANE_FRAMES;
  if (frames_per_group) *frames_per_group = BL_TPEAK_GROUP_FRAMES;
}

/* device time of a true-peak kernel since this was last asked for it: "tpeak_scan" or "tpeak_finish" */
double bl_amd_tpeak_profile_ms(const char *name, int *launches) {
  if (launches) *launches = 0;
  const int k = !name ? -1 : !strcmp(name, "tpeak_scan") ? TK_SCAN : !strcmp(name, "tpeak_finish") ? TK_FINISH : -1;
  if (k < 0) return -1.0;
  return side_profile_ms(SIDE_TPEAK, k, launches);
}

} /* extern "C" */
