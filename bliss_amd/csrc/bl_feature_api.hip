/*
 * bl_feature_api.hip — call paths and C-ABI of the six per-song features that keep their blocks in the context's own
 * workspace (include/bliss_amd.h: bl_amd_levels_*, bl_amd_timbre_*, bl_amd_rhythm_*, bl_amd_beats_*, bl_amd_chroma_*,
 * bl_amd_mel_*): the device forms, the *_batch_host forms and the forms on the caller's onset curves.  Host code only.
 * One file, not six: timbre and mel share frame_songs_fill, tempo and beats the launch-group planner (bl_groups.h), and
 * five of them the host form (host_form, WaveOut: bl_runtime.h); every device form goes through record_call.
 */
#include <algorithm>

#include "bl_groups.h"
#include "bl_runtime.h"

namespace {

/* ---- signal levels (bl_level_kernels.hip) ---------------------------------- */

int levels_device(bl_amd_ctx *c, bool dflt, const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs,
                  int silence, bl_amd_song_levels *d_levels, void *stream) {
  if (!d_pcm || ((uintptr_t)d_pcm & 15) || !h_desc || !d_levels || n_songs < 1 || silence < 0 || silence > 32767)
    return BL_UNEXPECTED;
  for (int i = 0; i < n_songs; ++i)
    if (!levels_song_ok(h_desc[i].pcm_offset, h_desc[i].n_samples, h_desc[i].channels)) return BL_UNEXPECTED;
  if (!(c = call_ctx(c, dflt))) return BL_UNEXPECTED;
  CtxGuard g(c);
  if (!g.ok()) return BL_UNEXPECTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  int max_n = 0;
  return record_call<bl_level_song>(c, s, c->level_songs, n_songs, [&](bl_level_song *hs) {
    for (int i = 0; i < n_songs; ++i) {
      hs[i].pcm_off = h_desc[i].pcm_offset;
      hs[i].n = h_desc[i].n_samples;
      hs[i].channels = h_desc[i].channels;
      max_n = std::max(max_n, h_desc[i].n_samples);
    }
    return BL_OK;
  }, [&](const bl_level_song *, bl_level_song *d_songs) {
    return blk_levels(s, d_pcm, d_songs, n_songs, max_n, silence, c->n_cu, d_levels);
  });
}

/* ---- per-frame spectral timbre (bl_timbre_kernels.hip) ------------------------ */

/* the records of the kernels that take one workgroup per song over the frames of the frequency pass (k_timbre, k_mel) */
int frame_songs_fill(const bl_amd_song_desc *h_desc, int n_songs, bl_timbre_song *hs) {
  long long frame_off = 0;
  for (int i = 0; i < n_songs; ++i) {
    hs[i].pcm_off = h_desc[i].pcm_offset;
    hs[i].frame_off = frame_off;
    hs[i].n_frames = bl_amd_timbre_frames(h_desc[i].n_samples, h_desc[i].channels);
    hs[i].channels = h_desc[i].channels;
    hs[i].out_idx = i;
    hs[i].reserved = 0;
    frame_off += hs[i].n_frames;
  }
  /* one workgroup per song, the longest first, as the analysis lays its songs out: the long songs start while there
   * are short ones left to fill the chip behind them */
  std::stable_sort(hs, hs + n_songs,
                   [](const bl_timbre_song &a, const bl_timbre_song &b) { return a.n_frames > b.n_frames; });
  return BL_OK;
}

int timbre_device(bl_amd_ctx *c, bool dflt, const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs, int pct,
                  uint64_t min_energy, bl_amd_song_timbre *d_songs_out, bl_amd_frame_timbre *d_frames_out,
                  long long n_frame_records, void *stream) {
  if (!d_pcm || ((uintptr_t)d_pcm & 15) || !h_desc || !d_songs_out || ((uintptr_t)d_songs_out & 7) ||
      ((uintptr_t)d_frames_out & 7) || n_songs < 1 || pct < 1 || pct > 100)
    return BL_UNEXPECTED;
  long long total = 0; /* the sum of F over the songs */
  for (int i = 0; i < n_songs; ++i) {
    if (!timbre_song_ok(h_desc[i].pcm_offset, h_desc[i].n_samples, h_desc[i].channels)) return BL_UNEXPECTED;
    total += bl_amd_timbre_frames(h_desc[i].n_samples, h_desc[i].channels);
  }
  if ((d_frames_out && n_frame_records != total) || !(c = call_ctx(c, dflt))) return BL_UNEXPECTED;
  CtxGuard g(c);
  if (!g.ok()) return BL_UNEXPECTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return record_call<bl_timbre_song>(c, s, c->timbre_songs, n_songs, [&](bl_timbre_song *hs) {
    return frame_songs_fill(h_desc, n_songs, hs);
  }, [&](const bl_timbre_song *, bl_timbre_song *d_songs) {
    return blk_timbre(s, d_pcm, d_songs, n_songs, c->tb, pct, min_energy, d_songs_out, d_frames_out);
  });
}

/* ---- tempo (bl_rhythm_kernels.hip): the call path of bl_amd_rhythm_batch_device and bl_amd_rhythm_from_onsets ---- */

/* One call on n_songs songs, from PCM (d_curve == nullptr) or from onset curves on the device; the caller holds the
 * context.  `song(i, rec)` writes pcm_off, hops and channels of song i in the caller's order.  The records are sorted
 * longest first, as the analysis lays its songs out, and cut into launch groups (bl_groups.h) of at most
 * c->group_songs songs and BL_RHYTHM_GROUP_HOPS = 2^25 hops (a longer song is a group of its own; H < 2^24, so there is
 * none).  The groups follow each other on the stream and share the scratch, which is therefore bounded whatever the
 * call: 4 bytes per hop = 128 MiB of novelty values, and per song 16 bytes of sums and, without d_acf_out, 4 KiB of lag
 * products = 128.5 MiB at 32 768 songs. */
template <class Song>
int rhythm_call(bl_amd_ctx *c, hipStream_t s, int n_songs, Song song, const int16_t *d_pcm, const uint32_t *d_curve,
                int lag_min, int lag_max, bl_amd_song_rhythm *d_songs_out, uint32_t *d_onsets_out,
                uint64_t *d_acf_out) {
  return record_call<bl_rhythm_song>(c, s, c->rhythm_songs, n_songs, [&](bl_rhythm_song *hs) {
    long long onset_off = 0;
    for (int i = 0; i < n_songs; ++i) {
      song(i, hs[i]);
      hs[i].onset_off = onset_off;
      hs[i].out_idx = i;
      hs[i].reserved = 0;
      onset_off += hs[i].hops;
    }
    bl_groups_plan(hs, n_songs, std::min(c->group_songs, BL_RHYTHM_GROUP_SONGS), BL_RHYTHM_GROUP_HOPS);
    return BL_OK;
  }, [&](const bl_rhythm_song *hs, bl_rhythm_song *d_songs) {
    long long hops, max_hops = 0;
    int max_songs = 0;
    for (int b = 0, e; b < n_songs; b = e) {
      e = bl_group_end(hs, b, n_songs, hops);
      max_hops = std::max(max_hops, hops);
      max_songs = std::max(max_songs, e - b);
    }
    if ((!d_curve && blr_ensure(c->rhythm_n, sizeof(uint32_t) * (size_t)max_hops) != BL_OK) ||
        blr_ensure(c->rhythm_rows, blk_rhythm_rows_bytes(max_songs, !d_acf_out)) != BL_OK)
      return BL_UNEXPECTED;
    if (d_acf_out)
      BL_HIP_CHECK(hipMemsetAsync(d_acf_out, 0, sizeof(uint64_t) * BL_AMD_RHYTHM_LAGS * (size_t)n_songs, s));
    for (int b = 0, e; b < n_songs; b = e) {
      e = bl_group_end(hs, b, n_songs, hops);
      if (blk_rhythm_group(s, d_pcm, d_curve, d_songs + b, e - b, hs[b].hops, lag_min, lag_max, c->n_cu,
                           static_cast<uint32_t *>(c->rhythm_n.p), c->rhythm_rows.p, d_songs_out, d_onsets_out,
                           d_acf_out, c->prof ? mark_cb : nullptr, c) != BL_OK)
        return BL_UNEXPECTED;
    }
    return BL_OK;
  });
}

int rhythm_device(bl_amd_ctx *c, bool dflt, const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs,
                  int lag_min, int lag_max, bl_amd_song_rhythm *d_songs_out, uint32_t *d_onsets_out, long long n_onsets,
                  uint64_t *d_acf_out, void *stream) {
  if (!d_pcm || ((uintptr_t)d_pcm & 15) || !h_desc || !d_songs_out || ((uintptr_t)d_songs_out & 7) ||
      ((uintptr_t)d_onsets_out & 3) || ((uintptr_t)d_acf_out & 7) || n_songs < 1 || !rhythm_lags_ok(lag_min, lag_max))
    return BL_UNEXPECTED;
  long long total = 0; /* the sum of H over the songs */
  for (int i = 0; i < n_songs; ++i) {
    if (!rhythm_song_ok(h_desc[i].pcm_offset, h_desc[i].n_samples, h_desc[i].channels)) return BL_UNEXPECTED;
    total += bl_amd_rhythm_hops(h_desc[i].n_samples, h_desc[i].channels);
  }
  if ((d_onsets_out && n_onsets != total) || !(c = call_ctx(c, dflt))) return BL_UNEXPECTED;
  CtxGuard g(c);
  if (!g.ok()) return BL_UNEXPECTED;
  return rhythm_call(c, static_cast<hipStream_t>(stream), n_songs, [&](int i, bl_rhythm_song &r) {
    r.pcm_off = h_desc[i].pcm_offset;
    r.hops = bl_amd_rhythm_hops(h_desc[i].n_samples, h_desc[i].channels);
    r.channels = h_desc[i].channels;
  }, d_pcm, nullptr, lag_min, lag_max, d_songs_out, d_onsets_out, d_acf_out);
}

/* what the forms on the caller's onset curves (tempo, beats) reject before anything is enqueued: a hop count outside
 * [1, 2^24) and, where the curves are in host memory (h_onsets), an onset of 2^18 or more; *total: the sum of H over
 * the songs */
bool curves_ok(const int32_t *h_hops, int n_songs, const uint32_t *h_onsets, long long *total) {
  if (!h_hops || n_songs < 1) return false;
  *total = 0;
  for (int i = 0; i < n_songs; ++i) {
    if (h_hops[i] < 1 || h_hops[i] >= (1 << 24)) return false;
    *total += h_hops[i];
  }
  for (long long k = 0; h_onsets && k < *total; ++k)
    if (h_onsets[k] >= (1u << 18)) return false;
  return true;
}

/* ---- beats (bl_beat_kernels.hip): the call path of bl_amd_beats_device and bl_amd_beats_host ---- */

bool beats_args_ok(const int32_t *h_hops, int n_songs, const uint32_t *h_onsets, int tight, long long *total) {
  return tight >= 0 && tight <= BL_AMD_BEATS_TIGHT_MAX && curves_ok(h_hops, n_songs, h_onsets, total);
}

/* One call on n_songs onset curves on the device; the caller holds the context and has checked the arguments.  As the
 * tempo call does, the records are sorted longest first, so that the long songs do not straggle at the end of the
 * grid, and cut into launch groups (bl_groups.h) of at most c->group_songs songs and BL_BEAT_GROUP_HOPS = 2^25 hops,
 * which follow each other on the stream and share the link scratch: 2 bytes per hop = 64 MiB, whatever the call. */
int beats_call(bl_amd_ctx *c, hipStream_t s, const uint32_t *d_onsets, const int32_t *h_hops, int n_songs,
               const void *d_period, int period_stride, int tight, bl_amd_song_beats *d_songs_out, uint8_t *d_flags_out,
               uint16_t *d_links_out, int64_t *d_scores_out) {
  return record_call<bl_beat_song>(c, s, c->beat_songs, n_songs, [&](bl_beat_song *hs) {
    long long onset_off = 0;
    for (int i = 0; i < n_songs; ++i) {
      hs[i].onset_off = onset_off;
      hs[i].hops = h_hops[i];
      hs[i].out_idx = i;
      onset_off += h_hops[i];
    }
    bl_groups_plan(hs, n_songs, std::min(c->group_songs, BL_BEAT_GROUP_SONGS), BL_BEAT_GROUP_HOPS);
    return BL_OK;
  }, [&](const bl_beat_song *hs, bl_beat_song *d_songs) {
    long long hops, max_hops = 0;
    for (int b = 0, e; b < n_songs; b = e) {
      e = bl_group_end(hs, b, n_songs, hops);
      max_hops = std::max(max_hops, hops);
    }
    if (!d_links_out && blr_ensure(c->beat_links, sizeof(uint16_t) * (size_t)max_hops) != BL_OK) return BL_UNEXPECTED;
    for (int b = 0, e; b < n_songs; b = e) {
      e = bl_group_end(hs, b, n_songs, hops);
      if (blk_beats_group(s, d_onsets, d_songs + b, e - b, d_period, period_stride, tight, d_songs_out, d_flags_out,
                          d_links_out, static_cast<uint16_t *>(c->beat_links.p), d_scores_out,
                          c->prof ? mark_cb : nullptr, c) != BL_OK)
        return BL_UNEXPECTED;
    }
    return BL_OK;
  });
}

int beats_device(bl_amd_ctx *c, bool dflt, const uint32_t *d_onsets, const int32_t *h_hops, int n_songs,
                 const void *d_period, int period_stride, int tight, bl_amd_song_beats *d_songs_out,
                 uint8_t *d_flags_out, uint16_t *d_links_out, int64_t *d_scores_out, void *stream) {
  long long total = 0;
  if (!d_onsets || ((uintptr_t)d_onsets & 3) || !d_period || ((uintptr_t)d_period & 3) || period_stride < 4 ||
      (period_stride & 3) || !d_songs_out || ((uintptr_t)d_songs_out & 7) || !d_flags_out ||
      ((uintptr_t)d_links_out & 1) || ((uintptr_t)d_scores_out & 7) ||
      !beats_args_ok(h_hops, n_songs, nullptr, tight, &total) || !(c = call_ctx(c, dflt)))
    return BL_UNEXPECTED;
  CtxGuard g(c);
  if (!g.ok()) return BL_UNEXPECTED;
  return beats_call(c, static_cast<hipStream_t>(stream), d_onsets, h_hops, n_songs, d_period, period_stride, tight,
                    d_songs_out, d_flags_out, d_links_out, d_scores_out);
}

/* ---- chroma and key (bl_chroma_kernels.hip) -------------------------------------- */

int chroma_device(bl_amd_ctx *c, bool dflt, const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs,
                  bl_amd_song_chroma *d_songs_out, bl_amd_frame_chroma *d_frames_out, long long n_frame_records,
                  void *stream) {
  if (!d_pcm || ((uintptr_t)d_pcm & 15) || !h_desc || !d_songs_out || ((uintptr_t)d_songs_out & 7) ||
      ((uintptr_t)d_frames_out & 7) || n_songs < 1)
    return BL_UNEXPECTED;
  long long total = 0; /* the sum of T over the songs */
  for (int i = 0; i < n_songs; ++i) {
    if (!chroma_song_ok(h_desc[i].pcm_offset, h_desc[i].n_samples, h_desc[i].channels)) return BL_UNEXPECTED;
    total += bl_amd_chroma_frames(h_desc[i].n_samples, h_desc[i].channels);
  }
  if ((d_frames_out && n_frame_records != total) || !blk_chroma_image_host() || !(c = call_ctx(c, dflt)))
    return BL_UNEXPECTED;
  CtxGuard g(c);
  if (!g.ok()) return BL_UNEXPECTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return record_call<bl_chroma_song>(c, s, c->chroma_songs, n_songs, [&](bl_chroma_song *hs) {
    long long frame_off = 0;
    for (int i = 0; i < n_songs; ++i) {
      hs[i].pcm_off = h_desc[i].pcm_offset;
      hs[i].frame_off = frame_off;
      hs[i].frames = bl_amd_chroma_frames(h_desc[i].n_samples, h_desc[i].channels);
      hs[i].channels = h_desc[i].channels;
      frame_off += hs[i].frames;
    }
    return BL_OK;
  }, [&](const bl_chroma_song *hs, bl_chroma_song *d_songs) {
    if (blr_ensure(c->chroma_acc, sizeof(uint64_t) * 12 * (size_t)n_songs) != BL_OK ||
        blr_ensure(c->chroma_image, blk_chroma_image_bytes()) != BL_OK)
      return BL_UNEXPECTED;
    if (!c->chroma_image_ready) { /* blocking, once per context: nothing on the device reads the block before it */
      BL_HIP_CHECK(hipMemcpy(c->chroma_image.p, blk_chroma_image_host(), blk_chroma_image_bytes(),
                             hipMemcpyHostToDevice));
      c->chroma_image_ready = true;
    }
    /* the caller's order, cut into launch groups of at most c->group_songs songs that follow each other on the stream */
    const int group_songs = std::min(c->group_songs, BL_CHROMA_GROUP_SONGS);
    for (int b = 0; b < n_songs; b += group_songs) {
      const int count = std::min(group_songs, n_songs - b);
      int max_frames = 0;
      for (int i = b; i < b + count; ++i) max_frames = std::max(max_frames, hs[i].frames);
      if (blk_chroma(s, d_pcm, d_songs + b, count, max_frames, c->n_cu, c->chroma_image.p,
                     static_cast<unsigned long long *>(c->chroma_acc.p) + 12 * (size_t)b, d_songs_out + b, d_frames_out,
                     c->prof ? mark_cb : nullptr, c) != BL_OK)
        return BL_UNEXPECTED;
    }
    return BL_OK;
  });
}

/* ---- mel bands, cepstrum and flatness (bl_mel_kernels.hip) ------------------------ */

int mel_device(bl_amd_ctx *c, bool dflt, const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs,
               uint64_t min_energy, bl_amd_song_mel *d_songs_out, bl_amd_frame_mel *d_frames_out, uint32_t *d_bands_out,
               long long n_frame_records, void *stream) {
  if (!d_pcm || ((uintptr_t)d_pcm & 15) || !h_desc || !d_songs_out || ((uintptr_t)d_songs_out & 7) ||
      ((uintptr_t)d_frames_out & 3) || ((uintptr_t)d_bands_out & 3) || n_songs < 1)
    return BL_UNEXPECTED;
  long long total = 0; /* the sum of F over the songs */
  for (int i = 0; i < n_songs; ++i) {
    if (!timbre_song_ok(h_desc[i].pcm_offset, h_desc[i].n_samples, h_desc[i].channels)) return BL_UNEXPECTED;
    total += bl_amd_timbre_frames(h_desc[i].n_samples, h_desc[i].channels);
  }
  if (((d_frames_out || d_bands_out) && n_frame_records != total) || !blk_mel_image_host() || !(c = call_ctx(c, dflt)))
    return BL_UNEXPECTED;
  CtxGuard g(c);
  if (!g.ok()) return BL_UNEXPECTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return record_call<bl_timbre_song>(c, s, c->mel_songs, n_songs, [&](bl_timbre_song *hs) {
    return frame_songs_fill(h_desc, n_songs, hs);
  }, [&](const bl_timbre_song *, bl_timbre_song *d_songs) {
    if (blr_ensure(c->mel_image, blk_mel_image_bytes()) != BL_OK) return BL_UNEXPECTED;
    if (!c->mel_image_ready) { /* blocking, once per context: nothing on the device reads the block before it */
      BL_HIP_CHECK(hipMemcpy(c->mel_image.p, blk_mel_image_host(), blk_mel_image_bytes(), hipMemcpyHostToDevice));
      c->mel_image_ready = true;
    }
    return blk_mel(s, d_pcm, d_songs, n_songs, c->tb, c->mel_image.p, min_energy, d_songs_out, d_frames_out,
                   d_bands_out);
  });
}

} // namespace

/* ========================================================================= */
/* C-ABI                                                                      */

extern "C" {

int bl_amd_ctx_levels_batch_device(bl_amd_ctx *c, const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs,
                                   int silence, bl_amd_song_levels *d_levels, void *stream) {
  return levels_device(c, false, d_pcm, h_desc, n_songs, silence, d_levels, stream);
}

int bl_amd_levels_batch_device(const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs, int silence,
                               bl_amd_song_levels *d_levels, void *stream) {
  return levels_device(nullptr, true, d_pcm, h_desc, n_songs, silence, d_levels, stream);
}

int bl_amd_ctx_timbre_batch_device(bl_amd_ctx *c, const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs,
                                   int pct, uint64_t min_energy, bl_amd_song_timbre *d_songs_out,
                                   bl_amd_frame_timbre *d_frames_out, long long n_frame_records, void *stream) {
  return timbre_device(c, false, d_pcm, h_desc, n_songs, pct, min_energy, d_songs_out, d_frames_out, n_frame_records,
                       stream);
}

int bl_amd_timbre_batch_device(const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs, int pct,
                               uint64_t min_energy, bl_amd_song_timbre *d_songs_out,
                               bl_amd_frame_timbre *d_frames_out, long long n_frame_records, void *stream) {
  return timbre_device(nullptr, true, d_pcm, h_desc, n_songs, pct, min_energy, d_songs_out, d_frames_out,
                       n_frame_records, stream);
}

int bl_amd_ctx_rhythm_batch_device(bl_amd_ctx *c, const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs,
                                   int lag_min, int lag_max, bl_amd_song_rhythm *d_songs_out, uint32_t *d_onsets_out,
                                   long long n_onsets, uint64_t *d_acf_out, void *stream) {
  return rhythm_device(c, false, d_pcm, h_desc, n_songs, lag_min, lag_max, d_songs_out, d_onsets_out, n_onsets,
                       d_acf_out, stream);
}

int bl_amd_rhythm_batch_device(const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs, int lag_min,
                               int lag_max, bl_amd_song_rhythm *d_songs_out, uint32_t *d_onsets_out,
                               long long n_onsets, uint64_t *d_acf_out, void *stream) {
  return rhythm_device(nullptr, true, d_pcm, h_desc, n_songs, lag_min, lag_max, d_songs_out, d_onsets_out, n_onsets,
                       d_acf_out, stream);
}

/* stages 7 and 8 on the caller's curves: uploaded, through the same launch as the device form, fetched */
int bl_amd_rhythm_from_onsets(const uint32_t *h_onsets, const int32_t *h_hops, int n_songs, int lag_min, int lag_max,
                              bl_amd_song_rhythm *h_songs_out, uint64_t *h_acf_out) {
  long long total = 0;
  if (!h_onsets || !h_songs_out || !rhythm_lags_ok(lag_min, lag_max) || !curves_ok(h_hops, n_songs, h_onsets, &total))
    return BL_UNEXPECTED;
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return BL_UNEXPECTED;
  CtxGuard g(c);
  if (!g.ok()) return BL_UNEXPECTED;
  DevMem curve(sizeof(uint32_t) * (size_t)total), out(sizeof(bl_amd_song_rhythm) * (size_t)n_songs),
      acf(h_acf_out ? sizeof(uint64_t) * BL_AMD_RHYTHM_LAGS * (size_t)n_songs : 0);
  if (!curve.ok() || !out.ok() || !acf.ok() || !curve.up(h_onsets)) return BL_UNEXPECTED;
  if (rhythm_call(c, nullptr, n_songs, [&](int i, bl_rhythm_song &r) {
        r.pcm_off = 0;
        r.hops = h_hops[i];
        r.channels = 1;
      }, nullptr, curve.as<uint32_t>(), lag_min, lag_max, out.as<bl_amd_song_rhythm>(), nullptr,
      acf.as<uint64_t>()) != BL_OK)
    return BL_UNEXPECTED;
  BL_HIP_CHECK(hipStreamSynchronize(nullptr));
  return out.down(h_songs_out) && (!h_acf_out || acf.down(h_acf_out)) ? BL_OK : BL_UNEXPECTED;
}

int bl_amd_ctx_beats_device(bl_amd_ctx *c, const uint32_t *d_onsets, const int32_t *h_hops, int n_songs,
                            const void *d_period, int period_stride, int tight, bl_amd_song_beats *d_songs_out,
                            uint8_t *d_flags_out, uint16_t *d_links_out, int64_t *d_scores_out, void *stream) {
  return beats_device(c, false, d_onsets, h_hops, n_songs, d_period, period_stride, tight, d_songs_out, d_flags_out,
                      d_links_out, d_scores_out, stream);
}

int bl_amd_beats_device(const uint32_t *d_onsets, const int32_t *h_hops, int n_songs, const void *d_period,
                        int period_stride, int tight, bl_amd_song_beats *d_songs_out, uint8_t *d_flags_out,
                        uint16_t *d_links_out, int64_t *d_scores_out, void *stream) {
  return beats_device(nullptr, true, d_onsets, h_hops, n_songs, d_period, period_stride, tight, d_songs_out,
                      d_flags_out, d_links_out, d_scores_out, stream);
}

/* the caller's curves and periods: uploaded, through the same launch as the device form, fetched */
int bl_amd_beats_host(const uint32_t *h_onsets, const int32_t *h_hops, int n_songs, const int32_t *h_period, int tight,
                      bl_amd_song_beats *h_songs_out, uint8_t *h_flags_out, uint16_t *h_links_out,
                      int64_t *h_scores_out) {
  long long total = 0;
  if (!h_onsets || !h_period || !h_songs_out || !h_flags_out ||
      !beats_args_ok(h_hops, n_songs, h_onsets, tight, &total))
    return BL_UNEXPECTED;
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return BL_UNEXPECTED;
  CtxGuard g(c);
  if (!g.ok()) return BL_UNEXPECTED;
  DevMem curve(sizeof(uint32_t) * (size_t)total), per(sizeof(int32_t) * (size_t)n_songs),
      out(sizeof(bl_amd_song_beats) * (size_t)n_songs), flags((size_t)total),
      links(h_links_out ? sizeof(uint16_t) * (size_t)total : 0), scores(h_scores_out ? sizeof(int64_t) * (size_t)total : 0);
  if (!curve.ok() || !per.ok() || !out.ok() || !flags.ok() || !links.ok() || !scores.ok() || !curve.up(h_onsets) ||
      !per.up(h_period))
    return BL_UNEXPECTED;
  if (beats_call(c, nullptr, curve.as<uint32_t>(), h_hops, n_songs, per.p, 4, tight, out.as<bl_amd_song_beats>(),
                 flags.as<uint8_t>(), links.as<uint16_t>(), scores.as<int64_t>()) != BL_OK)
    return BL_UNEXPECTED;
  BL_HIP_CHECK(hipStreamSynchronize(nullptr));
  return out.down(h_songs_out) && flags.down(h_flags_out) && (!h_links_out || links.down(h_links_out)) &&
                 (!h_scores_out || scores.down(h_scores_out))
             ? BL_OK
             : BL_UNEXPECTED;
}

int bl_amd_ctx_chroma_batch_device(bl_amd_ctx *c, const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs,
                                   bl_amd_song_chroma *d_songs_out, bl_amd_frame_chroma *d_frames_out,
                                   long long n_frame_records, void *stream) {
  return chroma_device(c, false, d_pcm, h_desc, n_songs, d_songs_out, d_frames_out, n_frame_records, stream);
}

int bl_amd_chroma_batch_device(const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs,
                               bl_amd_song_chroma *d_songs_out, bl_amd_frame_chroma *d_frames_out,
                               long long n_frame_records, void *stream) {
  return chroma_device(nullptr, true, d_pcm, h_desc, n_songs, d_songs_out, d_frames_out, n_frame_records, stream);
}

int bl_amd_ctx_mel_batch_device(bl_amd_ctx *c, const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs,
                                uint64_t min_energy, bl_amd_song_mel *d_songs_out, bl_amd_frame_mel *d_frames_out,
                                uint32_t *d_bands_out, long long n_frame_records, void *stream) {
  return mel_device(c, false, d_pcm, h_desc, n_songs, min_energy, d_songs_out, d_frames_out, d_bands_out,
                    n_frame_records, stream);
}

int bl_amd_mel_batch_device(const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs, uint64_t min_energy,
                            bl_amd_song_mel *d_songs_out, bl_amd_frame_mel *d_frames_out, uint32_t *d_bands_out,
                            long long n_frame_records, void *stream) {
  return mel_device(nullptr, true, d_pcm, h_desc, n_songs, min_energy, d_songs_out, d_frames_out, d_bands_out,
                    n_frame_records, stream);
}

/* The host forms of the signal levels, the spectral timbre, the tempo, the chroma and the mel call below share
 * host_form (bl_runtime.h), which checks the songs and cuts them into waves; each form's lambda runs its device form on
 * one wave and fetches what it computed (WaveOut). */

int bl_amd_levels_batch_host(const int16_t *const *h_pcm, const int32_t *n_samples, const int32_t *channels,
                             int n_songs, int silence, bl_amd_song_levels *h_levels) {
  return host_form(h_pcm, n_samples, channels, n_songs, h_levels && silence >= 0 && silence <= 32767, levels_song_ok,
                   [&](const int16_t *d_pcm, const bl_amd_song_desc *desc, int b, int e) {
    WaveOut<bl_amd_song_levels> out(h_levels, e - b);
    const bool ok = out.ok() && bl_amd_levels_batch_device(d_pcm, desc, e - b, silence, out.dev(), nullptr) == BL_OK &&
                    out.fetch();
    return ok ? BL_OK : BL_UNEXPECTED;
  });
}

int bl_amd_timbre_batch_host(const int16_t *const *h_pcm, const int32_t *n_samples, const int32_t *channels,
                             int n_songs, int pct, uint64_t min_energy, bl_amd_song_timbre *h_songs_out,
                             bl_amd_frame_timbre *h_frames_out) {
  return host_form(h_pcm, n_samples, channels, n_songs, h_songs_out && pct >= 1 && pct <= 100, timbre_song_ok,
                   [&](const int16_t *d_pcm, const bl_amd_song_desc *desc, int b, int e) {
    long long frames = 0;
    for (int i = b; i < e; ++i) frames += bl_amd_timbre_frames(n_samples[i], channels[i]);
    WaveOut<bl_amd_song_timbre> out(h_songs_out, e - b);
    WaveOut<bl_amd_frame_timbre> fout(h_frames_out, frames);
    const bool ok = out.ok() && fout.ok() &&
                    bl_amd_timbre_batch_device(d_pcm, desc, e - b, pct, min_energy, out.dev(), fout.dev(), frames,
                                               nullptr) == BL_OK &&
                    out.fetch() && fout.fetch();
    return ok ? BL_OK : BL_UNEXPECTED;
  });
}

int bl_amd_rhythm_batch_host(const int16_t *const *h_pcm, const int32_t *n_samples, const int32_t *channels,
                             int n_songs, int lag_min, int lag_max, bl_amd_song_rhythm *h_songs_out,
                             uint32_t *h_onsets_out, uint64_t *h_acf_out) {
  return host_form(h_pcm, n_samples, channels, n_songs, h_songs_out && rhythm_lags_ok(lag_min, lag_max), rhythm_song_ok,
                   [&](const int16_t *d_pcm, const bl_amd_song_desc *desc, int b, int e) {
    long long hops = 0;
    for (int i = b; i < e; ++i) hops += bl_amd_rhythm_hops(n_samples[i], channels[i]);
    /* the lag products are one row per song, so a wave's rows are found by its first song, not by a running cursor */
    uint64_t *h_rows = h_acf_out ? h_acf_out + (size_t)BL_AMD_RHYTHM_LAGS * (size_t)b : nullptr;
    WaveOut<bl_amd_song_rhythm> out(h_songs_out, e - b);
    WaveOut<uint32_t> oout(h_onsets_out, hops);
    WaveOut<uint64_t> aout(h_rows, (size_t)BL_AMD_RHYTHM_LAGS * (size_t)(e - b));
    const bool ok = out.ok() && oout.ok() && aout.ok() &&
                    bl_amd_rhythm_batch_device(d_pcm, desc, e - b, lag_min, lag_max, out.dev(), oout.dev(), hops,
                                               aout.dev(), nullptr) == BL_OK &&
                    out.fetch() && oout.fetch() && aout.fetch();
    return ok ? BL_OK : BL_UNEXPECTED;
  });
}

int bl_amd_chroma_batch_host(const int16_t *const *h_pcm, const int32_t *n_samples, const int32_t *channels,
                             int n_songs, bl_amd_song_chroma *h_songs_out, bl_amd_frame_chroma *h_frames_out) {
  return host_form(h_pcm, n_samples, channels, n_songs, h_songs_out != nullptr, chroma_song_ok,
                   [&](const int16_t *d_pcm, const bl_amd_song_desc *desc, int b, int e) {
    long long frames = 0;
    for (int i = b; i < e; ++i) frames += bl_amd_chroma_frames(n_samples[i], channels[i]);
    WaveOut<bl_amd_song_chroma> out(h_songs_out, e - b);
    WaveOut<bl_amd_frame_chroma> fout(h_frames_out, frames);
    const bool ok = out.ok() && fout.ok() &&
                    bl_amd_chroma_batch_device(d_pcm, desc, e - b, out.dev(), fout.dev(), frames, nullptr) == BL_OK &&
                    out.fetch() && fout.fetch();
    return ok ? BL_OK : BL_UNEXPECTED;
  });
}

int bl_amd_mel_batch_host(const int16_t *const *h_pcm, const int32_t *n_samples, const int32_t *channels, int n_songs,
                          uint64_t min_energy, bl_amd_song_mel *h_songs_out, bl_amd_frame_mel *h_frames_out,
                          uint32_t *h_bands_out) {
  return host_form(h_pcm, n_samples, channels, n_songs, h_songs_out != nullptr, timbre_song_ok,
                   [&](const int16_t *d_pcm, const bl_amd_song_desc *desc, int b, int e) {
    long long frames = 0;
    for (int i = b; i < e; ++i) frames += bl_amd_mel_frames(n_samples[i], channels[i]);
    WaveOut<bl_amd_song_mel> out(h_songs_out, e - b);
    WaveOut<bl_amd_frame_mel> fout(h_frames_out, frames);
    WaveOut<uint32_t> bout(h_bands_out, (size_t)BL_AMD_MEL_BANDS * (size_t)frames);
    const bool ok = out.ok() && fout.ok() && bout.ok() &&
                    bl_amd_mel_batch_device(d_pcm, desc, e - b, min_energy, out.dev(), fout.dev(), bout.dev(), frames,
                                            nullptr) == BL_OK &&
                    out.fetch() && fout.fetch() && bout.fetch();
    return ok ? BL_OK : BL_UNEXPECTED;
  });
}

} /* extern "C" */
