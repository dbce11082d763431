/*
 * bl_loud_api.hip — call path and C-ABI of the K-weighted gated loudness (include/bliss_amd.h: bl_amd_loud_*); the
 * kernels are bl_loud_kernels.hip's, the host arithmetic bl_api.c's.  Host code only.
 *
 * The loudness keeps a side workspace (bl_side_ws.h, which has the protocol): the records, and as extra blocks the hop
 * energies of a call without a hops output and the short-term sums.
 */
#include <string.h>

#include <algorithm>

#include "bl_loud.h"
#include "bl_side_ws.h"

namespace {

enum { X_Z, X_ST }; /* bl_side_ws::extra */

/* One call on n_songs songs, from PCM (d_z_in == nullptr) or from hop energies on the device; the caller holds the
 * context (CtxGuard).  `song(i, rec)` writes pcm_off, hops and channels of song i in the caller's order.  The records
 * are sorted stereo first: a wave of k_loud_filter whose lanes all have one channel count runs one shape.  Z goes to
 * d_hops_out where there is one and to the workspace otherwise; both kernels see the same pointer, so the records
 * cannot depend on which it is. */
template <class Song>
int loud_call(bl_amd_ctx *c, hipStream_t s, int n_songs, Song song, const int16_t *d_pcm, const uint64_t *d_z_in,
              const bl_amd_loud_params &p, bl_amd_song_loud *d_songs_out, uint64_t *d_hops_out) {
  long long hops = 0, starts = 0, chunks = 0;
  return side_call(SIDE_LOUD, c, s, sizeof(bl_loud_song) * (size_t)n_songs, [&](void *pinned) {
    bl_loud_song *hs = static_cast<bl_loud_song *>(pinned);
    for (int i = 0; i < n_songs; ++i) {
      song(i, hs[i]);
      hs[i].hop_off = hops;
      hs[i].st_off = starts;
      hs[i].out_idx = i;
      hs[i].reserved = 0;
      hops += hs[i].hops;
      starts += blk_loud_starts(hs[i].hops);
    }
    std::stable_sort(hs, hs + n_songs, [](const bl_loud_song &a, const bl_loud_song &b) { return a.channels > b.channels; });
    for (int i = 0; i < n_songs; ++i) {
      hs[i].chunk_off = chunks;
      chunks += (hs[i].hops + BL_AMD_LOUD_CHUNK - 1) / BL_AMD_LOUD_CHUNK;
    }
    return chunks > (1ll << 30) ? BL_UNEXPECTED : BL_OK;
  }, [&](hipStream_t s, bl_side_ws &w, blk_mark_fn mark, void *user) {
    unsigned long long *z = reinterpret_cast<unsigned long long *>(d_z_in ? const_cast<uint64_t *>(d_z_in) : d_hops_out);
    if (blr_ensure(w.extra[X_ST], 8 * (size_t)std::max(starts, 1ll)) != BL_OK ||
        (!z && blr_ensure(w.extra[X_Z], 16 * (size_t)std::max(hops, 1ll)) != BL_OK))
      return BL_UNEXPECTED;
    if (!z) z = static_cast<unsigned long long *>(w.extra[X_Z].p);
    const bl_loud_song *d_songs = static_cast<const bl_loud_song *>(w.recs.p);
    if (!d_z_in && blk_loud_filter(s, d_pcm, d_songs, n_songs, chunks, p, z, mark, user) != BL_OK) return BL_UNEXPECTED;
    return blk_loud_gate(s, z, d_songs, n_songs, p.abs_gate, static_cast<unsigned long long *>(w.extra[X_ST].p),
                         d_songs_out, mark, user);
  });
}

int loud_device(bl_amd_ctx *c, bool dflt, const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs,
                const bl_amd_loud_params *params, bl_amd_song_loud *d_songs_out, uint64_t *d_hops_out, long long n_hops,
                void *stream) {
  if (!d_pcm || ((uintptr_t)d_pcm & 15) || !h_desc || !d_songs_out || ((uintptr_t)d_songs_out & 7) ||
      ((uintptr_t)d_hops_out & 7) || n_songs < 1 || !loud_params_ok(params, false))
    return BL_UNEXPECTED;
  const bl_amd_loud_params p = *params;
  long long total = 0; /* the sum of H over the songs */
  for (int i = 0; i < n_songs; ++i) {
    if (!loud_song_ok(h_desc[i].pcm_offset, h_desc[i].n_samples, h_desc[i].channels)) return BL_UNEXPECTED;
    total += loud_hops(h_desc[i].n_samples, h_desc[i].channels, p.hop);
  }
  if ((d_hops_out && n_hops != total) || !(c = call_ctx(c, dflt))) return BL_UNEXPECTED;
  CtxGuard g(c);
  if (!g.ok()) return BL_UNEXPECTED;
  return loud_call(c, static_cast<hipStream_t>(stream), n_songs, [&](int i, bl_loud_song &r) {
    r.pcm_off = h_desc[i].pcm_offset;
    r.hops = loud_hops(h_desc[i].n_samples, h_desc[i].channels, p.hop);
    r.channels = h_desc[i].channels;
  }, d_pcm, nullptr, p, d_songs_out, d_hops_out);
}

} // namespace

/* ========================================================================= */
/* C-ABI                                                                      */

extern "C" {

int bl_amd_ctx_loud_batch_device(bl_amd_ctx *c, const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs,
                                 const bl_amd_loud_params *params, bl_amd_song_loud *d_songs_out, uint64_t *d_hops_out,
                                 long long n_hops, void *stream) {
  return loud_device(c, false, d_pcm, h_desc, n_songs, params, d_songs_out, d_hops_out, n_hops, stream);
}

int bl_amd_loud_batch_device(const int16_t *d_pcm, const bl_amd_song_desc *h_desc, int n_songs,
                             const bl_amd_loud_params *params, bl_amd_song_loud *d_songs_out, uint64_t *d_hops_out,
                             long long n_hops, void *stream) {
  return loud_device(nullptr, true, d_pcm, h_desc, n_songs, params, d_songs_out, d_hops_out, n_hops, stream);
}

/* stages 4 to 6 on the caller's hop energies: uploaded, through the same gate launch as the device form, fetched */
int bl_amd_loud_from_hops(const uint64_t *h_hop_energy, const int32_t *h_hops, int n_songs,
                          const bl_amd_loud_params *params, bl_amd_song_loud *h_songs_out) {
  if (!h_hops || !h_songs_out || n_songs < 1 || !loud_params_ok(params, true)) return BL_UNEXPECTED;
  long long total = 0;
  for (int i = 0; i < n_songs; ++i) {
    if (h_hops[i] < 0 || h_hops[i] > (1 << 27)) return BL_UNEXPECTED;
    total += h_hops[i];
  }
  if (total && !h_hop_energy) return BL_UNEXPECTED;
  for (long long k = 0; k < 2 * total; ++k)
    if (h_hop_energy[k] >= (1ull << 46)) return BL_UNEXPECTED;
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return BL_UNEXPECTED;
  CtxGuard g(c);
  if (!g.ok()) return BL_UNEXPECTED;
  DevMem zin(16 * (size_t)std::max(total, 1ll)), out(sizeof(bl_amd_song_loud) * (size_t)n_songs);
  if (!zin.ok() || !out.ok()) return BL_UNEXPECTED;
  if (total) BL_HIP_CHECK(hipMemcpy(zin.p, h_hop_energy, 16 * (size_t)total, hipMemcpyHostToDevice));
  if (loud_call(c, nullptr, n_songs, [&](int i, bl_loud_song &r) {
        r.pcm_off = 0;
        r.hops = h_hops[i];
        r.channels = 2;
      }, nullptr, zin.as<uint64_t>(), *params, out.as<bl_amd_song_loud>(), nullptr) != BL_OK)
    return BL_UNEXPECTED;
  BL_HIP_CHECK(hipStreamSynchronize(nullptr));
  return out.down(h_songs_out) ? BL_OK : BL_UNEXPECTED;
}

/* the songs in waves (host_form, bl_runtime.h): each is measured by the device form and fetched */
int bl_amd_loud_batch_host(const int16_t *const *h_pcm, const int32_t *n_samples, const int32_t *channels, int n_songs,
                           const bl_amd_loud_params *params, bl_amd_song_loud *h_songs_out, uint64_t *h_hops_out) {
  return host_form(h_pcm, n_samples, channels, n_songs, h_songs_out && loud_params_ok(params, false), loud_song_ok,
                   [&](const int16_t *d_pcm, const bl_amd_song_desc *desc, int b, int e) {
                     long long hops = 0;
                     for (int i = b; i < e; ++i) hops += loud_hops(n_samples[i], channels[i], params->hop);
                     WaveOut<bl_amd_song_loud> out(h_songs_out, e - b);
                     WaveOut<uint64_t> zout(h_hops_out, 2 * hops);
                     if (!out.ok() || !zout.ok() ||
                         bl_amd_loud_batch_device(d_pcm, desc, e - b, params, out.dev(), zout.dev(), hops, nullptr) != BL_OK)
                       return BL_UNEXPECTED;
                     BL_HIP_CHECK(hipStreamSynchronize(nullptr));
                     return out.fetch() && (!hops || zout.fetch()) ? BL_OK : BL_UNEXPECTED;
                   });
}

/* device time of a loudness kernel since this was last asked for it: "loud_filter" or "loud_gate" */
double bl_amd_loud_profile_ms(const char *name, int *launches) {
  if (launches) *launches = 0;
  const int k = !name ? -1 : !strcmp(name, "loud_filter") ? LK_FILTER : !strcmp(name, "loud_gate") ? LK_GATE : -1;
  if (k < 0) return -1.0;
  return side_profile_ms(SIDE_LOUD, k, launches);
}

} /* extern "C" */
