/*
 * bl_query_api.hip — the C-ABI of include/bliss_amd.h over force vectors: the pairwise matrix, playlists and the
 * vector queries (k nearest songs, song-to-song chains, radius lists, duplicate groups).  Host code only; contexts,
 * query_call, call_ctx, CtxGuard, DevGuard and DevMem come from bl_runtime.hip through bl_runtime.h, the kernels from
 * bl_launch.h.
 *
 * One static body per query holds its argument check, workspace choice and blk_ call; the public entry points call it
 * in one line, for the default context or a given one (`dflt`) and for the library's own rows or vectors outside it
 * (d_queries == nullptr is the self form, as in bl_launch.h).  Every argument is checked before any device work, so a
 * rejected call leaves the outputs untouched, and before the default context is fetched.  The scratch (cosine prep, a
 * column split's partial results) is the context's workspace, handed from call to call by ev_ws like the analysis
 * workspace: nothing here waits for the device.
 */
#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>

#include "bl_runtime.h"

static int matrix_device(const struct force_vector_s *d_vecs, int n, int row_begin, int n_rows,
                         float *d_out, void *stream, bool cosine) {
  if (n <= 0 || n_rows <= 0 || row_begin < 0 || row_begin + n_rows > n || !d_vecs || !d_out)
    return BL_UNEXPECTED;
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return BL_UNEXPECTED;
  CtxGuard g(c);
  if (!g.ok()) return BL_UNEXPECTED;
  return blk_pairwise(static_cast<hipStream_t>(stream), d_vecs, n, row_begin, n_rows, d_out, cosine,
                      c->prof ? mark_cb : nullptr, c);
}

static int matrix_host(const struct force_vector_s *h_vecs, int n, float *h_out, bool cosine) {
  if (n <= 0 || !h_vecs || !h_out) return BL_UNEXPECTED;
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return BL_UNEXPECTED;
  DevGuard dg(c->device);
  if (!dg.ok) return BL_UNEXPECTED;
  DevMem dv(sizeof(struct force_vector_s) * (size_t)n), dout(sizeof(float) * (size_t)n * n);
  return dv.up(h_vecs) && dout.ok() &&
                 matrix_device(dv.as<struct force_vector_s>(), n, 0, n, dout.as<float>(), nullptr, cosine) == BL_OK &&
                 dout.down(h_out)
             ? BL_OK
             : BL_UNEXPECTED;
}

/* Playlists.  seed == nullptr: the seed is row seed_index of the library; otherwise *seed, a vector that is no row of
 * it.  No context lock: a playlist uses no workspace. */
static int playlist_device(const struct force_vector_s *d_vecs, int n, int seed_index, const struct force_vector_s *seed,
                           int32_t *d_order, float *d_dist, void *stream) {
  if (n <= 0 || (!seed && (seed_index < 0 || seed_index >= n)) || !d_vecs || !d_order || !d_dist)
    return BL_UNEXPECTED;
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return BL_UNEXPECTED;
  DevGuard dg(c->device);
  if (!dg.ok) return BL_UNEXPECTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return seed ? blk_playlist_vec(s, d_vecs, n, *seed, d_order, d_dist)
              : blk_playlist(s, d_vecs, n, seed_index, d_order, d_dist);
}

static int playlist_host(const struct force_vector_s *h_vecs, int n, int seed_index, const struct force_vector_s *seed,
                         int32_t *h_order, float *h_dist) {
  if (n <= 0 || !h_vecs || !h_order) return BL_UNEXPECTED;
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return BL_UNEXPECTED;
  DevGuard dg(c->device);
  if (!dg.ok) return BL_UNEXPECTED;
  DevMem dv(sizeof(struct force_vector_s) * (size_t)n), dord(sizeof(int32_t) * (size_t)n), dd(sizeof(float) * (size_t)n);
  return dv.up(h_vecs) && dord.ok() && dd.ok() &&
                 playlist_device(dv.as<struct force_vector_s>(), n, seed_index, seed, dord.as<int32_t>(), dd.as<float>(),
                                 nullptr) == BL_OK &&
                 dord.down(h_order) && (!h_dist || dd.down(h_dist))
             ? BL_OK
             : BL_UNEXPECTED;
}

/* The queries of a kNN or radius call.  queries == nullptr: rows [row_begin, row_begin + n_rows) of the library.
 * Otherwise n_rows vectors of their own, and no candidate is excluded; the cross entry points refuse a NULL query
 * array themselves, since here it means the self form.  The host forms pass n_rows == n with it. */
static bool knn_args_ok(const void *queries, const void *vecs, int n, int row_begin, int n_rows, int k, int metric,
                        const void *index, const void *value) {
  return vecs && index && value && n > 0 && k >= 1 && k <= BL_AMD_KNN_MAX_K && metric_ok(metric) &&
         (queries ? n_rows > 0 : rows_ok(n, row_begin, n_rows));
}

static int knn_device(const struct force_vector_s *d_queries, const struct force_vector_s *d_vecs, int n, int row_begin,
                      int n_rows, int k, int metric, int32_t *d_index, float *d_value, void *stream) {
  if (!knn_args_ok(d_queries, d_vecs, n, row_begin, n_rows, k, metric, d_index, d_value)) return BL_UNEXPECTED;
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return BL_UNEXPECTED;
  const bool cosine = metric == BL_AMD_KNN_COSINE;
  return query_call(c, stream, c->knn, blk_knn_scratch_bytes(d_queries, n, n_rows, k, cosine, c->n_cu),
                    [&](hipStream_t s, void *scratch) {
                      return blk_knn(s, d_queries, d_vecs, n, row_begin, n_rows, k, cosine, c->n_cu, scratch, d_index,
                                     d_value);
                    });
}

static int knn_host(const struct force_vector_s *h_queries, int n_queries, const struct force_vector_s *h_vecs, int n,
                    int k, int metric, int32_t *h_index, float *h_value) {
  if (!knn_args_ok(h_queries, h_vecs, n, 0, n_queries, k, metric, h_index, h_index /* h_value may be NULL */))
    return BL_UNEXPECTED;
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return BL_UNEXPECTED;
  DevGuard dg(c->device);
  if (!dg.ok) return BL_UNEXPECTED;
  const size_t out = (size_t)n_queries * k;
  DevMem dq(h_queries ? sizeof(struct force_vector_s) * (size_t)n_queries : 0), dv(sizeof(struct force_vector_s) * (size_t)n);
  DevMem di(sizeof(int32_t) * out), dd(sizeof(float) * out);
  return (!h_queries || dq.up(h_queries)) && dv.up(h_vecs) && di.ok() && dd.ok() &&
                 knn_device(dq.as<struct force_vector_s>(), dv.as<struct force_vector_s>(), n, 0, n_queries, k, metric,
                            di.as<int32_t>(), dd.as<float>(), nullptr) == BL_OK &&
                 di.down(h_index) && (!h_value || dd.down(h_value))
             ? BL_OK
             : BL_UNEXPECTED;
}

static std::atomic<int> g_chain_force{BL_AMD_CHAIN_AUTO};
int blr_chain_force(void) { return g_chain_force.load(); }

static bool chain_args_ok(const void *vecs, int n, const void *seeds, int n_chains, int length, int metric,
                          const void *order, const void *value) {
  return vecs && seeds && order && value && n > 0 && n_chains > 0 && length > 0 && metric_ok(metric);
}

static int chain_device(bl_amd_ctx *c, bool dflt, const struct force_vector_s *d_vecs, int n, const int32_t *d_seeds,
                        int n_chains, int length, int metric, int32_t *d_order, float *d_value, void *stream) {
  if (!chain_args_ok(d_vecs, n, d_seeds, n_chains, length, metric, d_order, d_value) || !(c = call_ctx(c, dflt)))
    return BL_UNEXPECTED;
  const bool cosine = metric == BL_AMD_KNN_COSINE;
  const int force = g_chain_force.load();
  return query_call(c, stream, c->chain, blk_chain_scratch_bytes(n, n_chains, cosine, c->n_cu, force),
                    [&](hipStream_t s, void *scratch) {
                      return blk_chain(s, d_vecs, n, d_seeds, n_chains, length, cosine, c->n_cu, force, scratch, d_order,
                                       d_value);
                    });
}

/* Chains under rules: the chain's workspace, shape switch and call path */
static bool mix_args_ok(const void *vecs, int n, const void *seeds, const void *seed_vecs, int n_chains, int length,
                        int metric, const void *tags, int gap, const void *order, const void *value) {
  return vecs && order && value && n > 0 && n_chains > 0 && length > 0 && metric_ok(metric) &&
         (seeds != nullptr) != (seed_vecs != nullptr) && gap >= 0 && gap <= BL_AMD_MIX_MAX_GAP && (gap == 0 || tags);
}

static int mix_device(bl_amd_ctx *c, bool dflt, const struct force_vector_s *d_vecs, int n, const int32_t *d_seeds,
                      const struct force_vector_s *d_seed_vecs, int n_chains, int length, int metric,
                      const int32_t *d_tags, int gap, const uint8_t *d_exclude, int32_t *d_order, float *d_value,
                      void *stream) {
  if (!mix_args_ok(d_vecs, n, d_seeds, d_seed_vecs, n_chains, length, metric, d_tags, gap, d_order, d_value) ||
      !(c = call_ctx(c, dflt)))
    return BL_UNEXPECTED;
  const bool cosine = metric == BL_AMD_KNN_COSINE;
  const int force = g_chain_force.load();
  return query_call(c, stream, c->chain, blk_mix_scratch_bytes(n, n_chains, cosine, c->n_cu, force),
                    [&](hipStream_t s, void *scratch) {
                      return blk_mix(s, d_vecs, n, d_seeds, d_seed_vecs, n_chains, length, cosine, d_tags, gap, d_exclude,
                                     c->n_cu, force, scratch, d_order, d_value);
                    });
}

static bool radius_args_ok(const void *queries, const void *vecs, int n, int row_begin, int n_rows, int metric,
                           float radius, const void *out) {
  return vecs && out && n > 0 && metric_ok(metric) && radius == radius &&
         (queries ? n_rows > 0 : rows_ok(n, row_begin, n_rows));
}

static float radius_kernel_bound(int metric, float radius) {
  return metric == BL_AMD_KNN_COSINE ? radius : bl_amd_radius_bound(radius);
}

/* Both passes of a radius query.  fill = false: the count, which writes d_offset; d_index and d_value are not looked
 * at.  fill = true: the lists, which only reads d_offset and needs d_index. */
static int radius_device(bl_amd_ctx *c, bool dflt, bool fill, const struct force_vector_s *d_queries,
                         const struct force_vector_s *d_vecs, int n, int row_begin, int n_rows, int metric, float radius,
                         const int64_t *d_offset, int32_t *d_index, float *d_value, void *stream) {
  if (!radius_args_ok(d_queries, d_vecs, n, row_begin, n_rows, metric, radius, d_offset) || (fill && !d_index) ||
      !(c = call_ctx(c, dflt)))
    return BL_UNEXPECTED;
  const bool cosine = metric == BL_AMD_KNN_COSINE;
  const float bound = radius_kernel_bound(metric, radius);
  const long long *off = reinterpret_cast<const long long *>(d_offset);
  return query_call(c, stream, c->radius, blk_radius_scratch_bytes(d_queries, n, n_rows, cosine, c->n_cu),
                    [&](hipStream_t s, void *scratch) {
                      return fill ? blk_radius_fill(s, d_queries, d_vecs, n, row_begin, n_rows, cosine, bound, c->n_cu,
                                                    scratch, off, d_index, d_value)
                                  : blk_radius_count(s, d_queries, d_vecs, n, row_begin, n_rows, cosine, bound, c->n_cu,
                                                     scratch, const_cast<long long *>(off));
                    });
}

static int radius_host(const struct force_vector_s *h_queries, int n_queries, const struct force_vector_s *h_vecs, int n,
                       int metric, float radius, int64_t *h_offset, int32_t **h_index, float **h_value) {
  if (!radius_args_ok(h_queries, h_vecs, n, 0, n_queries, metric, radius, h_offset) || !h_index) return BL_UNEXPECTED;
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return BL_UNEXPECTED;
  DevGuard dg(c->device);
  if (!dg.ok) return BL_UNEXPECTED;
  std::vector<int64_t> off((size_t)n_queries + 1);
  DevMem dq(h_queries ? sizeof(struct force_vector_s) * (size_t)n_queries : 0), dv(sizeof(struct force_vector_s) * (size_t)n);
  DevMem doff(sizeof(int64_t) * off.size());
  if (!((!h_queries || dq.up(h_queries)) && dv.up(h_vecs) && doff.ok() &&
        radius_device(nullptr, true, false, dq.as<struct force_vector_s>(), dv.as<struct force_vector_s>(), n, 0,
                      n_queries, metric, radius, doff.as<int64_t>(), nullptr, nullptr, nullptr) == BL_OK &&
        doff.down(off.data())))
    return BL_UNEXPECTED;
  const size_t total = (size_t)off[(size_t)n_queries], slots = total ? total : 1; /* an empty result is still a free()-able block */
  int32_t *hi = static_cast<int32_t *>(malloc(sizeof(int32_t) * slots));
  float *hv = h_value ? static_cast<float *>(malloc(sizeof(float) * slots)) : nullptr;
  DevMem di(sizeof(int32_t) * slots), dd(h_value ? sizeof(float) * slots : 0);
  if (!(hi && (hv || !h_value) && di.ok() && dd.ok() &&
        radius_device(nullptr, true, true, dq.as<struct force_vector_s>(), dv.as<struct force_vector_s>(), n, 0,
                      n_queries, metric, radius, doff.as<int64_t>(), di.as<int32_t>(), dd.as<float>(), nullptr) == BL_OK &&
        di.down(hi, sizeof(int32_t) * total) && (!h_value || dd.down(hv, sizeof(float) * total)))) {
    free(hi);
    free(hv);
    return BL_UNEXPECTED;
  }
  memcpy(h_offset, off.data(), sizeof(int64_t) * off.size());
  *h_index = hi;
  if (h_value) *h_value = hv;
  return BL_OK;
}

static bool groups_args_ok(const void *vecs, int n, int metric, float radius, const void *group) {
  return vecs && group && n > 0 && metric_ok(metric) && radius == radius;
}

static int groups_device(bl_amd_ctx *c, bool dflt, const struct force_vector_s *d_vecs, int n, int metric, float radius,
                         int32_t *d_group, void *stream) {
  if (!groups_args_ok(d_vecs, n, metric, radius, d_group) || !(c = call_ctx(c, dflt))) return BL_UNEXPECTED;
  const bool cosine = metric == BL_AMD_KNN_COSINE;
  return query_call(c, stream, c->radius, blk_groups_scratch_bytes(n, cosine), [&](hipStream_t s, void *scratch) {
    return blk_groups(s, d_vecs, n, cosine, radius_kernel_bound(metric, radius), c->n_cu, scratch, d_group);
  });
}

extern "C" {

int bl_amd_distance_matrix_device(const struct force_vector_s *d_vecs, int n, int row_begin,
                                  int n_rows, float *d_out, void *stream) {
  return matrix_device(d_vecs, n, row_begin, n_rows, d_out, stream, false);
}

int bl_amd_cosine_matrix_device(const struct force_vector_s *d_vecs, int n, int row_begin,
                                int n_rows, float *d_out, void *stream) {
  return matrix_device(d_vecs, n, row_begin, n_rows, d_out, stream, true);
}

int bl_amd_distance_matrix_host(const struct force_vector_s *h_vecs, int n, float *h_out) {
  return matrix_host(h_vecs, n, h_out, false);
}
int bl_amd_cosine_matrix_host(const struct force_vector_s *h_vecs, int n, float *h_out) {
  return matrix_host(h_vecs, n, h_out, true);
}

int bl_amd_playlist_device(const struct force_vector_s *d_vecs, int n, int seed_index,
                           int32_t *d_order, float *d_dist, void *stream) {
  return playlist_device(d_vecs, n, seed_index, nullptr, d_order, d_dist, stream);
}

int bl_amd_playlist_host(const struct force_vector_s *h_vecs, int n, int seed_index,
                         int32_t *h_order, float *h_dist) {
  return playlist_host(h_vecs, n, seed_index, nullptr, h_order, h_dist);
}

int bl_amd_playlist_vec_device(const struct force_vector_s *d_vecs, int n, struct force_vector_s seed,
                               int32_t *d_order, float *d_dist, void *stream) {
  return playlist_device(d_vecs, n, 0, &seed, d_order, d_dist, stream);
}

int bl_amd_playlist_vec_host(const struct force_vector_s *h_vecs, int n, struct force_vector_s seed,
                             int32_t *h_order, float *h_dist) {
  return playlist_host(h_vecs, n, 0, &seed, h_order, h_dist);
}

int bl_amd_knn_device(const struct force_vector_s *d_vecs, int n, int row_begin, int n_rows, int k, int metric,
                      int32_t *d_index, float *d_value, void *stream) {
  return knn_device(nullptr, d_vecs, n, row_begin, n_rows, k, metric, d_index, d_value, stream);
}

int bl_amd_knn_host(const struct force_vector_s *h_vecs, int n, int k, int metric, int32_t *h_index,
                    float *h_value) {
  return knn_host(nullptr, n, h_vecs, n, k, metric, h_index, h_value);
}

int bl_amd_cross_knn_device(const struct force_vector_s *d_queries, int n_queries, const struct force_vector_s *d_vecs,
                            int n, int k, int metric, int32_t *d_index, float *d_value, void *stream) {
  return d_queries ? knn_device(d_queries, d_vecs, n, 0, n_queries, k, metric, d_index, d_value, stream) : BL_UNEXPECTED;
}

int bl_amd_cross_knn_host(const struct force_vector_s *h_queries, int n_queries, const struct force_vector_s *h_vecs,
                          int n, int k, int metric, int32_t *h_index, float *h_value) {
  return h_queries ? knn_host(h_queries, n_queries, h_vecs, n, k, metric, h_index, h_value) : BL_UNEXPECTED;
}

int bl_amd_ctx_chain_device(bl_amd_ctx *c, const struct force_vector_s *d_vecs, int n, const int32_t *d_seeds,
                            int n_chains, int length, int metric, int32_t *d_order, float *d_value, void *stream) {
  return chain_device(c, false, d_vecs, n, d_seeds, n_chains, length, metric, d_order, d_value, stream);
}

int bl_amd_chain_device(const struct force_vector_s *d_vecs, int n, const int32_t *d_seeds, int n_chains, int length,
                        int metric, int32_t *d_order, float *d_value, void *stream) {
  return chain_device(nullptr, true, d_vecs, n, d_seeds, n_chains, length, metric, d_order, d_value, stream);
}

int bl_amd_chain_host(const struct force_vector_s *h_vecs, int n, const int32_t *h_seeds, int n_chains, int length,
                      int metric, int32_t *h_order, float *h_value) {
  if (!chain_args_ok(h_vecs, n, h_seeds, n_chains, length, metric, h_order, h_order /* h_value may be NULL */))
    return BL_UNEXPECTED;
  for (int c = 0; c < n_chains; ++c)
    if (h_seeds[c] < 0 || h_seeds[c] >= n) return BL_UNEXPECTED;
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return BL_UNEXPECTED;
  DevGuard dg(c->device);
  if (!dg.ok) return BL_UNEXPECTED;
  const size_t out = (size_t)n_chains * length;
  DevMem dv(sizeof(struct force_vector_s) * (size_t)n), ds(sizeof(int32_t) * (size_t)n_chains), di(sizeof(int32_t) * out), dd(sizeof(float) * out);
  return dv.up(h_vecs) && ds.up(h_seeds) && di.ok() && dd.ok() &&
                 bl_amd_chain_device(dv.as<struct force_vector_s>(), n, ds.as<int32_t>(), n_chains, length, metric,
                                     di.as<int32_t>(), dd.as<float>(), nullptr) == BL_OK &&
                 di.down(h_order) && (!h_value || dd.down(h_value))
             ? BL_OK
             : BL_UNEXPECTED;
}

int bl_amd_ctx_mix_device(bl_amd_ctx *c, const struct force_vector_s *d_vecs, int n, const int32_t *d_seeds,
                          const struct force_vector_s *d_seed_vecs, int n_chains, int length, int metric,
                          const int32_t *d_tags, int gap, const uint8_t *d_exclude, int32_t *d_order, float *d_value,
                          void *stream) {
  return mix_device(c, false, d_vecs, n, d_seeds, d_seed_vecs, n_chains, length, metric, d_tags, gap, d_exclude, d_order,
                    d_value, stream);
}

int bl_amd_mix_device(const struct force_vector_s *d_vecs, int n, const int32_t *d_seeds,
                      const struct force_vector_s *d_seed_vecs, int n_chains, int length, int metric,
                      const int32_t *d_tags, int gap, const uint8_t *d_exclude, int32_t *d_order, float *d_value,
                      void *stream) {
  return mix_device(nullptr, true, d_vecs, n, d_seeds, d_seed_vecs, n_chains, length, metric, d_tags, gap, d_exclude,
                    d_order, d_value, stream);
}

int bl_amd_mix_host(const struct force_vector_s *h_vecs, int n, const int32_t *h_seeds,
                    const struct force_vector_s *h_seed_vecs, int n_chains, int length, int metric,
                    const int32_t *h_tags, int gap, const uint8_t *h_exclude, int32_t *h_order, float *h_value) {
  if (!mix_args_ok(h_vecs, n, h_seeds, h_seed_vecs, n_chains, length, metric, h_tags, gap, h_order,
                   h_order /* h_value may be NULL */))
    return BL_UNEXPECTED;
  for (int c = 0; h_seeds && c < n_chains; ++c)
    if (h_seeds[c] < 0 || h_seeds[c] >= n) return BL_UNEXPECTED;
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return BL_UNEXPECTED;
  DevGuard dg(c->device);
  if (!dg.ok) return BL_UNEXPECTED;
  const bool use_tags = gap > 0;
  const size_t out = (size_t)n_chains * length;
  DevMem dv(sizeof(struct force_vector_s) * (size_t)n), ds(h_seeds ? sizeof(int32_t) * (size_t)n_chains : 0);
  DevMem dq(h_seed_vecs ? sizeof(struct force_vector_s) * (size_t)n_chains : 0);
  DevMem dt(use_tags ? sizeof(int32_t) * (size_t)n : 0), dx(h_exclude ? (size_t)n : 0);
  DevMem di(sizeof(int32_t) * out), dd(sizeof(float) * out);
  return dv.up(h_vecs) && (!h_seeds || ds.up(h_seeds)) && (!h_seed_vecs || dq.up(h_seed_vecs)) &&
                 (!use_tags || dt.up(h_tags)) && (!h_exclude || dx.up(h_exclude)) && di.ok() && dd.ok() &&
                 bl_amd_mix_device(dv.as<struct force_vector_s>(), n, ds.as<int32_t>(), dq.as<struct force_vector_s>(),
                                   n_chains, length, metric, dt.as<int32_t>(), gap, dx.as<uint8_t>(), di.as<int32_t>(),
                                   dd.as<float>(), nullptr) == BL_OK &&
                 di.down(h_order) && (!h_value || dd.down(h_value))
             ? BL_OK
             : BL_UNEXPECTED;
}

/* Radius queries and duplicate groups: the distance is compared on the squared sum against
 * bl_amd_radius_bound(radius), computed here once per call. */
float bl_amd_radius_bound(float radius) {
  if (radius != radius) return radius;
  if (radius < 0.f) return -INFINITY;       /* no root is negative; -0 is not below 0 */
  if (radius == INFINITY) return INFINITY;  /* an overflowed sum has the root +inf */
  float s = radius * radius;
  if (!(s <= FLT_MAX)) s = FLT_MAX;
  while (s > 0.f && (float)sqrt((double)s) > radius) s = nextafterf(s, 0.f);
  while (s < FLT_MAX) {
    const float up = nextafterf(s, INFINITY);
    if ((float)sqrt((double)up) > radius) break;
    s = up;
  }
  return s;
}

int bl_amd_ctx_radius_count_device(bl_amd_ctx *c, const struct force_vector_s *d_vecs, int n, int row_begin, int n_rows,
                                   int metric, float radius, int64_t *d_offset, void *stream) {
  return radius_device(c, false, false, nullptr, d_vecs, n, row_begin, n_rows, metric, radius, d_offset, nullptr, nullptr,
                       stream);
}

int bl_amd_radius_count_device(const struct force_vector_s *d_vecs, int n, int row_begin, int n_rows, int metric,
                               float radius, int64_t *d_offset, void *stream) {
  return radius_device(nullptr, true, false, nullptr, d_vecs, n, row_begin, n_rows, metric, radius, d_offset, nullptr,
                       nullptr, stream);
}

int bl_amd_ctx_radius_fill_device(bl_amd_ctx *c, const struct force_vector_s *d_vecs, int n, int row_begin, int n_rows,
                                  int metric, float radius, const int64_t *d_offset, int32_t *d_index, float *d_value,
                                  void *stream) {
  return radius_device(c, false, true, nullptr, d_vecs, n, row_begin, n_rows, metric, radius, d_offset, d_index, d_value,
                       stream);
}

int bl_amd_radius_fill_device(const struct force_vector_s *d_vecs, int n, int row_begin, int n_rows, int metric,
                              float radius, const int64_t *d_offset, int32_t *d_index, float *d_value, void *stream) {
  return radius_device(nullptr, true, true, nullptr, d_vecs, n, row_begin, n_rows, metric, radius, d_offset, d_index,
                       d_value, stream);
}

int bl_amd_radius_host(const struct force_vector_s *h_vecs, int n, int metric, float radius, int64_t *h_offset,
                       int32_t **h_index, float **h_value) {
  return radius_host(nullptr, n, h_vecs, n, metric, radius, h_offset, h_index, h_value);
}

int bl_amd_ctx_cross_radius_count_device(bl_amd_ctx *c, const struct force_vector_s *d_queries, int n_queries,
                                         const struct force_vector_s *d_vecs, int n, int metric, float radius,
                                         int64_t *d_offset, void *stream) {
  return d_queries ? radius_device(c, false, false, d_queries, d_vecs, n, 0, n_queries, metric, radius, d_offset, nullptr,
                                   nullptr, stream) : BL_UNEXPECTED;
}

int bl_amd_cross_radius_count_device(const struct force_vector_s *d_queries, int n_queries,
                                     const struct force_vector_s *d_vecs, int n, int metric, float radius,
                                     int64_t *d_offset, void *stream) {
  return d_queries ? radius_device(nullptr, true, false, d_queries, d_vecs, n, 0, n_queries, metric, radius, d_offset,
                                   nullptr, nullptr, stream) : BL_UNEXPECTED;
}

int bl_amd_ctx_cross_radius_fill_device(bl_amd_ctx *c, const struct force_vector_s *d_queries, int n_queries,
                                        const struct force_vector_s *d_vecs, int n, int metric, float radius,
                                        const int64_t *d_offset, int32_t *d_index, float *d_value, void *stream) {
  return d_queries ? radius_device(c, false, true, d_queries, d_vecs, n, 0, n_queries, metric, radius, d_offset, d_index,
                                   d_value, stream) : BL_UNEXPECTED;
}

int bl_amd_cross_radius_fill_device(const struct force_vector_s *d_queries, int n_queries,
                                    const struct force_vector_s *d_vecs, int n, int metric, float radius,
                                    const int64_t *d_offset, int32_t *d_index, float *d_value, void *stream) {
  return d_queries ? radius_device(nullptr, true, true, d_queries, d_vecs, n, 0, n_queries, metric, radius, d_offset,
                                   d_index, d_value, stream) : BL_UNEXPECTED;
}

int bl_amd_cross_radius_host(const struct force_vector_s *h_queries, int n_queries, const struct force_vector_s *h_vecs,
                             int n, int metric, float radius, int64_t *h_offset, int32_t **h_index, float **h_value) {
  return h_queries ? radius_host(h_queries, n_queries, h_vecs, n, metric, radius, h_offset, h_index, h_value)
                   : BL_UNEXPECTED;
}

int bl_amd_ctx_groups_device(bl_amd_ctx *c, const struct force_vector_s *d_vecs, int n, int metric, float radius,
                             int32_t *d_group, void *stream) {
  return groups_device(c, false, d_vecs, n, metric, radius, d_group, stream);
}

int bl_amd_groups_device(const struct force_vector_s *d_vecs, int n, int metric, float radius, int32_t *d_group,
                         void *stream) {
  return groups_device(nullptr, true, d_vecs, n, metric, radius, d_group, stream);
}

int bl_amd_groups_host(const struct force_vector_s *h_vecs, int n, int metric, float radius, int32_t *h_group) {
  if (!groups_args_ok(h_vecs, n, metric, radius, h_group)) return BL_UNEXPECTED;
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return BL_UNEXPECTED;
  DevGuard dg(c->device);
  if (!dg.ok) return BL_UNEXPECTED;
  DevMem dv(sizeof(struct force_vector_s) * (size_t)n), dgrp(sizeof(int32_t) * (size_t)n);
  return dv.up(h_vecs) && dgrp.ok() &&
                 bl_amd_groups_device(dv.as<struct force_vector_s>(), n, metric, radius, dgrp.as<int32_t>(), nullptr) ==
                     BL_OK &&
                 dgrp.down(h_group)
             ? BL_OK
             : BL_UNEXPECTED;
}

int bl_amd_chain_shape(int n, int n_chains) {
  if (n < 1 || n_chains < 1) return BL_UNEXPECTED;
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return BL_UNEXPECTED;
  return blk_chain_shape(n, n_chains, c->n_cu, g_chain_force.load());
}

int bl_amd_chain_force_shape(int shape) {
  if (shape != BL_AMD_CHAIN_AUTO && shape != BL_AMD_CHAIN_PER_CHAIN && shape != BL_AMD_CHAIN_SPLIT)
    return BL_UNEXPECTED;
  return g_chain_force.exchange(shape);
}

} /* extern "C" */
