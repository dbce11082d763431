/*
 * bl_desc_api.hip — the C-ABI of include/bliss_amd.h over descriptors (bl_amd_desc_*): range, quantiser, the exact
 * nearest neighbours, the playlist chains and the harmonic mixes.  Host code only, built like bl_query_api.hip: one static body per call holds the argument check,
 * the workspace choice and the blk_ call; contexts, query_call, call_ctx, DevGuard and DevMem come from bl_runtime.h, the
 * kernels from bl_launch.h.  Every argument is checked before any device work and before the default context is
 * fetched, so a rejected call leaves the outputs untouched.  The workspace is the context's `desc` block, handed from
 * call to call by ev_ws: nothing here waits for the device except the *_host forms.
 */
#include "bl_runtime.h"

#define DESC_MAX_N (1 << 27) /* n of a kNN stays below it: the index bits of a key */

static bool matrix_ok(const void *x, int n, int d) { return x && n >= 1 && d >= 1 && d <= BL_AMD_DESC_DIMS; }

/* the scale of a call; false: an entry above the maximum */
static bool scale_fill(const uint16_t *h_scale, int d, blk_desc_scale *out) {
  for (int c = 0; c < BL_AMD_DESC_DIMS; ++c) {
    out->s[c] = c < d ? (h_scale ? h_scale[c] : (uint16_t)BL_AMD_DESC_SCALE_MAX) : (uint16_t)0;
    if (out->s[c] > BL_AMD_DESC_SCALE_MAX) return false;
  }
  return true;
}

static int range_device(const float *d_x, int n, int d, bl_amd_desc_range *d_range, void *stream) {
  if (!matrix_ok(d_x, n, d) || !d_range) return BL_UNEXPECTED;
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return BL_UNEXPECTED;
  return query_call(c, stream, c->desc, blk_desc_range_scratch_bytes(n, c->n_cu), [&](hipStream_t s, void *scratch) {
    return blk_desc_range(s, d_x, n, d, c->n_cu, scratch, d_range, c->prof ? mark_cb : nullptr, c);
  });
}

static int quantize_device(const float *d_x, int n, int d, const bl_amd_desc_range *d_range, const uint16_t *h_scale,
                           bl_amd_desc *d_out, void *stream) {
  blk_desc_scale scale;
  if (!matrix_ok(d_x, n, d) || !d_range || !d_out || !scale_fill(h_scale, d, &scale))
    return BL_UNEXPECTED;
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return BL_UNEXPECTED;
  CtxGuard g(c); /* no workspace, but the profile's events belong to the context */
  if (!g.ok()) return BL_UNEXPECTED;
  return blk_desc_quantize(static_cast<hipStream_t>(stream), d_x, n, d, d_range, scale, d_out,
                           c->prof ? mark_cb : nullptr, c);
}

/* queries == nullptr: rows [row_begin, row_begin + n_rows) of the library; otherwise n_rows vectors of their own */
static bool knn_args_ok(const void *queries, const void *lib, int n, int row_begin, int n_rows, int k, const void *index,
                        const void *dist2) {
  return lib && index && dist2 && n >= 1 && n < DESC_MAX_N && k >= 1 && k <= BL_AMD_KNN_MAX_K &&
         (queries ? n_rows > 0 : rows_ok(n, row_begin, n_rows));
}

static int knn_device(bl_amd_ctx *c, bool dflt, const bl_amd_desc *d_queries, const bl_amd_desc *d_lib, int n,
                      int row_begin, int n_rows, int k, int32_t *d_index, uint64_t *d_dist2, void *stream) {
  if (!knn_args_ok(d_queries, d_lib, n, row_begin, n_rows, k, d_index, d_dist2) || !(c = call_ctx(c, dflt)))
    return BL_UNEXPECTED;
  return query_call(c, stream, c->desc, blk_desc_knn_scratch_bytes(n, n_rows, k, c->n_cu),
                    [&](hipStream_t s, void *scratch) {
                      return blk_desc_knn(s, d_queries, d_lib, n, row_begin, n_rows, k, c->n_cu, scratch, d_index,
                                          d_dist2, c->prof ? mark_cb : nullptr, c);
                    });
}

/* Chains under rules: bl_amd_mix_device's checks, the kNN's bound on n, the shape switch of bl_amd_chain_force_shape */
static bool chain_args_ok(const void *lib, int n, const void *seeds, const void *seed_desc, int n_chains, int length,
                          const void *tags, int gap, const void *order, const void *dist2) {
  return lib && order && dist2 && n >= 1 && n < DESC_MAX_N && n_chains >= 1 && length >= 1 &&
         (seeds != nullptr) != (seed_desc != nullptr) && gap >= 0 && gap <= BL_AMD_MIX_MAX_GAP && (gap == 0 || tags);
}

static int chain_device(bl_amd_ctx *c, bool dflt, const bl_amd_desc *d_lib, int n, const int32_t *d_seeds,
                        const bl_amd_desc *d_seed_desc, int n_chains, int length, const int32_t *d_tags, int gap,
                        const uint8_t *d_exclude, int32_t *d_order, uint64_t *d_dist2, void *stream) {
  if (!chain_args_ok(d_lib, n, d_seeds, d_seed_desc, n_chains, length, d_tags, gap, d_order, d_dist2) ||
      !(c = call_ctx(c, dflt)))
    return BL_UNEXPECTED;
  const int force = blr_chain_force();
  return query_call(c, stream, c->desc, blk_desc_chain_scratch_bytes(n, n_chains, c->n_cu, force),
                    [&](hipStream_t s, void *scratch) {
                      return blk_desc_chain(s, d_lib, n, d_seeds, d_seed_desc, n_chains, length, d_tags, gap, d_exclude,
                                            c->n_cu, force, scratch, d_order, d_dist2);
                    });
}

/* Harmonic mixes: the chain's checks and the rule's.  The rule is copied here, into the launch's arguments. */
static bool hmix_rule_ok(const bl_amd_hmix_rule *rule, const void *attr) {
  const uint32_t all = BL_AMD_HMIX_KEY | BL_AMD_HMIX_TEMPO | BL_AMD_HMIX_HALF_DOUBLE;
  return rule && !(rule->flags & ~all) && (!(rule->flags & BL_AMD_HMIX_HALF_DOUBLE) || (rule->flags & BL_AMD_HMIX_TEMPO)) &&
         rule->tempo_tol <= 1000u && (!(rule->flags & (BL_AMD_HMIX_KEY | BL_AMD_HMIX_TEMPO)) || attr);
}

static int hmix_device(bl_amd_ctx *c, bool dflt, const bl_amd_desc *d_lib, const bl_amd_hmix_attr *d_attr, int n,
                       const bl_amd_hmix_rule *rule, const int32_t *d_seeds, const bl_amd_desc *d_seed_desc,
                       int n_chains, int length, const int32_t *d_tags, int gap, const uint8_t *d_exclude,
                       int32_t *d_order, uint64_t *d_dist2, void *stream) {
  if (!chain_args_ok(d_lib, n, d_seeds, d_seed_desc, n_chains, length, d_tags, gap, d_order, d_dist2) ||
      !hmix_rule_ok(rule, d_attr) || !(c = call_ctx(c, dflt)))
    return BL_UNEXPECTED;
  const int force = blr_chain_force();
  const bl_amd_hmix_rule r = *rule;
  return query_call(c, stream, c->desc, blk_desc_hmix_scratch_bytes(n, n_chains, r, c->n_cu, force),
                    [&](hipStream_t s, void *scratch) {
                      return blk_desc_hmix(s, d_lib, d_attr, n, r, d_seeds, d_seed_desc, n_chains, length, d_tags, gap,
                                           d_exclude, c->n_cu, force, scratch, d_order, d_dist2);
                    });
}

extern "C" {

int bl_amd_desc_range_device(const float *d_x, int n, int d, bl_amd_desc_range *d_range, void *stream) {
  return range_device(d_x, n, d, d_range, stream);
}

int bl_amd_desc_quantize_device(const float *d_x, int n, int d, const bl_amd_desc_range *d_range,
                                const uint16_t *h_scale, bl_amd_desc *d_out, void *stream) {
  return quantize_device(d_x, n, d, d_range, h_scale, d_out, stream);
}

int bl_amd_desc_knn_device(const bl_amd_desc *d_lib, int n, int row_begin, int n_rows, int k, int32_t *d_index,
                           uint64_t *d_dist2, void *stream) {
  return knn_device(nullptr, true, nullptr, d_lib, n, row_begin, n_rows, k, d_index, d_dist2, stream);
}

int bl_amd_desc_cross_knn_device(const bl_amd_desc *d_queries, int n_queries, const bl_amd_desc *d_lib, int n, int k,
                                 int32_t *d_index, uint64_t *d_dist2, void *stream) {
  return d_queries ? knn_device(nullptr, true, d_queries, d_lib, n, 0, n_queries, k, d_index, d_dist2, stream)
                   : BL_UNEXPECTED;
}

int bl_amd_ctx_desc_knn_device(bl_amd_ctx *ctx, const bl_amd_desc *d_lib, int n, int row_begin, int n_rows, int k,
                               int32_t *d_index, uint64_t *d_dist2, void *stream) {
  return knn_device(ctx, false, nullptr, d_lib, n, row_begin, n_rows, k, d_index, d_dist2, stream);
}

int bl_amd_ctx_desc_cross_knn_device(bl_amd_ctx *ctx, const bl_amd_desc *d_queries, int n_queries,
                                     const bl_amd_desc *d_lib, int n, int k, int32_t *d_index, uint64_t *d_dist2,
                                     void *stream) {
  return d_queries ? knn_device(ctx, false, d_queries, d_lib, n, 0, n_queries, k, d_index, d_dist2, stream)
                   : BL_UNEXPECTED;
}

int bl_amd_desc_build_host(const float *h_x, int n, int d, const uint16_t *h_scale, int fit, bl_amd_desc_range *h_range,
                           bl_amd_desc *h_out) {
  blk_desc_scale scale;
  if (!matrix_ok(h_x, n, d) || !h_range || !h_out || !scale_fill(h_scale, d, &scale))
    return BL_UNEXPECTED;
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return BL_UNEXPECTED;
  DevGuard dg(c->device);
  if (!dg.ok) return BL_UNEXPECTED;
  DevMem dx(sizeof(float) * (size_t)n * d), dr(sizeof(bl_amd_desc_range)), dout(sizeof(bl_amd_desc) * (size_t)n);
  bl_amd_desc_range fitted;
  if (!(dx.up(h_x) && dout.ok() &&
        (fit ? range_device(dx.as<float>(), n, d, dr.as<bl_amd_desc_range>(), nullptr) == BL_OK && dr.down(&fitted)
             : dr.up(h_range)) &&
        quantize_device(dx.as<float>(), n, d, dr.as<bl_amd_desc_range>(), h_scale, dout.as<bl_amd_desc>(), nullptr) ==
            BL_OK &&
        dout.down(h_out)))
    return BL_UNEXPECTED;
  if (fit) *h_range = fitted;
  return BL_OK;
}

int bl_amd_desc_knn_host(const bl_amd_desc *h_queries, int n_queries, const bl_amd_desc *h_lib, int n, int k,
                         int32_t *h_index, uint64_t *h_dist2) {
  if (!h_queries) n_queries = n;
  if (!knn_args_ok(h_queries, h_lib, n, 0, n_queries, k, h_index, h_index /* h_dist2 may be NULL */))
    return BL_UNEXPECTED;
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return BL_UNEXPECTED;
  DevGuard dg(c->device);
  if (!dg.ok) return BL_UNEXPECTED;
  const size_t out = (size_t)n_queries * k;
  DevMem dq(h_queries ? sizeof(bl_amd_desc) * (size_t)n_queries : 0), dl(sizeof(bl_amd_desc) * (size_t)n);
  DevMem di(sizeof(int32_t) * out), dd(sizeof(uint64_t) * out);
  return (!h_queries || dq.up(h_queries)) && dl.up(h_lib) && di.ok() && dd.ok() &&
                 knn_device(nullptr, true, dq.as<bl_amd_desc>(), dl.as<bl_amd_desc>(), n, 0, n_queries, k,
                            di.as<int32_t>(), dd.as<uint64_t>(), nullptr) == BL_OK &&
                 di.down(h_index) && (!h_dist2 || dd.down(h_dist2))
             ? BL_OK
             : BL_UNEXPECTED;
}

int bl_amd_desc_chain_device(const bl_amd_desc *d_lib, int n, const int32_t *d_seeds, const bl_amd_desc *d_seed_desc,
                             int n_chains, int length, const int32_t *d_tags, int gap, const uint8_t *d_exclude,
                             int32_t *d_order, uint64_t *d_dist2, void *stream) {
  return chain_device(nullptr, true, d_lib, n, d_seeds, d_seed_desc, n_chains, length, d_tags, gap, d_exclude, d_order,
                      d_dist2, stream);
}

int bl_amd_ctx_desc_chain_device(bl_amd_ctx *ctx, const bl_amd_desc *d_lib, int n, const int32_t *d_seeds,
                                 const bl_amd_desc *d_seed_desc, int n_chains, int length, const int32_t *d_tags,
                                 int gap, const uint8_t *d_exclude, int32_t *d_order, uint64_t *d_dist2, void *stream) {
  return chain_device(ctx, false, d_lib, n, d_seeds, d_seed_desc, n_chains, length, d_tags, gap, d_exclude, d_order,
                      d_dist2, stream);
}

int bl_amd_desc_chain_host(const bl_amd_desc *h_lib, int n, const int32_t *h_seeds, const bl_amd_desc *h_seed_desc,
                           int n_chains, int length, const int32_t *h_tags, int gap, const uint8_t *h_exclude,
                           int32_t *h_order, uint64_t *h_dist2) {
  if (!chain_args_ok(h_lib, n, h_seeds, h_seed_desc, n_chains, length, h_tags, gap, h_order,
                     h_order /* h_dist2 may be NULL */))
    return BL_UNEXPECTED;
  for (int c = 0; h_seeds && c < n_chains; ++c)
    if (h_seeds[c] < 0 || h_seeds[c] >= n) return BL_UNEXPECTED;
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return BL_UNEXPECTED;
  DevGuard dg(c->device);
  if (!dg.ok) return BL_UNEXPECTED;
  const bool use_tags = gap > 0;
  const size_t out = (size_t)n_chains * length;
  DevMem dl(sizeof(bl_amd_desc) * (size_t)n), ds(h_seeds ? sizeof(int32_t) * (size_t)n_chains : 0);
  DevMem dq(h_seed_desc ? sizeof(bl_amd_desc) * (size_t)n_chains : 0);
  DevMem dt(use_tags ? sizeof(int32_t) * (size_t)n : 0), dx(h_exclude ? (size_t)n : 0);
  DevMem di(sizeof(int32_t) * out), dd(sizeof(uint64_t) * out);
  return dl.up(h_lib) && (!h_seeds || ds.up(h_seeds)) && (!h_seed_desc || dq.up(h_seed_desc)) &&
                 (!use_tags || dt.up(h_tags)) && (!h_exclude || dx.up(h_exclude)) && di.ok() && dd.ok() &&
                 chain_device(nullptr, true, dl.as<bl_amd_desc>(), n, ds.as<int32_t>(), dq.as<bl_amd_desc>(), n_chains,
                              length, dt.as<int32_t>(), gap, dx.as<uint8_t>(), di.as<int32_t>(), dd.as<uint64_t>(),
                              nullptr) == BL_OK &&
                 di.down(h_order) && (!h_dist2 || dd.down(h_dist2))
             ? BL_OK
             : BL_UNEXPECTED;
}

int bl_amd_desc_hmix_device(const bl_amd_desc *d_lib, const bl_amd_hmix_attr *d_attr, int n,
                            const bl_amd_hmix_rule *rule, const int32_t *d_seeds, const bl_amd_desc *d_seed_desc,
                            int n_chains, int length, const int32_t *d_tags, int gap, const uint8_t *d_exclude,
                            int32_t *d_order, uint64_t *d_dist2, void *stream) {
  return hmix_device(nullptr, true, d_lib, d_attr, n, rule, d_seeds, d_seed_desc, n_chains, length, d_tags, gap,
                     d_exclude, d_order, d_dist2, stream);
}

int bl_amd_ctx_desc_hmix_device(bl_amd_ctx *ctx, const bl_amd_desc *d_lib, const bl_amd_hmix_attr *d_attr, int n,
                                const bl_amd_hmix_rule *rule, const int32_t *d_seeds, const bl_amd_desc *d_seed_desc,
                                int n_chains, int length, const int32_t *d_tags, int gap, const uint8_t *d_exclude,
                                int32_t *d_order, uint64_t *d_dist2, void *stream) {
  return hmix_device(ctx, false, d_lib, d_attr, n, rule, d_seeds, d_seed_desc, n_chains, length, d_tags, gap, d_exclude,
                     d_order, d_dist2, stream);
}

int bl_amd_desc_hmix_host(const bl_amd_desc *h_lib, const bl_amd_hmix_attr *h_attr, int n, const bl_amd_hmix_rule *rule,
                          const int32_t *h_seeds, const bl_amd_desc *h_seed_desc, int n_chains, int length,
                          const int32_t *h_tags, int gap, const uint8_t *h_exclude, int32_t *h_order,
                          uint64_t *h_dist2) {
  if (!chain_args_ok(h_lib, n, h_seeds, h_seed_desc, n_chains, length, h_tags, gap, h_order,
                     h_order /* h_dist2 may be NULL */) ||
      !hmix_rule_ok(rule, h_attr))
    return BL_UNEXPECTED;
  for (int c = 0; h_seeds && c < n_chains; ++c)
    if (h_seeds[c] < 0 || h_seeds[c] >= n) return BL_UNEXPECTED;
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return BL_UNEXPECTED;
  DevGuard dg(c->device);
  if (!dg.ok) return BL_UNEXPECTED;
  const bool use_tags = gap > 0, use_attr = rule->flags & (BL_AMD_HMIX_KEY | BL_AMD_HMIX_TEMPO);
  const size_t out = (size_t)n_chains * length;
  DevMem dl(sizeof(bl_amd_desc) * (size_t)n), ds(h_seeds ? sizeof(int32_t) * (size_t)n_chains : 0);
  DevMem dq(h_seed_desc ? sizeof(bl_amd_desc) * (size_t)n_chains : 0);
  DevMem da(use_attr ? sizeof(bl_amd_hmix_attr) * (size_t)n : 0);
  DevMem dt(use_tags ? sizeof(int32_t) * (size_t)n : 0), dx(h_exclude ? (size_t)n : 0);
  DevMem di(sizeof(int32_t) * out), dd(sizeof(uint64_t) * out);
  return dl.up(h_lib) && (!h_seeds || ds.up(h_seeds)) && (!h_seed_desc || dq.up(h_seed_desc)) &&
                 (!use_attr || da.up(h_attr)) && (!use_tags || dt.up(h_tags)) && (!h_exclude || dx.up(h_exclude)) &&
                 di.ok() && dd.ok() &&
                 hmix_device(nullptr, true, dl.as<bl_amd_desc>(), da.as<bl_amd_hmix_attr>(), n, rule, ds.as<int32_t>(),
                             dq.as<bl_amd_desc>(), n_chains, length, dt.as<int32_t>(), gap, dx.as<uint8_t>(),
                             di.as<int32_t>(), dd.as<uint64_t>(), nullptr) == BL_OK &&
                 di.down(h_order) && (!h_dist2 || dd.down(h_dist2))
             ? BL_OK
             : BL_UNEXPECTED;
}

int bl_amd_desc_chain_shape(int n, int n_chains) {
  if (n < 1 || n >= DESC_MAX_N || n_chains < 1) return BL_UNEXPECTED;
  bl_amd_ctx *c = blr_default_ctx();
  if (!c) return BL_UNEXPECTED;
  return blk_desc_chain_shape(n, n_chains, c->n_cu, blr_chain_force());
}

size_t bl_amd_desc_knn_scratch_bytes(int n, int n_rows, int k) {
  if (n < 1 || n >= DESC_MAX_N || n_rows < 1 || k < 1 || k > BL_AMD_KNN_MAX_K) return 0;
  bl_amd_ctx *c = blr_default_ctx();
  return c ? blk_desc_knn_scratch_bytes(n, n_rows, k, c->n_cu) : 0;
}

} /* extern "C" */
