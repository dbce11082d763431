/*
 * bl_desc_chain_kernels.hip — gfx950 kernels and launch layer of the playlist chains over descriptors
 * (bl_amd_desc_chain_*, include/bliss_amd.h): bl_amd_mix_device's rules with the exact integer d^2 of two descriptors
 * in place of the f32 metric.  Must be compiled with -ffp-contract=off like every kernel file (nothing here is f32).
 *
 * Kernels (PAIR: the variant of bl_amd_desc_hmix_*, the same chains under a rule on consecutive songs):
 *   k_desc_chain<PLAYED, TAGS, PAIR>    one workgroup per group of 16 chains, persistent over all steps
 *   k_desc_chain_init<PAIR>             column-split shape, start of a call: played words, state, slot 0, padding
 *   k_desc_chain_step<TAGS, PAIR>       column-split shape, slot t of every chain: one launch per step
 *
 * Pair arithmetic: k_desc_knn's (bl_desc_pair.h, the head of bl_desc_kernels.hip) — three int8 matrix products per
 * 16 x 16 tile, norms from the int16, d^2 in 64 bits, key (d^2 << 27) | index, nearest = the smallest key.
 *
 * What a tile's rows are.  The 16 rows of a tile are 16 chains advancing in lockstep, row r the current song of chain
 * 16 g + r of group g: one chain costs what sixteen do.  The A operand is reloaded after every pick, lane (col, grp)
 * loading the 16 bytes of dimensions 8 grp .. 8 grp + 7 of lib[cur[col]]; result register r of lane (col, grp) is chain
 * 4 grp + r against candidate col, as in k_desc_knn.
 *
 * Played state.  One 16-bit word per song and group, bit r = played in chain r of the group (two songs to a 32-bit
 * word), so a lane's four bits are one read per tile.  The exclusion mask costs nothing per step: a song's word
 * starts from 0xFFFF instead of 0.  The per-chain shape keeps the words in LDS while 2 n bytes fit and in the
 * workspace beyond that; the split shape always in the workspace.
 *
 * Tags.  The tags of a chain's last `gap` slots are a ring of 16 entries, entry t & 15 the tag of slot t and -1 where
 * there is none (no tag >= 0 equals it): after slot t is filled entry (t - gap) & 15 is cleared, so the ring holds
 * exactly the slots max(0, t + 1 - gap) .. t that the rule for slot t + 1 names.  The rings live in LDS (a copy per
 * wave in the per-chain shape, the copy of the chain's state in the split shape), not in 64 VGPRs per lane, and a
 * candidate's tag is tested only once its key would become the row's best: a blocked candidate changes no `best`.
 *
 * Pair rule (PAIR).  A song's attribute is one 32-bit word (bl_amd_hmix_attr: tempo in the low half, key in byte 2).
 * What a row needs of its previous song's attribute is eight words, the pair state (dch_pair_state): the key_ok word
 * of that song's key with the bits of the unknown keys set, and up to three closed tempo intervals as (low, width)
 * pairs.  It is computed once per pick and kept in LDS beside the rings (a copy per wave in the per-chain shape, the
 * copy of the chain's state in the split shape); a candidate's attribute is one more load in the tile's batch and,
 * like its tag, is tested only once its key would become the row's best, so a blocked candidate lowers no bound.
 *
 * Dead rows.  Rows of a partial group, rows whose chain has ended and rows with a bad seed are dead: their bit in the
 * wave-uniform live mask is clear, so no candidate ever passes for them, their minimum stays the empty key, they
 * produce no pick and write no slot.  Their A operand is padded with a readable row (the chain's last song, song 0 or
 * the group's last seed descriptor), as k_desc_knn pads its queries.
 */
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bl_desc_pair.h"
#include "bl_launch.h"
#include "bl_metric.h" /* BL_KEY_EMPTY, bl_wave_sync */

#define DCH_ROWS 16       /* chains per group: the rows of a tile */
#define DCH_MAX_WAVES 16  /* waves of a k_desc_chain workgroup, at most */
#define DCH_STEP_WAVES 4  /* waves of a k_desc_chain_step workgroup */
#define DCH_BATCH 4       /* tiles whose loads a wave of k_desc_chain keeps in flight: 16 waves leave 128 VGPRs each */
#define DCH_STEP_BATCH 8  /* the same in k_desc_chain_step */
#define DCH_RING BL_AMD_MIX_MAX_GAP
static_assert(DCH_RING == 16, "the ring index is t & 15");
/* dynamic LDS of k_desc_chain, front to back: the waves' row minima (two buffers), a tag ring per wave and row, the
 * rows' lengths, then (PLAYED == DCH_PLAYED_LDS) the played words.  Every offset is a multiple of 16. */
#define DCH_LDS_WMIN (2 * DCH_MAX_WAVES * DCH_ROWS * 8)
#define DCH_LDS_HIST (DCH_MAX_WAVES * DCH_ROWS * DCH_RING * 4)
#define DCH_LDS_LEN (DCH_ROWS * 4)
#define DCH_LDS_HEAD (DCH_LDS_WMIN + DCH_LDS_HIST + DCH_LDS_LEN)
/* PAIR: a pair state per wave and row follows the lengths, and the played words come after it */
#define DCH_PAIR_WORDS 8
#define DCH_LDS_PAIR (DCH_MAX_WAVES * DCH_ROWS * DCH_PAIR_WORDS * 4)
#define DCH_LDS_MAX (160 * 1024)

enum { DCH_PLAYED_LDS, DCH_PLAYED_GLOBAL, DCH_PLAYED_LAUNCH };

/* The played words of one group.  LDS: plain reads and LDS atomics.  GLOBAL (k_desc_chain beyond what LDS holds): words
 * change inside the launch, so they are read and set at the L2 by agent-scope atomics, past the CU's L1, and a set is
 * waited for before the setting wave reads again.  LAUNCH (k_desc_chain_step): a word is set by the last arriver of a
 * launch and read by the next launch, so the reads are plain. */
template <int PLAYED>
struct dch_played {
  unsigned *w;
  __device__ __forceinline__ unsigned get(int j) const {
    const unsigned x = PLAYED == DCH_PLAYED_GLOBAL
                           ? __hip_atomic_load(w + (j >> 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                           : w[j >> 1];
    return (x >> ((j & 1) * 16)) & 0xFFFFu;
  }
  __device__ __forceinline__ void set(int j, int row) const {
    const unsigned bit = 1u << (row + (j & 1) * 16);
    if (PLAYED == DCH_PLAYED_LDS) {
      atomicOr(w + (j >> 1), bit);
    } else {
      (void)__hip_atomic_fetch_or(w + (j >> 1), bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  }
};

/* the A operand of a wave: 16 current vectors, and the norms of the lane's four rows */
struct dch_query {
  ds_v4i a64;
  long ahh, all_;
  ds_u64 na[4];
  /* aw: the 16 bytes lane (col, grp) has loaded of row col's vector */
  __device__ __forceinline__ void set(const uint4 aw, int grp) {
    int ah[2], al[2];
    ds_planes(aw, ah, al);
    a64 = ds_v4i{ah[0], ah[1], al[0], al[1]};
    ahh = ds_pack(ah);
    all_ = ds_pack(al);
    const ds_u64 an = ds_norm(aw); /* row col's, in its four lanes; lane 4 grp + r is lane (col = 4 grp + r, grp 0) */
#pragma unroll
    for (int r = 0; r < 4; ++r) na[r] = (ds_u64)__shfl(an, 4 * grp + r);
  }
};

/* does the ring of a row hold the tag?  ring: 16 ints in LDS, 16-byte aligned */
__device__ __forceinline__ bool dch_blocked(const int *ring, int tag) {
  if (tag < 0) return false; /* untagged: never blocked */
  const int4 *p = reinterpret_cast<const int4 *>(ring);
  bool m = false;
#pragma unroll
  for (int k = 0; k < DCH_RING / 4; ++k) {
    const int4 h = p[k];
    m |= (h.x == tag) | (h.y == tag) | (h.z == tag) | (h.w == tag);
  }
  return m;
}

/* The rule of a bl_amd_desc_hmix_* call reaches the kernels by value, so it is copied when the call returns */
typedef bl_amd_hmix_rule dch_rule;
#define DCH_PAIR_PASS 0xFFFFFFFFu /* an interval (0, this) holds every tempo, (this, 0) none */

/* The pair state of a row whose previous song has attribute `at`, into st[0 .. 7]: st[0] the keys that may follow (bits
 * 24 .. 31 set: an unknown key passes as key 24), st[1 + 2 i], st[2 + 2 i] the low end and the width of tempo window i.
 * on == false (no previous song: slot 0 of a descriptor seed): everything passes.  1000 |b - a| <= tol a is
 * |b - a| <= floor(tol a / 1000) for integers, and likewise for 2 b against a and b against 2 a, so the windows are
 * exact; tol a <= 1000 * 65535 and the ends stay below 2^18. */
__device__ __forceinline__ void dch_pair_state(const dch_rule &rule, unsigned at, bool on, unsigned *st) {
  const unsigned a = at & 0xFFFFu, ka = (at >> 16) & 0xFFu;
  const bool keyed = on && (rule.flags & BL_AMD_HMIX_KEY) && ka < 24u;
  const unsigned word = rule.key_ok[keyed ? ka : 0u]; /* never indexed by a value >= 24 */
  st[0] = keyed ? word | 0xFF000000u : DCH_PAIR_PASS;
  unsigned lo[3] = {0u, DCH_PAIR_PASS, DCH_PAIR_PASS}, wd[3] = {DCH_PAIR_PASS, 0u, 0u};
  if (on && (rule.flags & BL_AMD_HMIX_TEMPO) && a != 0u) {
    const unsigned w = rule.tempo_tol * a / 1000u;
    lo[0] = a - w;
    wd[0] = 2u * w;
    if (rule.flags & BL_AMD_HMIX_HALF_DOUBLE) {
      const unsigned l2 = (a - w + 1u) / 2u, h2 = (a + w) / 2u; /* a - w <= 2 b <= a + w */
      if (h2 >= l2) {
        lo[1] = l2;
        wd[1] = h2 - l2;
      }
      const unsigned w2 = 2u * rule.tempo_tol * a / 1000u;
      lo[2] = 2u * a - w2;
      wd[2] = 2u * w2;
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    st[1 + 2 * i] = lo[i];
    st[2 + 2 * i] = wd[i];
  }
  st[7] = 0u;
}

/* does the pair state of a row (8 words in LDS, 16-byte aligned) block a candidate of attribute `at`? */
__device__ __forceinline__ bool dch_pair_blocked(const unsigned *st, unsigned at) {
  const uint4 s0 = reinterpret_cast<const uint4 *>(st)[0], s1 = reinterpret_cast<const uint4 *>(st)[1];
  const unsigned b = at & 0xFFFFu, kb = min((at >> 16) & 0xFFu, 24u);
  const bool key = (s0.x >> kb) & 1u;
  const bool tempo = b == 0u || b - s0.y <= s0.z || b - s0.w <= s1.x || b - s1.y <= s1.z;
  return !(key && tempo);
}

/* Tiles tile0, tile0 + tile_step, ... below tile_end of the columns below c1 (tile i = columns 16 i .. 16 i + 15) into
 * the running minimum keys of the lane's four rows.  live4: bit r = row 4 grp + r is live.  rings: the 16 rows' rings.
 * pairs (PAIR): the 16 rows' pair states; attr: the songs' attributes. */
template <int PLAYED, bool TAGS, bool PAIR, int BATCH>
__device__ __forceinline__ void dch_scan(const uint4 *__restrict__ lib, const int32_t *__restrict__ tags,
                                         const unsigned *__restrict__ attr, const dch_query &q, int tile0,
                                         int tile_step, int tile_end, int c1, unsigned live4,
                                         const dch_played<PLAYED> played, const int *rings, const unsigned *pairs,
                                         int col, int grp, ds_u64 (&best)[4]) {
  const ds_v4i zero = {0, 0, 0, 0};
  for (int tile = tile0; tile < tile_end; tile += tile_step * BATCH) {
    /* BATCH tiles' loads in flight, then the arithmetic: one load per tile leaves the scan latency-bound.
     * Addressing: the index times 64 bytes passes 2^31 from 2^25 songs on, so it is formed in size_t. */
    uint4 bw[BATCH];
    unsigned pw[BATCH];
    int tg[BATCH];
    unsigned at[BATCH];
#pragma unroll
    for (int u = 0; u < BATCH; ++u) {
      const int jc = min((tile + u * tile_step) * DS_TILE + col, c1 - 1);
      bw[u] = lib[(size_t)jc * 4 + grp];
      pw[u] = played.get(jc);
      tg[u] = TAGS ? tags[jc] : -1;
      at[u] = PAIR ? attr[jc] : 0u;
    }
#pragma unroll
    for (int u = 0; u < BATCH; ++u) {
      if (tile + u * tile_step >= tile_end) break; /* wave-uniform */
      const int j = (tile + u * tile_step) * DS_TILE + col;
      const bool valid = j < c1;
      const unsigned mine = (pw[u] >> (4 * grp)) & 0xFu;
      const int tag = tg[u];
      int bh[2], bl[2];
      ds_planes(bw[u], bh, bl);
      const ds_v4i b64 = {bl[0], bl[1], bh[0], bh[1]};
      const ds_u64 nb = ds_norm(bw[u]);
      const ds_v4i x = __builtin_amdgcn_mfma_i32_16x16x64_i8(q.a64, b64, zero, 0, 0, 0);
      const ds_v4i hh = __builtin_amdgcn_mfma_i32_16x16x32_i8(q.ahh, ds_pack(bh), zero, 0, 0, 0);
      const ds_v4i ll = __builtin_amdgcn_mfma_i32_16x16x32_i8(q.all_, ds_pack(bl), zero, 0, 0, 0);
      const unsigned free4 = valid ? live4 & ~mine : 0u; /* rows for which column j is unplayed, unmasked and real */
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long long dot = ((long long)hh[r] << 16) + ((long long)x[r] << 8) + (long long)ll[r];
        const ds_u64 d2 = q.na[r] + nb - (ds_u64)(2 * dot);
        const ds_u64 key = (d2 << DS_IDX_BITS) | (unsigned)j;
        const bool pass = ((free4 >> r) & 1u) && key < best[r];
        if (TAGS || PAIR) {
          /* Tag test cost: only a candidate that would become the row's best reads the ring, and a blocked one leaves
           * best[r] as it was, so it can shadow no allowed candidate behind it.  The pair test is made the same way, and
           * first: it reads half of what the tag test reads and blocks most of what reaches it. */
          if (pass && !(PAIR && dch_pair_blocked(pairs + (4 * grp + r) * DCH_PAIR_WORDS, at[u])) &&
              !(TAGS && dch_blocked(rings + (4 * grp + r) * DCH_RING, tag)))
            best[r] = key;
        } else {
          best[r] = pass ? key : best[r];
        }
      }
    }
  }
  /* the rows' minima over the 16 lanes of equal grp */
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) best[r] = min(best[r], (ds_u64)__shfl_xor(best[r], off));
}

/* ------------------------------------------------------------------------- */
/* one workgroup per group of 16 chains                                         */

/* blockIdx.x: the group, chains 16 g .. 16 g + 15 (the last group may be partial).  blockDim.x = 64 nw, nw a power of
 * two up to DCH_MAX_WAVES: wave w scans the tiles i with (i & (nw - 1)) == w, so song j belongs to wave
 * (j >> 4) & (nw - 1) for the whole call.  Exactly one of seeds / seed_desc is non-null; tags is non-null exactly when
 * TAGS; exclude is null or n bytes.  g_played: words 32-bit words per group (PLAYED == DCH_PLAYED_GLOBAL).
 *
 * A step: every wave its tiles, the rows' minima over the lanes by shuffles, one LDS word per wave and row (two
 * buffers by the step's parity, like k_chain's wmin: a wave that runs ahead writes the other buffer, and cannot reach
 * this one again before everybody has left it through the next barrier), ONE workgroup barrier, then every wave reads
 * all waves' words and so knows all 16 picks.  Nothing else crosses waves:
 *   Barrier order.  A pick's played bit is set after the step's barrier and read in the next step, and there is no
 *   second barrier: the bit is set by the wave that owns the song's tile, which is the only wave that ever reads it
 *   (a wave's LDS accesses execute in order; in the workspace the set is waited for).  The tag rings are a copy per
 *   wave, written and read by that wave alone, and the current songs and the live mask are registers every wave derives
 *   from the same LDS words.
 *   Uniform exit.  The live mask is wave-uniform and the same in every wave, since all of them compute it from the
 *   same words after the same barrier; the step loop is left on it alone (and on t), so no wave waits at a barrier the
 *   others never reach.  A group runs until its last live chain ends.
 *   Pair state (PAIR).  Like the rings a copy per wave: at the top of a step every wave loads the attribute of its
 *   rows' current songs beside the A operand and writes the 16 pair states it reads in the scan.  Slot 0 of a
 *   descriptor seed has no previous song and runs with states that pass everything. */
template <int PLAYED, bool TAGS, bool PAIR>
__global__ __launch_bounds__(1024) void k_desc_chain(const uint4 *__restrict__ lib, int n,
                                                     const int32_t *__restrict__ seeds,
                                                     const uint4 *__restrict__ seed_desc, int n_chains, int length,
                                                     const int32_t *__restrict__ tags, int gap,
                                                     const unsigned char *__restrict__ exclude, unsigned *g_played,
                                                     size_t words, int32_t *__restrict__ out_order,
                                                     ds_u64 *__restrict__ out_d2, const unsigned *__restrict__ attr,
                                                     const dch_rule rule) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dch_smem[];
  ds_u64 *wmin = reinterpret_cast<ds_u64 *>(dch_smem);
  const int tid = threadIdx.x, lane = tid & 63, col = lane & 15, grp = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nw = blockDim.x >> 6;
  int *rings = reinterpret_cast<int *>(dch_smem + DCH_LDS_WMIN) + wave * (DCH_ROWS * DCH_RING);
  int *len_sh = reinterpret_cast<int *>(dch_smem + DCH_LDS_WMIN + DCH_LDS_HIST);
  unsigned *pairs = reinterpret_cast<unsigned *>(dch_smem + DCH_LDS_HEAD) + wave * (DCH_ROWS * DCH_PAIR_WORDS);
  const dch_played<PLAYED> played{PLAYED == DCH_PLAYED_LDS
                                      ? reinterpret_cast<unsigned *>(dch_smem + DCH_LDS_HEAD + (PAIR ? DCH_LDS_PAIR : 0))
                                      : g_played + (size_t)blockIdx.x * words};
  const int c_base = blockIdx.x * DCH_ROWS, rows = min(DCH_ROWS, n_chains - c_base);
  const int steps = min(length, n), tiles = (n + DS_TILE - 1) / DS_TILE;
  /* played words from the mask (word w: songs 2 w and 2 w + 1), empty rings */
  for (size_t w = tid; w < words; w += blockDim.x) {
    unsigned x = 0u;
    if (exclude) {
      const size_t j = 2 * w;
      x = exclude[j] ? 0xFFFFu : 0u;
      if (j + 1 < (size_t)n && exclude[j + 1]) x |= 0xFFFF0000u;
    }
    played.w[w] = x;
  }
#pragma unroll
  for (int i = 0; i < DCH_ROWS * DCH_RING / 64; ++i) rings[i * 64 + lane] = -1;
  if (PLAYED == DCH_PLAYED_GLOBAL) __threadfence(); /* the words are at the L2 before anybody reads them there */
  __syncthreads();
  /* the lane's row is `col`: its current song, whether it is live, how many slots it has written */
  bool live = col < rows;
  int cur = 0, mylen = 0, t = 0;
  if (!seed_desc) {
    const int s = live ? seeds[c_base + col] : -1;
    live = live && s >= 0 && s < n; /* a bad seed: a dead row, which the padding below fills with -1 */
    cur = live ? s : 0;
    if (live && grp == 0) {
      /* slot 0 is the seed whatever the mask says; its bit is set by the wave that owns its tile */
      if (((cur >> 4) & (nw - 1)) == wave) played.set(cur, col);
      if (TAGS) rings[col * DCH_RING] = tags[cur];
      if (wave == 0) {
        out_order[(size_t)(c_base + col) * length] = cur;
        out_d2[(size_t)(c_base + col) * length] = 0;
      }
    }
    mylen = live ? 1 : 0;
    t = 1;
  }
  unsigned livemask = (unsigned)__ballot(live) & 0xFFFFu; /* lanes 0 .. 15 are (col, grp 0): bit r = row r */
  for (; t < steps && livemask != 0u; ++t) {
    /* the query of a step: the rows' current songs, or (slot 0 of descriptor seeds) the seeds themselves */
    const uint4 *src = t == 0 ? seed_desc + (size_t)(c_base + min(col, rows - 1)) * 4 : lib + (size_t)cur * 4;
    uint4 aw;
    if (PAIR) { /* the attribute's load beside the A operand's, not after it */
      aw = src[grp];
      if (grp == 0) dch_pair_state(rule, t == 0 ? 0u : attr[cur], t != 0, pairs + col * DCH_PAIR_WORDS);
    }
    bl_wave_sync(); /* this wave's ring, pair and played writes since the last scan, before its reads of this one */
    if (!PAIR) aw = src[grp];
    dch_query q;
    q.set(aw, grp);
    ds_u64 best[4] = {BL_KEY_EMPTY, BL_KEY_EMPTY, BL_KEY_EMPTY, BL_KEY_EMPTY};
    dch_scan<PLAYED, TAGS, PAIR, DCH_BATCH>(lib, tags, attr, q, wave, nw, tiles, n, (livemask >> (4 * grp)) & 0xFu, played,
                                            rings, pairs, col, grp, best);
    ds_u64 *slot = wmin + (t & 1) * (DCH_MAX_WAVES * DCH_ROWS);
    if (col == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) slot[wave * DCH_ROWS + 4 * grp + r] = best[r];
    }
    __syncthreads();
    /* row col's minimum over the waves: lane (col, grp) takes waves grp, grp + 4, ... */
    ds_u64 m = BL_KEY_EMPTY;
    for (int w = grp; w < nw; w += 4) m = min(m, slot[w * DCH_ROWS + col]);
    m = min(m, (ds_u64)__shfl_xor(m, 16));
    m = min(m, (ds_u64)__shfl_xor(m, 32));
    /* no allowed song: the chain has ended (a dead row's minimum is the empty key already) */
    live = live && m != BL_KEY_EMPTY;
    if (live) {
      const int pick = (int)((unsigned)m & DS_IDX_MASK);
      if (grp == 0) {
        if (((pick >> 4) & (nw - 1)) == wave) played.set(pick, col);
        if (TAGS) {
          rings[col * DCH_RING + (t & 15)] = tags[pick];
          if (gap < DCH_RING) rings[col * DCH_RING + ((t - gap) & 15)] = -1;
        }
        if (wave == 0) {
          out_order[(size_t)(c_base + col) * length + t] = pick;
          out_d2[(size_t)(c_base + col) * length + t] = m >> DS_IDX_BITS;
        }
      }
      cur = pick;
      mylen = t + 1;
    }
    livemask = (unsigned)__ballot(live) & 0xFFFFu;
  }
  /* the slots a row never wrote: past n, past the chain's end, or all of a bad seed's row.  Nobody else wrote them. */
  if (wave == 0 && grp == 0) len_sh[col] = mylen;
  __syncthreads();
  for (int row = 0; row < rows; ++row)
    for (int u = len_sh[row] + tid; u < length; u += blockDim.x) {
      out_order[(size_t)(c_base + row) * length + u] = -1;
      out_d2[(size_t)(c_base + row) * length + u] = BL_KEY_EMPTY;
    }
}

/* ------------------------------------------------------------------------- */
/* columns split over workgroups, one launch per step                           */

/* one per group of the column-split shape: k_chain_step's arrival protocol with 16 minima.  `best`, `count` and the
 * rest on different 128-byte lines. */
struct dch_state {
  ds_u64 best[DCH_ROWS]; /* the step's minimum key per row: atomic min by every slice, taken by the last arriver */
  unsigned count;        /* slices that have arrived */
  unsigned pad0[31];
  int cur[DCH_ROWS];     /* the rows' current songs, -1 = dead; published for the next launch */
  int pad1[16];
  int ring[DCH_ROWS][DCH_RING];
  unsigned pair[DCH_ROWS][DCH_PAIR_WORDS]; /* PAIR: the rows' pair states, published with `cur` */
};
static_assert(sizeof(dch_state) % 128 == 0, "a group's state begins on a line of its own");

/* start of a call.  grid (any, n_groups): the played words of the group from the mask and the index seeds (word w of
 * group g at played[g * words + w]), every slot of the rows padded (a chain may end at any slot) except slot 0 of an
 * index seed, and the state.  A descriptor seed (seeds == nullptr) leaves slot 0 to the step launched with t = 0.
 * PAIR: the pair state of a row is its index seed's, which binds slot 1 whatever the mask says; rows without one (a
 * descriptor seed, whose slot 0 is under no pair rule, a bad seed, a row past the last chain) pass everything. */
template <bool PAIR>
__global__ __launch_bounds__(256) void k_desc_chain_init(int n, const int32_t *__restrict__ seeds, int n_chains,
                                                         int length, const int32_t *__restrict__ tags,
                                                         const unsigned char *__restrict__ exclude, size_t words,
                                                         dch_state *__restrict__ state, unsigned *__restrict__ played,
                                                         int32_t *__restrict__ out_order, ds_u64 *__restrict__ out_d2,
                                                         const unsigned *__restrict__ attr, const dch_rule rule) {
  __shared__ int sd[DCH_ROWS]; /* the rows' index seeds; -1: none, bad, or a row past the last chain */
  const int g = blockIdx.y, tid = threadIdx.x;
  const int c_base = g * DCH_ROWS, rows = min(DCH_ROWS, n_chains - c_base);
  if (tid < DCH_ROWS) {
    int s = -1;
    if (seeds && tid < rows) {
      s = seeds[c_base + tid];
      if (s < 0 || s >= n) s = -1;
    }
    sd[tid] = s;
  }
  __syncthreads();
  const size_t gid = (size_t)blockIdx.x * 256 + tid, stride = (size_t)gridDim.x * 256;
  for (size_t w = gid; w < words; w += stride) {
    unsigned x = 0u;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const size_t j = 2 * w + half;
      if (j >= (size_t)n) continue;
      unsigned bits = exclude && exclude[j] ? 0xFFFFu : 0u;
#pragma unroll
      for (int r = 0; r < DCH_ROWS; ++r) bits |= (unsigned)(sd[r] == (int)j) << r; /* the seed is played */
      x |= bits << (16 * half);
    }
    played[(size_t)g * words + w] = x;
  }
  for (size_t i = gid; i < (size_t)rows * length; i += stride) {
    const int row = (int)(i / length);
    const bool at_seed = i % length == 0 && sd[row] >= 0;
    out_order[(size_t)c_base * length + i] = at_seed ? sd[row] : -1;
    out_d2[(size_t)c_base * length + i] = at_seed ? 0ull : BL_KEY_EMPTY;
  }
  if (blockIdx.x == 0 && tid < DCH_ROWS) {
    dch_state *st = state + g;
    st->best[tid] = BL_KEY_EMPTY;
    if (tid == 0) st->count = 0u;
    st->cur[tid] = seeds ? sd[tid] : (tid < rows ? 0 : -1); /* descriptor seeds: live, the song is not read at t = 0 */
#pragma unroll
    for (int k = 0; k < DCH_RING; ++k) st->ring[tid][k] = -1;
    if (tags && sd[tid] >= 0) st->ring[tid][0] = tags[sd[tid]];
    if (PAIR) dch_pair_state(rule, sd[tid] >= 0 ? attr[sd[tid]] : 0u, sd[tid] >= 0, st->pair[tid]);
  }
}

/* slot t of every chain.  grid (slices, n_groups); workgroup x scans the columns [x * cols, (x + 1) * cols), cols a
 * multiple of 16 * DCH_STEP_WAVES, its waves taking the slice's tiles in turn.  seed_desc != nullptr (t = 0 of a call
 * with descriptor seeds): the query of chain c is seed_desc[c].  A slice's row minima go into the group's `best` by
 * agent-scope atomic mins, which are waited for before the slice adds itself to `count`; the slice whose add came last
 * takes the 16 minima (exchanges that re-arm them), sets the bits, writes the slots and publishes the current songs and
 * rings for the next launch.  No polling, nobody waits: everything else crosses a kernel boundary.  PAIR: the rows'
 * pair states are read like the rings, and the last arriver publishes the state of its row's pick; the step of a
 * descriptor seed's slot 0 reads the states k_desc_chain_init left, which pass everything. */
template <bool TAGS, bool PAIR>
__global__ __launch_bounds__(256) void k_desc_chain_step(const uint4 *__restrict__ lib, int n, int cols, int t,
                                                         int length, const uint4 *__restrict__ seed_desc, int n_chains,
                                                         const int32_t *__restrict__ tags, int gap, size_t words,
                                                         dch_state *__restrict__ state, unsigned *__restrict__ played_all,
                                                         int32_t *__restrict__ out_order, ds_u64 *__restrict__ out_d2,
                                                         const unsigned *__restrict__ attr, const dch_rule rule) {
  __shared__ __attribute__((aligned(16))) int rings[DCH_ROWS * DCH_RING];
  __shared__ __attribute__((aligned(16))) unsigned pairs[DCH_ROWS * DCH_PAIR_WORDS];
  __shared__ ds_u64 wmin[DCH_STEP_WAVES][DCH_ROWS];
  const int g = blockIdx.y, tid = threadIdx.x, lane = tid & 63, col = lane & 15, grp = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c_base = g * DCH_ROWS, rows = min(DCH_ROWS, n_chains - c_base);
  dch_state *st = state + g;
  const int cur = st->cur[col]; /* published by the previous launch */
  const bool live = cur >= 0;
  const unsigned livemask = (unsigned)__ballot(live) & 0xFFFFu;
  /* Uniform exit: every wave of every slice of the group reads the same 16 words, so a group whose rows are all dead
   * (bad seeds, ended chains) leaves as a whole and nobody arrives */
  if (livemask == 0u) return;
  if (TAGS) rings[tid] = reinterpret_cast<const int *>(st->ring)[tid];
  if (PAIR && tid < DCH_ROWS * DCH_PAIR_WORDS) pairs[tid] = reinterpret_cast<const unsigned *>(st->pair)[tid];
  if (TAGS || PAIR) __syncthreads();
  const dch_played<DCH_PLAYED_LAUNCH> played{played_all + (size_t)g * words};
  const uint4 *src = seed_desc ? seed_desc + (size_t)(c_base + min(col, rows - 1)) * 4 : lib + (size_t)max(cur, 0) * 4;
  dch_query q;
  q.set(src[grp], grp);
  const long long c0 = (long long)blockIdx.x * cols; /* slices * cols < n + cols */
  const int c1 = (int)min((long long)n, c0 + cols);
  ds_u64 best[4] = {BL_KEY_EMPTY, BL_KEY_EMPTY, BL_KEY_EMPTY, BL_KEY_EMPTY};
  dch_scan<DCH_PLAYED_LAUNCH, TAGS, PAIR, DCH_STEP_BATCH>(lib, tags, attr, q, (int)(c0 / DS_TILE) + wave, DCH_STEP_WAVES,
                                                          (c1 + DS_TILE - 1) / DS_TILE, c1,
                                                          (livemask >> (4 * grp)) & 0xFu, played, rings, pairs, col, grp,
                                                          best);
  if (col == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) wmin[wave][4 * grp + r] = best[r];
  }
  __syncthreads();
  if (wave != 0) return;
  /* wave 0, lane r < 16 = (col r, grp 0): row r.  Its `cur` and `live` above are that row's. */
  const bool row_lane = lane < DCH_ROWS;
  if (row_lane) {
    const ds_u64 m = min(min(wmin[0][lane], wmin[1][lane]), min(wmin[2][lane], wmin[3][lane]));
    /* `best` only falls during a launch, so a minimum that does not beat the value read now (at the L2, past the L1)
     * can change nothing later either: with hundreds of slices most of them skip the atomic on the group's line */
    if (m < __hip_atomic_load(&st->best[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      (void)__hip_atomic_fetch_min(&st->best[lane], m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  /* the wave's mins have been performed before the arrival is counted */
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  unsigned ticket = 0u;
  if (lane == 0) ticket = __hip_atomic_fetch_add(&st->count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  ticket = (unsigned)__shfl((int)ticket, 0);
  if (ticket != gridDim.x - 1u || !row_lane) return;
  /* every slice's mins were performed before its add, and every add before this one returned */
  const ds_u64 key = __hip_atomic_exchange(&st->best[lane], BL_KEY_EMPTY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (lane == 0) __hip_atomic_store(&st->count, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (!live) return; /* a dead row: no pick, no slot */
  if (key == BL_KEY_EMPTY) { /* no song is allowed: the chain has ended, the row keeps k_desc_chain_init's padding */
    __hip_atomic_store(&st->cur[lane], -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  const int pick = (int)((unsigned)key & DS_IDX_MASK);
  atomicOr(played.w + (pick >> 1), 1u << (lane + (pick & 1) * 16)); /* two rows may share a word */
  out_order[(size_t)(c_base + lane) * length + t] = pick;
  out_d2[(size_t)(c_base + lane) * length + t] = key >> DS_IDX_BITS;
  if (TAGS) { /* every workgroup of this launch has read the rings before it arrived */
    __hip_atomic_store(&st->ring[lane][t & 15], tags[pick], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (gap < DCH_RING)
      __hip_atomic_store(&st->ring[lane][(t - gap) & 15], -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (PAIR) { /* like the rings: every workgroup of this launch has read the states before it arrived */
    unsigned ps[DCH_PAIR_WORDS];
    dch_pair_state(rule, attr[pick], true, ps);
#pragma unroll
    for (int k = 0; k < DCH_PAIR_WORDS; ++k)
      __hip_atomic_store(&st->pair[lane][k], ps[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __hip_atomic_store(&st->cur[lane], pick, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

/* ========================================================================= */
/* launchers (declared in bl_launch.h)                                        */

int blk_desc_chain_configure_device(void) {
  for (const void *fn : {reinterpret_cast<const void *>(k_desc_chain<DCH_PLAYED_LDS, false, false>),
                         reinterpret_cast<const void *>(k_desc_chain<DCH_PLAYED_LDS, true, false>)})
    BL_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, DCH_LDS_MAX));
  return BL_OK;
}

/* Shape of a call: the rule of chain_make_plan (bl_query_kernels.hip) with groups of 16 chains in place of chains.
 * DESIGN §4.17 has the tables (tools/desc_chain_bench.py, profiles/desc_chain.json) and says which constants are
 * measured crossovers and which are not.  One group: the split shape is faster from 4 096 songs on (7.8 against 11.7 us
 * per step; at 2 048 it is 7.7 against 6.9).  Many groups: the split shape wins at every measured n while the groups
 * leave half the compute units idle (128 groups: 38 against 61 us at 16 384 songs, 133 against 240 at 65 536, 2 071
 * against 3 958 at 1 048 576) and loses by a few per cent once one workgroup per group fills the chip (256 groups: 69
 * against 61, 261 against 241, 4 157 against 3 994).  `force`: 0 = this rule, 1 / 2 = that shape. */
#define DCH_SPLIT_MIN_N 4096      /* fewer songs: one workgroup per group */
#define DCH_SPLIT_FILL 2          /* split while groups * this <= CUs */
#define DCH_SPLIT_COLS 512        /* columns of a slice, at least: one batch of tiles per wave */
#define DCH_SPLIT_MAX_SLICES 512  /* slices of a group, at most: every slice adds itself to the group's counter */
#define DCH_SPLIT_MAX_GROUPS 65535 /* gridDim.y */
#define DCH_SMALL_N 1024          /* up to here a k_desc_chain workgroup has 4 waves, beyond 16: 6.9 against 11.8 us per
                                   * step at 2 048 songs, 11.8 against 22.2 at 4 096 */

struct dch_plan {
  int shape, groups;
  size_t words; /* 32-bit played words of a group */
  /* 1 */
  int threads;
  bool lds;
  size_t lds_bytes;
  /* 2 */
  int slices, cols;
};

/* pair: the call is under a pair rule, whose states follow the head of the per-chain shape's LDS */
static dch_plan dch_make_plan(int n, int n_chains, int n_cu, int force, bool pair) {
  dch_plan p{};
  p.groups = (n_chains + DCH_ROWS - 1) / DCH_ROWS;
  p.words = ((size_t)n + 1) / 2;
  p.shape = (n >= DCH_SPLIT_MIN_N && (long long)p.groups * DCH_SPLIT_FILL <= n_cu) ? 2 : 1;
  if (force == 1 || force == 2) p.shape = force;
  if (p.groups > DCH_SPLIT_MAX_GROUPS) p.shape = 1;
  if (p.shape == 1) {
    p.threads = n <= DCH_SMALL_N ? 256 : 1024;
    const size_t head = DCH_LDS_HEAD + (pair ? DCH_LDS_PAIR : 0);
    p.lds_bytes = head + sizeof(unsigned) * p.words;
    p.lds = p.lds_bytes <= DCH_LDS_MAX;
    if (!p.lds) p.lds_bytes = head;
  } else {
    const long long want = ((long long)n + DCH_SPLIT_COLS - 1) / DCH_SPLIT_COLS;
    const long long cap = std::min((long long)DCH_SPLIT_MAX_SLICES, std::max(1LL, 4LL * n_cu / p.groups));
    const long long slices = std::max(1LL, std::min(want, cap));
    const int unit = DS_TILE * DCH_STEP_WAVES;
    p.cols = (int)((((long long)n + slices - 1) / slices + unit - 1) / unit * unit);
    p.slices = (int)(((long long)n + p.cols - 1) / p.cols);
  }
  return p;
}

int blk_desc_chain_shape(int n, int n_chains, int n_cu, int force) {
  return dch_make_plan(n, n_chains, n_cu, force, false).shape; /* the rule plays no part in the shape */
}

static size_t dch_scratch_bytes(const dch_plan &p) {
  const size_t bits = sizeof(unsigned) * p.words * p.groups;
  if (p.shape == 1) return p.lds ? 0 : bits;
  return sizeof(dch_state) * (size_t)p.groups + bits;
}

size_t blk_desc_chain_scratch_bytes(int n, int n_chains, int n_cu, int force) {
  return dch_scratch_bytes(dch_make_plan(n, n_chains, n_cu, force, false));
}

static bool dch_ruled(const bl_amd_hmix_rule &rule) { return rule.flags & (BL_AMD_HMIX_KEY | BL_AMD_HMIX_TEMPO); }

size_t blk_desc_hmix_scratch_bytes(int n, int n_chains, const bl_amd_hmix_rule &rule, int n_cu, int force) {
  return dch_scratch_bytes(dch_make_plan(n, n_chains, n_cu, force, dch_ruled(rule)));
}

#define DCH_LDS_DEFAULT (64 * 1024) /* dynamic LDS a kernel may ask for without an attribute */

template <bool TAGS, bool PAIR>
static void dch_launch(hipStream_t s, const dch_plan &p, const uint4 *lib, int n, const int32_t *d_seeds,
                       const uint4 *seed_desc, int n_chains, int length, const int32_t *d_tags, int gap,
                       const unsigned char *d_exclude, void *d_scratch, int32_t *d_order, ds_u64 *d_d2,
                       const unsigned *attr, const dch_rule &rule) {
  if (p.shape == 1) {
    unsigned *g_played = static_cast<unsigned *>(d_scratch);
    const auto kernel = p.lds ? k_desc_chain<DCH_PLAYED_LDS, TAGS, PAIR> : k_desc_chain<DCH_PLAYED_GLOBAL, TAGS, PAIR>;
    /* The PAIR kernels get their dynamic-LDS attribute here, on the current device, by the launch that needs it, and
     * not in blk_desc_chain_configure_device: what a process does that never calls bl_amd_desc_hmix_* is unchanged.
     * A host-side setting of the function, no device work; a failure shows as the launch's error. */
    if (PAIR && p.lds_bytes > DCH_LDS_DEFAULT)
      (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                DCH_LDS_MAX);
    hipLaunchKernelGGL(kernel, dim3(p.groups), dim3(p.threads), p.lds_bytes, s, lib, n, d_seeds, seed_desc, n_chains,
                       length, d_tags, gap, d_exclude, g_played, p.words, d_order, d_d2, attr, rule);
    return;
  }
  dch_state *state = static_cast<dch_state *>(d_scratch);
  unsigned *played = reinterpret_cast<unsigned *>(state + p.groups);
  const size_t fill = std::max(p.words, (size_t)DCH_ROWS * length);
  hipLaunchKernelGGL(k_desc_chain_init<PAIR>, dim3((unsigned)std::min((size_t)256, (fill + 255) / 256), p.groups),
                     dim3(256), 0, s, n, d_seeds, n_chains, length, d_tags, d_exclude, p.words, state, played, d_order,
                     d_d2, attr, rule);
  const int steps = std::min(length, n);
  for (int t = seed_desc ? 0 : 1; t < steps; ++t) /* a descriptor seed's slot 0 is a step of its own */
    hipLaunchKernelGGL((k_desc_chain_step<TAGS, PAIR>), dim3(p.slices, p.groups), dim3(64 * DCH_STEP_WAVES), 0, s, lib,
                       n, p.cols, t, length, t == 0 ? seed_desc : nullptr, n_chains, d_tags, gap, p.words, state,
                       played, d_order, d_d2, attr, rule);
}

/* A rule with neither BL_AMD_HMIX_KEY nor BL_AMD_HMIX_TEMPO is no rule: the call runs the kernels of
 * bl_amd_desc_chain_device, reads no attribute and so gives that call's bytes. */
int blk_desc_hmix(hipStream_t s, const bl_amd_desc *d_lib, const bl_amd_hmix_attr *d_attr, int n,
                  const bl_amd_hmix_rule &rule, const int32_t *d_seeds, const bl_amd_desc *d_seed_desc, int n_chains,
                  int length, const int32_t *d_tags, int gap, const uint8_t *d_exclude, int n_cu, int force,
                  void *d_scratch, int32_t *d_order, uint64_t *d_dist2) {
  if (n < 1 || (unsigned)n > DS_IDX_MASK) return BL_UNEXPECTED; /* the index bits of a key */
  const bool pair = dch_ruled(rule);
  if (pair && !d_attr) return BL_UNEXPECTED;
  const uint4 *lib = reinterpret_cast<const uint4 *>(d_lib), *q = reinterpret_cast<const uint4 *>(d_seed_desc);
  const unsigned *attr = reinterpret_cast<const unsigned *>(d_attr);
  const dch_plan p = dch_make_plan(n, n_chains, n_cu, force, pair);
  const int32_t *tags = gap > 0 ? d_tags : nullptr;
  ds_u64 *d2 = reinterpret_cast<ds_u64 *>(d_dist2);
  const auto launch = pair ? (tags ? dch_launch<true, true> : dch_launch<false, true>)
                           : (tags ? dch_launch<true, false> : dch_launch<false, false>);
  launch(s, p, lib, n, d_seeds, q, n_chains, length, tags, gap, d_exclude, d_scratch, d_order, d2, attr, rule);
  BL_HIP_CHECK(hipGetLastError());
  return BL_OK;
}

int blk_desc_chain(hipStream_t s, const bl_amd_desc *d_lib, int n, const int32_t *d_seeds,
                   const bl_amd_desc *d_seed_desc, int n_chains, int length, const int32_t *d_tags, int gap,
                   const uint8_t *d_exclude, int n_cu, int force, void *d_scratch, int32_t *d_order,
                   uint64_t *d_dist2) {
  const bl_amd_hmix_rule none{};
  return blk_desc_hmix(s, d_lib, nullptr, n, none, d_seeds, d_seed_desc, n_chains, length, d_tags, gap, d_exclude, n_cu,
                       force, d_scratch, d_order, d_dist2);
}
