"""The beat grid of include/bliss_amd.h (bl_amd_song_beats) restated in Python ints and numpy int64: the penalty from a
restatement of bl_ilog2_q12 (bliss_amd/csrc/bl_ilog2.h), the scores hop by hop exactly as the header words them, the
end and the back-trace.  Every intermediate stays below 2^54 (the header's bounds), so int64 holds it exactly.

track() is the definition: one hop after the other.  track_blocks() evaluates the same recurrence the way the kernel
does, in blocks of lo = (L + 1) >> 1 hops whose scores do not depend on each other;
tests/test_beat_reference_host.py shows the two to be equal on the corpus, and tests/test_gpu_beats.py uses the faster
one for its long curves.

The switches make, on purpose, the mistakes a kernel is likely to make (as tests/rhythm_reference.py does for the
tempo); tests/test_beat_reference_host.py shows that each of them changes a named curve of CORPUS (WITNESS says which),
so tests/test_gpu_beats.py, which runs the whole corpus, would catch a kernel that made it.

    tie_largest_d      ties of best(t) to the largest d
    link_nonneg        a link when best(t) >= 0 instead of > 0
    hi_short           hi = 2 L - 1
    lo_floor           lo = L >> 1
    shift27            the penalty shifted by 27
    linear_pen         the penalty from e instead of e^2
    tail_wide          the end searched over [H - L - 1, H - 1]
    tail_smallest_t    ties of the end to the smallest t
    own_block_zero     blocks of lo + 1 hops: the one predecessor inside the hop's own block is read as 0
    unclipped          the window not clipped at t < d: hops before the song's start are read from a ring that nobody
                       cleared (STALE stands for what lies there)
    trunc32            C kept to 32 bits
    omax_head          omax over the first 256 hops only

hi_short and tail_wide alone cannot show, and that is a property of the definition, not of the corpus: d = L is always
in [lo, hi] and costs nothing, so C[t] >= o[t] + C[t - L] >= C[t - L] wherever t - L is a hop.  Hence C[t - L] - pen(L)
>= C[t - 2 L] - pen(2 L) and the tie goes to the smaller d: d = 2 L is never chosen.  And C[H - 1] >= C[H - L - 1] with
the tie going to the larger hop: hop H - L - 1 is never the end.  Each shows together with the tie rule next to it
(PAIRED), which is how the host test pins it: a kernel with the wrong window and the right tie rule computes the
definition.
"""
import math

import numpy as np

BL_OK, BL_UNEXPECTED = 0, -2
FIELDS = ("score", "pen_scale", "hops", "period", "n_beats", "first", "last", "status")
L_MIN, L_MAX, TIGHT_MAX = 2, 510, 4096
STALE = (1 << 40) + 12345          # what `unclipped` finds in front of the song
SWITCHES = ("tie_largest_d", "link_nonneg", "hi_short", "lo_floor", "shift27", "linear_pen", "tail_wide",
            "tail_smallest_t", "own_block_zero", "unclipped", "trunc32", "omax_head")


def ilog2_q12(x):
    """bl_ilog2_q12 of bl_ilog2.h for 1 <= x < 2^64, in Python ints"""
    e = x.bit_length() - 1
    m = (x << (30 - e)) if e <= 30 else (x >> (e - 30))
    m &= 0xFFFFFFFF
    acc = e
    for _ in range(12):
        t = ((m * m) >> 30) & 0xFFFFFFFF
        bit = t >> 31
        m = t >> bit
        acc = 2 * acc + bit
    return acc & 0xFFFFFFFF


def log_error(L, d):
    return abs(ilog2_q12(d) - ilog2_q12(L))


def bounds(L, hi_short=False, lo_floor=False):
    return (L >> 1) if lo_floor else (L + 1) >> 1, 2 * L - 1 if hi_short else 2 * L


def penalties(L, W, lo, hi, shift27=False, linear_pen=False):
    """pen(d) for d = lo .. hi as an int64 array"""
    out = []
    for d in range(lo, hi + 1):
        e = log_error(L, d) if d >= 1 else 0
        out.append((W * (e if linear_pen else e * e)) >> (27 if shift27 else 28))
    return np.array(out, dtype=np.int64)


def invalid(H, L):
    rec = dict.fromkeys(FIELDS, 0)
    rec.update(hops=H, period=L, status=BL_UNEXPECTED)
    return dict(rec=rec, flags=np.zeros(H, np.uint8), links=np.zeros(H, np.uint16), scores=np.zeros(H, np.int64))


def _scale(o, tight, omax_head):
    return tight * int((o[:256] if omax_head else o).max())


def _finish(o, L, W, C, P, tail_wide=False, tail_smallest_t=False):
    """stages 4 and 5 from the scores and links"""
    H = o.size
    a = max(0, H - L - (1 if tail_wide else 0))
    tail = C[a:]
    best = int(tail.max())
    at = np.flatnonzero(tail == best)
    t_end = a + int(at[0] if tail_smallest_t else at[-1])
    flags = np.zeros(H, np.uint8)
    beats = []
    if best != 0:
        t = t_end
        while True:
            beats.append(t)
            if P[t] == 0 or P[t] > t:                # P > t: only `unclipped` links to a hop before the song
                break
            t -= int(P[t])
    flags[beats] = 1
    rec = dict(score=best, pen_scale=W, hops=H, period=L, n_beats=len(beats), first=min(beats) if beats else -1,
               last=max(beats) if beats else -1, status=BL_OK)
    return dict(rec=rec, flags=flags, links=P.astype(np.uint16), scores=C)


def track(o, L, tight, **sw):
    """dict(rec, flags, links, scores) of one song: the definition, hop by hop"""
    unknown = set(sw) - set(SWITCHES)
    assert not unknown, unknown
    o = np.asarray(o, dtype=np.int64)
    H = int(o.size)
    if L < L_MIN or L > L_MAX:
        return invalid(H, L)
    W = _scale(o, tight, sw.get("omax_head"))
    lo, hi = bounds(L, sw.get("hi_short"), sw.get("lo_floor"))
    pen = penalties(L, W, lo, hi, sw.get("shift27"), sw.get("linear_pen"))
    C, P = np.zeros(H, np.int64), np.zeros(H, np.int64)
    blk = lo + 1                                     # own_block_zero: the (wrong) block length
    for t in range(H):
        dmax = hi if sw.get("unclipped") else min(hi, t)
        best, dstar = None, 0
        if dmax >= lo:
            n = dmax - lo + 1
            d = np.arange(lo, dmax + 1)
            src = t - d
            prev = np.where(src >= 0, C[np.maximum(src, 0)], STALE)
            if sw.get("own_block_zero"):
                prev = np.where(src >= t // blk * blk, 0, prev)
            vals = prev - pen[:n]
            k = n - 1 - int(np.argmax(vals[::-1])) if sw.get("tie_largest_d") else int(np.argmax(vals))
            best, dstar = int(vals[k]), lo + k
        if best is None or (best < 0 if sw.get("link_nonneg") else best <= 0):
            C[t], P[t] = o[t], 0
        else:
            C[t], P[t] = o[t] + best, dstar
        if sw.get("trunc32"):
            C[t] &= 0xFFFFFFFF
    return _finish(o, L, W, C, P, sw.get("tail_wide"), sw.get("tail_smallest_t"))


def track_blocks(o, L, tight):
    """the same as track() without switches, evaluated in blocks of lo hops: all scores of a block at once"""
    o = np.asarray(o, dtype=np.int64)
    H = int(o.size)
    if L < L_MIN or L > L_MAX:
        return invalid(H, L)
    W = _scale(o, tight, False)
    lo, hi = bounds(L)
    pen = penalties(L, W, lo, hi)
    none = -(1 << 62)
    pad = hi                                          # Cp[pad + t] = C[t]; the hops before the song never win
    Cp = np.full(pad + H, none, np.int64)
    P = np.zeros(H, np.int64)
    d = np.arange(lo, hi + 1)
    for t0 in range(0, H, lo):
        t = np.arange(t0, min(t0 + lo, H))
        vals = Cp[pad + t[:, None] - d[None, :]] - pen[None, :]      # every source is below t0: already final
        k = np.argmax(vals, axis=1)                                  # the first maximum: the smallest d
        best = vals[np.arange(t.size), k]
        link = best > 0
        Cp[pad + t] = o[t] + np.where(link, best, 0)
        P[t] = np.where(link, lo + k, 0)
    return _finish(o, L, W, Cp[pad:].copy(), P)


def beat_hops(flags):
    return [int(h) for h in np.flatnonzero(np.asarray(flags))]


def grid_bpm(rec, rate=22050):
    """bl_amd_beats_bpm as the header words it, in Python floats (doubles)"""
    if rec["n_beats"] < 2:
        return math.nan
    return 60.0 * rate * (rec["n_beats"] - 1) / (128.0 * (rec["last"] - rec["first"]))


# ---- the material of the tests -------------------------------------------------------------------------------------

OMAX = (1 << 18) - 1
PERIODS = (2, 3, 4, 5, 7, 8, 31, 32, 33, 63, 64, 65, 127, 128, 255, 256, 509, 510)
TIGHTS = (0, 1, 16, 128, 4096)
BAD_PERIODS = (0, 1, 511, -5)
LONG_HOPS, LONG_PERIOD = 40000, 86


def lengths_for(L):
    lo = (L + 1) >> 1
    return sorted({1, 2, lo, lo + 1, 2 * L, 2 * L + 1, 2 * L + lo, 2047, 2048, 2049, 3000})


def spikes(H, at, value=100000, floor=0):
    o = np.full(H, floor, np.int64)
    o[list(at)] = value
    return o


def jitter_clicks(period, hops, seed, jitter=2):
    """clicks every `period` hops, each moved by up to `jitter` hops, over a low random floor"""
    rng = np.random.default_rng(seed)
    o = rng.integers(0, 300, hops)
    for at in range(period // 2, hops - 1, period):
        h = min(hops - 1, max(0, at + int(rng.integers(-jitter, jitter + 1))))
        o[h] = 40000 + int(rng.integers(0, 20000))
    return o.astype(np.int64)


def corpus():
    """name -> (curve as int64 array, L, tight), in a fixed order"""
    rng = np.random.default_rng(8100)
    c = {}
    c["random_L7"] = (rng.integers(0, 1 << 18, 300), 7, 16)
    c["random_L33_tight128"] = (rng.integers(0, 1 << 18, 700), 33, 128)
    c["random_L64_tight0"] = (rng.integers(0, 1 << 18, 500), 64, 0)
    c["sparse_L12"] = (rng.integers(0, 1 << 18, 400) * (rng.integers(0, 8, 400) == 0), 12, 16)
    c["zeros"] = (np.zeros(90, np.int64), 9, 16)
    c["constant_tight0"] = (np.full(120, 1000, np.int64), 8, 0)
    c["constant_tight16"] = (np.full(120, 1000, np.int64), 8, 16)
    c["spikes_2L"] = (spikes(200, range(3, 200, 20)), 10, 1)
    c["spikes_half_L7"] = (spikes(100, range(1, 100, 3)), 7, 0)
    c["spike_first_tight0"] = (spikes(100, [0]), 10, 0)
    c["spike_middle"] = (spikes(101, [50]), 10, 16)
    c["spike_last"] = (spikes(100, [99]), 10, 16)
    c["late_max"] = (np.concatenate([rng.integers(0, 500, 300), rng.integers(0, 1 << 18, 300)]), 20, 128)
    c["bounds_L510"] = (np.full(2300, OMAX, np.int64), 510, 4096)
    c["bounds_long_L2"] = (np.full(20000, OMAX, np.int64), 2, 0)      # C passes 2^32 at hop 16 384
    c["jitter_86"] = (jitter_clicks(86, 1400, 3), 86, 128)
    return {k: (np.asarray(o, dtype=np.int64), L, tight) for k, (o, L, tight) in c.items()}


# the curve of the corpus that each switch changes; the switches of PAIRED change it together with the named tie rule,
# against that tie rule alone (see the module's docstring)
PAIRED = {"hi_short": "tie_largest_d", "tail_wide": "tail_smallest_t"}
WITNESS = {
    "tie_largest_d": "constant_tight0", "link_nonneg": "zeros", "hi_short": "spike_first_tight0", "lo_floor": "spikes_half_L7",
    "shift27": "random_L33_tight128", "linear_pen": "random_L33_tight128", "tail_wide": "spike_first_tight0",
    "tail_smallest_t": "spike_first_tight0", "own_block_zero": "random_L64_tight0", "unclipped": "random_L7",
    "trunc32": "bounds_long_L2", "omax_head": "late_max",
}


def same(a, b):
    return (a["rec"] == b["rec"] and np.array_equal(a["flags"], b["flags"]) and np.array_equal(a["links"], b["links"])
            and np.array_equal(a["scores"], b["scores"]))
