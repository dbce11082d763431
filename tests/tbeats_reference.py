"""The beat grid that follows the tempo over time (include/bliss_amd.h: bl_amd_song_tbeats) restated in numpy int64 and
Python ints, on top of tests/beat_reference.py: its ilog2_q12, penalties and _finish.  Every intermediate stays below
2^54 (the header's bounds), so int64 holds it exactly.

track() is the definition: one hop after the other, every hop with the period of its own frame.  track_runs() evaluates
the same recurrence the way the kernel does: run by run, the penalty table rebuilt at a run's start, inside a run in
blocks of lo hops whose scores do not depend on each other.  tests/test_tbeats_reference_host.py shows the two to be
equal on the corpus; tests/test_gpu_tbeats.py uses the faster one.

The switches make, on purpose, the mistakes a kernel is likely to make; tests/test_tbeats_reference_host.py shows that
each of them changes a named input (named()), which tests/test_gpu_tbeats.py runs, so the GPU test would catch a kernel
that made it.  song() takes any of them.

  in track_runs()
    stale_pen          the penalty table not rebuilt at a run change
    stale_bounds       lo and hi of the previous run in a run's first block (sources inside the block read as 0)
  in track()
    cross_block        blocks of the lo of the run they start in, not cut at the run's end: in a run with a smaller lo
                       the sources inside the hop's own block read as 0
    pen_at_source      the penalty's L taken at the source hop
  in both
    no_origin          origin ignored
    g_rounded          g rounded to the nearest frame instead of floored
    wrap_frames        hops past the last frame wrap to frame 0 instead of clamping
    end_l0             the end window from L(0)
    run_max            W from the run's own maximum
    tie_later          fill ties to the later frame
    forward_only       the fill from the frames before only (the leading invalid frames from the first valid one)
    tile_loss          the fill loses the nearest frame across a tile edge: a candidate in the frame's own tile of
                       TILE frames hides the one in another tile
    fold_round_up      the fold halves by (q + 1) >> 1
    fold_first         the fold applied to the raw lags, before the validity test
    period_at_ends     period_first and period_last taken at hops 0 and H - 1
"""
import functools

import numpy as np

from tests import beat_reference as br

BL_OK, BL_UNEXPECTED = br.BL_OK, br.BL_UNEXPECTED
FIELDS = ("score", "pen_scale", "hops", "frames", "n_beats", "first", "last", "status", "period_first", "period_last",
          "n_runs", "n_filled", "n_folded", "reserved")
SONG_DTYPE = np.dtype([("score", "<i8"), ("pen_scale", "<u8")] + [(k, "<i4") for k in FIELDS[2:]])
assert SONG_DTYPE.itemsize == 64
L_MIN, L_MAX = br.L_MIN, br.L_MAX
TILE = 256                                          # bl_amd_tbeats_shape's track_tile
RUN_SWITCHES = ("stale_pen", "stale_bounds")
HOP_SWITCHES = ("cross_block", "pen_at_source")
SWITCHES = RUN_SWITCHES + HOP_SWITCHES + ("no_origin", "g_rounded", "wrap_frames", "end_l0", "run_max", "tie_later",
                                          "forward_only", "tile_loss", "fold_round_up", "fold_first", "period_at_ends")


def params(seg=128, origin=0, tight=128, fold=0):
    return dict(seg=seg, origin=origin, tight=tight, fold=fold)


def params_ok(p):
    return 16 <= p["seg"] <= 16384 and 0 <= p["origin"] < 1 << 24 and 0 <= p["tight"] <= 4096 and p["fold"] in (0, 1)


def from_tgram(tp, tight=128, fold=0):
    """bl_amd_tbeats_params_from_tgram on a tests.tgram_reference.params()"""
    return params(tp["stride"], (tp["blocks"] - 1) * tp["stride"] // 2, tight, fold)


def valid(lag):
    return L_MIN <= lag <= L_MAX


def fold_one(q, A, round_up=False, unchecked=False):
    """stage 3 on one lag; unchecked: on a raw lag, which may be anything"""
    q2 = q
    if 3 * q <= 2 * A:
        q2 = 2 * q
    elif 3 * q > 4 * A:
        q2 = (q + 1) >> 1 if round_up else q >> 1
    return q2 if valid(q2) and (unchecked or q2 != q) else q


def period_track(lags, anchor, p, **sw):
    """stages 1 to 3: (q as an int64 array, n_filled, n_folded), or None for a song without a tempo"""
    lags = [int(x) for x in lags]
    folding = bool(p["fold"]) and anchor is not None and valid(int(anchor))
    if sw.get("fold_first") and folding:
        lags = [fold_one(x, int(anchor), sw.get("fold_round_up"), unchecked=True) if x > 0 else x for x in lags]
    F = len(lags)
    at = [f for f in range(F) if valid(lags[f])]
    if not at:
        return None
    ok = np.zeros(F, bool)
    ok[at] = True
    idx = np.arange(F)
    before = np.maximum.accumulate(np.where(ok, idx, -1))                      # the last valid frame at or before f
    behind = np.minimum.accumulate(np.where(ok, idx, F)[::-1])[::-1]           # the first at or behind f, F: none
    q, n_filled, n_folded = [], 0, 0
    for f in range(F):
        if ok[f]:
            x = lags[f]
        else:
            n_filled += 1
            a, b = int(before[f]), int(behind[f])
            a, b = (a if a >= 0 else None), (b if b < F else None)
            if sw.get("forward_only") and a is not None:
                b = None
            if sw.get("tile_loss") and a is not None and b is not None and (a // TILE == f // TILE) != (b // TILE == f // TILE):
                a, b = (a, None) if a // TILE == f // TILE else (None, b)
            if a is None or b is None:
                x = lags[a if b is None else b]
            elif sw.get("tie_later"):
                x = lags[a if f - a < b - f else b]
            else:
                x = lags[a if f - a <= b - f else b]
        if folding and not sw.get("fold_first"):
            y = fold_one(x, int(anchor), sw.get("fold_round_up"))
            n_folded += y != x
            x = y
        q.append(x)
    return np.array(q, np.int64), n_filled, n_folded


def frames_of(H, F, p, **sw):
    """g(t) for t = 0 .. H-1"""
    t = np.arange(H, dtype=np.int64) - (0 if sw.get("no_origin") else p["origin"])
    g = (t + p["seg"] // 2) // p["seg"] if sw.get("g_rounded") else t // p["seg"]         # floor division
    g = np.maximum(g, 0)
    return g % F if sw.get("wrap_frames") else np.minimum(g, F - 1)


def runs_of(Lt):
    """[(first hop, one past the last hop)] of the maximal stretches of equal L(t)"""
    cut = [0] + [int(i) + 1 for i in np.flatnonzero(Lt[1:] != Lt[:-1])] + [int(Lt.size)]
    return list(zip(cut, cut[1:]))


@functools.lru_cache(maxsize=None)
def _penalties(L, W):
    lo, hi = br.bounds(L)
    return br.penalties(L, W, lo, hi)


@functools.lru_cache(maxsize=None)
def _log():
    return np.array([0] + [br.ilog2_q12(x) for x in range(1, 2 * L_MAX + 1)], np.int64)


def invalid(H, F):
    rec = dict.fromkeys(FIELDS, 0)
    rec.update(hops=H, frames=F, status=BL_UNEXPECTED)
    return dict(rec=rec, flags=np.zeros(H, np.uint8), links=np.zeros(H, np.uint16), scores=np.zeros(H, np.int64),
                track=np.zeros(F, np.int32))


def _prelude(o, lags, anchor, p, sw):
    unknown = set(sw) - set(SWITCHES)
    assert not unknown, unknown
    assert params_ok(p), p
    o = np.asarray(o, dtype=np.int64)
    H, F = int(o.size), len(lags)
    assert 1 <= H < 1 << 24 and 0 <= F <= 1 << 20 and int(o.min()) >= 0 and int(o.max()) < 1 << 18
    pt = period_track(lags, anchor, p, **sw)
    if pt is None:
        return o, None, None, None, None
    Lt = pt[0][frames_of(H, F, p, **sw)]
    runs = runs_of(Lt)
    if sw.get("run_max"):
        Wt = np.zeros(H, np.int64)
        for a, b in runs:
            Wt[a:b] = p["tight"] * int(o[a:b].max())
    else:
        Wt = np.full(H, p["tight"] * int(o.max()), np.int64)
    return o, pt, Lt, runs, Wt


def _record(o, pt, Lt, runs, Wt, C, P, sw):
    H = int(o.size)
    out = br._finish(o, int(Lt[0] if sw.get("end_l0") else Lt[-1]), p_scale(o, Wt, sw), C, P)
    b, rec = out["rec"], dict.fromkeys(FIELDS, 0)
    rec.update({k: b[k] for k in ("score", "pen_scale", "hops", "n_beats", "first", "last", "status")})
    a, z = (0, H - 1) if sw.get("period_at_ends") else (b["first"], b["last"])
    rec.update(frames=int(pt[0].size), n_runs=len(runs), n_filled=pt[1], n_folded=pt[2],
               period_first=int(Lt[a]) if b["n_beats"] else 0, period_last=int(Lt[z]) if b["n_beats"] else 0)
    return dict(rec=rec, flags=out["flags"], links=out["links"], scores=out["scores"], track=pt[0].astype(np.int32))


def p_scale(o, Wt, sw):
    """the record's pen_scale: W of the whole song (run_max: of the last run)"""
    return int(Wt[-1])


def track(o, lags, anchor, p, **sw):
    """dict(rec, flags, links, scores, track) of one song: the definition, hop by hop"""
    assert not set(sw) & set(RUN_SWITCHES), sw
    o, pt, Lt, runs, Wt = _prelude(o, lags, anchor, p, sw)
    H = int(o.size)
    if pt is None:
        return invalid(H, len(lags))
    C, P = np.zeros(H, np.int64), np.zeros(H, np.int64)
    log = _log()
    blk = 0                                              # cross_block: the start of the block that holds t
    blk_end = (int(Lt[0]) + 1) >> 1
    for t in range(H):
        L, W = int(Lt[t]), int(Wt[t])
        lo, hi = br.bounds(L)
        if t >= blk_end:
            blk, blk_end = blk_end, blk_end + ((L + 1) >> 1)
        dmax = min(hi, t)
        best, dstar = None, 0
        if dmax >= lo:
            d = np.arange(lo, dmax + 1)
            prev = C[t - d]
            if sw.get("cross_block"):
                prev = np.where(t - d >= blk, 0, prev)
            if sw.get("pen_at_source"):
                e = np.abs(log[d] - log[Lt[t - d]])
                pen = (W * e * e) >> 28
            else:
                pen = _penalties(L, W)[:d.size]
            vals = prev - pen
            k = int(np.argmax(vals))                     # the first maximum: the smallest d
            best, dstar = int(vals[k]), lo + k
        if best is None or best <= 0:
            C[t], P[t] = o[t], 0
        else:
            C[t], P[t] = o[t] + best, dstar
    return _record(o, pt, Lt, runs, Wt, C, P, sw)


def track_runs(o, lags, anchor, p, **sw):
    """the same as track(), evaluated run by run in blocks of lo hops: all scores of a block at once"""
    assert not set(sw) & set(HOP_SWITCHES), sw
    o, pt, Lt, runs, Wt = _prelude(o, lags, anchor, p, sw)
    H = int(o.size)
    if pt is None:
        return invalid(H, len(lags))
    none = -(1 << 62)
    pad = 2 * L_MAX                                      # Cp[pad + t] = C[t]; the hops before the song never win
    Cp = np.full(pad + H, none, np.int64)
    P = np.zeros(H, np.int64)
    table = np.zeros(2 * L_MAX, np.int64)                # the kernel's table: pen(d) at d - lo
    before = None                                        # the bounds of the run before
    for r0, r1 in runs:
        L, W = int(Lt[r0]), int(Wt[r0])
        lo, hi = br.bounds(L)
        if before is None or not sw.get("stale_pen"):
            table[:hi - lo + 1] = _penalties(L, W)
        for t0 in range(r0, r1, lo):
            t = np.arange(t0, min(t0 + lo, r1))
            if sw.get("stale_bounds") and before is not None and t0 == r0:
                d = np.arange(before[0], before[1] + 1)
                src = t[:, None] - d[None, :]
                prev = np.where(src >= t0, 0, Cp[pad + np.minimum(src, t0 - 1)])
                vals = prev - br.penalties(L, W, before[0], before[1])[None, :]
                first = before[0]
            else:
                d = np.arange(lo, hi + 1)
                vals = Cp[pad + t[:, None] - d[None, :]] - table[None, :hi - lo + 1]  # every source is below t0
                first = lo
            k = np.argmax(vals, axis=1)                  # the first maximum: the smallest d
            best = vals[np.arange(t.size), k]
            link = best > 0
            Cp[pad + t] = o[t] + np.where(link, best, 0)
            P[t] = np.where(link, first + k, 0)
        before = (lo, hi)
    return _record(o, pt, Lt, runs, Wt, Cp[pad:].copy(), P, sw)


def song(o, lags, anchor, p, **sw):
    """track_runs() unless a switch asks for track()"""
    return (track if set(sw) & set(HOP_SWITCHES) else track_runs)(o, lags, anchor, p, **sw)


def batch(songs, p, **sw):
    """songs: [(curve, lags, anchor or None)].  (records SONG_DTYPE, flags uint8, links uint16, scores int64, track
    int32) of a call, songs concatenated"""
    outs = [song(o, lags, a, p, **sw) for o, lags, a in songs]
    recs = np.array([tuple(r["rec"][k] for k in FIELDS) for r in outs], dtype=SONG_DTYPE)
    cat = lambda k, dt: np.concatenate([r[k] for r in outs]).astype(dt)
    return recs, cat("flags", np.uint8), cat("links", np.uint16), cat("scores", np.int64), cat("track", np.int32)


def same(a, b):
    return (a["rec"] == b["rec"] and np.array_equal(a["flags"], b["flags"]) and np.array_equal(a["links"], b["links"])
            and np.array_equal(a["scores"], b["scores"]) and np.array_equal(a["track"], b["track"]))


def edge_bpm(flags, rate, n, at_end):
    """bl_amd_tbeats_edge_bpm in Python floats (doubles)"""
    beats = br.beat_hops(flags)
    k = min(n, len(beats))
    if k < 2 or rate < 1:
        return float("nan")
    part = beats[-k:] if at_end else beats[:k]
    return 60.0 * rate * (k - 1) / (128.0 * (part[-1] - part[0]))


# ---- the material of the tests -------------------------------------------------------------------------------------

OMAX = br.OMAX


def noise(hops, seed, top=1 << 18):
    return np.random.default_rng(seed).integers(0, top, hops).astype(np.int64)


def click_hops(periods):
    """the hops of clicks whose distances are `periods`, the first at hop 0"""
    return np.concatenate([[0], np.cumsum(periods)]).astype(np.int64)


def accelerating(n_clicks=139, first=60.0, rate=0.995, floor=30, amp=50000, seed=5):
    """(curve, click hops): clicks whose period shrinks from `first` by 0.5 % per click, over a low random floor"""
    per, periods = first, []
    for _ in range(n_clicks - 1):
        periods.append(max(floor, int(round(per))))
        per *= rate
    at = click_hops(periods)
    o = noise(int(at[-1]) + 40, seed, 300)
    o[at] = amp
    return o, at


def hits(flags, clicks):
    """the number of clicks that carry a beat"""
    return int(np.asarray(flags)[np.asarray(clicks)].sum())


def corpus():
    """name -> (curve, lags, anchor, params): small inputs with every kind of run change, in a fixed order"""
    c = {}
    c["two_runs"] = (noise(900, 1), [40] * 4 + [90] * 4, None, params(64, 96, 128))
    c["short_runs_L510"] = (noise(700, 2), [510, 2, 510, 2, 510, 300] * 6, None, params(16, 0, 16))
    c["g_change"] = (noise(1200, 3), [255, 256] * 10 + [2, 510] * 6, None, params(32, 48, 1))
    c["gaps"] = (noise(800, 4), [0, 0, 40, 0, 0, 0, 90, 0, 511, 20, 0], None, params(48, 100, 128))
    c["folded"] = (noise(800, 5), [42, 88, 20, 0, 170, 42], 42, params(64, 32, 16, 1))
    c["tight0"] = (noise(600, 6), [7, 33, 7], None, params(128, 0, 0))
    c["below_origin"] = (noise(90, 7), [12, 50, 12], None, params(16, 200, 16))
    c["below_seg"] = (noise(50, 8), [9, 70], None, params(64, 0, 16))
    c["one_frame"] = (noise(400, 9), [64], None, params(16, 5, 128))
    c["no_frame"] = (noise(100, 10), [], None, params())
    c["all_invalid"] = (noise(100, 11), [0, 1, 511, -7], 40, params(16, 0, 16, 1))
    c["zeros"] = (np.zeros(300, np.int64), [9, 20, 9], None, params(32, 0, 16))
    c["sparse"] = (noise(900, 12) * (noise(900, 13, 8) == 0), [12, 30, 12, 5, 64], None, params(128, 64, 16))
    c["full_scale"] = (np.full(2600, OMAX, np.int64), [510] * 2 + [2] * 2 + [510] * 2, None, params(400, 0, 4096))
    return {k: (np.asarray(o, np.int64), list(lags), a, p) for k, (o, lags, a, p) in c.items()}


def named():
    """switch -> (curve, lags, anchor, params): the input that each mistake of this file changes"""
    busy = noise(1500, 21)
    edge = [40] * 252 + [0] * 5 + [90] * 43                     # frame 255: 4 frames from 251, 2 from 257 in the next tile
    return {
        "stale_pen": (busy, [40] * 6 + [90] * 6, None, params(64, 96, 128)),
        "stale_bounds": (busy, [40] * 6 + [90] * 6, None, params(64, 96, 128)),
        "cross_block": (busy, [200] * 3 + [16] * 20, None, params(64, 0, 16)),
        "pen_at_source": (busy, [40] * 6 + [90] * 6, None, params(64, 96, 128)),
        "no_origin": (busy, [40] * 6 + [90] * 6, None, params(64, 96, 128)),
        "g_rounded": (busy, [40] * 6 + [90] * 6, None, params(64, 96, 128)),
        "wrap_frames": (busy, [40] * 6 + [90] * 6, None, params(64, 96, 128)),
        # the last 90 hops hold the largest score at hop 1440, the last 40 do not
        "end_l0": (np.concatenate([noise(1440, 22), [OMAX], np.zeros(59, np.int64)]), [40] * 6 + [90] * 6, None,
                   params(64, 96, 128)),
        "run_max": (np.concatenate([noise(700, 23, 1000), noise(800, 24)]), [40] * 6 + [90] * 6, None, params(64, 96, 128)),
        "tie_later": (busy, [40, 0, 90, 0, 0, 0, 40], None, params(128, 0, 128)),
        "forward_only": (busy, [40, 0, 0, 90, 90, 0, 0, 0, 33], None, params(128, 0, 128)),
        "tile_loss": (noise(4900, 25), edge, None, params(16, 0, 128)),
        "fold_round_up": (busy, [40] * 6 + [85] * 6, 40, params(64, 96, 128, 1)),
        "fold_first": (busy, [300] * 6 + [600] * 3 + [200] * 3, 300, params(64, 96, 128, 1)),
        # silence in front, so the first beat lies behind frame 0; the end at the spike of hop 1500, in front of the
        # last frame, which begins at hop 1504
        "period_at_ends": (np.concatenate([np.zeros(300, np.int64), noise(1200, 26), [OMAX], np.zeros(13, np.int64)]),
                           [30] + [40] * 5 + [90] * 5 + [70], None, params(128, 96, 128)),
    }
