"""The tempo over time of include/bliss_amd.h (bl_amd_tgram_frame, bl_amd_song_tgram) restated in numpy int64 and Python
ints: stages 1 to 6 exactly as the header defines them.  Each frame's row is formed directly from the curve, never
from shared block rows, so the sharing in the kernel is checked against something that does not share.  Every
intermediate stays below 2^50 (the header's bounds), so int64 holds it exactly; np.correlate on int64 stays in integers.

The switches make, on purpose, the mistakes a kernel is likely to make (as tests/rhythm_reference.py does for the tempo):
tests/test_tgram_reference_host.py shows that each of them changes a named input, which tests/test_gpu_tgram.py runs, so
the GPU test would catch a kernel that made it.

    frames_over_h      F from H instead of T = H - 511: frames whose right factors leave the song
    long_window        a window that runs one block long: (m + 1) S terms
    no_retire          a ring row not retired: frame f >= 1 still includes block f - 1
    past_h             T taken one too large, and the hops from H on read as this value (what lies behind the song)
    no_local_max       a pick without the local-maximum condition
    whole_row          a pick over the lags 1 .. 510 instead of the caller's range
    argmax             the pick as the plain arg-max (tests.rhythm_reference.pick has it)
    upper_median       the element at index n_tempo >> 1
    silent_breaks      a frame without a tempo breaks a pair: the jump across it is not counted
    asym_octave        near() with tol M instead of tol 2 M on the L = 2 M side
    tol_percent        tol read as per cent
    ends_all_frames    first and last taken over all frames instead of the frames that have a tempo
    swap_neighbours    r_prev and r_next swapped
"""
import numpy as np

from tests import rhythm_reference as rr

LAGS = rr.LAGS
BL_OK, BL_UNEXPECTED = rr.BL_OK, rr.BL_UNEXPECTED
FRAME_DTYPE = np.dtype([("r0", "<u8"), ("r_prev", "<u8"), ("r_lag", "<u8"), ("r_next", "<u8"), ("lag", "<i4"),
                        ("lag_peak", "<i4")])
SONG_FIELDS = ("hops", "frames", "n_tempo", "status", "frame_first", "frame_last", "lag_first", "lag_last", "lag_low",
               "lag_high", "lag_median", "n_near", "n_jumps", "reserved")
SONG_DTYPE = np.dtype([(k, "<i4") for k in SONG_FIELDS])
assert FRAME_DTYPE.itemsize == 40 and SONG_DTYPE.itemsize == 56


def params(stride=128, blocks=16, lag_min=20, lag_max=200, tol=60, octaves=1):
    return dict(stride=stride, blocks=blocks, lag_min=lag_min, lag_max=lag_max, tol=tol, octaves=octaves)


def params_ok(p):
    return (16 <= p["stride"] <= 1024 and p["stride"] % 16 == 0 and 1 <= p["blocks"] <= 16 and
            1 <= p["lag_min"] <= p["lag_max"] <= 510 and 0 <= p["tol"] <= 1000 and p["octaves"] in (0, 1))


def frames_count(hops, p, frames_over_h=False):
    T = hops if frames_over_h else hops - (LAGS - 1)
    W = p["stride"] * p["blocks"]
    return (T - W) // p["stride"] + 1 if T >= W else 0


def hops_for(frames, p, extra=0):
    """the shortest song with `frames` >= 1 frames, plus `extra` < S hops that add no frame"""
    return LAGS - 1 + p["stride"] * (p["blocks"] + frames - 1) + extra


def near(L, M, tol, octaves, asym_octave=False, tol_percent=False):
    k = 100 if tol_percent else 1000
    if k * abs(L - M) <= tol * M:
        return True
    if not octaves:
        return False
    return k * abs(2 * L - M) <= tol * M or k * abs(L - 2 * M) <= tol * (M if asym_octave else 2 * M)


def frame_row(o, first, terms, behind=0):
    """sum over h in [first, first + terms) of o_h o_{h+tau}, tau = 0 .. 511, as Python ints; hops from H on read as
    `behind` (no correct frame reads one)"""
    need = first + terms + LAGS - 1
    if need > o.size:
        o = np.concatenate([o, np.full(need - o.size, behind, np.int64)])
    R = np.correlate(o[first:need], o[first:first + terms], mode="valid")
    assert R.dtype == np.int64 and R.size == LAGS
    return [int(x) for x in R]


def pick(R, lag_min, lag_max, no_local_max=False, whole_row=False, argmax=False):
    if whole_row:
        lag_min, lag_max = 1, LAGS - 2
    if no_local_max:
        r_peak = max(R[lag_min:lag_max + 1])
        if r_peak == 0:
            return 0, 0, 0
        lag_peak = next(t for t in range(lag_min, lag_max + 1) if R[t] == r_peak)
        return next(t for t in range(lag_min, lag_max + 1) if 16 * R[t] >= 15 * r_peak), lag_peak, r_peak
    return rr.pick(R, lag_min, lag_max, argmax=argmax)


def song(o, p, gram=False, frames_over_h=False, long_window=False, no_retire=False, past_h=None, no_local_max=False,
         whole_row=False, argmax=False, upper_median=False, silent_breaks=False, asym_octave=False, tol_percent=False,
         ends_all_frames=False, swap_neighbours=False):
    """(song record as a dict, frame records as a FRAME_DTYPE array, rows as a uint64 (F, 512) array or None)"""
    o = np.asarray(o, dtype=np.int64)
    assert params_ok(p) and 1 <= o.size < 1 << 24 and int(o.min()) >= 0 and int(o.max()) < 1 << 18
    H, S, m = int(o.size), p["stride"], p["blocks"]
    F = frames_count(H + (past_h is not None), p, frames_over_h)
    rec = dict.fromkeys(SONG_FIELDS, 0)
    rec["hops"] = H
    if F == 0:
        rec["status"] = BL_UNEXPECTED
        return rec, np.zeros(0, FRAME_DTYPE), (np.zeros((0, LAGS), np.uint64) if gram else None)
    frames = np.zeros(F, FRAME_DTYPE)
    rows = np.zeros((F, LAGS), np.uint64) if gram else None
    for f in range(F):
        first, terms = f * S, (m + 1 if long_window else m) * S
        if no_retire and f >= 1:
            first, terms = first - S, terms + S
        R = frame_row(o, first, terms, behind=past_h or 0)
        lag, lag_peak, _ = pick(R, p["lag_min"], p["lag_max"], no_local_max, whole_row, argmax)
        prev, nxt = (R[lag - 1], R[lag + 1]) if lag else (0, 0)
        if swap_neighbours:
            prev, nxt = nxt, prev
        frames[f] = (R[0], prev, R[lag] if lag else 0, nxt, lag, lag_peak)
        if gram:
            rows[f] = R
    lags = [int(x) for x in frames["lag"]]
    rec.update(song_record(H, lags, p, upper_median, silent_breaks, asym_octave, tol_percent, ends_all_frames))
    return rec, frames, rows


def song_record(H, lags, p, upper_median=False, silent_breaks=False, asym_octave=False, tol_percent=False,
                ends_all_frames=False):
    """stage 6 over the lags of a song's F >= 1 frames"""
    nr = lambda L, M: near(L, M, p["tol"], p["octaves"], asym_octave, tol_percent)
    rec = dict.fromkeys(SONG_FIELDS, 0)
    at = [f for f, l in enumerate(lags) if l]
    tl = [lags[f] for f in at]
    rec.update(hops=H, frames=len(lags), n_tempo=len(tl), status=BL_OK, frame_first=-1, frame_last=-1)
    if ends_all_frames:
        rec.update(frame_first=0, frame_last=len(lags) - 1, lag_first=lags[0], lag_last=lags[-1])
    if not tl:
        return rec
    if not ends_all_frames:
        rec.update(frame_first=at[0], frame_last=at[-1], lag_first=tl[0], lag_last=tl[-1])
    med = sorted(tl)[len(tl) >> 1 if upper_median else (len(tl) - 1) >> 1]
    pairs = zip(at, at[1:])
    rec.update(lag_low=min(tl), lag_high=max(tl), lag_median=med, n_near=sum(nr(l, med) for l in tl),
               n_jumps=sum(not nr(lags[b], lags[a]) for a, b in pairs if not silent_breaks or b == a + 1))
    return rec


def batch(curves, p, gram=True, **switches):
    """(song records SONG_DTYPE, frame records FRAME_DTYPE, rows uint64 (sum F, 512)) of a call, songs concatenated"""
    recs, frames, rows = [], [], []
    for o in curves:
        r, fr, g = song(o, p, gram=gram, **switches)
        recs.append(tuple(r[k] for k in SONG_FIELDS))
        frames.append(fr)
        rows.append(g)
    return (np.array(recs, dtype=SONG_DTYPE), np.concatenate(frames),
            np.concatenate(rows) if gram else None)


def bpm(frame, rate=22050):
    """bl_amd_tgram_bpm: tests.rhythm_reference.bpm on a frame's values"""
    return rr.bpm(dict(lag=int(frame["lag"]), r_prev=int(frame["r_prev"]), r_lag=int(frame["r_lag"]),
                       r_next=int(frame["r_next"])), rate)


def seconds(frame, p, rate=22050):
    return rr.HOP * (frame * p["stride"] + 0.5 * p["stride"] * p["blocks"]) / rate


def steadiness(rec):
    return rec["n_near"] / rec["n_tempo"] if rec["n_tempo"] else 0.0


# ---- the material of the tests -------------------------------------------------------------------------------------

def clicks(period, hops, amp=5000):
    o = np.zeros(hops, dtype=np.int64)
    o[::period] = amp
    o[1::period] = amp // 2
    return o


WORKED = params(stride=64, blocks=8, lag_min=20, lag_max=200, tol=60, octaves=1)


def worked_curve():
    """clicks of period 40 for 2 000 hops, 300 silent hops, clicks of period 50 for 2 211 hops, noise below 40 on the
    clicks' stretches: H = 4 511.  Under WORKED: 55 frames, the lags 30 x 40 then 25 x 50, lag_first 40, lag_last 50,
    lag_median 40, n_near 30, n_jumps 1."""
    o = np.concatenate([clicks(40, 2000), np.zeros(300, dtype=np.int64), clicks(50, 2211)])
    o = o + np.random.default_rng(1).integers(0, 40, o.size)
    o[2000:2300] = 0
    return o


def noise(hops, seed, top=1 << 18):
    return np.random.default_rng(seed).integers(0, top, hops).astype(np.int64)


SMALL = params(stride=32, blocks=4, lag_min=20, lag_max=200, tol=60, octaves=1)
TINY = params(stride=16, blocks=2, lag_min=20, lag_max=200, tol=60, octaves=1)


def gapped_curve():
    """silence, clicks of period 40, a silent stretch longer than SMALL's window so that some frames have no tempo,
    clicks of period 90: the first frames have no tempo and the pair across the silent frames is a jump"""
    z = lambda n: np.zeros(n, dtype=np.int64)
    return np.concatenate([z(200), clicks(40, 700) + noise(700, 11, 30), z(400), clicks(90, 900) + noise(900, 12, 30)])


def octave_curve():
    """clicks of period 42, then of period 88: 88 is near twice 42 within 60 per mille of 84, not of 42"""
    return np.concatenate([clicks(42, 800), clicks(88, 1200)]) + noise(2000, 13, 30)


def named():
    """switch -> (curve, parameters, the switch's value): the input that each mistake of this file changes"""
    busy = noise(hops_for(10, TINY), 21)
    return {
        "frames_over_h": (busy, TINY, True),
        "long_window": (busy, TINY, True),
        "no_retire": (busy, TINY, True),
        "past_h": (noise(hops_for(3, SMALL, extra=31), 22), SMALL, 7),
        "no_local_max": (busy, TINY, True),
        "whole_row": (busy, TINY, True),
        "argmax": (busy, TINY, True),
        "upper_median": (busy, TINY, True),
        "silent_breaks": (gapped_curve(), SMALL, True),
        "asym_octave": (octave_curve(), SMALL, True),
        "tol_percent": (worked_curve(), WORKED, True),
        "ends_all_frames": (gapped_curve(), SMALL, True),
        "swap_neighbours": (busy, TINY, True),
    }
