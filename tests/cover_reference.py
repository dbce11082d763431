"""Reference for the cover and version matching (include/bliss_amd.h: bl_amd_cover_match, bl_amd_cover_*): the
transposition from the songs' profiles and the local alignment of their units with its origin and best cell, in numpy
int64 and Python integers.  align_slow goes cell by cell, straight from the definition; align goes by anti-diagonals and
takes the long inputs; match_batch runs sets, pairs and parameters.  SWITCHES make a kernel's plausible mistakes on
purpose (in align), so that the tests can show that their inputs would catch each of them.  The units are those of
tests/form_reference.py."""
import numpy as np

from tests.form_reference import unit_bytes, units  # noqa: F401  (the units are the structure call's)

UNITS_MAX = 8192
NO_MATCH, TOO_LONG, BAD_INDEX = 1, 2, 4
S_MAX, THR_MAX, GAP_MAX = 16129, 16128, 1 << 20
STRIP = 64                                  # the columns one wavefront owns at a time (bl_amd_cover_shape)

COVER_DTYPE = np.dtype([("score", "<u4"), ("a_start", "<i4"), ("a_end", "<i4"), ("b_start", "<i4"), ("b_end", "<i4"),
                        ("transpose", "<i4"), ("units_a", "<i4"), ("units_b", "<i4"), ("status", "<i4"),
                        ("reserved", "<i4")])

# the mistakes a kernel could plausibly make
SWITCHES = (
    "rot_minus",        # b rotated by k - r
    "oti_tie_large",    # the larger r wins a tie of C
    "profile_short",    # the profile misses a song's last unit
    "gap_diag",         # gap charged on the diagonal as well
    "no_floor",         # H = max(d, u, l), no floor at 0
    "up_first",         # up before diagonal on ties
    "left_first",       # left before up on ties
    "origin_prev",      # a fresh path's origin is (i - 1, j - 1)
    "best_late_i",      # the later i wins a tie of the best cell
    "best_j_first",     # j compared before i in the best cell's key
    "strip_left_zero",  # H_left read as 0 in the first column of a strip of 64
    "strip_diag_row",   # the diagonal of a strip's first column taken from row i, not i - 1
    "row_overrun",      # the row loop runs one unit into the song that follows a
    "rot16",            # b rotated over all 16 bytes of a unit
)


def params(thr=12000, gap=4000, transpose=-1, reserved=0):
    return dict(thr=thr, gap=gap, transpose=transpose, reserved=reserved)


def profile(q, sw=frozenset()):
    """g[k] of one song's units, Python ints"""
    q = np.asarray(q, dtype=np.int64).reshape(-1, 12)
    if "profile_short" in sw:
        q = q[:-1]
    return [int(v) for v in q.sum(axis=0)]


def pick_r(qa, qb, transpose=-1, sw=frozenset()):
    """the transposition: the smallest r with the largest C(r), or the one given"""
    if transpose >= 0:
        return transpose
    ga, gb = profile(qa, sw), profile(qb, sw)
    C = [sum(ga[k] * gb[(k + r) % 12] for k in range(12)) for r in range(12)]
    best = max(C)
    at = [r for r in range(12) if C[r] == best]
    return at[-1] if "oti_tie_large" in sw else at[0]


def rotate(qb, r, sw=frozenset()):
    """row j holds q_b,j[(k + r) mod 12] at k"""
    qb = np.asarray(qb, dtype=np.int64).reshape(-1, 12)
    if "rot16" in sw:
        wide = np.concatenate([qb, np.zeros((qb.shape[0], 4), np.int64)], axis=1)
        return np.roll(wide, -r, axis=1)[:, :12]
    return np.roll(qb, r if "rot_minus" in sw else -r, axis=1)


def align_slow(qa, qb, thr, gap, r):
    """(score, a_start, a_end, b_start, b_end) of the best cell, or None when the best H is 0: every cell in Python
    integers, straight from the definition"""
    A = [[int(v) for v in row] for row in np.asarray(qa).reshape(-1, 12)]
    B = [[int(v) for v in row] for row in np.asarray(qb).reshape(-1, 12)]
    Ua, Ub = len(A), len(B)
    H, O = {}, {}
    best = None
    for i in range(Ua):
        for j in range(Ub):
            S = sum(A[i][k] * B[j][(k + r) % 12] for k in range(12))
            hd = H.get((i - 1, j - 1), 0)
            d, u, l = hd + S - thr, H.get((i - 1, j), 0) - gap, H.get((i, j - 1), 0) - gap
            h = max(0, d, u, l)
            H[i, j] = h
            if h <= 0:
                continue
            if d == h:
                O[i, j] = (i, j) if hd == 0 else O[i - 1, j - 1]
            elif u == h:
                O[i, j] = O[i - 1, j]
            else:
                O[i, j] = O[i, j - 1]
            key = (h << 26) + ((8191 - i) << 13) + (8191 - j)
            if best is None or key > best[0]:
                best = (key, h, i, j)
    if best is None:
        return None
    _, h, i, j = best
    return h, O[i, j][0], i, O[i, j][1], j


def align(qa, qb, thr, gap, r, sw=frozenset(), tail_a=None):
    """what align_slow returns, by anti-diagonals in int64.  tail_a: the unit that follows the song in set a's
    concatenated array, which row_overrun reads."""
    qa = np.asarray(qa, dtype=np.int64).reshape(-1, 12)
    if "row_overrun" in sw and tail_a is not None and qa.shape[0]:
        qa = np.concatenate([qa, np.asarray(tail_a, np.int64).reshape(1, 12)])
    qb = rotate(qb, r, sw)
    Ua, Ub = qa.shape[0], qb.shape[0]
    if Ua == 0 or Ub == 0:
        return None
    # index i + 1 is row i; index 0 is row -1.  x1: the previous anti-diagonal, x2: the one before; 0 outside the matrix
    z = lambda: np.zeros(Ua + 1, dtype=np.int64)
    H1, H2, Oi1, Oi2, Oj1, Oj2 = z(), z(), z(), z(), z(), z()
    gd = gap if "gap_diag" in sw else 0
    best_key, best = -1, None
    for s in range(Ua + Ub - 1):
        lo, hi = max(0, s - Ub + 1), min(Ua - 1, s)
        i = np.arange(lo, hi + 1)
        j = s - i
        S = (qa[i] * qb[j]).sum(axis=1)
        hd, od_i, od_j = H2[i], Oi2[i], Oj2[i]
        hu, ou_i, ou_j = H1[i], Oi1[i], Oj1[i]
        hl, ol_i, ol_j = H1[i + 1], Oi1[i + 1], Oj1[i + 1]
        first = (j % STRIP == 0) & (j > 0)                       # the first column of a strip that is not the first
        if "strip_left_zero" in sw:
            hl, ol_i, ol_j = np.where(first, 0, hl), np.where(first, 0, ol_i), np.where(first, 0, ol_j)
        if "strip_diag_row" in sw:
            hd, od_i, od_j = np.where(first, hl, hd), np.where(first, ol_i, od_i), np.where(first, ol_j, od_j)
        d, u, l = hd + S - thr - gd, hu - gap, hl - gap
        h = np.maximum(np.maximum(d, u), l)
        if "no_floor" not in sw:
            h = np.maximum(h, 0)
        fresh = hd == 0
        si, sj = (i - 1, j - 1) if "origin_prev" in sw else (i, j)
        di, dj = np.where(fresh, si, od_i), np.where(fresh, sj, od_j)
        if "up_first" in sw:
            oi = np.where(u == h, ou_i, np.where(d == h, di, ol_i))
            oj = np.where(u == h, ou_j, np.where(d == h, dj, ol_j))
        elif "left_first" in sw:
            oi = np.where(d == h, di, np.where(l == h, ol_i, ou_i))
            oj = np.where(d == h, dj, np.where(l == h, ol_j, ou_j))
        else:
            oi = np.where(d == h, di, np.where(u == h, ou_i, ol_i))
            oj = np.where(d == h, dj, np.where(u == h, ou_j, ol_j))
        live = h > 0
        if "no_floor" not in sw:
            oi, oj = np.where(live, oi, 0), np.where(live, oj, 0)
        if live.any():
            ki = i if "best_late_i" in sw else 8191 - i
            key = ((h << 26) + ((8191 - j) << 13) + ki) if "best_j_first" in sw else ((h << 26) + (ki << 13) + (8191 - j))
            key = np.where(live, key, -1)
            at = int(np.argmax(key))
            if int(key[at]) > best_key:
                best_key, best = int(key[at]), (int(h[at]), int(oi[at]), int(i[at]), int(oj[at]), int(j[at]))
        H2, Oi2, Oj2 = H1, Oi1, Oj1
        H1, Oi1, Oj1 = z(), z(), z()
        H1[i + 1], Oi1[i + 1], Oj1[i + 1] = h, oi, oj
    return best


def match_one(qa, qb, p, sw=frozenset(), tail_a=None, slow=False):
    """the record of one pair as a tuple in COVER_DTYPE's order"""
    Ua, Ub = int(np.asarray(qa).reshape(-1, 12).shape[0]), int(np.asarray(qb).reshape(-1, 12).shape[0])
    if Ua > UNITS_MAX or Ub > UNITS_MAX:
        return (0, 0, 0, 0, 0, 0, Ua, Ub, TOO_LONG, 0)
    if Ua == 0 or Ub == 0:
        return (0, 0, 0, 0, 0, 0, Ua, Ub, NO_MATCH, 0)
    r = pick_r(qa, qb, p["transpose"], sw)
    m = align_slow(qa, qb, p["thr"], p["gap"], r) if slow else align(qa, qb, p["thr"], p["gap"], r, sw, tail_a)
    if m is None:
        return (0, 0, 0, 0, 0, r, Ua, Ub, NO_MATCH, 0)
    h, a0, a1, b0, b1 = m
    return (h, a0, a1, b0, b1, r, Ua, Ub, 0, 0)


def match_batch(set_a, set_b, pairs, p, sw=frozenset(), slow=False):
    """the records of the pairs (n, 2) over the sets, each a list of (U, 12) unit arrays; one alignment per distinct
    pair"""
    rec = np.zeros(len(pairs), dtype=COVER_DTYPE)
    done = {}
    for n, (ia, ib) in enumerate(np.asarray(pairs).reshape(-1, 2).tolist()):
        if not (0 <= ia < len(set_a) and 0 <= ib < len(set_b)):
            rec[n] = (0, 0, 0, 0, 0, 0, 0, 0, BAD_INDEX, 0)
            continue
        if (ia, ib) not in done:
            tail = next((np.asarray(x).reshape(-1, 12)[0] for x in set_a[ia + 1:] if len(x)), None)
            done[ia, ib] = match_one(set_a[ia], set_b[ib], p, sw, tail, slow)
        rec[n] = done[ia, ib]
    return rec


def score(rec, thr):
    """score / ((16129 - thr) min(units_a, units_b)) of one record; nan where the status is not 0"""
    den = (S_MAX - thr) * min(int(rec["units_a"]), int(rec["units_b"]))
    return float(rec["score"]) / den if int(rec["status"]) == 0 and den > 0 else float("nan")


def cat(songs):
    """a set's units concatenated as the (n, 16) uint8 the device reads"""
    return np.concatenate([unit_bytes(np.asarray(q, np.int64).reshape(-1, 12)) for q in songs] +
                          [np.zeros((0, 16), np.uint8)])


# ---- inputs --------------------------------------------------------------------------------------------------------

def alphabet(seed, letters):
    """`letters` distinct units of a seeded generator, (letters, 12) int64 in 0 .. 127, each of norm near 127"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < letters:
        x = rng.integers(0, 1 << 30, size=(1, 12), dtype=np.int64)
        x[0, rng.choice(12, size=3, replace=False)] = rng.integers(1 << 33, 1 << 34, size=3)
        q = units(x, 1)[0]
        if not any((q == o).all() for o in out):
            out.append(q)
    return np.stack(out)


def letters_song(seed, n, abc):
    """n units drawn from the alphabet abc"""
    return abc[np.random.default_rng(seed).integers(0, abc.shape[0], size=n)]


def chord_song(seed, n_chords=40, hold=6):
    """(T, 12) chroma frames: random triads held `hold` frames each over a floor below 2^20, as
    tests/form_reference.py's chord songs"""
    rng = np.random.default_rng(seed)
    chords = [tuple(rng.choice(12, size=3, replace=False)) for _ in range(n_chords)]
    X = rng.integers(0, 1 << 20, size=(n_chords * hold, 12), dtype=np.int64)
    for t in range(X.shape[0]):
        X[t, list(chords[t // hold])] = rng.integers(1 << 30, 1 << 32, size=3, dtype=np.int64)
    return X


def transposed(X, semitones):
    """the frames `semitones` up: class k moves to k + semitones"""
    return np.roll(X, semitones, axis=1)


def stretched(X, factor):
    """the frames played `factor` times as slowly (nearest earlier frame)"""
    n = int(X.shape[0] * factor)
    return X[np.minimum((np.arange(n) / factor).astype(np.int64), X.shape[0] - 1)]


def noisy(X, seed, level=1 << 29):
    return X + np.random.default_rng(seed).integers(0, level, size=X.shape, dtype=np.int64)


def with_lead_in(X, seed, frames=20):
    return np.concatenate([chord_song(seed, n_chords=-(-frames // 5), hold=5)[:frames], X])


def melody(seed, seconds=20.0, semitones=0, slow=1.0, amp=8000.0, rate=22050):
    """tests/fprint_reference.py's melody (the same seeded notes and envelope; identical for semitones 0 and slow 1),
    played `semitones` higher and `slow` times as slowly: mono int16 at 22 050 Hz"""
    rng = np.random.default_rng(seed)
    n = int(seconds * rate)
    x = np.zeros(int(n * slow) + rate)
    at = src = 0
    while src < n:
        dur0 = int(rng.integers(rate // 4, rate // 2))
        f = 220.0 * 2.0 ** ((int(rng.integers(0, 36)) + semitones) / 12.0)
        m0 = min(dur0, n - src)
        dur, m = int(round(dur0 * slow)), int(round(m0 * slow))
        tt = np.arange(m) / rate
        x[at:at + m] += amp * np.exp(-3.0 * tt * rate / dur) * (np.sin(2 * np.pi * f * tt) + 0.5 * np.sin(4 * np.pi * f * tt))
        at, src = at + dur, src + dur0
    return np.round(x[:int(n * slow)]).astype(np.int16)


def single(k):
    """the unit of a frame with one non-zero class"""
    q = np.zeros(12, dtype=np.int64)
    q[k] = 127
    return q


def lettered(seed, letters, ua, ub):
    abc = alphabet(20 + seed % 5, letters)
    return letters_song(1000 + seed, ua, abc), letters_song(2000 + seed, ub, abc)


def switch_inputs():
    """switch -> (a, b, parameters, the unit that follows a in its set)"""
    X = chord_song(4, n_chords=8, hold=2)
    up3 = units(X, 1), units(transposed(X, 3), 1)
    a0, b0 = lettered(0, 3, 8, 7)
    base = alphabet(9, 1)[0]
    rotations = np.stack([np.roll(base, k) for k in range(12)])   # a flat profile: every C(r) ties
    x = np.array([90, 80, 40] + [0] * 9, dtype=np.int64)
    y = np.roll(x, 6)                                             # S(x, x) = S(y, y) = 16100, S(x, y) = 0
    const = np.repeat(alphabet(12, 1), 5, axis=0)
    fixed = lambda **kw: params(thr=12000, gap=3000, transpose=0, **kw)
    return {
        "rot_minus": (*up3, params(transpose=3), None),
        "oti_tie_large": (rotations, units(X, 1), params(), None),
        "profile_short": (np.stack([single(5), single(0), single(0)]), np.stack([single(7), single(7)]), params(), None),
        "gap_diag": (a0, b0, fixed(), None),
        "no_floor": (a0, b0, fixed(), None),
        "up_first": (*lettered(38, 2, 7, 5), params(gap=0, transpose=0), None),
        "left_first": (*lettered(7, 3, 8, 9), params(gap=0, transpose=0), None),
        "origin_prev": (a0, b0, fixed(), None),
        "best_late_i": (const, const[:3], params(transpose=0), None),
        "best_j_first": (np.stack([x, y]), np.stack([y, x]), params(thr=4000, transpose=0), None),
        "strip_left_zero": (*lettered(10, 3, 79, 85), fixed(), None),
        "strip_diag_row": (*lettered(0, 3, 74, 103), fixed(), None),
        "row_overrun": (a0, np.concatenate([a0, a0[:1]]), fixed(), a0[0]),
        "rot16": (*up3, params(transpose=3), None),
    }
