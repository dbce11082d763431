"""Reference for the song structure (include/bliss_amd.h: bl_amd_song_form, bl_amd_form_*): the units of a chromagram,
the thumbnail over the diagonals of their self-similarity and the checkerboard novelty with its boundaries, in numpy
int64 and Python integers, switches that make a kernel's plausible mistakes on purpose, so that the tests can show that
their inputs would catch each of them, and the seeded songs of the two claims."""
import numpy as np

UNITS_MAX = 8192
NO_THUMB, TOO_LONG = 1, 2
X_MAX = 631_000_000_000            # a chroma value stays below 2^39.2 (include/bliss_amd.h, the chroma block's bounds)
LOW20 = (1 << 20) - 1

FORM_DTYPE = np.dtype([("units", "<i4"), ("status", "<i4"), ("thumb_start", "<i4"), ("thumb_lag", "<i4"),
                       ("thumb_score", "<u4"), ("thumb_self", "<u4"), ("boundaries", "<i4"), ("nov_max_unit", "<i4"),
                       ("nov_max", "<u8"), ("reserved", "<u8")])

# the mistakes a kernel could plausibly make
SWITCHES = (
    "keep_partial",   # the trailing frames that do not fill a unit make one more
    "norm_max",       # r is the largest y, not the root of the squares
    "round_div",      # q rounded to nearest instead of floored
    "shift19",        # s = bitlength - 19
    "lag_start",      # lags start at minlag + 1
    "lag_end",        # lags end at U - M - 1
    "window_past",    # starts run to U - M for every lag: the window runs past U, over zeros
    "tie_lag",        # the larger lag wins a tie
    "tie_start",      # the later start wins a tie
    "weights_lm",     # w_a = L - a
    "both_from_u",    # the past half ends at u, not at u - 1
    "peak_le",        # N(v) <= N(u) on the left side
    "batch_max",      # the threshold is taken against the largest novelty of the batch
    "cross_edge",     # as window_past, but over the units that follow in the concatenated array
)
UNIT_SWITCHES = SWITCHES[:4]


def params(pool=1, seg=48, min_lag=48, nov=16, peak_num=1, peak_den=4, reserved=0):
    return dict(pool=pool, seg=seg, min_lag=min_lag, nov=nov, peak_num=peak_num, peak_den=peak_den, reserved=reserved)


def units_count(frames, pool, sw=frozenset()):
    return -(-frames // pool) if "keep_partial" in sw else frames // pool


def isqrt(x):
    import math
    return math.isqrt(int(x))


def unit_slow(X, u, P, sw=frozenset()):
    """q_u of the chromagram X in Python integers, straight from the definition"""
    rows = [[int(v) for v in row] for row in np.asarray(X).reshape(-1, 12)[u * P:(u + 1) * P]]
    Y = [sum(r[k] for r in rows) for k in range(12)]
    m = max(Y)
    if m == 0:
        return [0] * 12
    s = max(0, m.bit_length() - (19 if "shift19" in sw else 20))
    y = [v >> s for v in Y]
    r = max(y) if "norm_max" in sw else isqrt(sum(v * v for v in y))
    return [(127 * v + (r // 2 if "round_div" in sw else 0)) // r for v in y]


def units(X, P, sw=frozenset()):
    """the units of one song's chromagram X (T, 12): int64 (U, 12), values 0 .. 127"""
    X = np.asarray(X, dtype=np.int64).reshape(-1, 12)
    U = units_count(X.shape[0], P, sw)
    if U == 0:
        return np.zeros((0, 12), dtype=np.int64)
    pad = U * P - X.shape[0]
    if pad > 0:
        X = np.concatenate([X, np.zeros((pad, 12), np.int64)])
    Y = X[:U * P].reshape(U, P, 12).sum(axis=1)                       # < 2^43.2
    q = np.zeros((U, 12), dtype=np.int64)
    for u in np.flatnonzero(Y.max(axis=1) > 0):
        m = int(Y[u].max())
        s = max(0, m.bit_length() - (19 if "shift19" in sw else 20))
        y = [int(v) >> s for v in Y[u]]
        r = max(y) if "norm_max" in sw else isqrt(sum(v * v for v in y))
        q[u] = [(127 * v + (r // 2 if "round_div" in sw else 0)) // r for v in y]
    return q


def unit_bytes(q):
    """(U, 12) units as the (U, 16) uint8 the device writes: twelve q and four zero bytes"""
    out = np.zeros((q.shape[0], 16), dtype=np.uint8)
    out[:, :12] = q
    return out


def sim(q, u, v):
    return sum(int(a) * int(b) for a, b in zip(q[u], q[v]))


def f_slow(q, u, l, M):
    return sum(sim(q, u + j, u + l + j) for j in range(M))


def thumb(q, M, minlag, sw=frozenset(), tail=None):
    """(dict of the record's thumbnail fields and status bit, rep as uint32 (U, 2)) of one song's units.  tail: the
    units that follow the song in the concatenated array, which cross_edge reads."""
    U = q.shape[0]
    rep_r, rep_l = np.zeros(U, dtype=np.int64), np.zeros(U, dtype=np.int64)
    past = "window_past" in sw or "cross_edge" in sw
    ext = q
    if past:
        t = np.zeros((U, 12), dtype=np.int64)
        if "cross_edge" in sw and tail is not None:
            t[:min(U, tail.shape[0])] = tail[:U]
        ext = np.concatenate([q, t])
    best = None
    for l in range(minlag + ("lag_start" in sw), U - M - ("lag_end" in sw) + 1):
        n = U - M + 1 if past else U - M - l + 1                      # starts 0 .. n - 1
        if n <= 0:
            continue
        s = (ext[:n + M - 1] * ext[l:l + n + M - 1]).sum(axis=1)
        c = np.concatenate([[0], np.cumsum(s)])
        F = c[M:] - c[:-M]
        fm = int(F.max())
        at = np.flatnonzero(F == fm)
        u = int(at[-1] if "tie_start" in sw else at[0])
        key = (fm, l if "tie_lag" in sw else -l, u if "tie_start" in sw else -u)
        if best is None or key > best[0]:
            best = (key, fm, l, u)
        upd = F >= rep_r[:n] if "tie_lag" in sw else F > rep_r[:n]
        upd &= F > 0
        rep_r[:n][upd] = F[upd]
        rep_l[:n][upd] = l
    rep = np.stack([rep_r, rep_l], axis=1).astype(np.uint32)
    if best is None or best[1] == 0:
        return dict(status=NO_THUMB, thumb_start=0, thumb_lag=0, thumb_score=0, thumb_self=0), rep
    _, fm, l, u = best
    return dict(status=0, thumb_start=u, thumb_lag=l, thumb_score=fm,
                thumb_self=int((ext[u:u + M] * ext[u:u + M]).sum())), rep


def novelty(q, L, sw=frozenset()):
    """N(u) of one song's units as a list of Python ints"""
    U = q.shape[0]
    N = [0] * U
    if U < 2 * L:
        return N
    us = np.arange(L, U - L + 1)
    D = np.zeros((us.size, 12), dtype=np.int64)
    for a in range(1, L + 1):
        w = L - a if "weights_lm" in sw else L + 1 - a
        D += w * (q[us - a + (1 if "both_from_u" in sw else 0)] - q[us + a - 1])
    for u, v in zip(us, (D * D).sum(axis=1)):
        N[int(u)] = int(v)
    return N


def novelty_slow(q, u, L):
    U = len(q)
    if not L <= u <= U - L:
        return 0
    P = [sum((L + 1 - a) * int(q[u - a][k]) for a in range(1, L + 1)) for k in range(12)]
    G = [sum((L + 1 - a) * int(q[u + a - 1][k]) for a in range(1, L + 1)) for k in range(12)]
    return sum((p - g) ** 2 for p, g in zip(P, G))


def boundaries(N, L, peak_num, peak_den, sw=frozenset(), threshold_max=None):
    """(flags as uint8 (U,), Nmax, nov_max_unit) from the novelty values"""
    U = len(N)
    flags = np.zeros(U, dtype=np.uint8)
    nmax = max(N) if U else 0
    at = N.index(nmax) if nmax else 0
    tmax = nmax if threshold_max is None else threshold_max
    for u in range(U):
        n = N[u]
        if n <= 0 or n * peak_den < tmax * peak_num:
            continue
        left = N[max(0, u - L):u]
        right = N[u + 1:min(U - 1, u + L) + 1]
        if all(v <= n if "peak_le" in sw else v < n for v in left) and all(v <= n for v in right):
            flags[u] = 1
    return flags, nmax, at


def form_batch(X, counts, p, sw=frozenset()):
    """(records as FORM_DTYPE, units uint8 (n, 16), rep uint32 (n, 2), novelty uint64 (n,), flags uint8 (n,)) of songs
    whose frames are concatenated in X, counts[i] frames each, under the parameter dict p"""
    X = np.asarray(X, dtype=np.int64).reshape(-1, 12)
    P, M, minlag, L = p["pool"], p["seg"], p["min_lag"], p["nov"]
    qs, at = [], 0
    for t in counts:
        qs.append(units(X[at:at + t], P, sw))
        at += t
    novs = [novelty(q, L, sw) if q.shape[0] <= UNITS_MAX else [0] * q.shape[0] for q in qs]
    batch_max = max([max(n) for n in novs if n] + [0])
    rec = np.zeros(len(counts), dtype=FORM_DTYPE)
    reps, flags = [], []
    for i, q in enumerate(qs):
        U = q.shape[0]
        rec["units"][i] = U
        if U > UNITS_MAX:
            rec["status"][i] = NO_THUMB | TOO_LONG
            reps.append(np.zeros((U, 2), np.uint32))
            flags.append(np.zeros(U, np.uint8))
            continue
        tail = np.concatenate(qs[i + 1:] + [np.zeros((0, 12), np.int64)])
        th, rep = thumb(q, M, minlag, sw, tail)
        fl, nmax, at_max = boundaries(novs[i], L, p["peak_num"], p["peak_den"], sw,
                                      batch_max if "batch_max" in sw else None)
        for k, v in th.items():
            rec[k][i] = v
        rec["boundaries"][i], rec["nov_max_unit"][i], rec["nov_max"][i] = int(fl.sum()), at_max, nmax
        reps.append(rep)
        flags.append(fl)
    cat = lambda parts, shape, dt: np.concatenate(parts + [np.zeros(shape, dt)])
    return (rec, cat([unit_bytes(q) for q in qs], (0, 16), np.uint8), cat(reps, (0, 2), np.uint32),
            cat([np.array(n, dtype=np.uint64) for n in novs], (0,), np.uint64), cat(flags, (0,), np.uint8))


def sections(flags, n_units):
    """the (start, end) unit ranges between the boundaries of one song"""
    cuts = [0] + [int(u) for u in np.flatnonzero(np.asarray(flags[:n_units]) & 1) if u > 0] + [n_units]
    return [(a, b) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]


# ---- inputs --------------------------------------------------------------------------------------------------------

def random_frames(seed, T, hi=1 << 30):
    """(T, 12) chroma values of a seeded generator, int64"""
    return np.random.default_rng(seed).integers(0, hi, size=(T, 12), dtype=np.int64)


def shift_frame():
    """a frame whose unit tells s = bitlength - 20 from bitlength - 19: the second class is so small that it adds 1 to
    the root at 20 bits (q = 126 in the first class) and nothing at 19 (q = 127)"""
    x = np.zeros((1, 12), dtype=np.int64)
    x[0, 0], x[0, 1] = (1 << 39) + 12345, 10 * (1 << 27) + (1 << 19)
    return x


SECTIONS = (("intro", 40), ("A", 64), ("B", 80), ("A", 64), ("outro", 30))      # frames; boundaries at 40, 104, 184, 248


def _chord_frames(rng, chords):
    """one frame per entry of chords: its three pitch classes loud (2^30 .. 2^32) over a floor below 2^20"""
    X = rng.integers(0, 1 << 20, size=(len(chords), 12), dtype=np.int64)
    for t, c in enumerate(chords):
        X[t, list(c)] = rng.integers(1 << 30, 1 << 32, size=3, dtype=np.int64)
    return X


def section_song(seed, hold=4):
    """intro / A / B / A / outro: chords held `hold` frames and drawn at random per section, A's sequence reused.
    hold = None: one chord per section (homogeneous sections)."""
    rng = np.random.default_rng(seed)
    seqs, chords = {}, []
    for name, n in SECTIONS:
        if name not in seqs:
            k = 1 if hold is None else -(-n // hold)
            picks = [tuple(rng.choice(12, size=3, replace=False)) for _ in range(k)]
            seqs[name] = [picks[0 if hold is None else t // hold] for t in range(n)]
        chords += seqs[name]
    return _chord_frames(rng, chords)
