"""Reference for the audio fingerprints (include/bliss_amd.h: bl_amd_fprint_match, bl_amd_fprint_*): the words of a
chromagram and the match of two word sequences in numpy int64 and Python integers, switches that make a kernel's
plausible mistakes on purpose, so that the tests can show that their inputs would catch each of them, and the seeded
melodies of the robustness table."""
import numpy as np

FRAMES, HALF, HOP, RATE = 16, 8, 2048, 22050
SHIFT_MAX = 1024
X_MAX = 631_000_000_000            # a chroma value stays below 2^39.2 (include/bliss_amd.h, the chroma block's bounds)
BL_OK, BL_UNEXPECTED = 0, -2
NO_SCORE = 0xFFFFFFFF

MATCH_DTYPE = np.dtype([("errors", "<u4"), ("overlap", "<u4"), ("offset", "<i4"), ("score", "<u4"), ("status", "<i4"),
                        ("reserved", "<i4")])

# the mistakes a kernel could plausibly make
SWITCHES = (
    "ge",           # >= for > in the three bit groups
    "half7",        # S1 over 7 frames
    "next_down",    # the neighbour of class k is k - 1
    "no_wrap",      # class 11's neighbour (class 0's with next_down) taken as absent: its sums read as 0
    "count16",      # W = T - 16
    "d_sign",       # b[i - d]
    "overlap_gt",   # a candidate needs n > min_overlap
    "tie_far",      # the larger shift wins a tie
    "tie_pos",      # positive before negative
    "round_score",  # s rounded to nearest instead of floored
    "full_len",     # s divides by Wa, not by n
    "pop16",        # the low half of a word counted only
)
WORD_SWITCHES = SWITCHES[:5]

_POP16 = np.array([bin(i).count("1") for i in range(1 << 16)], dtype=np.int64)


def popcount(x, low_half=False):
    """per-element population count of a uint32 array, int64"""
    x = np.asarray(x, dtype=np.uint32)
    lo = _POP16[x & np.uint32(0xFFFF)]
    return lo if low_half else lo + _POP16[x >> np.uint32(16)]


def words_count(frames, sw=frozenset()):
    return max(0, frames - (FRAMES if "count16" in sw else FRAMES - 1))


def words(X, sw=frozenset()):
    """the words of one song's chromagram X (T, 12), uint32 (W,)"""
    X = np.asarray(X, dtype=np.int64).reshape(-1, 12)
    W = words_count(X.shape[0], sw)
    if W == 0:
        return np.zeros(0, dtype=np.uint32)
    c = np.concatenate([np.zeros((1, 12), np.int64), np.cumsum(X, axis=0)])      # c[t] = sum of frames [0, t): < 2^60
    t = np.arange(W)
    s1 = c[t + (HALF - 1 if "half7" in sw else HALF)] - c[t]
    s2 = c[t + FRAMES] - c[t + HALF]
    a = s1 + s2
    shift = 1 if "next_down" in sw else -1                                       # np.roll(v, -1)[k] = v[k + 1]
    s1n, s2n, an = (np.roll(v, shift, axis=1) for v in (s1, s2, a))
    if "no_wrap" in sw:
        k = 0 if "next_down" in sw else 11
        s1n[:, k] = s2n[:, k] = an[:, k] = 0
    gt = np.greater_equal if "ge" in sw else np.greater
    bits = np.concatenate([gt(s2, s1), gt(a, an), gt(s1 + s2n, s2 + s1n)[:, :8]], axis=1)   # (W, 32)
    return (bits.astype(np.uint64) << np.arange(32, dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint32)


def words_slow(X, t):
    """word t of X in Python integers, straight from the definition"""
    X = [[int(v) for v in row] for row in np.asarray(X).reshape(-1, 12)]
    s1 = [sum(X[t + f][k] for f in range(8)) for k in range(12)]
    s2 = [sum(X[t + 8 + f][k] for f in range(8)) for k in range(12)]
    a = [s1[k] + s2[k] for k in range(12)]
    w = 0
    for k in range(12):
        n = (k + 1) % 12
        w |= int(s2[k] > s1[k]) << k
        w |= int(a[k] > a[n]) << (12 + k)
        if k < 8:
            w |= int(s1[k] + s2[n] > s2[k] + s1[n]) << (24 + k)
    return w


def words_batch(X, counts, sw=frozenset()):
    """the concatenated words of songs whose frames are concatenated in X, counts[i] frames each"""
    out, at = [], 0
    for t in counts:
        out.append(words(X[at:at + t], sw))
        at += t
    return np.concatenate(out) if out else np.zeros(0, np.uint32)


def profile(a, b, D, sw=frozenset()):
    """(e(d), n(d)) for d = -D .. D as two Python-int lists"""
    a, b = np.asarray(a, dtype=np.uint32), np.asarray(b, dtype=np.uint32)
    e, n = [], []
    for d in range(-D, D + 1):
        dd = -d if "d_sign" in sw else d
        lo, hi = max(0, -dd), min(a.size, b.size - dd)
        if hi <= lo:
            e.append(0)
            n.append(0)
            continue
        e.append(int(popcount(a[lo:hi] ^ b[lo + dd:hi + dd], "pop16" in sw).sum()))
        n.append(hi - lo)
    return e, n


def match(a, b, D, min_overlap=1, sw=frozenset()):
    """(record as a dict of Python ints, e list, n list) of one pair"""
    e, n = profile(a, b, D, sw)
    best = None
    for j, d in enumerate(range(-D, D + 1)):
        if n[j] < 1 or n[j] < min_overlap or ("overlap_gt" in sw and n[j] == min_overlap):
            continue
        den = len(a) if "full_len" in sw else n[j]
        s = (e[j] * 65536 + (den // 2 if "round_score" in sw else 0)) // den
        r = 2 * abs(d) - int(d > 0 if "tie_pos" in sw else d < 0)
        key = s * 2 ** 32 + ((2 ** 32 - 1 - r) if "tie_far" in sw else r)
        if best is None or key < best[0]:
            best = (key, e[j], n[j], d, s)
    if best is None:
        return failed(), e, n
    return dict(errors=best[1], overlap=best[2], offset=best[3], score=best[4], status=BL_OK, reserved=0), e, n


def failed():
    return dict(errors=0, overlap=0, offset=0, score=NO_SCORE, status=BL_UNEXPECTED, reserved=0)


def match_batch(words_a, counts_a, words_b, counts_b, pairs, D, min_overlap=1, sw=frozenset()):
    """(records as a MATCH_DTYPE array, the profile as uint32 (n_pairs, 2 D + 1, 2)) of a pair list over two sets of
    concatenated words; a pair with an index outside its set gets the failed record and a profile of zeros"""
    offs = [np.concatenate([[0], np.cumsum(c)]).astype(np.int64) for c in (counts_a, counts_b)]
    rec = np.zeros(len(pairs), dtype=MATCH_DTYPE)
    prof = np.zeros((len(pairs), 2 * D + 1, 2), dtype=np.uint32)
    memo = {}
    for p, (ia, ib) in enumerate(pairs):
        ia, ib = int(ia), int(ib)
        if not (0 <= ia < len(counts_a) and 0 <= ib < len(counts_b)):
            r, e, n = failed(), [0] * (2 * D + 1), [0] * (2 * D + 1)
        else:
            if (ia, ib) not in memo:
                memo[ia, ib] = match(words_a[offs[0][ia]:offs[0][ia + 1]], words_b[offs[1][ib]:offs[1][ib + 1]], D,
                                     min_overlap, sw)
            r, e, n = memo[ia, ib]
        for k in MATCH_DTYPE.names:
            rec[k][p] = r[k]
        prof[p, :, 0], prof[p, :, 1] = e, n
    return rec, prof


def ber(record):
    return record["errors"] / (32.0 * record["overlap"]) if record["status"] == BL_OK else float("nan")


# ---- inputs --------------------------------------------------------------------------------------------------------

def random_frames(seed, T, hi=1 << 30):
    """(T, 12) chroma values of a seeded generator, int64"""
    return np.random.default_rng(seed).integers(0, hi, size=(T, 12), dtype=np.int64)


def random_words(seed, W):
    return np.random.default_rng(seed).integers(0, 1 << 32, size=W, dtype=np.uint64).astype(np.uint32)


def noisy_copy(w, seed, flips_per_word=2):
    """w with a few seeded bit flips per word: a plausible re-encode"""
    rng = np.random.default_rng(seed)
    out = np.array(w, dtype=np.uint32)
    for _ in range(flips_per_word):
        out ^= (np.uint32(1) << rng.integers(0, 32, size=out.size).astype(np.uint32))
    return out


def melody(seed, seconds=40.0, amp=8000.0):
    """mono int16 melody at 22 050 Hz: seeded random notes (A3 .. G#6, a quarter to half a second long) of two
    partials under a decaying envelope"""
    rng = np.random.default_rng(seed)
    n = int(seconds * RATE)
    x = np.zeros(n)
    at = 0
    while at < n:
        dur = int(rng.integers(RATE // 4, RATE // 2))
        f = 220.0 * 2.0 ** (int(rng.integers(0, 36)) / 12.0)
        m = min(dur, n - at)
        tt = np.arange(m) / RATE
        x[at:at + m] += amp * np.exp(-3.0 * tt * RATE / dur) * (np.sin(2 * np.pi * f * tt) +
                                                               0.5 * np.sin(4 * np.pi * f * tt))
        at += dur
    return np.round(x).astype(np.int16)


def variants(x, seed):
    """the same-recording variants of the mono melody x: name -> (pcm, channels, the offset the trim should give or
    None)"""
    rng = np.random.default_rng(seed)
    x64 = x.astype(np.int64)

    def noisy(amp):
        return np.clip(x64 + rng.integers(-amp, amp + 1, size=x.size), -32768, 32767).astype(np.int16)

    stereo = np.empty(2 * x.size, dtype=np.int16)
    stereo[0::2], stereo[1::2] = x, np.round(0.6 * x64).astype(np.int16)
    return {
        "half gain": (np.round(0.5 * x64).astype(np.int16), 1, 0),
        "stereo, unequal channels": (stereo, 2, 0),
        "noise 300": (noisy(300), 1, 0),
        "noise 1000": (noisy(1000), 1, 0),
        "noise 3000": (noisy(3000), 1, 0),
        "trimmed 5 hops": (x[5 * HOP:], 1, -5),
        "trimmed 3.25 hops": (x[13 * HOP // 4:], 1, None),
        "trimmed 5.5 hops": (x[11 * HOP // 2:], 1, None),
    }
