"""The tempo of include/bliss_amd.h (bl_amd_song_rhythm) restated in numpy int64 and Python ints: stages 1 to 8 exactly
as the header defines them, with math.isqrt for the root.  Every intermediate stays below 2^60 (the header's bounds), so
int64 holds it exactly; np.correlate on int64 stays in integers.

The switches make, on purpose, the mistakes a kernel is likely to make (as tests/stats_reference.py does for the
statistics): tests/test_rhythm_reference_host.py shows that each of them changes a named song of the GPU test's
corpus, so tests/test_gpu_rhythm.py would catch a kernel that made it.

    trunc32            m^2 kept to 32 bits (m = -65536 squares to 0)
    across_start       d[0] = m[0] - m_before instead of 0: the difference taken across the song's start
    forget_at          a window that forgets the hops in front of hop `forget_at` (a run boundary of the hop pass)
    float_isqrt        the root by float32 rounding
    float_acf          R accumulated in float64
    lag_terms          the number of terms depending on the lag (H - tau instead of T)
    argmax             the pick as the plain arg-max
"""
import math

import numpy as np

HOP, LAGS = 128, 512
FIELDS = ("r0", "r_prev", "r_lag", "r_next", "r_peak", "onset_sum", "onset_max", "hops", "terms", "lag", "lag_peak",
          "status")
BL_OK, BL_UNEXPECTED = 0, -2


def hops_of(n_samples, channels):
    return (n_samples // channels) // HOP


def mix(pcm, channels):
    """m over the song's 128 H whole frames, int64"""
    H = hops_of(pcm.size, channels)
    x = np.asarray(pcm[:H * HOP * channels], dtype=np.int64)
    return x[0::2] + x[1::2] if channels == 2 else 2 * x


def _isqrt(x, float_isqrt):
    return int(np.sqrt(np.float32(x))) if float_isqrt else math.isqrt(x)


def novelty(pcm, channels, trunc32=False, across_start=None, forget_at=None, float_isqrt=False):
    """(n, a, b, A, B) per hop, lists of Python ints / int64 arrays (stages 1 to 4)"""
    m = mix(pcm, channels)
    H = m.size // HOP
    d = np.zeros_like(m)
    d[1:] = m[1:] - m[:-1]
    if across_start is not None:
        d[0] = m[0] - across_start
    sq = m * m
    if trunc32:
        sq &= 0xFFFFFFFF
    A = sq.reshape(H, HOP).sum(axis=1)
    B = (d * d).reshape(H, HOP).sum(axis=1)

    def amplitudes(E):
        out = []
        for h in range(H):
            lo = max(h - 3, 0)
            if forget_at is not None and h >= forget_at:
                lo = max(lo, forget_at)
            out.append(_isqrt(int(E[lo:h + 1].sum()) >> 9, float_isqrt))
        return out
    a, b = amplitudes(A), amplitudes(B)
    n = [0] + [max(0, a[h] - a[h - 1]) + max(0, b[h] - b[h - 1]) for h in range(1, H)]
    return n, a, b, A, B


def onsets_from_novelty(n):
    """stages 5 and 6: the onset curve o as an int64 array"""
    H = len(n)
    pad = np.zeros(H + 16, dtype=np.int64)
    pad[8:8 + H] = n
    local = np.zeros(H, dtype=np.int64)
    for k in range(16):                      # n_{h-8} .. n_{h+7}
        local += pad[k:k + H]
    q = np.maximum(0, 16 * pad[8:8 + H] - local) >> 4
    qp = np.zeros(H + 2, dtype=np.int64)
    qp[1:1 + H] = q
    return (qp[0:H] + 2 * qp[1:1 + H] + qp[2:2 + H]) >> 2


def onsets(pcm, channels, **switches):
    return onsets_from_novelty(novelty(pcm, channels, **switches)[0])


def lag_products(o, float_acf=False, lag_terms=False):
    """R[0 .. 511] as a list of Python ints; all 0 for H < 512"""
    o = np.asarray(o, dtype=np.int64)
    H = o.size
    T = H - (LAGS - 1)
    if T <= 0:
        return [0] * LAGS
    if lag_terms:
        return [int(np.dot(o[:H - t], o[t:])) for t in range(LAGS)]
    if float_acf:
        f = o.astype(np.float64)
        return [int(np.dot(f[:T], f[t:t + T])) for t in range(LAGS)]
    R = np.correlate(o, o[:T], mode="valid")
    assert R.dtype == np.int64 and R.size == LAGS
    return [int(x) for x in R]


def pick(R, lag_min, lag_max, argmax=False):
    """(lag, lag_peak, r_peak) of stage 8"""
    r_peak = max(R[lag_min:lag_max + 1])
    lag_peak = next(t for t in range(lag_min, lag_max + 1) if R[t] == r_peak)
    if r_peak == 0:
        return 0, 0, 0
    if argmax:
        return lag_peak, lag_peak, r_peak
    for t in range(lag_min, lag_max + 1):
        if R[t] >= R[t - 1] and R[t] >= R[t + 1] and 16 * R[t] >= 15 * r_peak:
            return t, lag_peak, r_peak
    return lag_peak, lag_peak, r_peak


def record_from_onsets(o, lag_min, lag_max, float_acf=False, lag_terms=False, argmax=False):
    """(record dict, R) of a curve: stages 7 and 8, and the record's conventions for a short song"""
    o = np.asarray(o, dtype=np.int64)
    H = int(o.size)
    if H < LAGS:
        rec = dict.fromkeys(FIELDS, 0)
        rec.update(hops=H, status=BL_UNEXPECTED)
        return rec, [0] * LAGS
    R = lag_products(o, float_acf=float_acf, lag_terms=lag_terms)
    lag, lag_peak, r_peak = pick(R, lag_min, lag_max, argmax=argmax)
    rec = dict(r0=R[0], r_prev=R[lag - 1] if lag else 0, r_lag=R[lag] if lag else 0, r_next=R[lag + 1] if lag else 0,
               r_peak=r_peak, onset_sum=int(o.sum()), onset_max=int(o.max()), hops=H, terms=H - (LAGS - 1), lag=lag,
               lag_peak=lag_peak, status=BL_OK)
    return rec, R


def song(pcm, channels, lag_min, lag_max, **switches):
    """(record dict, onset curve as int64 array, R as a list) of one song"""
    acf_kw = {k: switches.pop(k) for k in ("float_acf", "lag_terms", "argmax") if k in switches}
    o = onsets(pcm, channels, **switches)
    rec, R = record_from_onsets(o, lag_min, lag_max, **acf_kw)
    return rec, o, R


def bpm(rec, rate=22050):
    """bl_amd_rhythm_bpm as the header words it, in Python floats (doubles)"""
    if rec["lag"] == 0:
        return math.nan
    p, c, n = float(rec["r_prev"]), float(rec["r_lag"]), float(rec["r_next"])
    den = p - 2.0 * c + n
    delta = 0.5 * (p - n) / den if den < 0 and c >= p and c >= n else 0.0
    delta = min(0.5, max(-0.5, delta))
    return 60.0 * rate / (HOP * (rec["lag"] + delta))


def strength(rec):
    return float(rec["r_lag"]) / float(rec["r0"]) if rec["r0"] else 0.0


# ---- the material of the tests -------------------------------------------------------------------------------------

def click_track(period, hops, channels, seed):
    """a click every `period` hops over two sine tones and noise"""
    rng = np.random.default_rng(seed)
    F = hops * HOP
    t = np.arange(F)
    x = 1500.0 * np.sin(2 * np.pi * 220.0 * t / 22050) + 900.0 * np.sin(2 * np.pi * 331.0 * t / 22050)
    x += rng.normal(0.0, 300.0, F)
    for at in range(period * HOP // 2, F - 400, period * HOP):
        x[at:at + 400] += 14000.0 * np.exp(-np.arange(400) / 60.0) * rng.choice([-1.0, 1.0], 400)
    mono = np.clip(np.rint(x), -32768, 32767).astype(np.int16)
    if channels == 1:
        return mono
    st = np.empty(2 * F, np.int16)
    st[0::2] = mono
    st[1::2] = np.clip(np.rint(0.7 * x + rng.normal(0.0, 200.0, F)), -32768, 32767).astype(np.int16)
    return st


CLICKS = ((43, 1100, 1), (86, 1400, 2), (130, 1700, 1), (200, 2000, 2))   # (period, hops, channels)
SHAPES = (1, 3, 4, 19, 511, 512, 513, 640, 1023, 1024, 1500)              # H: 511 is short, 512 has T = 1
LOUDNESS = (30, 1000, 12000, 32767)
DC = (1, -1, 3, -3, 12345, 32767, -32768)
LAG_MIN, LAG_MAX = 20, 450      # the range the corpus is picked over: 517 down to 23 bpm at 22 050 Hz
ARENA_FILL = 32767              # what the GPU test puts around the songs
LONG_HOPS = 40000


def dual_mono(pcm):
    return np.repeat(pcm, 2)


def corpus():
    """name -> (pcm, channels): the songs of tests/test_gpu_rhythm.py, in a fixed order.  Frame counts that are no
    multiple of 128 and, for stereo, odd sample counts are spread over the shapes."""
    rng = np.random.default_rng(7100)
    songs = {}
    for k, H in enumerate(SHAPES):
        for ch in (1, 2):
            extra = (0, 5, 127)[(k + ch) % 3] * ch + (ch == 2 and k % 2)
            amp = LOUDNESS[(k + ch) % 4]
            songs[f"noise_H{H}_{ch}ch"] = (rng.integers(-amp, amp + 1, H * HOP * ch + extra).astype(np.int16), ch)
    for period, hops, ch in CLICKS:
        songs[f"click_{period}"] = (click_track(period, hops, ch, seed=period), ch)
    for k, c in enumerate(DC):
        ch = 1 + k % 2
        songs[f"dc_{c}"] = (np.full(600 * HOP * ch + 3, c, np.int16), ch)
    songs["all_min_stereo"] = (np.full(520 * HOP * 2, -32768, np.int16), 2)
    nyq = np.tile(np.array([32767, -32768], np.int16), 700 * HOP // 2)
    nyq.reshape(700, HOP)[0::2] = 0          # hops alternate between silence and full-scale Nyquist
    songs["nyquist_hops"] = (nyq, 1)
    songs["nyquist_hops_stereo"] = (dual_mono(nyq), 2)
    songs["silence"] = (np.zeros(600 * HOP + 77, np.int16), 1)
    late = np.zeros(1500 * HOP * 2, np.int16)
    late[-600 * HOP * 2:] = rng.integers(-9000, 9001, 600 * HOP * 2)
    songs["late"] = (late, 2)
    return songs


def long_song(channels):
    """LONG_HOPS hops: noise whose loudness steps every 37 hops, so the onset curve is busy along the whole song"""
    rng = np.random.default_rng(7200 + channels)
    F = LONG_HOPS * HOP
    env = np.repeat(rng.integers(200, 30000, F // (37 * HOP) + 1), 37 * HOP)[:F].astype(np.float64)
    x = np.rint(rng.uniform(-1.0, 1.0, F * channels) * np.repeat(env, channels))
    return np.clip(x, -32768, 32767).astype(np.int16)


def big_curve():
    """140 000 values random in [2^17, 2^18), drawn so that every R[tau] passes 2^53, where a float64 accumulator
    starts to round and a 32-bit one has long wrapped.  139 489 products of values spread evenly over that range would
    stop at 5.6e15 < 2^53 = 9.0e15 (the largest R possible is 9.6e15), so fifteen values of sixteen lie in the top
    4 096 of the range and every sixteenth anywhere in it: R is about 9.15e15."""
    rng = np.random.default_rng(7300)
    o = rng.integers((1 << 18) - (1 << 12), 1 << 18, 140000)
    o[::16] = rng.integers(1 << 17, 1 << 18, o[::16].size)
    return o.astype(np.uint32)
