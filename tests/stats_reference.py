"""A reference for what the analysis derives from the raw statistics of a song that is NOT the code under test — TEST
INFRASTRUCTURE, shared by tests/test_stats_reference_host.py (which proves it against the oracle and shows what each
kind of error does to it) and tests/test_gpu_stats.py (which holds k_pcm_scan, k_trim, k_song_prep, k_variance_wrap,
k_amp_finish, k_force and the stand-alone bl_mean / bl_variance to it, bit for bit).

The arithmetic follows the reference's definitions (src/helpers.c:30-49, src/amplitude_sort.c:26-79,
src/analyze.c:63-80) in numpy and Python integers: the int32 accumulator of bl_mean wraps, C's divisions truncate, every
(sample - mean)^2 of bl_variance is an int32 product that wraps, the histogram is a float that stops growing at 2^24.
Every function takes switches that make one error on purpose (the mutations of the host test); the defaults are right.

Also here: a mirror of the launch geometry of k_pcm_scan (scan_geometry), the designed songs (song_set) and the long
songs that make a single-song launch run the kernel's steady-state loop (long_songs).
"""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from tests import freq_reference

RATE = 22050
SHORTEST = 5120          # the least the entry points take
CLOSED_FORM_LIMIT = 13571   # |mean| up to which no (sample - mean)^2 leaves an int32: 32768 + 13571 = 46339 <= 46340
BL_UNEXPECTED = -2


# ---- mean and variance --------------------------------------------------------------------------------------------

def _div(a, b, floor=False):
    """C's a / b for Python integers, b > 0 (floor: the WRONG division, Python's own)"""
    return a // b if floor or a >= 0 else -(-a // b)


def _wrap32(a):
    return (a + 2 ** 31) % 2 ** 32 - 2 ** 31


def _samples(pcm):
    return np.asarray(pcm, dtype=np.int16).astype(np.int64)


def mean_wrapped(pcm, floor=False, wrap=True):
    """ref helpers.c:30-37: the int32 sum of the samples, wrapped, divided towards zero.  floor, wrap=False: the two
    WRONG forms."""
    s = _samples(pcm)
    total = int(s.sum())
    return _div(_wrap32(total) if wrap else total, s.size, floor)


def variance_closed(pcm, mean):
    """(sumsq - 2 mean sum + n mean^2) / n in exact integers: bl_variance while no square wraps"""
    s = _samples(pcm)
    return _div(int((s * s).sum()) - 2 * mean * int(s.sum()) + s.size * mean * mean, s.size)


def variance_wrapped(pcm, mean, floor=False, wrap=True, closed_form=False):
    """ref helpers.c:39-49 for any caller-given mean with |mean| <= 2^30: the sum of int32((s - mean)^2 mod 2^32) in
    exact integers, divided towards zero.  floor, wrap=False, closed_form: the WRONG forms (closed_form is right up to
    |mean| = 13 571, which is asserted here whenever it applies)."""
    mean = int(mean)
    assert abs(mean) <= 2 ** 30
    if closed_form:
        return variance_closed(pcm, mean)
    v = _samples(pcm) - mean            # |v| < 2^31: v * v fits an int64
    sq = v * v
    if wrap:
        sq &= 0xFFFFFFFF
        sq -= (sq >> 31) << 32           # the low 32 bits read as a signed int
    out = _div(int(sq.sum()), v.size, floor)
    if wrap and not floor and abs(mean) <= CLOSED_FORM_LIMIT:
        assert out == variance_closed(pcm, mean), (mean, out)
    return out


# ---- trim, amplitude, force ---------------------------------------------------------------------------------------

def trim(pcm):
    """(start, end): the first and the last non-zero sample (ref amplitude_sort.c:26-31)"""
    nz = np.flatnonzero(np.asarray(pcm))
    return int(nz[0]), int(nz[-1])


H = 4096                      # the central histogram: value v at v + 2048
PASSES = 301
INT_LO, INT_HI = 2048 - 1 - 1000, 2048 - 1 + 1000   # reference bins 32767 -+ 1000
SATURATION = 2 ** 24


def _pass(h, lo, hi):
    """bins lo..hi of one smoothing pass over the padded array h (bin i at h[i + 3]): f32 sum left to right, times
    (double)(1 / 27), stored as f32 (ref amplitude_sort.c:49-55)"""
    a, b = lo + 3, hi + 4
    acc = h[a - 3:b - 3] + np.float32(3) * h[a - 2:b - 2]
    acc = acc + np.float32(6) * h[a - 1:b - 1]
    acc = acc + np.float32(7) * h[a:b]
    acc = acc + np.float32(6) * h[a + 1:b + 1]
    acc = acc + np.float32(3) * h[a + 2:b + 2]
    acc = acc + h[a + 3:b + 3]
    return ((1. / 27.) * acc.astype(np.float64)).astype(np.float32)


def amplitude(hist, start, end, n, reach_short=None, saturate=True, saturate_before_trim=False):
    """(hist_integral, amplitude) as np.float32 from the 4096 central counts of ALL samples of a song of n samples
    trimmed to [start, end] (ref amplitude_sort.c:26-79).  The zeros outside [start, end] come off bin 2048, then every
    count stops at 2^24 (`float += 1`), then 301 passes over every bin.

    reach_short: None is the plain loop.  An integer runs the PRUNED loop of k_amp_finish instead — two buffers, pass g
    writes only the bins within reach = 3 * (300 - g) - reach_short of the integral window, the others keep what the
    buffer held two passes earlier: 0 must give the plain loop's bits, 1 and 3 are the mutations.
    saturate=False, saturate_before_trim=True: the other two mutations."""
    counts = np.array(hist, dtype=np.int64)
    assert counts.shape == (H,)
    zeros_outside = start + (n - 1 - end)
    if saturate and saturate_before_trim:
        counts = np.minimum(counts, SATURATION)
    counts[2048] -= zeros_outside
    if saturate and not saturate_before_trim:
        counts = np.minimum(counts, SATURATION)
    cur = np.zeros(H + 6, dtype=np.float32)
    cur[3:-3] = counts
    if reach_short is None:
        for _ in range(PASSES):
            cur[3:-3] = _pass(cur, 0, H - 1)
    else:
        other = np.zeros(H + 6, dtype=np.float32)
        for g in range(PASSES):
            reach = 3 * (PASSES - 1 - g) - reach_short
            lo, hi = max(INT_LO - reach, 0), min(INT_HI + reach, H - 1)
            if lo <= hi:
                other[lo + 3:hi + 4] = _pass(cur, lo, hi)
            cur, other = other, cur
    with np.errstate(divide="ignore", invalid="ignore"):
        v = cur[INT_LO + 3:INT_HI + 4] / np.float32(start - end)          # ref :62-66
        v = np.abs((v.astype(np.float64) * 100.).astype(np.float32))
        integral = np.float32(np.cumsum(v, dtype=np.float32)[-1])         # :69-71, one f32 add per bin, in order
        return integral, np.float32(np.float32(np.float32(-0.2) * integral) + np.float32(6.0))   # :79


LOUD, CALM, UNKNOWN = 0, 1, 2


def force_of(tempo, amplitude_, frequency, attack, ge=False):
    """(force as np.float32, calm_or_loud) per k_force / ref analyze.c:63-80: fmax(tempo, 0) + amplitude + frequency +
    fmax(attack, 0) added in double from the left, stored as float; LOUD if it is above 0, CALM if below, UNKNOWN
    otherwise (0 or NaN).  fmax returns the other argument for a NaN.  ge: the WRONG test, >= for >."""
    def fmax0(x):
        x = float(np.float32(x))
        return x if x > 0 else 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        rating = np.float32(np.float64(fmax0(tempo)) + np.float64(np.float32(amplitude_))
                            + np.float64(np.float32(frequency)) + np.float64(fmax0(attack)))
    loud = rating >= 0 if ge else rating > 0
    return rating, LOUD if loud else (CALM if rating < 0 else UNKNOWN)


def same_bits(a, b):
    """equal f32 bit patterns; two NaNs count as equal (a NaN's sign and payload are the machine's, not the arithmetic's)"""
    a, b = np.float32(a), np.float32(b)
    return bool((np.isnan(a) and np.isnan(b)) or a.view(np.uint32) == b.view(np.uint32))


# ---- the launch geometry of k_pcm_scan ----------------------------------------------------------------------------

STRUCTURAL = ("single_only", "paired_no_leftover", "paired_leftover", "paired_twice", "idle_block_lanes")
ALL_CLASSES = frozenset(STRUCTURAL) | frozenset(f"tail_{r}" for r in range(8))
PAIRED = frozenset(c for c in STRUCTURAL if c.startswith("paired"))


def scan_grid_x(max_n, n_songs, n_cu):
    """scan_grid_x of bl_stats_kernels.hip: grid_x_for(ceil(max_n / 8 / 256), n_songs, 8, n_cu)"""
    units = (max_n // 8 + 255) // 256
    want = max(1, (8 * n_cu + n_songs - 1) // n_songs)
    return min(max(1, min(want, units)), 65535)


def scan_geometry(n, n_songs, n_cu, max_n=None):
    """The set of classes a song of n samples reaches in k_pcm_scan when it is launched with n_songs songs of up to
    max_n (default: n) samples on n_cu compute units.  A lane starts at vector v0 = block * 256 + tid of nvec = n / 8
    and takes vectors v and v + gstride together while v + gstride < nvec, then one more if v < nvec:
        single_only         some lane loads one vector and never two together
        paired_no_leftover  some lane pairs and has nothing left
        paired_leftover     some lane pairs and then loads one more
        paired_twice        some lane runs the paired loop more than once
        idle_block_lanes    some lane has v0 >= nvec
        tail_r              r = n & 7 samples behind the last whole vector"""
    gs = 256 * scan_grid_x(n if max_n is None else max_n, n_songs, n_cu)
    nvec = n >> 3
    v0 = np.arange(gs, dtype=np.int64)
    pairs = np.maximum(0, -((v0 + gs - nvec) // (2 * gs)))     # ceil((nvec - gs - v0) / (2 gs)), at least 0
    left = v0 + 2 * gs * pairs < nvec
    out = {f"tail_{n & 7}"}
    for name, hit in (("single_only", (pairs == 0) & left), ("paired_no_leftover", (pairs > 0) & ~left),
                      ("paired_leftover", (pairs > 0) & left), ("paired_twice", pairs > 1),
                      ("idle_block_lanes", v0 >= nvec)):
        if hit.any():
            out.add(name)
    return out


# ---- the songs ----------------------------------------------------------------------------------------------------

def _ro(a):
    a = np.ascontiguousarray(a, dtype=np.int16)
    a.setflags(write=False)
    return a


def duration_of(n, channels):
    return max(1, n // (RATE * channels))


def song_with_total(n, total, rng, spread, lo=-32768, hi=32767):
    """n samples in [lo, hi], noise of +-spread around the DC level total / n, whose exact sum is `total`: single
    samples are moved by one step until it is.  The only way to put a wrapped mean exactly on a threshold."""
    dc = int(round(total / n))
    assert lo <= dc <= hi, (n, total, dc)
    s = np.clip(dc + rng.integers(-spread, spread + 1, n), lo, hi).astype(np.int64)
    d = total - int(s.sum())
    step = 1 if d > 0 else -1
    room = np.flatnonzero(s < hi if d > 0 else s > lo)
    while d:                                    # at most a few rounds: every round moves up to len(room) samples
        assert room.size, (n, total)
        take = room[:abs(d)]
        s[take] += step
        d -= step * take.size
        room = np.flatnonzero(s < hi if step > 0 else s > lo)
    assert int(s.sum()) == total and s.min() >= lo and s.max() <= hi
    return s


@functools.lru_cache(maxsize=None)
def window_share():
    """4096 f64: the share of a sample in bin b that the 301 passes leave inside the integral window — the model the
    search of zero_force_song plans with; every step of the search is then taken by amplitude(), not by this"""
    r = np.array([1.0])
    for _ in range(PASSES):
        r = np.convolve(r, np.array([1, 3, 6, 7, 6, 3, 1]) / 27.)
    c = r.size // 2
    cum = np.concatenate([[0.0], np.cumsum(r)])
    share = np.zeros(H)
    for b in range(H):
        lo, hi = max(0, c + INT_LO - b), min(r.size - 1, c + INT_HI - b)
        share[b] = cum[hi + 1] - cum[lo] if hi >= lo else 0.0
    return share


ZF_FRAMES, ZF_TAIL = 12, 500


def zero_force_song(oracle):
    """A mono song whose force is exactly 0 — calm_or_loud UNKNOWN, the one result that `>=` for `>` changes — found by
    a search, since tempo and attack are far below 0 and so amplitude == -frequency has to hold to the last bit.

    The body, 12 frames of low-passed noise, alone decides `frequency`; its level is set by bisection so that the
    amplitude comes out about 0.75 above -frequency.  The 500 samples behind the last whole frame enter no frame but do
    enter the histogram: they start outside the reach of the integral window, and are moved into it one by one (each
    takes 100 / (n - 1) * 0.2 off the amplitude), the last ones onto the window's edge where they count in part, until
    amplitude() gives -frequency exactly.  Two samples on the edge serve as verniers for a last scan if the f32
    roundings of the smoothing keep the planned steps from landing.  The search adapts to what it measures with the
    reference itself; the host test then asserts the oracle's force bits, so a search gone wrong cannot pass."""
    rng = np.random.default_rng(4400)
    nb, nt = 512 * ZF_FRAMES, ZF_TAIL
    n = nb + nt
    e = rng.standard_normal(nb + 600)
    x = np.zeros_like(e)
    for t in range(1, e.size):
        x[t] = 0.97 * x[t - 1] + e[t]
    x = x[600:] / x[600:].std()

    def song(scale, tail):
        body = np.clip(np.rint(x * scale), -32768, 32767)
        body[body == 0] = 1
        return np.concatenate([body, tail]).astype(np.int16)

    def miss(pcm):
        """amplitude + frequency, exact in f64"""
        amp = amplitude(freq_reference.statistics(pcm)[2], 0, n - 1, n)[1]
        return float(amp) + float(np.float32(oracle.frequency(pcm, 1)))

    tail = np.where(np.arange(nt) % 2 == 0, 5000, -5000)
    lo, hi = 500., 30000.
    for _ in range(14):
        scale = (lo * hi) ** .5
        lo, hi = (lo, scale) if miss(song(scale, tail)) > 0.75 else (scale, hi)
    share, per_sample = window_share(), 100.0 / (n - 1)
    verniers = (nt - 2, 1081), (nt - 3, 1091)     # the slope of the share there: about one ulp of the integral per bin
    for at, v in verniers:
        tail[at] = v
    used, d = 0, miss(song(scale, tail))
    for _ in range(60):
        need = 5 * d                              # of the integral
        if need < 4e-6:
            break
        whole = int(need / (per_sample * share[2049]))
        if whole:
            tail[used:used + whole] = 1
            used += whole
        else:                                     # the largest partial step that does not overshoot
            steps = per_sample * share[2049:]
            tail[used] = 1 + int(np.argmax(np.where(steps <= 0.999 * need, steps, -1.0)))
            used += 1
        assert used < nt - 3
        d = miss(song(scale, tail))
    if d != 0:
        for k, k2 in ((k, k2) for k in range(-40, 41) for k2 in range(-5, 6)):
            trial = tail.copy()
            trial[verniers[0][0]], trial[verniers[1][0]] = verniers[0][1] + k, verniers[1][1] + k2
            d = miss(song(scale, trial))
            if d == 0:
                tail = trial
                break
    assert d == 0, d
    return song(scale, tail)


def _song(name, pcm, channels, **flags):
    pcm = _ro(pcm)
    assert pcm.size >= SHORTEST, name
    d = dict(name=name, pcm=pcm, channels=channels, duration=duration_of(pcm.size, channels),
             var0=False, one_sample=False)
    d.update(flags)
    return d


@functools.lru_cache(maxsize=None)
def song_set(oracle):
    """The designed songs, a tuple of dicts: name, pcm (read-only int16), channels, duration, var0 (the variance is 0:
    the reference divides by it), one_sample (start == end: the amplitude is 0 / 0).  Mono and stereo, 5 120 to 300 000
    samples, every n & 7."""
    rng = np.random.default_rng(4100)
    W32 = 2 ** 32
    out = []

    def add(name, pcm, channels=None, **flags):
        out.append(_song(name, pcm, channels or 1 + len(out) % 2, **flags))

    def material(seed, n, div, dc):
        """the synthetic song of the other suites, scaled down and moved to a DC level"""
        base = oracle.synth(seed, RATE, 1 + len(out) % 2, n).astype(np.int64)
        return np.clip(np.sign(base) * (np.abs(base) // div) + dc, -32768, 32767)

    # sums that wrap: once upward to a negative mean, once downward to a positive one, twice
    add("wrap_up", material(4101, 100000, 600, 32700))            # mean about -10 250
    add("wrap_down", material(4102, 100001, 600, -32700))         # mean about +10 250
    add("wrap_twice", material(4103, 300002, 16, 30000))          # 9e9 = 2 * 2^32 + ...
    # wrapped sums with a quotient between -1 and 0 (C gives 0, a floor -1), of -1 exactly, and just below
    add("quotient_-0", song_with_total(150003, W32 - 5, rng, 300))
    add("quotient_-1", song_with_total(150004, W32 - 150004, rng, 300))
    add("quotient_-1-", song_with_total(150005, W32 - 150005 - 7, rng, 300))
    # means exactly on both sides of the closed form's limit, under a wrapped sum (the DC level has the other sign) ...
    for m, n in ((13571, 100006), (13572, 100007), (-13571, 100008), (-13572, 100009)):
        sign = 1 if m > 0 else -1
        total = m * n + sign * (n // 3) - sign * W32     # the remainder has the mean's sign: the quotient truncates to m
        add(f"wrapped_mean{m:+d}", song_with_total(n, total, rng, 200))
    # ... and without a wrap
    for m, n in ((13571, 60002), (13572, 60003), (-13571, 60004), (-13572, 60005)):
        sign = 1 if m > 0 else -1
        add(f"mean{m:+d}", song_with_total(n, m * n + sign * (n - 1), rng, 2000))
    # the floor of the range: 70 000 samples of -32768 have mean +28 588 and variance -530 408 560; a noisy one; the ceiling
    add("floor", np.full(70000, -32768))
    add("floor_noisy", -32768 + rng.integers(0, 40, 70001))
    add("ceiling", np.full(70003, 32767))
    # DC 30 000 under a sum that wraps once: mean about -16 000, every (s - mean)^2 about 46 000^2, just inside an int32
    add("large_variance", 30000 + rng.integers(-100, 101, 93368))
    # variance 0: constant, and constant but for one sample one step away
    add("constant", np.full(8195, 1234), var0=True)
    one_off = np.full(9001, -77)
    one_off[4000] = -76
    add("constant_but_one", one_off, var0=True)
    # all of the histogram at the edges of the integral window, where only an exact `reach` of the pruned loop shows
    add("edge_spikes", np.array([-1004, -1001, -998, 996, 999, 1002])[rng.integers(0, 6, 20006)])
    add("constant-1002", np.full(6001, -1002), var0=True)
    add("constant+1000", np.full(7004, 1000), var0=True)
    # all of the central histogram's mass in one bin on either side of its ends; a loud sample now and then keeps the
    # variance away from 0
    for v in (-2048, 2047, 2048, -2049):
        s = np.full(12000 + len(out), v)
        s[5::97] = 30000
        s[50::97] = -30000
        add(f"mass{v:+d}", s)
    # zeros in the middle and silence on both ends: what comes off the zero bin is neither 0 nor all of it
    z = material(4104, 44107, 8, 0)
    z[:1031] = 0
    z[-2050:] = 0
    z[20000:26000] = 0
    add("zeros_inside", z)
    # one non-zero sample: in the middle, and among the samples behind the last whole vector
    s = np.zeros(9005)
    s[4097] = 20000
    add("one_sample", s, one_sample=True)
    s = np.zeros(8199)
    s[8197] = -1500
    add("one_sample_tail", s, one_sample=True)
    # two adjacent samples: start - end == -1
    s = np.zeros(10002)
    s[5003], s[5004] = 900, -700
    add("two_samples", s)
    # force exactly 0: calm_or_loud is UNKNOWN, and LOUD if the kernel tests >= for >
    add("zero_force", zero_force_song(oracle), channels=1)
    assert 24 <= len(out) <= 40 and len({s["name"] for s in out}) == len(out)
    return tuple(out)


LONG_TAILS = (0, 1, 5, 7, 3)


@functools.lru_cache(maxsize=None)
def _long_block():
    """65 536 random samples, a third of them inside the central histogram, with runs of adjacent -32768: a packed
    word then holds two of them, the largest sum of squares a word can have"""
    rng = np.random.default_rng(4200)
    b = np.where(rng.random(65536) < 0.33, rng.integers(-2100, 2100, 65536), rng.integers(-32768, 32768, 65536))
    for at in rng.integers(0, 65536 - 8, 200):
        b[at:at + 2 + at % 5] = -32768
    b[0] = 77          # no song built from it starts with silence
    return b.astype(np.int16)


@functools.lru_cache(maxsize=None)
def long_songs(n_cu):
    """name -> read-only int16 song: what makes k_pcm_scan, launched for ONE song on n_cu compute units, run its paired
    loop.  With g = 8 * n_cu * 256 vectors (the launch's stride): 1.5 g, 2 g, 2 g + 1, 2.5 g and 3.5 g vectors plus 0,
    1, 5, 7 and 3 samples; and the two songs with more than 2^24 equal samples (see saturation_songs)."""
    g = 8 * n_cu * 256
    out = {}
    for (name, nvec), tail in zip((("1.5g", 3 * g // 2), ("2g", 2 * g), ("2g+1", 2 * g + 1), ("2.5g", 5 * g // 2),
                                   ("3.5g", 7 * g // 2)), LONG_TAILS):
        s = np.resize(_long_block(), 8 * nvec + tail).copy()
        s[-1] = -5     # nor ends with it
        out[name] = _ro(s)
    out.update(saturation_songs())
    return out


@functools.lru_cache(maxsize=None)
def saturation_songs():
    """sat_value: 2^24 + 5000 samples of value 5 between noisy ends of 2 000 samples — the count of one bin passes
    2^24.  sat_zero: 2^24 - 10 zeros in the middle of loud samples, and 2 500 zeros of silence on each end: the zero
    bin passes 2^24 raw and lies below it once the silence is taken off."""
    rng = np.random.default_rng(4300)
    ends = rng.integers(-1500, 1501, 4000)
    ends[ends == 0] = 3
    sat_value = np.concatenate([ends[:2000], np.full(2 ** 24 + 5000, 5), ends[2000:], [9, -9]])   # n & 7 == 2
    loud = rng.integers(-1500, 1501, 6004)
    loud[loud == 0] = -3
    sat_zero = np.concatenate([np.zeros(2500), loud[:3000], np.zeros(2 ** 24 - 10), loud[3000:], np.zeros(2500)])
    assert sat_value.size & 7 == 2 and sat_zero.size & 7 == 2, (sat_value.size & 7, sat_zero.size & 7)
    return {"sat_value": _ro(sat_value), "sat_zero": _ro(sat_zero)}


# ---- the expected values, computed once ---------------------------------------------------------------------------

def expected(pcm):
    """dict of what the reference's definitions give for one song: start, end, mean, variance, status, hist_integral,
    amplitude (np.float32), sum, sumsq, hist"""
    total, sumsq, hist = freq_reference.statistics(pcm)
    start, end = trim(pcm)
    mean = mean_wrapped(pcm)
    variance = variance_wrapped(pcm, mean)
    integral, amp = amplitude(hist, start, end, len(pcm))
    hist.setflags(write=False)
    return dict(start=start, end=end, mean=mean, variance=variance, status=BL_UNEXPECTED if variance == 0 else 0,
                hist_integral=integral, amplitude=amp, sum=total, sumsq=sumsq, hist=hist)


@functools.lru_cache(maxsize=None)
def reference(oracle):
    """name -> (expected(pcm), the oracle's full record) of every designed song, computed once per process"""
    songs = song_set(oracle)
    oracle.analyze(songs[0]["pcm"], songs[0]["channels"], 1)   # the oracle's tables are built by its first call

    def one(sg):
        with np.errstate(all="ignore"):
            return expected(sg["pcm"]), oracle.analyze(sg["pcm"], sg["channels"], sg["duration"])
    with ThreadPoolExecutor(8) as pool:
        return dict(zip((s["name"] for s in songs), pool.map(one, songs)))
