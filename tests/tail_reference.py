"""Array-form restatement of parts 2 and 3 of the envelope analysis — TEST INFRASTRUCTURE.

What oracle/bliss_oracle.c:194-251 does after the window energies, written again in numpy f64 with the arrays
t1, t2, wa, ss materialised: log compression, zero stuffing, the 6th-order recurrence, the onset difference, the
weighting, atk_sum, two box filters of width 19 that keep the destination's old edge cells, the peak count, tempo and
attack.  Not the streaming form of bliss_amd/csrc/bl_tail.h and not derived from it: the GPU tail is compared with
this, and this with the oracle (tests/test_tail_reference_host.py, bit for bit).

Every operation keeps the oracle's order and rounding; songs are vectorised elementwise (one array column per step j,
one row per song, rows padded with zeros past their own N — every quantity at step j depends on earlier or own-row
cells only), nothing is reassociated.
"""
import math

import numpy as np

BOX = 19
HALF = 10   # (int)round(19 / 2.)
BUT_B = (1.9510e-05, 1.1706e-04, 2.9266e-04, 3.9021e-04, 2.9266e-04, 1.1706e-04, 1.9510e-05)
BUT_A = (1.00000, -4.59007, 8.91034, -9.34191, 5.56998, -1.78845, 0.24136)
LAMBDA = np.float32(0.8)
ONE_MINUS_LAMBDA = float(np.float32(1) - LAMBDA)        # f32, widened
LAMBDA_172 = float(LAMBDA * np.float32(172))            # f32, widened
EPSILON = float(np.float32(0.000001))
MU = float(np.float32(100.0))
LOG_1_MU = math.log(float(np.float32(1) + np.float32(100.0)))


def compress(energies):
    """log(1 + mu f) / log(1 + mu) with the C library's log, one window energy (f32) at a time"""
    return np.array([math.log(1 + MU * float(f)) / LOG_1_MU for f in np.asarray(energies, dtype=np.float32)],
                    dtype=np.float64)


def nb_frames_of(n_samples):
    return (n_samples - n_samples % 512) * 2 // 512


def _box(old, inp, n):
    """orc_rect_filter(out, in, N, 19) for rows of different N (n: column vector); old: the destination's contents"""
    rows, width = inp.shape
    col = np.arange(width)[None, :]
    run = np.zeros(rows)
    for k in range(BOX):
        run = run + inp[:, k]
    mid = np.zeros_like(inp)
    for k in range(width - BOX):
        mid[:, k + HALF - 1] = run
        run = run - inp[:, k]
        run = run + inp[:, k + BOX]
    out = np.where((col >= HALF - 1) & (col <= n - HALF - 1), mid, old)
    last = np.take_along_axis(inp, n + np.arange(-BOX, 0)[None, :], axis=1)
    acc = np.take_along_axis(old, n - HALF, axis=1)[:, 0]
    for k in range(BOX):
        acc = acc + last[:, k]
    np.put_along_axis(out, n - HALF, acc[:, None], axis=1)
    return np.where(col < n, out / BOX, 0.0)


def tail_reference(n_samples, durations, energies=None, x=None):
    """Parts 2-3 for a list of songs.  Per song either `energies` (f32 window energies) or `x` (the compressed
    envelope) with at least n_windows = nb_frames - 2 values; whatever follows them is never read (the oracle's
    filtered_array is zero there).  Returns a dict of per-song arrays beat, atk_sum (f64), tempo, attack (f32),
    nb_frames, n_windows, margin (the oracle's min_peak_margin) and the list `peaks` of peak positions j."""
    assert (energies is None) != (x is None)
    n_samples = np.asarray(n_samples, dtype=np.int64)
    rows = len(n_samples)
    nbf = np.array([nb_frames_of(int(v)) for v in n_samples], dtype=np.int64)
    n = (2 * nbf)[:, None]
    assert n.min() >= 2 * BOX + 2
    width = int(n.max())
    col = np.arange(width)[None, :]
    t1 = np.zeros((rows, width))
    for i in range(rows):
        nw = int(nbf[i]) - 2
        src = compress(energies[i][:nw]) if x is None else np.asarray(x[i], dtype=np.float64)[:nw]
        assert src.size == nw and np.all(np.isfinite(src))
        t1[i, 0:2 * nw:2] = src
    # the recurrence
    t2 = np.zeros((rows, width))
    xr = [np.zeros(rows) for _ in range(7)]
    yr = [np.zeros(rows) for _ in range(7)]
    y = np.zeros(rows)
    for j in range(width):
        xr = [t1[:, j]] + xr[:6]
        yr = [y] + yr[:6]
        d = np.zeros(rows)
        c = np.zeros(rows)
        for k in range(7):
            d = d + BUT_B[k] * xr[k]
        for k in range(1, 7):
            c = c + BUT_A[k] * yr[k - 1]
        y = (d - c) / BUT_A[0]
        t2[:, j] = y
    # onset difference, weighting
    dj = t2[:, 1:] - t2[:, :-1]
    t1 = np.concatenate([t2[:, :1], np.where(dj > 0, dj, 0.0)], axis=1)
    wa = ONE_MINUS_LAMBDA * t2 + LAMBDA_172 * t1 / 10
    wa = np.where(col < n, wa, 0.0)
    ss = np.where(col < n - 1, 0.0 + wa, 0.0)
    atk_sum = np.take_along_axis(np.cumsum(ss, axis=1), n - 2, axis=1)[:, 0]   # cumsum adds in index order
    # box filters: the first writes over wa (old edge cells stay), the second over zeros
    wa = _box(wa, ss, n)
    ss = _box(np.zeros_like(wa), wa, n)
    # peaks
    dl = ss[:, 1:-1] - ss[:, :-2]
    dr = ss[:, 1:-1] - ss[:, 2:]
    inside = col[:, 1:-1] <= n - 2
    is_peak = inside & (dl > EPSILON) & (dr > EPSILON)
    beat = is_peak.sum(axis=1)
    m = np.where(is_peak, np.minimum(dl, dr) - EPSILON,
                 np.where(dl > EPSILON, EPSILON - dr,
                          np.where(dr > EPSILON, EPSILON - dl, np.maximum(EPSILON - dl, EPSILON - dr))))
    m = np.where(inside & ~((dl == 0) & (dr == 0)), m, 1e300)
    margin = m.min(axis=1)
    peaks = [np.nonzero(is_peak[i])[0] + 1 for i in range(rows)]
    dur = np.asarray(durations, dtype=np.uint64).astype(np.float32)
    tempo = ((np.float32(4) * beat.astype(np.float32) / dur).astype(np.float64) - 30.4).astype(np.float32)
    attack = attack_of(atk_sum, n_samples)
    return dict(beat=beat.astype(np.int64), atk_sum=atk_sum, tempo=tempo, attack=attack, nb_frames=nbf,
                n_windows=nbf - 2, margin=margin, peaks=peaks)


def attack_of(atk_sum, n_samples):
    """-1.74 * atk_sum * 10000 / n + 58.3 in f64, rounded to f32"""
    return (-1.74 * np.asarray(atk_sum, dtype=np.float64) * 10000 / np.asarray(n_samples, dtype=np.int64)
            + 58.3).astype(np.float32)


# ---- the songs of the sweeps ---------------------------------------------------------------------------------------

SWEEP_M = range(10, 125)   # floor(n / 512): two periods (57) of (N mod 38, n_blocks mod 6)


def sweep_lengths(seed=20240):
    """one n per m of SWEEP_M with a varying n % 512"""
    rng = np.random.default_rng(seed)
    return [512 * m + int(r) for m, r in zip(SWEEP_M, rng.integers(0, 512, len(SWEEP_M)))]


def sweep_duration(n):
    return 1 + (n // 512) % 7


def bursty_song(n, seed):
    """int16 noise gated at a period of 2200-5200 samples over a quiet noise floor: 1-13 beats in these lengths where
    the synthetic generator gives 1-5"""
    rng = np.random.default_rng([seed, n])
    period = int(rng.integers(2200, 5201))
    duty = rng.uniform(0.15, 0.5)
    phase = int(rng.integers(0, period))
    t = np.arange(n)
    gate = ((t + phase) % period) < duty * period
    loud = rng.integers(-12000, 12001, n)
    floor = rng.integers(-40, 41, n)
    return np.where(gate, loud, floor).astype(np.int16)
