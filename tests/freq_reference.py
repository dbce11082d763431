"""A reference for the frequency pass and the statistics that ride along with it that is NOT the code under test —
TEST INFRASTRUCTURE, shared by tests/test_freq_reference_host.py (which proves it against the oracle and shows what
each kind of error does to it) and tests/test_gpu_freq_spectrum.py (which holds the kernels to it, bit for bit).

oracle/bliss_oracle.c:83-125 (orc_frequency) restated per bin in numpy f32, one rounding per C operation: the window,
the stereo average, the transform (orc_rdft512_f32 through ctypes, frame by frame), re*re and im*im rounded separately
and added, the frames added one after the other into f32; then the finish (square root, peak, dB, bands).  The
statistics are exact integers.  Also here: the song set of the two tests, the smallest shapes that reach every edge of
the kernels' frame loop.
"""
import functools
import math

import numpy as np

W = 512
RATE = 22050
PLANTED = (-32768, -2049, -2048, 2047, 2048, 32767)   # the ends of the 16-bit range and of the central histogram


@functools.lru_cache(maxsize=None)
def hann():
    """oracle/bliss_oracle.c:86-87: .5f * (1.0f - cos(2 pi i / 511)) in double (libm's cos), rounded to f32"""
    return np.array([0.5 * (1.0 - math.cos(2 * math.pi * i / (W - 1))) for i in range(W)], dtype=np.float32)


def windowed_frames(pcm, channels, floor_average=False):
    """(n_frames, 512) f32: the transform's input (oracle :89-97).  Stereo: int add, C's truncating / 2, f32 multiply.
    floor_average: the WRONG average, an arithmetic shift (the mutation of the host test)."""
    pcm = np.asarray(pcm, dtype=np.int16)
    n_frames = (pcm.size // channels) // W
    s = pcm[:n_frames * W * channels].astype(np.int32)
    if channels == 2:
        s = s[0::2] + s[1::2]
        s = (s >> 1) if floor_average else (s + (s < 0)) >> 1   # trunc(s / 2) = floor((s + [s < 0]) / 2)
    return s.astype(np.float32).reshape(n_frames, W) * hann()[None, :]


def transform(oracle, x):
    """every row through orc_rdft512_f32, in place; returns x"""
    assert x.dtype == np.float32 and x.flags.c_contiguous and x.shape[1] == W
    for f in range(x.shape[0]):
        oracle.rdft512_f32(x[f])
    return x


def frame_power(x, contracted=False):
    """(n_frames, 256) f32: re*re + im*im of bins 0..255 of every transformed frame (oracle :100-104), the products
    rounded separately.  Column 0 is set to 0: the reference overwrites ps[0] and never reads it.
    contracted: the WRONG form, one rounding of the exact re*re + im*im (what a fused multiply-add gives, up to the
    double rounding through f64)."""
    re, im = x[:, 0::2], x[:, 1::2]
    if contracted:
        p = (re.astype(np.float64) * re.astype(np.float64) + im.astype(np.float64) * im.astype(np.float64)).astype(np.float32)
    else:
        p = (re * re) + (im * im)
    p = np.ascontiguousarray(p, dtype=np.float32)
    p[:, 0] = 0
    return p


def accumulate(power, order=None):
    """256 f32: the frames' power values added one after the other into f32 (oracle :103), in frame order or in
    `order`, a sequence of frame indices (a frame may be missing or appear twice: the mutations)"""
    ps = np.zeros(power.shape[1], dtype=np.float32)
    for f in (range(power.shape[0]) if order is None else order):
        ps = ps + power[f]
    return ps


def finish(ps):
    """(frequency, peak) as np.float32 from the 256 summed power values (oracle :106-124; bin 0 is not read and
    ps[256] stays 0, which cannot be the peak)"""
    ps = np.asarray(ps, dtype=np.float32)
    amp = np.zeros(257, dtype=np.float32)
    amp[1:256] = np.sqrt((ps[1:256] / np.float32(W)).astype(np.float64)).astype(np.float32)
    peak = np.float32(amp[1:].max())
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = (amp / peak).astype(np.float32)
    db = np.array([20 * math.log10(float(r)) - 3 if r > 0 else (-math.inf if r == 0 else math.nan) for r in ratio],
                  dtype=np.float64).astype(np.float32)

    def run(lo, hi):   # f32 sum in index order, from 0
        acc = np.float32(0)
        for i in range(lo, hi + 1):
            acc = np.float32(acc + db[i])
        return acc
    b0 = np.float32(np.float32(db[2] + db[4]) / np.float32(2))
    b1 = np.float32(np.float32(db[6] + db[8]) / np.float32(2))
    b2 = np.float32(run(10, 60) / np.float32(50))
    b3 = np.float32(run(61, 118) / np.float32(57))
    b4 = np.float32(run(119, 234) / np.float32(115))
    total = np.float32(np.float32(np.float32(np.float32(b4 + b3) + b2) - b0) - b1)
    return np.float32((1. / 3.) * float(total) + 68. / 3.), peak


def statistics(pcm):
    """(sum, sum of squares, 4096 counts) of ALL samples, exact: the histogram counts s in [-2048, 2048) at s + 2048"""
    s = np.asarray(pcm, dtype=np.int16).astype(np.int64)
    central = s[(s >= -2048) & (s < 2048)]
    return int(s.sum()), int((s * s).sum()), np.bincount(central + 2048, minlength=4096).astype(np.int64)


def mean_variance(total, sumsq, n):
    """(mean, variance) the way the reference derives them (oracle :18-33): the int32 accumulator wraps, C's
    truncating divisions; the variance in exact integers, valid while (sample - mean)^2 fits an int32"""
    def trunc_div(a, b):
        return abs(a) // b * (1 if a >= 0 else -1)
    wrapped = (total + 2 ** 31) % 2 ** 32 - 2 ** 31
    mean = trunc_div(wrapped, n)
    assert abs(mean) <= 13571
    return mean, trunc_div(sumsq - 2 * mean * total + n * mean * mean, n)


def hist_integral(hist, start, end, n):
    """np.float32: the integral of the 301 times smoothed histogram around the zero bin (oracle :42-79) from the 4096
    central counts of ALL samples.  The zeros outside [start, end] come off bin 2048 first, in integers; then every
    count stops at 2^24, where the reference's `float += 1` stops growing.  301 passes of a +-3 stencil reach 903 bins,
    so neither the bins outside the central 4096 nor the array's ends can reach the window of +-1000."""
    counts = np.array(hist, dtype=np.int64)
    counts[2048] -= start + (n - 1 - end)
    h = np.zeros(4096 + 6, dtype=np.float32)
    h[3:-3] = np.minimum(counts, 2 ** 24)
    third = np.float32(3)
    for _ in range(301):
        acc = h[0:-6] + third * h[1:-5]
        acc = acc + np.float32(6) * h[2:-4]
        acc = acc + np.float32(7) * h[3:-3]
        acc = acc + np.float32(6) * h[4:-2]
        acc = acc + third * h[5:-1]
        acc = acc + h[6:]
        s = ((1. / 27.) * acc.astype(np.float64)).astype(np.float32)
        h[3:-3] = s
    lo = 3 + 2048 - 1 - 1000   # reference bins 32767 - 1000 .. 32767 + 1000; local bin of value v is v + 2048
    with np.errstate(divide="ignore", invalid="ignore"):   # start == end: the reference divides by 0
        v = h[lo:lo + 2001] / np.float32(start - end)
        v = np.abs((v.astype(np.float64) * 100.).astype(np.float32))
        return np.float32(np.cumsum(v, dtype=np.float32)[-1])


# ---- the song set -------------------------------------------------------------------------------------------------

def _extras(count, channels):
    """`count` different numbers of samples behind the last whole frame, the edges first"""
    span = W * channels
    out = [0, 1, 7, span - 1]
    k = 0
    while len(out) < count:
        e = (k * 37 + 11) % span
        k += 1
        if e not in out:
            out.append(e)
    return out


_GAIN = (1024, 981, 939, 899, 861, 825, 790, 756, 724, 693, 664, 636, 609, 583, 558, 535)   # ~1024 * 2^(-j / 16)


def make_song(oracle, seed, channels, n_frames, extra, dc):
    """Analysable material, mostly inside the central histogram, whose level rises by six binades from the first frame
    to the last, with the edge values of both ranges planted in the last whole frame, the one before it and the
    samples behind it.

    The rise is what lets the ORDER of the f32 adds show in the sum's bits.  (S + a) + b and (S + b) + a differ only
    in the bins whose running sum S changes binade on the way, and the one-ulp difference then has to survive every
    later add: with frames of one level a swap in a song of a hundred frames moves a handful of bins at best, and with a
    level cycling up and down (tried first) the swap of two quiet frames moves none.  With the power growing by 2^12
    over the song the last frames are each comparable to the whole sum before them (about n / 8 frames' worth), so the
    order of the last frames and blocks shows in tens of bins of every song, and since n_frames takes every value the
    last frames fall on every wave and lane group of the kernels.

    The planted values stand at the start of a frame, where the window is ~0: they reach the statistics in full and
    leave the spectrum the material's."""
    n = n_frames * W * channels + extra
    base = oracle.synth(seed, RATE, channels, n).astype(np.int64)
    frame_of = np.minimum(np.arange(n) // (W * channels), n_frames - 1)   # the samples behind: the last frame's level
    sixteenths = (96 * (n_frames - 1 - frame_of)) // (n_frames - 1)      # 0 .. 96 sixteenths of a binade below full level
    gain = np.array(_GAIN, dtype=np.int64)[sixteenths % 16]
    div = (8 * 1024) << (sixteenths // 16)
    pcm = np.sign(base) * (np.abs(base) * gain // div) + dc               # truncating division, as C's
    for at in ((n_frames - 1) * W * channels, (n_frames - 2) * W * channels, n_frames * W * channels):
        k = max(0, min(len(PLANTED), n - at))
        pcm[at:at + k] = PLANTED[:k]
    assert pcm.min() >= -32768 and pcm.max() <= 32767
    return pcm.astype(np.int16)


def duration_of(pcm, channels):
    return max(1, pcm.size // (RATE * channels))


@functools.lru_cache(maxsize=None)
def song_set(oracle):
    """Stereo songs of every n_frames in 5..136 and mono songs of every n_frames in 10..136 (5120 samples is the least
    the entry points take), in a fixed shuffled order: every remainder of the 64-frame iteration of k_freq_scan twice
    and of the 32-frame one of k_freq_frames four times, one to three (five) iterations, every count of live frames in
    every wave, waves and lane groups with no live frame, odd and even counts.  Every song has its own number of
    samples behind the last frame.  Returns a tuple of dicts: pcm, channels, n_frames, extra, duration."""
    songs = []
    for channels, first in ((2, 5), (1, 10)):
        counts = list(range(first, 137))
        for n_frames, extra in zip(counts, _extras(len(counts), channels)):
            songs.append((channels, n_frames, extra))
    order = np.random.default_rng(20).permutation(len(songs))
    out = []
    for i, j in enumerate(order):
        channels, n_frames, extra = songs[j]
        pcm = make_song(oracle, 30000 + i, channels, n_frames, extra, 200 + 25 * (i % 9))
        pcm.setflags(write=False)
        out.append(dict(pcm=pcm, channels=channels, n_frames=n_frames, extra=extra,
                        duration=duration_of(pcm, channels)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def equal_length_set(oracle):
    """Eight songs of one length, mono and stereo: a batch the runtime leaves in the caller's order"""
    n = 40 * W * 2 + 6
    out = []
    for i in range(8):
        channels = 2 - i % 2
        n_frames = (n // channels) // W
        pcm = make_song(oracle, 31000 + i, channels, n_frames, n - n_frames * W * channels, 250 + 10 * i)
        pcm.setflags(write=False)
        out.append(dict(pcm=pcm, channels=channels, n_frames=n_frames, extra=n - n_frames * W * channels,
                        duration=duration_of(pcm, channels)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def reference(oracle, which="main"):
    """Per song of song_set (or equal_length_set with which="equal"): (spectrum (256,) f32, sum, sumsq, hist) —
    computed once per process and shared; the arrays are read-only"""
    out = []
    for sg in (song_set(oracle) if which == "main" else equal_length_set(oracle)):
        ps = accumulate(frame_power(transform(oracle, windowed_frames(sg["pcm"], sg["channels"]))))
        ps.setflags(write=False)
        total, sumsq, hist = statistics(sg["pcm"])
        hist.setflags(write=False)
        out.append((ps, total, sumsq, hist))
    return tuple(out)
