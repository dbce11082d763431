"""A reference for the mel call (include/bliss_amd.h: bl_amd_frame_mel, bl_amd_song_mel, the band levels) that is NOT
the code under test — TEST INFRASTRUCTURE, shared by tests/test_mel_reference_host.py (which runs it on designed spectra
and shows what each kind of error does to it) and tests/test_gpu_mel.py (which holds the kernel to it with ==).

The definitions of the header restated in Python ints on top of tests/timbre_reference.py's power_of and sixteenths (the
per-frame power values the frequency kernels are already held to, bit for bit).  The band edges are recomputed from the
mel formula in double, the weights and the cosine table are rebuilt from the definitions, none of them read from
bl_mel_table.h.  Nothing here can overflow: Python ints, and every S, T and song sum is asserted to stay below 2^63.

The keyword switches (SWITCHES) are the WRONG forms, the mutations of the host test; all default to the right one.
"""
import functools
import math

import numpy as np

from tests import chroma_reference as cr
from tests import timbre_reference as tr

BANDS, COEFFS, RATE, NFFT = 32, 13, 22050.0, 512
LIMIT = 1 << 63
SWITCHES = ("closed_left", "round_w", "no_plus1", "iters11", "norm31", "even_dct", "trunc_shift", "bands31",
            "strict_used")
EDGES = (16, 40, 66, 95, 126, 159, 196, 236, 279, 326, 377, 432, 493, 558, 630, 707, 792, 883, 983, 1091, 1209, 1337,
         1477, 1628, 1793, 1972, 2166, 2378, 2608, 2858, 3130, 3425, 3747, 4096)   # the header's literals, to compare with


# ---- the tables --------------------------------------------------------------------------------------------------

def edges_exact():
    """the 34 edges before rounding, in sixteenths of a bin: equally spaced in mel from bin 1 to bin 256"""
    def mel(f):
        return 2595.0 * math.log10(1.0 + f / 700.0)
    lo, hi = mel(1 * RATE / NFFT), mel(256 * RATE / NFFT)
    out = []
    for i in range(BANDS + 2):
        m = lo + (hi - lo) * i / (BANDS + 1)
        f = 700.0 * (10.0 ** (m / 2595.0) - 1.0)
        out.append(16.0 * f * NFFT / RATE)
    return out


@functools.lru_cache(maxsize=None)
def edges():
    return tuple(int(math.floor(x + 0.5)) for x in edges_exact())


def weight(b, d, closed_left=False, round_w=False):
    x, (a, c, z) = 16 * d, edges()[b:b + 3]

    def div(n, m):
        return (n + m // 2) // m if round_w else n // m
    if (a <= x < c) if closed_left else (a < x <= c):
        return div(64 * (x - a), c - a)
    if c < x < z:
        return div(64 * (z - x), z - c)
    return 0


@functools.lru_cache(maxsize=None)
def weights(closed_left=False, round_w=False):
    """tuple of 32 rows of 256 ints; bin 0 takes no part"""
    return tuple(tuple(0 if d == 0 else weight(b, d, closed_left, round_w) for d in range(256)) for b in range(BANDS))


@functools.lru_cache(maxsize=None)
def dct(even_dct=False):
    """tuple of 13 rows of 32 ints: floor(16384 cos(pi k (2 b + 1) / 64) + 0.5), the cosine bl_chroma_cossin's"""
    rows = []
    for k in range(COEFFS):
        t = np.array([((k * (2 * b + (0 if even_dct else 1))) % 128) / 128.0 for b in range(BANDS)])
        c, _ = cr.cossin(t)
        rows.append(tuple(int(v) for v in np.floor(16384.0 * c + 0.5)))
    return tuple(rows)


def ilog2(x, iters11=False, norm31=False):
    """L(x), 1 <= x < 2^64.  iters11: eleven squarings, the result brought to the same scale; norm31: the mantissa
    normalised to [2^31, 2^32) with the squarings left as they are — both WRONG."""
    assert 1 <= x < 1 << 64
    e = x.bit_length() - 1
    top = 31 if norm31 else 30
    m = x << (top - e) if e <= top else x >> (e - top)
    acc = e
    n = 11 if iters11 else 12
    for _ in range(n):
        t = (m * m) >> 30
        bit = t >> 31
        m = t >> bit
        acc = 2 * acc + bit
    return acc << (12 - n)


def ilog2_np(x):
    """L of a uint64 array, every step as in ilog2 (m * m < 2^62 fits): for the sweeps of the host test"""
    x = np.asarray(x, dtype=np.uint64)
    assert x.min() >= 1
    e = np.zeros(x.shape, dtype=np.uint64)
    for s in (32, 16, 8, 4, 2, 1):
        hit = (x >> (e + np.uint64(s))) > 0
        e = np.where(hit, e + np.uint64(s), e)
    up = e <= 30
    m = np.where(up, x << np.where(up, np.uint64(30) - e, np.uint64(0)), x >> np.where(up, np.uint64(0), e - np.uint64(30)))
    acc = e.copy()
    for _ in range(12):
        t = (m * m) >> np.uint64(30)
        bit = t >> np.uint64(31)
        m = t >> bit
        acc = np.uint64(2) * acc + bit
    return acc


# ---- a frame -----------------------------------------------------------------------------------------------------

def frame_of_q(q, *, closed_left=False, round_w=False, no_plus1=False, iters11=False, norm31=False, even_dct=False,
               trunc_shift=False, bands31=False, strict_used=False):
    """dict(energy, S, E, mfcc, flat) of one frame from its 256 ints Q (index 0 is ignored)"""
    del strict_used   # a song-level switch
    w = weights(closed_left, round_w)
    energy = sum(q[1:256])
    S = [sum(w[b][d] * q[d] for d in range(1, 256) if w[b][d]) for b in range(BANDS)]
    assert energy < LIMIT and all(s < LIMIT for s in S)

    def L(x):
        return ilog2(x, iters11, norm31)
    E = [(L(s) if s > 0 else 0) if no_plus1 else L(s + 1) for s in S]
    D = dct(even_dct)
    mfcc = []
    for k in range(COEFFS):
        acc = sum(D[k][b] * E[b] for b in range(BANDS))
        mfcc.append(-((-acc) >> 14) if trunc_shift and acc < 0 else acc >> 14)
    nb = BANDS - 1 if bands31 else BANDS
    T = sum(s + 1 for s in S[:nb])
    assert T < LIMIT
    flat = 32 * L(T) - 160 * 4096 - sum(E[:nb])
    return dict(energy=energy, S=S, E=E, mfcc=mfcc, flat=flat)


def frame_record(power_row, **sw):
    return frame_of_q(tr.sixteenths(power_row), **sw)


def song_record(frames, min_energy, strict_used=False):
    """dict with the fields of bl_amd_song_mel from the list of frame dicts"""
    used = [f for f in frames if f["energy"] > 0 and (f["energy"] > min_energy if strict_used else
                                                      f["energy"] >= min_energy)]
    rec = dict(mfcc_sum=[sum(f["mfcc"][k] for f in used) for k in range(COEFFS)],
               mfcc_sumsq=[sum(f["mfcc"][k] ** 2 for f in used) for k in range(COEFFS)],
               flat_sum=sum(f["flat"] for f in used), flat_sumsq=sum(f["flat"] ** 2 for f in used),
               band_sum=[sum(f["E"][b] for f in used) for b in range(BANDS)],
               frames=len(frames), used=len(used), status=0, reserved=0)
    assert all(abs(v) < LIMIT for v in rec["mfcc_sum"] + rec["mfcc_sumsq"] + rec["band_sum"])
    assert abs(rec["flat_sum"]) < LIMIT and rec["flat_sumsq"] < LIMIT
    return rec


def from_power(power_rows, min_energy=0, **sw):
    """(list of frame dicts, song dict) from per-frame power values, (F, 256)"""
    frames = [frame_record(row, **sw) for row in power_rows]
    return frames, song_record(frames, min_energy, sw.get("strict_used", False))


def song(oracle, pcm, channels, min_energy=0, **sw):
    """(list of frame dicts, song dict) of one song"""
    return from_power(tr.power_of(oracle, pcm, channels), min_energy, **sw)
