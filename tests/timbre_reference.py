"""A reference for the spectral timbre (include/bliss_amd.h: bl_amd_frame_timbre, bl_amd_song_timbre) that is NOT the
code under test — TEST INFRASTRUCTURE, shared by tests/test_timbre_reference_host.py (which runs it on designed spectra
and shows what each kind of error does to it) and tests/test_gpu_timbre.py (which holds the kernel to it with ==).

The definitions of the header restated in Python ints, on top of tests/freq_reference.py's per-frame power values
(frame_power: what the frequency kernels are already held to, bit for bit).  Nothing here can overflow or round: the
only floating-point step is 16 * P, a power-of-two scaling of an f32 held in a double, and its floor.

The keyword arguments of frame_record() that default to False are the WRONG forms, the mutations of the host test.
"""
import numpy as np

from tests import freq_reference as fr

BINS = range(1, 256)


def sixteenths(power_row, round_q=False):
    """256 Python ints: Q[d] = floor(16 P[d]) of one frame's power values (f32 or anything float() takes); index 0 is
    kept as computed, the callers decide whether it takes part (it does not).  round_q: the WRONG form, to nearest."""
    p = np.asarray(power_row, dtype=np.float64) * 16.0
    assert p.shape == (256,) and np.all(p >= 0) and np.all(p < 2.0 ** 62)
    return np.floor(p + 0.5 if round_q else p).astype(np.int64).tolist()


def frame_record(power_row, pct, *, exclusive=False, strict=False, bin0=False, round_q=False):
    """(energy, moment, rolloff, peak) of one frame.  Mutations: exclusive = the prefix without the bin itself,
    strict = > instead of >=, bin0 = bin 0 takes part, round_q = Q rounded to nearest."""
    assert isinstance(pct, int) and 1 <= pct <= 100
    q = sixteenths(power_row, round_q)
    bins = range(0, 256) if bin0 else BINS
    energy = sum(q[d] for d in bins)
    moment = sum(d * q[d] for d in bins)
    rolloff, c = None, 0
    for d in bins:
        incl = c + q[d]
        lhs = 100 * (c if exclusive else incl)
        if (lhs > pct * energy) if strict else (lhs >= pct * energy):
            rolloff = d
            break
        c = incl
    if rolloff is None:   # only a mutation gets here
        rolloff = 256
    top = max(q[d] for d in bins)
    peak = min(d for d in bins if q[d] == top)
    return energy, moment, rolloff, peak


def centroid(energy, moment, rounded=False):
    """floor(4096 moment / energy); rounded: the WRONG form, to nearest"""
    assert energy > 0
    return ((moment << 12) + energy // 2) // energy if rounded else (moment << 12) // energy


def song_record(frames, min_energy):
    """dict with the fields of bl_amd_song_timbre from the list of (energy, moment, rolloff, peak)"""
    used = [f for f in frames if f[0] > 0 and f[0] >= min_energy]
    cs = [centroid(e, m) for e, m, _, _ in used]
    return dict(centroid_sum=sum(cs), centroid_sumsq=sum(c * c for c in cs),
                rolloff_sum=sum(f[2] for f in used), rolloff_sumsq=sum(f[2] ** 2 for f in used),
                peak_sum=sum(f[3] for f in used), peak_sumsq=sum(f[3] ** 2 for f in used),
                energy_max=max((f[0] for f in frames), default=0), frames=len(frames), used=len(used), status=0,
                reserved=0)


def power_of(oracle, pcm, channels):
    """(F, 256) f32: the per-frame power values of a song, F = (n / channels) / 512; the samples behind are not read"""
    return fr.frame_power(fr.transform(oracle, fr.windowed_frames(pcm, channels)))


def song(oracle, pcm, channels, pct, min_energy):
    """(list of per-frame tuples, song dict) of one song"""
    frames = [frame_record(row, pct) for row in power_of(oracle, pcm, channels)]
    return frames, song_record(frames, min_energy)
