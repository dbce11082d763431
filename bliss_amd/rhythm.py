"""Per-song tempo (include/bliss_amd.h: bl_amd_song_rhythm, bl_amd_rhythm_*): the beat period of a song as a lag of its
onset curve, in exact integers, and the beats per minute and beat strength read off them; and the beat grid
(bl_amd_song_beats, bl_amd_beats_*): where the beats are, by dynamic programming over that curve at that period.

This module is imported explicitly (`import bliss_amd.rhythm`): the package's own namespace is unchanged."""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._args import host_pcm, int_in, songs_check
from ._lib import check
from .records import BEATS_DTYPE, RHYTHM_DTYPE

HOP, LAGS = 128, 512   # BL_AMD_RHYTHM_HOP, BL_AMD_RHYTHM_LAGS
PERIOD_MAX, TIGHT_MAX = 510, 4096   # BL_AMD_BEATS_PERIOD_MAX, BL_AMD_BEATS_TIGHT_MAX
_SHORTEST = (HOP, 2 * HOP)   # the least interleaved samples of a mono and of a stereo song: one hop


def _lags_check(lag_min, lag_max):
    lag_min = int_in("lag_min", lag_min, 1, LAGS - 2)
    return lag_min, int_in("lag_max", lag_max, lag_min, LAGS - 2)


def _hops(lengths, channels):
    return [int(ln) // ch // HOP for ln, ch in zip(lengths, channels)]


def lags_for_bpm(bpm_min, bpm_max, rate=22050):
    """(lag_min, lag_max) in hops of 128 frames for tempi in [bpm_min, bpm_max]:
    (ceil(60 rate / (128 bpm_max)), floor(60 rate / (128 bpm_min))); ValueError when that leaves 1 .. 510 or is empty."""
    if not (0 < bpm_min <= bpm_max) or not math.isfinite(bpm_max) or rate < 1:
        raise ValueError(f"need 0 < bpm_min <= bpm_max and rate >= 1, got {bpm_min!r}, {bpm_max!r}, {rate!r}")
    lo, hi = math.ceil(60.0 * rate / (HOP * bpm_max)), math.floor(60.0 * rate / (HOP * bpm_min))
    if lo < 1 or hi > LAGS - 2 or lo > hi:
        raise ValueError(f"[{bpm_min!r}, {bpm_max!r}] bpm at {rate!r} Hz is lags [{lo}, {hi}]: need 1 <= lag_min <= "
                         f"lag_max <= {LAGS - 2}")
    return lo, hi


def rhythm_to_numpy(raw):
    """bytes / uint8 array of bl_amd_song_rhythm records -> structured numpy array with the header's field names."""
    return np.frombuffer(bytes(raw), dtype=RHYTHM_DTYPE).copy()


def rhythm_device(corpus, lag_min, lag_max, onsets=True, acf=False, ctx=None):
    """Enqueue the tempo of every song of a DeviceCorpus (bl_amd_rhythm_batch_device) on torch's current stream; returns
    the CUDA tensors (records as uint8, onset curve as int32 holding the uint32 values or None, lag products as int64
    holding the uint64 values, shape (n_songs, 512), or None) the corpus owns; fetch_rhythm() reads them.  ctx: an
    explicit Context."""
    lag_min, lag_max = _lags_check(lag_min, lag_max)
    lengths, channels = corpus._songs()
    total = sum(_hops(lengths, songs_check(lengths, channels, _SHORTEST)))
    torch, n = corpus.torch, corpus.n_songs
    with torch.cuda.device(corpus.device):
        rec = torch.zeros(n * RHYTHM_DTYPE.itemsize, dtype=torch.uint8, device=corpus.device)
        ons = torch.zeros(total, dtype=torch.int32, device=corpus.device) if onsets else None
        rows = torch.zeros((n, LAGS), dtype=torch.int64, device=corpus.device) if acf else None
    corpus._call("rhythm_batch_device", ctx, C.c_void_p(corpus.pcm.data_ptr()), corpus.desc, n, lag_min, lag_max,
                 C.c_void_p(rec.data_ptr()), C.c_void_p(ons.data_ptr()) if onsets else C.c_void_p(), total,
                 C.c_void_p(rows.data_ptr()) if acf else C.c_void_p(), corpus._stream())
    corpus.rhythm_raw, corpus.rhythm_onsets, corpus.rhythm_acf = rec, ons, rows
    return rec, ons, rows


def fetch_rhythm(corpus):
    """Wait for the device and return what the last rhythm_device() call on this corpus computed: (records, onsets,
    acf); onsets a uint32 array of all hops, songs one behind the other, acf a uint64 array of shape (n_songs, 512),
    each None unless it was asked for."""
    if getattr(corpus, "rhythm_raw", None) is None:
        raise RuntimeError("rhythm_device() has not been called on this corpus")
    corpus.torch.cuda.synchronize(corpus.device)
    ons, rows = corpus.rhythm_onsets, corpus.rhythm_acf
    return (rhythm_to_numpy(corpus.rhythm_raw.cpu().numpy().tobytes()),
            None if ons is None else ons.cpu().numpy().view(np.uint32),
            None if rows is None else rows.cpu().numpy().view(np.uint64))


def rhythm_batch_host(pcm_list, channels, lag_min, lag_max, onsets=True, acf=False):
    """Tempo of songs in host memory (bl_amd_rhythm_batch_host): pcm_list a list of 1-D int16 arrays (interleaved),
    channels per song or one for all.  Returns (records, onsets, acf) as fetch_rhythm() does."""
    lag_min, lag_max = _lags_check(lag_min, lag_max)
    arrs, ptrs, ns = host_pcm(pcm_list, np.int16)
    n = len(arrs)
    sizes = [a.size for a in arrs]
    channels = songs_check(sizes, channels, _SHORTEST)
    chs = (C.c_int32 * n)(*channels)
    out = (_lib.SongRhythm * n)()
    ons = np.zeros(sum(_hops(sizes, channels)), dtype=np.uint32) if onsets else None
    rows = np.zeros((n, LAGS), dtype=np.uint64) if acf else None
    check(_lib.load().bl_amd_rhythm_batch_host(
        ptrs, ns, chs, n, lag_min, lag_max, out, ons.ctypes.data_as(C.POINTER(C.c_uint32)) if onsets else None,
        rows.ctypes.data_as(C.POINTER(C.c_uint64)) if acf else None), "bl_amd_rhythm_batch_host")
    return rhythm_to_numpy(bytes(out)), ons, rows


def _curves_check(onsets_list):
    """the curves as arrays, once there is one and each is 1-D, of integers in [0, 2^18) and of 1 to 2^24 - 1 hops"""
    curves = [np.asarray(o) for o in onsets_list]
    if not curves:
        raise ValueError("at least one onset curve is needed")
    for o in curves:
        if o.ndim != 1 or o.size < 1 or o.size >= 1 << 24 or not np.issubdtype(o.dtype, np.integer):
            raise ValueError(f"an onset curve must be a 1-D integer array of 1 .. 2^24 - 1 values, got shape {o.shape} "
                             f"of {o.dtype}")
        if int(o.min()) < 0 or int(o.max()) >= 1 << 18:
            raise ValueError(f"onset values must lie in [0, 2^18), got [{int(o.min())}, {int(o.max())}]")
    return curves


def rhythm_from_onsets(onsets_list, lag_min, lag_max, acf=False):
    """Stages 7 and 8 alone (bl_amd_rhythm_from_onsets) on onset curves of the caller's: a list of 1-D arrays of
    integers in [0, 2^18), one per song, of 1 to 2^24 - 1 hops each.  Returns the records, or (records, acf)."""
    lag_min, lag_max = _lags_check(lag_min, lag_max)
    curves = _curves_check(onsets_list)
    n = len(curves)
    flat = np.ascontiguousarray(np.concatenate(curves), dtype=np.uint32)
    hops = (C.c_int32 * n)(*[o.size for o in curves])
    out = (_lib.SongRhythm * n)()
    rows = np.zeros((n, LAGS), dtype=np.uint64) if acf else None
    check(_lib.load().bl_amd_rhythm_from_onsets(
        flat.ctypes.data_as(C.POINTER(C.c_uint32)), hops, n, lag_min, lag_max, out,
        rows.ctypes.data_as(C.POINTER(C.c_uint64)) if acf else None), "bl_amd_rhythm_from_onsets")
    rec = rhythm_to_numpy(bytes(out))
    return (rec, rows) if acf else rec


def rhythm_bpm(records, rate=22050):
    """(bpm, strength) float64 arrays of bl_amd_song_rhythm records (bl_amd_rhythm_bpm, bl_amd_rhythm_strength): the
    tempo in beats per minute, NaN where lag == 0, and r_lag / r0."""
    rec = np.ascontiguousarray(records)
    if rec.dtype != RHYTHM_DTYPE or rec.ndim != 1 or rec.size < 1:
        raise ValueError("records must be a non-empty 1-D array of bl_amd_song_rhythm records (rhythm_to_numpy)")
    rate = int_in("rate", rate, 1, 2 ** 31 - 1)
    lib = _lib.load()
    p = rec.ctypes.data_as(C.POINTER(_lib.SongRhythm))
    bpm = np.array([lib.bl_amd_rhythm_bpm(C.byref(p[i]), rate) for i in range(rec.size)], dtype=np.float64)
    strength = np.array([lib.bl_amd_rhythm_strength(C.byref(p[i])) for i in range(rec.size)], dtype=np.float64)
    return bpm, strength


# ---- beats -----------------------------------------------------------------------------------------------------------

def beats_to_numpy(raw):
    """bytes / uint8 array of bl_amd_song_beats records -> structured numpy array with the header's field names."""
    return np.frombuffer(bytes(raw), dtype=BEATS_DTYPE).copy()


def _hops_check(hops):
    hops = [int_in("hops", h, 1, (1 << 24) - 1) for h in hops]
    if not hops:
        raise ValueError("at least one song is needed")
    return hops


def beats_device(onsets, hops, period, tight=128, links=False, scores=False, ctx=None):
    """Enqueue the beat grids of n songs (bl_amd_beats_device) on torch's current stream.  onsets: a contiguous int32
    CUDA tensor holding the uint32 onset curves one behind the other (what rhythm_device() returns); hops: the n hop
    counts; period: an int32 CUDA tensor of n periods in hops, or the uint8 record tensor of rhythm_device(), whose
    `lag` fields are then read in place (stride 72, no copy).  A song whose period lies outside 2 .. 510 (a lag of 0:
    no tempo) gets a record with status BL_UNEXPECTED and no beats.  Returns the CUDA tensors (records as uint8, flags
    as uint8, links as int16 holding the uint16 values or None, scores as int64 or None); beats_to_numpy() reads the
    records once the stream has been waited for.  ctx: an explicit Context.

    tight weighs staying on the period against landing on onsets: 16 prices one octave off the period at one maximal
    onset.  The default of 128 has not been tuned against annotated music: on synthetic click curves with jitter every
    value from 16 to 256 followed every click."""
    import torch
    from .queries import _on_device_of
    hops = _hops_check(hops)
    n, total = len(hops), sum(hops)
    tight = int_in("tight", tight, 0, TIGHT_MAX)
    if onsets.dtype != torch.int32 or not onsets.is_cuda or not onsets.is_contiguous() or onsets.dim() != 1 or \
            onsets.numel() != total:
        raise ValueError(f"onsets must be a contiguous 1-D int32 CUDA tensor of sum(hops) = {total} values")
    if not period.is_cuda or period.device != onsets.device or not period.is_contiguous() or period.dim() != 1:
        raise ValueError("period must be a contiguous 1-D CUDA tensor on the device of onsets")
    if period.dtype == torch.int32 and period.numel() == n:
        at, stride = period.data_ptr(), 4
    elif period.dtype == torch.uint8 and period.numel() == n * RHYTHM_DTYPE.itemsize:
        at, stride = period.data_ptr() + RHYTHM_DTYPE.fields["lag"][1], RHYTHM_DTYPE.itemsize
    else:
        raise ValueError(f"period must hold {n} int32 periods or, as uint8, {n} bl_amd_song_rhythm records")
    lib = _lib.load()
    dev = onsets.device
    rec = torch.empty(n * BEATS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    flags = torch.empty(total, dtype=torch.uint8, device=dev)
    lk = torch.empty(total, dtype=torch.int16, device=dev) if links else None
    sc = torch.empty(total, dtype=torch.int64, device=dev) if scores else None
    with _on_device_of(lib, onsets, None) as cur:
        args = (C.c_void_p(onsets.data_ptr()), (C.c_int32 * n)(*hops), n, C.c_void_p(at), stride, tight,
                C.c_void_p(rec.data_ptr()), C.c_void_p(flags.data_ptr()), C.c_void_p(lk.data_ptr()) if links else None,
                C.c_void_p(sc.data_ptr()) if scores else None, C.c_void_p(cur.cuda_stream))
        if ctx is None:
            check(lib.bl_amd_beats_device(*args), "bl_amd_beats_device")
        else:
            check(lib.bl_amd_ctx_beats_device(ctx.handle, *args), "bl_amd_ctx_beats_device")
    return rec, flags, lk, sc


def beats_host(onsets_list, periods, tight=128, links=False, scores=False):
    """Beat grids of onset curves in host memory (bl_amd_beats_host), blocking: onsets_list as rhythm_from_onsets()
    takes it, periods one int per song.  Returns (records, flags, links or None, scores or None): the records as
    beats_to_numpy() gives them, the arrays over all hops, songs one behind the other.  tight: see beats_device()."""
    curves = _curves_check(onsets_list)
    n = len(curves)
    periods = [int_in("period", p, -2 ** 31, 2 ** 31 - 1) for p in periods]
    if len(periods) != n:
        raise ValueError(f"{n} curves but {len(periods)} periods")
    tight = int_in("tight", tight, 0, TIGHT_MAX)
    flat = np.ascontiguousarray(np.concatenate(curves), dtype=np.uint32)
    out = (_lib.SongBeats * n)()
    flags = np.empty(flat.size, dtype=np.uint8)
    lk = np.empty(flat.size, dtype=np.uint16) if links else None
    sc = np.empty(flat.size, dtype=np.int64) if scores else None
    check(_lib.load().bl_amd_beats_host(
        flat.ctypes.data_as(C.POINTER(C.c_uint32)), (C.c_int32 * n)(*[o.size for o in curves]), n,
        (C.c_int32 * n)(*periods), tight, out, flags.ctypes.data_as(C.POINTER(C.c_uint8)),
        lk.ctypes.data_as(C.POINTER(C.c_uint16)) if links else None,
        sc.ctypes.data_as(C.POINTER(C.c_int64)) if scores else None), "bl_amd_beats_host")
    return beats_to_numpy(bytes(out)), flags, lk, sc


def beat_list(flags, rate=22050):
    """(hops int32, seconds float64) of the beats of one song from its flags (bl_amd_beats_list): the indices of the set
    flags and 128 hop / rate."""
    f = np.ascontiguousarray(flags, dtype=np.uint8)
    if f.ndim != 1:
        raise ValueError("flags must be 1-D: the flags of one song")
    rate = int_in("rate", rate, 1, 2 ** 31 - 1)
    lib = _lib.load()
    p = f.ctypes.data_as(C.POINTER(C.c_uint8))
    count = lib.bl_amd_beats_list(p, f.size, rate, None, None, 0)
    if count < 0:
        raise RuntimeError("bl_amd_beats_list rejected its arguments")
    hop, sec = np.empty(count, dtype=np.int32), np.empty(count, dtype=np.float64)
    lib.bl_amd_beats_list(p, f.size, rate, hop.ctypes.data_as(C.POINTER(C.c_int32)),
                          sec.ctypes.data_as(C.POINTER(C.c_double)), count)
    return hop, sec


def beats_bpm(records, rate=22050):
    """float64 array of the tempo of each grid of bl_amd_song_beats records (bl_amd_beats_bpm):
    60 rate (n_beats - 1) / (128 (last - first)), NaN for fewer than two beats."""
    rec = np.ascontiguousarray(records)
    if rec.dtype != BEATS_DTYPE or rec.ndim != 1 or rec.size < 1:
        raise ValueError("records must be a non-empty 1-D array of bl_amd_song_beats records (beats_to_numpy)")
    rate = int_in("rate", rate, 1, 2 ** 31 - 1)
    lib = _lib.load()
    p = rec.ctypes.data_as(C.POINTER(_lib.SongBeats))
    return np.array([lib.bl_amd_beats_bpm(C.byref(p[i]), rate) for i in range(rec.size)], dtype=np.float64)
