"""True peak (include/bliss_amd.h: bl_amd_song_tpeak, bl_amd_tpeak_*): the peak of the four times oversampled signal
of ITU-R BS.1770 in dBTP, the number of interpolated points above a ceiling, an optional per-block profile, and the
gain to a loudness target that keeps the true peak under a ceiling.  Everything the device computes is an exact integer,
so two runs agree to the bit.

This module is imported explicitly (`import bliss_amd.truepeak`): the package's own namespace is unchanged."""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._args import host_pcm, int_in, songs_check
from ._lib import check
from .loudness import HOP_MAX
from .records import LOUD_DTYPE, TPEAK_DTYPE

CEILING_MAX, BLOCK_MAX = 65535, 65536
FULL_SCALE = 1 << 29   # a full-scale sample through a unit-gain phase
_SHORTEST = (1, 1)     # the least interleaved samples of a mono and of a stereo song


def table():
    """The interpolator G as an int32 array of shape (4, 12), Q14 (bl_amd_tpeak_table)."""
    out = (C.c_int32 * 48)()
    _lib.load().bl_amd_tpeak_table(out)
    return np.array(out, dtype=np.int32).reshape(4, 12)


def shape():
    """(frames one lane owns, frames one workgroup owns) of the kernel (bl_amd_tpeak_shape): the lengths at which its
    paths change."""
    a, b = C.c_int(), C.c_int()
    _lib.load().bl_amd_tpeak_shape(C.byref(a), C.byref(b))
    return a.value, b.value


def blocks_of(lengths, channels, block):
    """ceil(F / block) of each song, F = interleaved samples / channels"""
    return [(int(ln) // ch + block - 1) // block for ln, ch in zip(lengths, channels)]


def _args_check(ceiling, block):
    ceiling = int_in("ceiling", ceiling, 0, CEILING_MAX)
    return ceiling, None if block is None else int_in("block", block, 1, BLOCK_MAX)


def tpeak_to_numpy(raw):
    """bytes / uint8 array of bl_amd_song_tpeak records -> structured numpy array with the header's field names."""
    return np.frombuffer(bytes(raw), dtype=TPEAK_DTYPE).copy()


def tpeak_device(corpus, ceiling=32767, block=None, ctx=None):
    """Enqueue the true peak of every song of a DeviceCorpus (bl_amd_tpeak_batch_device) on torch's current stream.
    ceiling: the level, in sample units, above which interpolated points are counted.  block: None, or the frames per
    block of the profile.  Returns the CUDA tensors (records as uint8, the profile as int32 of shape (sum of
    ceil(F / block), 2), whose values stay below 2^30, or None); tpeak_to_numpy() reads the records once the stream has
    been waited for.  ctx: an explicit Context."""
    ceiling, block = _args_check(ceiling, block)
    lengths, channels = corpus._songs()
    channels = songs_check(lengths, channels, _SHORTEST)
    total = sum(blocks_of(lengths, channels, block)) if block else 0
    torch, n = corpus.torch, corpus.n_songs
    with torch.cuda.device(corpus.device):
        rec = torch.empty(n * TPEAK_DTYPE.itemsize, dtype=torch.uint8, device=corpus.device)
        prof = torch.empty((total, 2), dtype=torch.int32, device=corpus.device) if block else None
    corpus._call("tpeak_batch_device", ctx, C.c_void_p(corpus.pcm.data_ptr()), corpus.desc, n, ceiling, block or 1,
                 C.c_void_p(rec.data_ptr()), C.c_void_p(prof.data_ptr()) if block else C.c_void_p(), total,
                 corpus._stream())
    return rec, prof


def tpeak_host(pcm_list, channels, ceiling=32767, block=None):
    """True peak of songs in host memory (bl_amd_tpeak_batch_host), blocking: pcm_list a list of 1-D int16 arrays
    (interleaved), channels per song or one for all.  Returns (records, the profile as a uint32 array of shape (sum of
    ceil(F / block), 2), or None)."""
    ceiling, block = _args_check(ceiling, block)
    arrs, ptrs, ns = host_pcm(pcm_list, np.int16)
    n = len(arrs)
    sizes = [a.size for a in arrs]
    channels = songs_check(sizes, channels, _SHORTEST)
    out = (_lib.SongTpeak * max(n, 1))()
    prof = np.zeros((sum(blocks_of(sizes, channels, block)), 2), dtype=np.uint32) if block else None
    check(_lib.load().bl_amd_tpeak_batch_host(
        ptrs, ns, (C.c_int32 * n)(*channels), n, ceiling, block or 1, out,
        prof.ctypes.data_as(C.POINTER(C.c_uint32)) if block else None), "bl_amd_tpeak_batch_host")
    return tpeak_to_numpy(bytes(out)), prof


def _records(records, dtype, struct, what):
    rec = np.ascontiguousarray(records)
    if rec.dtype != dtype or rec.ndim != 1 or rec.size < 1:
        raise ValueError(f"records must be a non-empty 1-D array of {what} records")
    return rec, rec.ctypes.data_as(C.POINTER(struct))


def dbtp(records):
    """(per channel, per song) true peak in dBTP: a float64 array of shape (n, 2) (bl_amd_tpeak_dbtp; -inf for a
    channel that is all zeros and for channel 1 of a mono song) and one of shape (n,) (bl_amd_tpeak_song_dbtp: the
    larger channel)."""
    rec, ptr = _records(records, TPEAK_DTYPE, _lib.SongTpeak, "bl_amd_song_tpeak")
    lib = _lib.load()
    per = np.array([[lib.bl_amd_tpeak_dbtp(C.byref(ptr[i]), c) for c in (0, 1)] for i in range(rec.size)],
                   dtype=np.float64)
    song = np.array([lib.bl_amd_tpeak_song_dbtp(C.byref(ptr[i])) for i in range(rec.size)], dtype=np.float64)
    return per, song


def gain_db(loud_records, hop, tpeak_records, target_lufs=-18.0, ceiling_dbtp=-1.0):
    """float64 array of the gain in dB that brings each song to target_lufs without lifting its true peak above
    ceiling_dbtp (bl_amd_tpeak_gain_db): min(loudness gain, ceiling_dbtp - true peak).  -1 dBTP is EBU R128's maximum
    permitted true peak."""
    lrec, lptr = _records(loud_records, LOUD_DTYPE, _lib.SongLoud, "bl_amd_song_loud")
    trec, tptr = _records(tpeak_records, TPEAK_DTYPE, _lib.SongTpeak, "bl_amd_song_tpeak")
    if lrec.size != trec.size:
        raise ValueError(f"{lrec.size} loudness records but {trec.size} true-peak records")
    hop = int_in("hop", hop, 1, HOP_MAX)
    target, ceil_db = float(target_lufs), float(ceiling_dbtp)
    if not math.isfinite(target) or not math.isfinite(ceil_db):
        raise ValueError(f"target_lufs and ceiling_dbtp must be finite, got {target_lufs!r}, {ceiling_dbtp!r}")
    lib = _lib.load()
    return np.array([lib.bl_amd_tpeak_gain_db(C.byref(lptr[i]), hop, target, C.byref(tptr[i]), ceil_db)
                     for i in range(lrec.size)], dtype=np.float64)
