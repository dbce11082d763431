"""K-weighted gated loudness (include/bliss_amd.h: bl_amd_loud_params, bl_amd_song_loud, bl_amd_loud_*): the programme
loudness of ITU-R BS.1770 / EBU R128 in LUFS, the gain to a target and the loudness range of EBU Tech 3342, one record
per song.  The filter is f64 in a fixed order and everything behind it exact integers, so two runs agree to the bit.

This module is imported explicitly (`import bliss_amd.loudness`): the package's own namespace is unchanged."""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._args import host_pcm, int_in, songs_check
from ._lib import check
from .records import LOUD_DTYPE

CHUNK = 16                            # BL_AMD_LOUD_CHUNK
HOP_MAX, WARM_MAX = 4800, 8192
ABS_GATE_LIMIT, HOP_VALUE_LIMIT, FROM_HOPS_MAX = 1 << 56, 1 << 46, 1 << 27
_SHORTEST = (1, 1)   # the least interleaved samples of a mono and of a stereo song


def kweight(rate):
    """The parameter record of a sample rate (bl_amd_loud_kweight): the K-weighting coefficients, hop = rate / 10,
    warm = 4096 and the -70 LUFS gate.  rate: 8000 .. 48000, a multiple of 10."""
    rate = int_in("rate", rate, 8000, 48000)
    if rate % 10:
        raise ValueError(f"rate must be a multiple of 10, got {rate!r}")
    p = _lib.LoudParams()
    check(_lib.load().bl_amd_loud_kweight(rate, C.byref(p)), "bl_amd_loud_kweight")
    return p


def params(s1_b, s1_a, s2_a, hop, warm, abs_gate):
    """A parameter record of the caller's own: s1_b = (b0, b1, b2), s1_a = (a1, a2), s2_a = (a1, a2).  The caller keeps
    the filter's output below 2^17 in magnitude (see the header); nothing checks that."""
    coef = [float(x) for x in (*s1_b, *s1_a, *s2_a)]
    if len(s1_b) != 3 or len(s1_a) != 2 or len(s2_a) != 2 or not all(math.isfinite(x) for x in coef):
        raise ValueError(f"need 3 + 2 + 2 finite coefficients, got {s1_b!r}, {s1_a!r}, {s2_a!r}")
    p = _lib.LoudParams()
    p.s1_b[:], p.s1_a[:], p.s2_a[:] = coef[:3], coef[3:5], coef[5:]
    p.hop, p.warm = int_in("hop", hop, 1, HOP_MAX), int_in("warm", warm, 0, WARM_MAX)
    p.abs_gate = int_in("abs_gate", abs_gate, 0, ABS_GATE_LIMIT - 1)
    return p


def _params_check(p):
    if not isinstance(p, _lib.LoudParams):
        raise ValueError(f"params must be a LoudParams record (kweight(), params()), got {type(p).__name__}")
    params(p.s1_b, p.s1_a, p.s2_a, p.hop, p.warm, p.abs_gate)
    return p


def hops_of(lengths, channels, hop):
    """H of each song: (interleaved samples / channels) / hop"""
    return [int(ln) // ch // hop for ln, ch in zip(lengths, channels)]


def loud_to_numpy(raw):
    """bytes / uint8 array of bl_amd_song_loud records -> structured numpy array with the header's field names."""
    return np.frombuffer(bytes(raw), dtype=LOUD_DTYPE).copy()


def loud_device(corpus, p, hops=False, ctx=None):
    """Enqueue the loudness of every song of a DeviceCorpus (bl_amd_loud_batch_device) on torch's current stream.
    Returns the CUDA tensors (records as uint8, hop energies as int64 of shape (sum of H, 2) holding the uint64 values,
    or None); loud_to_numpy() reads the records once the stream has been waited for.  ctx: an explicit Context."""
    p = _params_check(p)
    lengths, channels = corpus._songs()
    total = sum(hops_of(lengths, songs_check(lengths, channels, _SHORTEST), p.hop))
    torch, n = corpus.torch, corpus.n_songs
    with torch.cuda.device(corpus.device):
        rec = torch.empty(n * LOUD_DTYPE.itemsize, dtype=torch.uint8, device=corpus.device)
        z = torch.empty((total, 2), dtype=torch.int64, device=corpus.device) if hops else None
    corpus._call("loud_batch_device", ctx, C.c_void_p(corpus.pcm.data_ptr()), corpus.desc, n, C.byref(p),
                 C.c_void_p(rec.data_ptr()), C.c_void_p(z.data_ptr()) if hops else C.c_void_p(), total,
                 corpus._stream())
    return rec, z


def loud_host(pcm_list, channels, p, hops=False):
    """Loudness of songs in host memory (bl_amd_loud_batch_host), blocking: pcm_list a list of 1-D int16 arrays
    (interleaved), channels per song or one for all.  Returns (records, hop energies as a uint64 array of shape
    (sum of H, 2), or None)."""
    p = _params_check(p)
    arrs, ptrs, ns = host_pcm(pcm_list, np.int16)
    n = len(arrs)
    sizes = [a.size for a in arrs]
    channels = songs_check(sizes, channels, _SHORTEST)
    out = (_lib.SongLoud * max(n, 1))()
    z = np.empty((sum(hops_of(sizes, channels, p.hop)), 2), dtype=np.uint64) if hops else None
    check(_lib.load().bl_amd_loud_batch_host(
        ptrs, ns, (C.c_int32 * n)(*channels), n, C.byref(p), out,
        z.ctypes.data_as(C.POINTER(C.c_uint64)) if hops else None), "bl_amd_loud_batch_host")
    return loud_to_numpy(bytes(out)), z


def from_hops(energies_list, p):
    """Stages 4 to 6 alone (bl_amd_loud_from_hops) on hop energies of the caller's: a list of integer arrays of shape
    (H, 2) (or (H,): one channel), one per song, 0 <= H <= 2^27, values in [0, 2^46).  Only p.abs_gate is read.  Returns
    the records."""
    if not isinstance(p, _lib.LoudParams):
        raise ValueError(f"params must be a LoudParams record, got {type(p).__name__}")
    int_in("abs_gate", p.abs_gate, 0, ABS_GATE_LIMIT - 1)
    songs = []
    for e in energies_list:
        a = np.asarray(e)
        if a.ndim == 1:
            a = np.stack([a, np.zeros_like(a)], axis=1) if a.size else a.reshape(0, 2)
        if a.ndim != 2 or a.shape[1] != 2 or a.shape[0] > FROM_HOPS_MAX:
            raise ValueError(f"hop energies must have shape (H,) or (H, 2) with H <= 2^27, got {a.shape}")
        if a.size and (a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer)):
            raise ValueError(f"hop energies must be integers, got dtype {a.dtype}")
        if a.size and (int(a.min()) < 0 or int(a.max()) >= HOP_VALUE_LIMIT):
            raise ValueError(f"hop energies must lie in [0, 2^46), got [{int(a.min())}, {int(a.max())}]")
        songs.append(np.ascontiguousarray(a, dtype=np.uint64))
    if not songs:
        raise ValueError("at least one song is needed")
    n = len(songs)
    flat = np.ascontiguousarray(np.concatenate(songs, axis=0))
    out = (_lib.SongLoud * n)()
    check(_lib.load().bl_amd_loud_from_hops(
        flat.ctypes.data_as(C.POINTER(C.c_uint64)) if flat.size else None,
        (C.c_int32 * n)(*[s.shape[0] for s in songs]), n, C.byref(p), out), "bl_amd_loud_from_hops")
    return loud_to_numpy(bytes(out))


def _records(records):
    rec = np.ascontiguousarray(records)
    if rec.dtype != LOUD_DTYPE or rec.ndim != 1 or rec.size < 1:
        raise ValueError("records must be a non-empty 1-D array of bl_amd_song_loud records (loud_to_numpy)")
    return rec, rec.ctypes.data_as(C.POINTER(_lib.SongLoud))


def lufs(records, hop):
    """(integrated, momentary maximum, short-term maximum) in LUFS of each record, float64 arrays (bl_amd_loud_lufs,
    bl_amd_loud_momentary_max_lufs, bl_amd_loud_short_max_lufs); -inf where nothing passed the gates."""
    rec, ptr = _records(records)
    hop = int_in("hop", hop, 1, HOP_MAX)
    lib = _lib.load()
    return tuple(np.array([f(C.byref(ptr[i]), hop) for i in range(rec.size)], dtype=np.float64)
                 for f in (lib.bl_amd_loud_lufs, lib.bl_amd_loud_momentary_max_lufs, lib.bl_amd_loud_short_max_lufs))


def range_lu(records):
    """float64 array of the loudness range in LU of each record (bl_amd_loud_range_lu); 0 where no short-term block
    passed the gates."""
    rec, ptr = _records(records)
    lib = _lib.load()
    return np.array([lib.bl_amd_loud_range_lu(C.byref(ptr[i])) for i in range(rec.size)], dtype=np.float64)


def gain_db(records, hop, target_lufs=-18.0):
    """float64 array of the gain in dB that brings each song to target_lufs (bl_amd_loud_gain_db); 0 for a song that
    is silent to the gates.  -18 LUFS is ReplayGain 2.0's reference level, -23 EBU R128's."""
    rec, ptr = _records(records)
    hop = int_in("hop", hop, 1, HOP_MAX)
    target = float(target_lufs)
    if not math.isfinite(target):
        raise ValueError(f"target_lufs must be finite, got {target_lufs!r}")
    lib = _lib.load()
    return np.array([lib.bl_amd_loud_gain_db(C.byref(ptr[i]), hop, target) for i in range(rec.size)],
                    dtype=np.float64)
