"""Versions of a piece (include/bliss_amd.h: bl_amd_cover_match, bl_amd_cover_*): whether two files are the same piece in
another recording (a live take, a remaster at another speed, a cover in another key, an edit with a different intro).
The songs' chroma units are aligned locally (Smith-Waterman over their cross-similarity) after one has been rotated to
the other's key; a record holds the score, the aligned stretch of either song and the transposition.  Everything the
device computes is an exact integer, so two runs agree to the bit.

The default thresholds (thr 12000, gap 4000) separate synthetic chord songs from their transposed, slower, faster,
noisy and re-cut copies.  They have not been tuned on recorded music.

This module is imported explicitly (`import bliss_amd.cover`): the package's own namespace is unchanged."""
import ctypes as C

import numpy as np

from . import _lib
from ._args import int_in
from ._lib import check
from .chroma import chroma_batch_host
from .fingerprint import pairs_from_knn  # noqa: F401  (the pair list of a kNN result is the fingerprints')
from .records import COVER_MATCH_DTYPE, FRAME_CHROMA_DTYPE

UNITS_MAX, COUNT_MAX = 8192, (1 << 20) - 1     # BL_AMD_FORM_UNITS_MAX, counts < 2^20
NO_MATCH, TOO_LONG, BAD_INDEX = 1, 2, 4        # BL_AMD_COVER_NO_MATCH, BL_AMD_COVER_TOO_LONG, BL_AMD_COVER_BAD_INDEX
THR_MAX, GAP_MAX, S_MAX = 16128, 1 << 20, 16129
HOP = 2048                                     # BL_AMD_CHROMA_HOP


def _pool(pool):
    return int_in("pool", pool, 1, 16)


def params(thr=12000, gap=4000, transpose=-1):
    """A bl_amd_cover_params: a pair of units counts for the alignment by how far its similarity (0 .. 16129) lies
    above `thr`, a step along one song alone costs `gap`, and b is taken `transpose` semitones above a (-1: found from
    the songs' chroma profiles).  The defaults are those of a prototype on synthetic chord songs and are not tuned on
    music."""
    return _lib.CoverParams(int_in("thr", thr, 1, THR_MAX), int_in("gap", gap, 0, GAP_MAX),
                            int_in("transpose", transpose, -1, 11), 0)


def _params(p):
    if not isinstance(p, _lib.CoverParams):
        raise ValueError("params must come from bliss_amd.cover.params()")
    return p


def shape():
    """(columns of b one wavefront owns at a time, rows of a it fetches at a time) (bl_amd_cover_shape): the lengths at
    which the alignment's path changes."""
    v = [C.c_int() for _ in range(2)]
    _lib.load().bl_amd_cover_shape(*[C.byref(x) for x in v])
    return tuple(x.value for x in v)


def _counts(name, counts):
    """(list, ctypes int32 array) of per-song counts, once there is a song and every count lies in [0, 2^20)"""
    vals = [int_in(name, c, 0, COUNT_MAX) for c in counts]
    if not vals:
        raise ValueError("at least one song is needed")
    return vals, (C.c_int32 * len(vals))(*vals)


def _call(name, ctx, *args):
    """bl_amd_<name>(*args) on the thread's default context, or bl_amd_ctx_<name>(ctx, *args) on an explicit one"""
    lib = _lib.load()
    if ctx is None:
        check(getattr(lib, "bl_amd_" + name)(*args), "bl_amd_" + name)
    else:
        check(getattr(lib, "bl_amd_ctx_" + name)(ctx.handle, *args), "bl_amd_ctx_" + name)


def _stream(torch, device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def units_device(frames, counts, pool=1, ctx=None):
    """Enqueue the units of songs whose chroma frame records sit in the CUDA uint8 tensor `frames`, concatenated,
    counts[i] frames each (bl_amd_cover_units_device), on torch's current stream.  Returns (units as a CUDA uint8 tensor
    of shape (n, 16), the per-song unit counts)."""
    import torch
    pool = _pool(pool)
    vals, arr = _counts("frames", counts)
    if frames.dtype != torch.uint8 or frames.numel() < sum(vals) * FRAME_CHROMA_DTYPE.itemsize:
        raise ValueError("frames must be a uint8 tensor that holds every song's frame records")
    ucounts = [t // pool for t in vals]
    n = sum(ucounts)
    dev = frames.device
    with torch.cuda.device(dev):
        check(_lib.load().bl_amd_init(dev.index or 0), "bl_amd_init")
        units = torch.empty((max(n, 1), 16), dtype=torch.uint8, device=dev)
        # a tensor without elements has no pointer the library would take: one record stands in for it
        fr = frames if frames.numel() else torch.zeros(FRAME_CHROMA_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        _call("cover_units_device", ctx, C.c_void_p(fr.data_ptr()), arr, len(vals), pool, C.c_void_p(units.data_ptr()),
              n, _stream(torch, dev))
    return units[:n], ucounts


def _frame_records(frames):
    """frame records as a contiguous uint64 array of shape (T, 12): FRAME_CHROMA_DTYPE records or such an array"""
    a = np.asarray(frames)
    if a.dtype == FRAME_CHROMA_DTYPE:
        a = a["x"]
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.ndim != 2 or a.shape[1] != 12:
        raise ValueError(f"frames must be bl_amd_frame_chroma records or have shape (T, 12), got {a.shape}")
    return a


def units_host(frames, counts, pool=1):
    """The units of songs whose chroma frames are in host memory (bl_amd_cover_units_host), blocking: frames the records
    of all songs concatenated (FRAME_CHROMA_DTYPE records or uint64 (T, 12)), counts[i] frames each.  Returns (units
    uint8 (n, 16), per-song unit counts)."""
    pool = _pool(pool)
    x = _frame_records(frames)
    vals, arr = _counts("frames", counts)
    if x.shape[0] != sum(vals):
        raise ValueError(f"{x.shape[0]} frame records but the counts add up to {sum(vals)}")
    ucounts = [t // pool for t in vals]
    n = sum(ucounts)
    units = np.zeros((max(n, 1), 16), dtype=np.uint8)
    if x.shape[0] == 0:
        x = np.zeros((1, 12), dtype=np.uint64)
    check(_lib.load().bl_amd_cover_units_host(C.c_void_p(x.ctypes.data), arr, len(vals), pool,
                                              C.c_void_p(units.ctypes.data)), "bl_amd_cover_units_host")
    return units[:n], ucounts


def from_pcm(pcm_list, channels, pool=1):
    """(units, counts) of songs in host memory: chroma_batch_host with frames, then units_host."""
    songs, frames = chroma_batch_host(pcm_list, channels, frames=True)
    return units_host(frames, [int(t) for t in songs["frames"]], pool)


def _pairs_shape_check(shape):
    if len(shape) != 2 or shape[1] != 2 or shape[0] < 1:
        raise ValueError(f"pairs must have shape (n, 2) with n >= 1, got {tuple(shape)}")


def match_to_numpy(raw):
    """bytes / uint8 array of bl_amd_cover_match records -> structured numpy array with the header's field names."""
    return np.frombuffer(bytes(raw), dtype=COVER_MATCH_DTYPE).copy()


def match_device(units_a, counts_a, pairs, p=None, units_b=None, counts_b=None, ctx=None):
    """Enqueue the alignment of every pair (bl_amd_cover_match_device) on torch's current stream.  units_a: CUDA uint8
    tensor of set a's units (16 bytes each), counts_a its per-song unit counts; units_b / counts_b: set b, or None for
    the self form.  pairs: (n, 2) int32, a CUDA tensor or a host array (uploaded on the stream).  p: params(), None for
    the defaults.  Returns the records as a CUDA uint8 tensor; match_to_numpy() reads them once the stream has been
    waited for."""
    import torch
    p = params() if p is None else _params(p)
    if units_b is None:
        units_b, counts_b = units_a, counts_a
    va, arr_a = _counts("counts_a", counts_a)
    vb, arr_b = _counts("counts_b", counts_b)
    for name, u, v in (("units_a", units_a, va), ("units_b", units_b, vb)):
        if u.dtype != torch.uint8 or u.numel() < 16 * sum(v) or u.device != units_a.device or not u.is_contiguous():
            raise ValueError(f"{name} must be a contiguous uint8 tensor on one device that holds every song's units")
    dev = units_a.device
    with torch.cuda.device(dev):
        check(_lib.load().bl_amd_init(dev.index or 0), "bl_amd_init")
        if not torch.is_tensor(pairs):
            pairs = torch.from_numpy(np.ascontiguousarray(pairs, dtype=np.int32)).to(dev, non_blocking=False)
        _pairs_shape_check(pairs.shape)
        if pairs.dtype != torch.int32 or pairs.device != dev or not pairs.is_contiguous():
            raise ValueError("pairs must be a contiguous int32 tensor on the units' device")
        n = pairs.shape[0]
        rec = torch.empty(n * COVER_MATCH_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        # a tensor without elements has no pointer the library would take: one unit stands in for it
        pa = units_a if units_a.numel() else torch.zeros(16, dtype=torch.uint8, device=dev)
        pb = units_b if units_b.numel() else pa
        _call("cover_match_device", ctx, C.c_void_p(pa.data_ptr()), arr_a, len(va), C.c_void_p(pb.data_ptr()), arr_b,
              len(vb), C.c_void_p(pairs.data_ptr()), n, C.byref(p), C.c_void_p(rec.data_ptr()), _stream(torch, dev))
    return rec


def _unit_bytes(name, units, total):
    u = np.ascontiguousarray(units, dtype=np.uint8).reshape(-1)
    if u.size < 16 * total:
        raise ValueError(f"{name} must hold every song's units, 16 bytes each")
    return u if u.size else np.zeros(16, dtype=np.uint8)


def match_host(units_a, counts_a, pairs, p=None, units_b=None, counts_b=None):
    """The alignment of every pair with everything in host memory (bl_amd_cover_match_host), blocking.  Returns the
    records as a structured array."""
    p = params() if p is None else _params(p)
    va, arr_a = _counts("counts_a", counts_a)
    a = _unit_bytes("units_a", units_a, sum(va))
    if units_b is None:
        b, vb, arr_b = a, va, arr_a
    else:
        vb, arr_b = _counts("counts_b", counts_b)
        b = _unit_bytes("units_b", units_b, sum(vb))
    pr = np.ascontiguousarray(pairs, dtype=np.int32)
    _pairs_shape_check(pr.shape)
    n = pr.shape[0]
    out = (_lib.CoverMatch * n)()
    check(_lib.load().bl_amd_cover_match_host(C.c_void_p(a.ctypes.data), arr_a, len(va), C.c_void_p(b.ctypes.data),
                                              arr_b, len(vb), C.c_void_p(pr.ctypes.data), n, C.byref(p), out),
          "bl_amd_cover_match_host")
    return match_to_numpy(bytes(out))


def _records(records):
    rec = np.ascontiguousarray(records)
    if rec.dtype != COVER_MATCH_DTYPE or rec.ndim != 1 or rec.size < 1:
        raise ValueError("records must be a non-empty 1-D array of bl_amd_cover_match records")
    return rec, rec.ctypes.data_as(C.POINTER(_lib.CoverMatch))


def score(records, thr=12000):
    """float64 array of score / ((16129 - thr) min(units_a, units_b)) of each record (bl_amd_cover_score): the share of
    the shorter song that aligns perfectly; NaN for a record whose status is not 0.  thr: the one the match ran with."""
    rec, ptr = _records(records)
    thr = int_in("thr", thr, 1, THR_MAX)
    lib = _lib.load()
    return np.array([lib.bl_amd_cover_score(C.byref(ptr[i]), thr) for i in range(rec.size)], dtype=np.float64)


def tempo_ratio(records):
    """float64 array of (b_end - b_start + 1) / (a_end - a_start + 1) of each record (bl_amd_cover_tempo_ratio): above 1
    where b takes longer over the aligned stretch; NaN for a record whose status is not 0."""
    rec, ptr = _records(records)
    lib = _lib.load()
    return np.array([lib.bl_amd_cover_tempo_ratio(C.byref(ptr[i])) for i in range(rec.size)], dtype=np.float64)


def seconds(unit, pool=1, rate=22050):
    """The time at which unit `unit` starts (bl_amd_cover_seconds): unit * pool * 2048 / rate."""
    return _lib.load().bl_amd_cover_seconds(int_in("unit", unit, 0), _pool(pool), int_in("rate", rate, 1))
