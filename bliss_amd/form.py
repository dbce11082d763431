"""Song structure (include/bliss_amd.h: bl_amd_song_form, bl_amd_form_*): from a song's chroma frames, the start and lag
of its most strongly repeated stretch (a preview snippet: the chorus, where there is one) and a novelty curve with the
section boundaries picked from it (mix-in and mix-out points).  Everything the device computes is an exact integer, so
two runs agree to the bit.

This module is imported explicitly (`import bliss_amd.form`): the package's own namespace is unchanged."""
import ctypes as C

import numpy as np

from . import _lib
from ._args import int_in
from ._lib import check
from .chroma import _frames, chroma_batch_host, chroma_device
from .records import FORM_DTYPE, FRAME_CHROMA_DTYPE

UNITS_MAX, COUNT_MAX = 8192, (1 << 20) - 1   # BL_AMD_FORM_UNITS_MAX, T < 2^20
NO_THUMB, TOO_LONG = 1, 2                    # BL_AMD_FORM_NO_THUMB, BL_AMD_FORM_TOO_LONG
HOP = 2048                                   # BL_AMD_CHROMA_HOP


def _pool(pool):
    return int_in("pool", pool, 1, 16)


def units_count(frames, pool=1):
    """U of a song with `frames` chroma frames pooled `pool` to a unit (bl_amd_form_units)."""
    return _lib.load().bl_amd_form_units(int_in("frames", frames, 0), _pool(pool))


def shape():
    """(lags a workgroup of the thumbnail kernel takes at a time, units a workgroup of the units kernel owns)
    (bl_amd_form_shape): the lengths at which the kernels' paths change."""
    v = [C.c_int() for _ in range(2)]
    _lib.load().bl_amd_form_shape(*[C.byref(x) for x in v])
    return tuple(x.value for x in v)


def params(pool=1, seg=161, min_lag=None, nov=43, peak_num=1, peak_den=4):
    """A bl_amd_form_params: `pool` frames to a unit, a thumbnail of `seg` units that repeats at least `min_lag` units
    later (None: seg), a novelty kernel of `nov` units to either side, and boundaries at peaks of at least
    peak_num / peak_den of the song's largest novelty.  The defaults are 15 s and 4 s at 22 050 Hz and pool 1, in units
    of 2048 / 22050 s: round(15 * 22050 / 2048) = 161 and round(4 * 22050 / 2048) = 43."""
    seg = int_in("seg", seg, 2, 1024)
    peak_den = int_in("peak_den", peak_den, 1, 256)
    return _lib.FormParams(_pool(pool), seg, int_in("min_lag", seg if min_lag is None else min_lag, 1, UNITS_MAX),
                           int_in("nov", nov, 1, 64), int_in("peak_num", peak_num, 0, peak_den), peak_den, 0)


def _counts(counts):
    """(list, ctypes int32 array) of per-song frame counts, once there is a song and every count lies in [0, 2^20)"""
    vals = [int_in("frames", c, 0, COUNT_MAX) for c in counts]
    if not vals:
        raise ValueError("at least one song is needed")
    return vals, (C.c_int32 * len(vals))(*vals)


def _params(p):
    if not isinstance(p, _lib.FormParams):
        raise ValueError("params must come from bliss_amd.form.params()")
    return p


def form_to_numpy(raw):
    """bytes / uint8 array of bl_amd_song_form records -> structured numpy array with the header's field names."""
    return np.frombuffer(bytes(raw), dtype=FORM_DTYPE).copy()


def form_device(frames, counts, p, units=False, rep=False, novelty=False, flags=False, ctx=None):
    """Enqueue the structure of songs whose chroma frame records sit in the CUDA uint8 tensor `frames`, concatenated,
    counts[i] frames each (bl_amd_form_device), on torch's current stream.  Returns a dict: "records" (CUDA uint8 tensor,
    form_to_numpy() reads it once the stream has been waited for), "units" (the per-song unit counts) and, for each
    output asked for, "unit_bytes" (uint8 (n, 16)), "rep" (int32 (n, 2) holding the uint32 patterns), "novelty" (int64
    (n,) holding the uint64 values, which stay below 2^40) and "flags" (uint8 (n,)), concatenated over the songs."""
    import torch
    p = _params(p)
    vals, arr = _counts(counts)
    if frames.dtype != torch.uint8 or frames.numel() < sum(vals) * FRAME_CHROMA_DTYPE.itemsize:
        raise ValueError("frames must be a uint8 tensor that holds every song's frame records")
    ucounts = [t // p.pool for t in vals]
    n = sum(ucounts)
    dev = frames.device
    out = {"units": ucounts}
    with torch.cuda.device(dev):
        check(_lib.load().bl_amd_init(dev.index or 0), "bl_amd_init")
        out["records"] = torch.empty(len(vals) * FORM_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        for name, on, shp, dt in (("unit_bytes", units, (max(n, 1), 16), torch.uint8),
                                  ("rep", rep, (max(n, 1), 2), torch.int32),
                                  ("novelty", novelty, (max(n, 1),), torch.int64),
                                  ("flags", flags, (max(n, 1),), torch.uint8)):
            out[name] = torch.empty(shp, dtype=dt, device=dev) if on else None
        # a tensor without elements has no pointer the library would take: one record stands in for it
        fr = frames if frames.numel() else torch.zeros(FRAME_CHROMA_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p()
        args = (ptr(fr), arr, len(vals), C.byref(p), ptr(out["records"]), ptr(out["unit_bytes"]), ptr(out["rep"]),
                ptr(out["novelty"]), ptr(out["flags"]), n, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        lib = _lib.load()
        if ctx is None:
            check(lib.bl_amd_form_device(*args), "bl_amd_form_device")
        else:
            check(lib.bl_amd_ctx_form_device(ctx.handle, *args), "bl_amd_ctx_form_device")
    for name in ("unit_bytes", "rep", "novelty", "flags"):
        if out[name] is None:
            del out[name]
        else:
            out[name] = out[name][:n]
    return out


def _frame_records(frames):
    """frame records as a contiguous uint64 array of shape (T, 12): FRAME_CHROMA_DTYPE records or such an array"""
    a = np.asarray(frames)
    if a.dtype == FRAME_CHROMA_DTYPE:
        a = a["x"]
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.ndim != 2 or a.shape[1] != 12:
        raise ValueError(f"frames must be bl_amd_frame_chroma records or have shape (T, 12), got {a.shape}")
    return a


def form_host(frames, counts, p, units=False, rep=False, novelty=False, flags=False):
    """The structure of songs whose chroma frames are in host memory (bl_amd_form_host), blocking: frames the records
    of all songs concatenated (FRAME_CHROMA_DTYPE records or uint64 (T, 12)), counts[i] frames each.  Returns the dict
    form_device returns, with numpy arrays: "records" structured, "rep" uint32, "novelty" uint64."""
    p = _params(p)
    x = _frame_records(frames)
    vals, arr = _counts(counts)
    if x.shape[0] != sum(vals):
        raise ValueError(f"{x.shape[0]} frame records but the counts add up to {sum(vals)}")
    ucounts = [t // p.pool for t in vals]
    n = sum(ucounts)
    if x.shape[0] == 0:
        x = np.zeros((1, 12), dtype=np.uint64)
    rec = (_lib.SongForm * len(vals))()
    out = {"units": ucounts}
    for name, on, shp, dt in (("unit_bytes", units, (max(n, 1), 16), np.uint8), ("rep", rep, (max(n, 1), 2), np.uint32),
                              ("novelty", novelty, (max(n, 1),), np.uint64), ("flags", flags, (max(n, 1),), np.uint8)):
        out[name] = np.zeros(shp, dtype=dt) if on else None
    ptr = lambda a: C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p()
    check(_lib.load().bl_amd_form_host(ptr(x), arr, len(vals), C.byref(p), rec, ptr(out["unit_bytes"]), ptr(out["rep"]),
                                       ptr(out["novelty"]), ptr(out["flags"])), "bl_amd_form_host")
    out["records"] = form_to_numpy(bytes(rec))
    for name in ("unit_bytes", "rep", "novelty", "flags"):
        if out[name] is None:
            del out[name]
        else:
            out[name] = out[name][:n]
    return out


def from_device_corpus(corpus, p, ctx=None, **outputs):
    """Chroma frames, then structure, of every song of a DeviceCorpus on torch's current stream (chroma_device with
    frames, bl_amd_form_device).  Returns what form_device returns."""
    songs, frames = chroma_device(corpus, frames=True, ctx=ctx)
    return form_device(frames, _frames(*corpus._songs()), p, ctx=ctx, **outputs)


def from_pcm(pcm_list, channels, p, **outputs):
    """The structure of songs in host memory: chroma_batch_host with frames, then form_host."""
    songs, frames = chroma_batch_host(pcm_list, channels, frames=True)
    return form_host(frames, [int(t) for t in songs["frames"]], p, **outputs)


def _records(records):
    rec = np.ascontiguousarray(records)
    if rec.dtype != FORM_DTYPE or rec.ndim != 1 or rec.size < 1:
        raise ValueError("records must be a non-empty 1-D array of bl_amd_song_form records")
    return rec, rec.ctypes.data_as(C.POINTER(_lib.SongForm))


def score(records):
    """float64 array of thumb_score / thumb_self of each record (bl_amd_form_score): near 1 for a stretch that comes
    back unchanged; NaN for a song without a thumbnail."""
    rec, ptr = _records(records)
    lib = _lib.load()
    return np.array([lib.bl_amd_form_score(C.byref(ptr[i])) for i in range(rec.size)], dtype=np.float64)


def seconds(unit, pool=1, rate=22050):
    """The time at which unit `unit` starts (bl_amd_form_seconds): unit * pool * 2048 / rate."""
    return _lib.load().bl_amd_form_seconds(int_in("unit", unit, 0), _pool(pool), int_in("rate", rate, 1))


def sections(flags, units):
    """The (start, end) unit ranges between the boundaries of one song: flags its `units` flag bytes (bit 0 = boundary).
    A boundary at unit 0 opens no section of its own."""
    units = int_in("units", units, 0)
    f = np.asarray(flags).reshape(-1)
    if f.size < units:
        raise ValueError(f"{f.size} flags for {units} units")
    cuts = [0] + [int(u) for u in np.flatnonzero(f[:units].astype(np.uint8) & 1) if u > 0] + [units]
    return [(a, b) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
