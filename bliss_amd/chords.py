"""Chord sequences (include/bliss_amd.h: bl_amd_song_chords, bl_amd_chords_*): which of the 24 major and minor triads,
or no chord, sounds in every unit of a song.  The units are those of the structure call and the version matching
(bliss_amd.cover.units_device / units_host); triad templates over a unit's twelve chroma values are decoded by Viterbi
under a table of transition costs, so a label holds until the evidence against it outweighs a change.  Everything the
device computes is an exact integer, so two runs agree to the bit.

The defaults (none 150, change 60, related 15) label synthetic triad progressions, silence and noise correctly
(DESIGN.md 4.25).  There is no annotated music to learn them from here: they have not been tuned on recorded music.

This module is imported explicitly (`import bliss_amd.chords`): the package's own namespace is unchanged."""
import ctypes as C

import numpy as np

from . import _lib
from ._args import int_in
from ._lib import check
from .cover import from_pcm as _units_from_pcm
from .records import CHORDS_DTYPE

LABELS, NONE, EMPTY = 25, 24, 1                # BL_AMD_CHORDS_LABELS, BL_AMD_CHORDS_NONE, BL_AMD_CHORDS_EMPTY
COST_MAX, EMISSION_MAX = 1024, 381             # BL_AMD_CHORDS_COST_MAX, BL_AMD_CHORDS_EMISSION_MAX
COUNT_MAX = (1 << 20) - 1                      # counts < 2^20


def costs(change=60, related=15):
    """The (25, 25) uint16 table of bl_amd_chords_costs: 0 on the diagonal, `change` to and from N, and between two
    chords change - related x (the pitch classes they share).  Needs 0 <= 2 related <= change <= 1024."""
    change, related = int_in("change", change, 0, COST_MAX), int_in("related", related, 0, COST_MAX)
    if 2 * related > change:
        raise ValueError(f"2 related must not exceed change, got related {related!r} and change {change!r}")
    out = (C.c_uint16 * (LABELS * LABELS))()
    check(_lib.load().bl_amd_chords_costs(change, related, out), "bl_amd_chords_costs")
    return np.array(out, dtype=np.uint16).reshape(LABELS, LABELS)


def params(none=150, change=60, related=15, cost=None):
    """A bl_amd_chords_params: `none` is what "no chord" scores in every unit (0 .. 381, against the sum of a triad's
    three chroma values), and the transition costs are costs(change, related) or, if given, `cost`: (25, 25) integers
    in 0 .. 1024, cost[a][b] for going from label a to label b, the diagonal included.  The defaults are those of a
    prototype on synthetic progressions and are not tuned on music."""
    none = int_in("none", none, 0, EMISSION_MAX)
    if cost is None:
        table = costs(change, related)
    else:
        table = np.asarray(cost)
        if table.shape != (LABELS, LABELS) or table.dtype == np.bool_ or not np.issubdtype(table.dtype, np.integer):
            raise ValueError(f"cost must be (25, 25) integers, got shape {table.shape} of {table.dtype}")
        if table.min() < 0 or table.max() > COST_MAX:
            raise ValueError(f"every cost must lie in [0, {COST_MAX}], got {int(table.min())} .. {int(table.max())}")
    p = _lib.ChordsParams()
    p.none, p.reserved = none, 0
    p.cost[:] = [int(v) for v in np.asarray(table).reshape(-1)]
    return p


def _params(p):
    if not isinstance(p, _lib.ChordsParams):
        raise ValueError("params must come from bliss_amd.chords.params()")
    return p


def shape():
    """(units the forward kernel takes at a time, units the back-trace takes at a time, songs that share a wavefront)
    (bl_amd_chords_shape): the lengths at which the kernels change path."""
    v = [C.c_int() for _ in range(3)]
    _lib.load().bl_amd_chords_shape(*[C.byref(x) for x in v])
    return tuple(x.value for x in v)


def name(label):
    """"C" .. "B", "Cm" .. "Bm", "N" (bl_amd_chords_name); "" for any other label."""
    return _lib.load().bl_amd_chords_name(int_in("label", label, -2 ** 31, 2 ** 31 - 1)).decode()


def segments(labels):
    """The runs of equal labels (bl_amd_chords_segments) as (first units int32, labels uint8); a unit's time is
    bliss_amd.cover.seconds(unit, pool)."""
    lab = np.ascontiguousarray(labels, dtype=np.uint8).reshape(-1)
    lib = _lib.load()
    ptr = C.c_void_p(lab.ctypes.data) if lab.size else None
    n = lib.bl_amd_chords_segments(ptr, lab.size, None, None, 0)
    if n < 0:
        raise ValueError("labels were refused")
    starts, chords = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint8)
    if n:
        lib.bl_amd_chords_segments(ptr, lab.size, C.c_void_p(starts.ctypes.data), C.c_void_p(chords.ctypes.data), n)
    return starts, chords


def _counts(counts):
    vals = [int_in("counts", c, 0, COUNT_MAX) for c in counts]
    if not vals:
        raise ValueError("at least one song is needed")
    return vals, (C.c_int32 * len(vals))(*vals)


def chords_to_numpy(raw):
    """bytes / uint8 array of bl_amd_song_chords records -> structured numpy array with the header's field names."""
    return np.frombuffer(bytes(raw), dtype=CHORDS_DTYPE).copy()


def chords_device(units, counts, p=None, labels=False, hist=False, ctx=None):
    """Enqueue the chords of songs whose units sit in the CUDA uint8 tensor `units` (16 bytes each, concatenated,
    counts[i] units per song) on torch's current stream (bl_amd_chords_device).  p: params(), None for the defaults.
    Returns a dict of CUDA tensors: "records" (uint8, 32 bytes per song; chords_to_numpy() reads them once the stream
    has been waited for) and, where asked for, "labels" (uint8 per unit) and "hist" (int32 (songs, 25), the units per
    label)."""
    import torch
    p = params() if p is None else _params(p)
    vals, arr = _counts(counts)
    total = sum(vals)
    if units.dtype != torch.uint8 or units.numel() < 16 * total or not units.is_contiguous():
        raise ValueError("units must be a contiguous uint8 tensor that holds every song's units, 16 bytes each")
    dev = units.device
    with torch.cuda.device(dev):
        check(_lib.load().bl_amd_init(dev.index or 0), "bl_amd_init")
        out = {"records": torch.empty(len(vals) * CHORDS_DTYPE.itemsize, dtype=torch.uint8, device=dev)}
        if labels:
            out["labels"] = torch.empty(total, dtype=torch.uint8, device=dev)
        if hist:
            out["hist"] = torch.empty((len(vals), LABELS), dtype=torch.int32, device=dev)
        # a tensor without elements has no pointer the library would take: one unit / one byte stands in for it
        u = units if units.numel() else torch.zeros(16, dtype=torch.uint8, device=dev)
        lab = None
        if labels:
            lab = out["labels"] if total else torch.zeros(1, dtype=torch.uint8, device=dev)
        args = (C.c_void_p(u.data_ptr()), arr, len(vals), total, C.byref(p), C.c_void_p(out["records"].data_ptr()),
                C.c_void_p(lab.data_ptr()) if labels else None, C.c_void_p(out["hist"].data_ptr()) if hist else None,
                C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        lib = _lib.load()
        if ctx is None:
            check(lib.bl_amd_chords_device(*args), "bl_amd_chords_device")
        else:
            check(lib.bl_amd_ctx_chords_device(ctx.handle, *args), "bl_amd_ctx_chords_device")
    return out


def chords_host(units, counts, p=None, labels=False, hist=False):
    """The chords of songs whose units are in host memory (bl_amd_chords_host), blocking.  Returns the records as a
    structured array, or (records, labels uint8 per unit or None, hist uint32 (songs, 25) or None) when either is
    asked for."""
    p = params() if p is None else _params(p)
    vals, arr = _counts(counts)
    total = sum(vals)
    u = np.ascontiguousarray(units, dtype=np.uint8).reshape(-1)
    if u.size < 16 * total:
        raise ValueError("units must hold every song's units, 16 bytes each")
    if not u.size:
        u = np.zeros(16, dtype=np.uint8)
    rec = (_lib.SongChords * len(vals))()
    lab = np.zeros(max(total, 1), dtype=np.uint8) if labels else None
    hs = np.zeros((len(vals), LABELS), dtype=np.uint32) if hist else None
    check(_lib.load().bl_amd_chords_host(C.c_void_p(u.ctypes.data), arr, len(vals), C.byref(p), rec,
                                         C.c_void_p(lab.ctypes.data) if labels else None,
                                         C.c_void_p(hs.ctypes.data) if hist else None), "bl_amd_chords_host")
    records = chords_to_numpy(bytes(rec))
    if not labels and not hist:
        return records
    return records, (lab[:total] if labels else None), hs


def from_pcm(pcm_list, channels, pool=1, p=None):
    """(records, labels, per-song unit counts) of songs in host memory: the chroma call with frames, then the units
    (bliss_amd.cover.from_pcm), then chords_host with the labels."""
    units, counts = _units_from_pcm(pcm_list, channels, pool)
    records, labels, _ = chords_host(units, counts, p, labels=True)
    return records, labels, counts
