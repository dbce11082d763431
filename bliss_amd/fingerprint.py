"""Audio fingerprints and offset matching (include/bliss_amd.h: bl_amd_fprint_match, bl_amd_fprint_*): one 32-bit word
per chroma frame, and for a pair of songs the shift at which their words disagree least, with the bit-error rate there.
A low rate says "the same recording", the shift says how much earlier one copy starts.  Everything the device computes
is an exact integer, so two runs agree to the bit.

This module is imported explicitly (`import bliss_amd.fingerprint`): the package's own namespace is unchanged."""
import ctypes as C

import numpy as np

from . import _lib
from ._args import int_in
from ._lib import check
from .chroma import _frames, chroma_batch_host, chroma_device
from .records import FPRINT_MATCH_DTYPE, FRAME_CHROMA_DTYPE

FRAMES, SHIFT_MAX, COUNT_MAX = 16, 1024, (1 << 20) - 1   # BL_AMD_FPRINT_FRAMES, BL_AMD_FPRINT_SHIFT_MAX, T < 2^20


def words_count(frames):
    """W of a song with `frames` chroma frames (bl_amd_fprint_words)."""
    return _lib.load().bl_amd_fprint_words(int_in("frames", frames, 0))


def shape(max_shift):
    """(words per workgroup of the words kernel, words of `a` a lane walks per tile, words of `a` per tile, offsets a
    workgroup takes at a time) at max_shift (bl_amd_fprint_shape): the lengths at which the kernels' paths change."""
    v = [C.c_int() for _ in range(4)]
    _lib.load().bl_amd_fprint_shape(int_in("max_shift", max_shift, 0, SHIFT_MAX), *[C.byref(x) for x in v])
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


def words_from_frames_device(frames, counts, ctx=None):
    """Enqueue the words of songs whose chroma frame records sit in the CUDA uint8 tensor `frames`, concatenated, counts[i]
    frames each (bl_amd_fprint_words_device), on torch's current stream.  Returns (words as a CUDA int32 tensor holding
    the 32-bit patterns, the per-song word counts)."""
    import torch
    vals, arr = _counts("frames", counts)
    if frames.dtype != torch.uint8 or frames.numel() < sum(vals) * FRAME_CHROMA_DTYPE.itemsize:
        raise ValueError("frames must be a uint8 tensor that holds every song's frame records")
    wcounts = [max(0, t - (FRAMES - 1)) for t in vals]
    total = sum(wcounts)
    with torch.cuda.device(frames.device):
        check(_lib.load().bl_amd_init(frames.device.index or 0), "bl_amd_init")
        words = torch.empty(max(total, 1), dtype=torch.int32, device=frames.device)
        _call("fprint_words_device", ctx, C.c_void_p(frames.data_ptr()), arr, len(vals), C.c_void_p(words.data_ptr()),
              total, _stream(torch, frames.device))
    return words[:total], wcounts


def words_device(corpus, ctx=None):
    """Chroma frames, then words, of every song of a DeviceCorpus on torch's current stream (chroma_device with frames,
    bl_amd_fprint_words_device).  Returns (words, counts) as words_from_frames_device does."""
    songs, frames = chroma_device(corpus, frames=True, ctx=ctx)
    return words_from_frames_device(frames, _frames(*corpus._songs()), ctx=ctx)


def _frame_records(frames):
    """frame records as a contiguous uint64 array of shape (T, 12): FRAME_CHROMA_DTYPE records or such an array"""
    a = np.asarray(frames)
    if a.dtype == FRAME_CHROMA_DTYPE:
        a = a["x"]
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.ndim != 2 or a.shape[1] != 12:
        raise ValueError(f"frames must be bl_amd_frame_chroma records or have shape (T, 12), got {a.shape}")
    return a


def words_host(frames, counts):
    """The words of songs whose chroma frames are in host memory (bl_amd_fprint_words_host), blocking: frames the
    records of all songs concatenated (FRAME_CHROMA_DTYPE records or uint64 (T, 12)), counts[i] frames each.  Returns
    (words uint32, per-song word counts)."""
    x = _frame_records(frames)
    vals, arr = _counts("frames", counts)
    if x.shape[0] != sum(vals):
        raise ValueError(f"{x.shape[0]} frame records but the counts add up to {sum(vals)}")
    wcounts = [max(0, t - (FRAMES - 1)) for t in vals]
    words = np.zeros(max(sum(wcounts), 1), dtype=np.uint32)
    if x.shape[0] == 0:
        x = np.zeros((1, 12), dtype=np.uint64)
    check(_lib.load().bl_amd_fprint_words_host(C.c_void_p(x.ctypes.data), arr, len(vals), C.c_void_p(words.ctypes.data)),
          "bl_amd_fprint_words_host")
    return words[:sum(wcounts)], wcounts


def from_pcm(pcm_list, channels):
    """(words, counts) of songs in host memory: chroma_batch_host with frames, then words_host."""
    songs, frames = chroma_batch_host(pcm_list, channels, frames=True)
    return words_host(frames, [int(t) for t in songs["frames"]])


def pairs_from_knn(indices):
    """An (n, k) array of neighbour indices (row i: the neighbours of song i, as knn() returns them) as the (n k, 2)
    int32 pair list (i, neighbour).  Empty slots (-1) stay: the match answers them with a failed record."""
    idx = np.asarray(indices)
    if idx.ndim != 2 or idx.dtype == np.bool_ or not np.issubdtype(idx.dtype, np.integer):
        raise ValueError(f"indices must be an integer array of shape (n, k), got {idx.dtype} {idx.shape}")
    n, k = idx.shape
    out = np.empty((n * k, 2), dtype=np.int32)
    out[:, 0] = np.repeat(np.arange(n, dtype=np.int32), k)
    out[:, 1] = idx.reshape(-1)
    return out


def _match_args(max_shift, min_overlap):
    return int_in("max_shift", max_shift, 0, SHIFT_MAX), int_in("min_overlap", min_overlap, 1, 2 ** 31 - 1)


def _pairs_shape_check(shape):
    if len(shape) != 2 or shape[1] != 2 or shape[0] < 1:
        raise ValueError(f"pairs must have shape (n, 2) with n >= 1, got {tuple(shape)}")


def match_to_numpy(raw):
    """bytes / uint8 array of bl_amd_fprint_match records -> structured numpy array with the header's field names."""
    return np.frombuffer(bytes(raw), dtype=FPRINT_MATCH_DTYPE).copy()


def match_device(words_a, counts_a, pairs, max_shift=64, min_overlap=1, words_b=None, counts_b=None, profile=False,
                 ctx=None):
    """Enqueue the match of every pair (bl_amd_fprint_match_device) on torch's current stream.  words_a: CUDA int32
    tensor of set a's words, counts_a its per-song counts; words_b / counts_b: set b, or None for the self form.
    pairs: (n, 2) int32, a CUDA tensor or a host array (uploaded on the stream).  Returns (records as a CUDA uint8
    tensor, the profile as a CUDA int32 tensor of shape (n, 2 max_shift + 1, 2) or None); match_to_numpy() reads the
    records once the stream has been waited for."""
    import torch
    max_shift, min_overlap = _match_args(max_shift, min_overlap)
    if words_b is None:
        words_b, counts_b = words_a, counts_a
    va, arr_a = _counts("counts_a", counts_a)
    vb, arr_b = _counts("counts_b", counts_b)
    for name, w, v in (("words_a", words_a, va), ("words_b", words_b, vb)):
        if w.dtype != torch.int32 or w.numel() < sum(v) or w.device != words_a.device:
            raise ValueError(f"{name} must be an int32 tensor on one device that holds every song's words")
    dev = words_a.device
    with torch.cuda.device(dev):
        check(_lib.load().bl_amd_init(dev.index or 0), "bl_amd_init")
        if not torch.is_tensor(pairs):
            pairs = torch.from_numpy(np.ascontiguousarray(pairs, dtype=np.int32)).to(dev, non_blocking=False)
        _pairs_shape_check(pairs.shape)
        if pairs.dtype != torch.int32 or pairs.device != dev or not pairs.is_contiguous():
            raise ValueError("pairs must be a contiguous int32 tensor on the words' device")
        n = pairs.shape[0]
        rec = torch.empty(n * FPRINT_MATCH_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        prof = torch.empty((n, 2 * max_shift + 1, 2), dtype=torch.int32, device=dev) if profile else None
        # a tensor without elements has no pointer the library would take: one word stands in for it
        pa = words_a if words_a.numel() else torch.zeros(1, dtype=torch.int32, device=dev)
        pb = words_b if words_b.numel() else pa
        _call("fprint_match_device", ctx, C.c_void_p(pa.data_ptr()), arr_a, len(va), C.c_void_p(pb.data_ptr()), arr_b,
              len(vb), C.c_void_p(pairs.data_ptr()), n, max_shift, min_overlap, C.c_void_p(rec.data_ptr()),
              C.c_void_p(prof.data_ptr()) if profile else C.c_void_p(), _stream(torch, dev))
    return rec, prof


def match_host(words_a, counts_a, pairs, max_shift=64, min_overlap=1, words_b=None, counts_b=None, profile=False):
    """The match of every pair with everything in host memory (bl_amd_fprint_match_host), blocking.  Returns (records,
    the profile as a uint32 array of shape (n, 2 max_shift + 1, 2) or None)."""
    max_shift, min_overlap = _match_args(max_shift, min_overlap)
    a = np.ascontiguousarray(words_a, dtype=np.uint32).reshape(-1)
    va, arr_a = _counts("counts_a", counts_a)
    if words_b is None:
        b, vb, arr_b = a, va, arr_a
    else:
        b = np.ascontiguousarray(words_b, dtype=np.uint32).reshape(-1)
        vb, arr_b = _counts("counts_b", counts_b)
    if a.size < sum(va) or b.size < sum(vb):
        raise ValueError("the words must hold every song's words")
    if a.size == 0:
        a = np.zeros(1, dtype=np.uint32)
    if b.size == 0:
        b = a
    p = np.ascontiguousarray(pairs, dtype=np.int32)
    _pairs_shape_check(p.shape)
    n = p.shape[0]
    out = (_lib.FprintMatch * n)()
    prof = np.zeros((n, 2 * max_shift + 1, 2), dtype=np.uint32) if profile else None
    check(_lib.load().bl_amd_fprint_match_host(
        C.c_void_p(a.ctypes.data), arr_a, len(va), C.c_void_p(b.ctypes.data), arr_b, len(vb), C.c_void_p(p.ctypes.data),
        n, max_shift, min_overlap, out, C.c_void_p(prof.ctypes.data) if profile else C.c_void_p()),
        "bl_amd_fprint_match_host")
    return match_to_numpy(bytes(out)), prof


def _records(records):
    rec = np.ascontiguousarray(records)
    if rec.dtype != FPRINT_MATCH_DTYPE or rec.ndim != 1 or rec.size < 1:
        raise ValueError("records must be a non-empty 1-D array of bl_amd_fprint_match records")
    return rec, rec.ctypes.data_as(C.POINTER(_lib.FprintMatch))


def ber(records):
    """float64 array of the bit-error rate at each record's best offset (bl_amd_fprint_ber): errors / (32 overlap), NaN
    for a failed record."""
    rec, ptr = _records(records)
    lib = _lib.load()
    return np.array([lib.bl_amd_fprint_ber(C.byref(ptr[i])) for i in range(rec.size)], dtype=np.float64)


def offset_seconds(records, rate=22050):
    """float64 array of each record's offset in seconds (bl_amd_fprint_offset_seconds): offset * 2048 / rate, positive
    when the second song of the pair carries more lead-in; NaN for a failed record."""
    rec, ptr = _records(records)
    rate = int_in("rate", rate, 1)
    lib = _lib.load()
    return np.array([lib.bl_amd_fprint_offset_seconds(C.byref(ptr[i]), rate) for i in range(rec.size)],
                    dtype=np.float64)
