"""Tempo over time (include/bliss_amd.h: bl_amd_tgram_frame, bl_amd_song_tgram, bl_amd_tgram_*): the lag products of the
tempo call over a sliding window of the onset curve and its pick on every window, so that a player can tell whether a
song's tempo is steady and what it is at the song's two ends.  Everything the device computes is an exact integer, so
two runs agree to the bit.

The defaults (a stride of 128 hops, 16 blocks: windows of 11.9 s every 0.74 s at 22 050 Hz; tol 60 per mille; octaves
on) have not been tuned on recorded music: there is none here.

This module is imported explicitly (`import bliss_amd.tempogram`): the package's own namespace is unchanged."""
import ctypes as C

import numpy as np

from . import _lib
from ._args import int_in
from ._lib import check
from .records import TBEATS_DTYPE, TGRAM_DTYPE, TGRAM_FRAME_DTYPE
from .rhythm import HOP, LAGS, _curves_check, _hops_check, _lags_check

STRIDE_MAX, BLOCKS_MAX, TOL_MAX = 1024, 16, 1000


def params(stride=128, blocks=16, lag_min=20, lag_max=200, tol=60, octaves=True):
    """A bl_amd_tgram_params: the window moves by `stride` hops (a multiple of 16 in 16 .. 1024) and is `blocks`
    (1 .. 16) strides long; the pick is over lag_min .. lag_max (within 1 .. 510); two lags are near each other within
    `tol` per mille (0 .. 1000) and, with `octaves`, also when one is twice the other within it."""
    stride = int_in("stride", stride, 16, STRIDE_MAX)
    if stride % 16:
        raise ValueError(f"stride must be a multiple of 16, got {stride!r}")
    p = _lib.TgramParams()
    p.stride, p.blocks = stride, int_in("blocks", blocks, 1, BLOCKS_MAX)
    p.lag_min, p.lag_max = _lags_check(lag_min, lag_max)
    p.tol, p.octaves = int_in("tol", tol, 0, TOL_MAX), 1 if octaves else 0
    return p


def _params(p):
    if p is None:
        return params()
    if not isinstance(p, _lib.TgramParams):
        raise ValueError("params must come from bliss_amd.tempogram.params()")
    return p


def frames_count(hops, p=None):
    """F of a song of `hops` hops (bl_amd_tgram_frames): (T - W) / S + 1 with T = hops - 511, or 0 when T < W."""
    n = _lib.load().bl_amd_tgram_frames(int_in("hops", hops, 1, (1 << 24) - 1), C.byref(_params(p)))
    if n < 0:
        raise ValueError("the parameters were refused")
    return n


def shape():
    """(terms of the curve the block kernel stages at a time, frames of one run of it) (bl_amd_tgram_shape): the
    lengths at which the kernels change path."""
    v = [C.c_int() for _ in range(2)]
    _lib.load().bl_amd_tgram_shape(*[C.byref(x) for x in v])
    return tuple(x.value for x in v)


def tgram_to_numpy(raw_songs, raw_frames=None):
    """bytes / uint8 arrays of bl_amd_song_tgram (and bl_amd_tgram_frame) records -> structured numpy arrays with the
    header's field names.  Returns the song array, or (songs, frames) when raw_frames is given."""
    songs = np.frombuffer(bytes(raw_songs), dtype=TGRAM_DTYPE).copy()
    if raw_frames is None:
        return songs
    return songs, np.frombuffer(bytes(raw_frames), dtype=TGRAM_FRAME_DTYPE).copy()


def tgram_device(onsets, hops, p=None, gram=False, ctx=None):
    """Enqueue the tempograms of n songs (bl_amd_tgram_device) on torch's current stream.  onsets: a contiguous 1-D
    int32 CUDA tensor holding the uint32 onset curves one behind the other (what bliss_amd.rhythm.rhythm_device()
    returns); hops: the n hop counts.  Returns a dict of CUDA tensors: "songs" (uint8, 56 bytes per song), "frames"
    (uint8, 40 bytes per frame, songs concatenated) and, where asked for, "gram" (int64 holding the uint64 lag products,
    shape (frames, 512)); tgram_to_numpy() reads the records once the stream has been waited for.  "counts" holds the
    frames per song as a list."""
    import torch
    from .queries import _on_device_of
    p = _params(p)
    hops = _hops_check(hops)
    n, total = len(hops), sum(hops)
    if onsets.dtype != torch.int32 or not onsets.is_cuda or not onsets.is_contiguous() or onsets.dim() != 1 or \
            onsets.numel() != total:
        raise ValueError(f"onsets must be a contiguous 1-D int32 CUDA tensor of sum(hops) = {total} values")
    counts = [frames_count(h, p) for h in hops]
    nf = sum(counts)
    lib = _lib.load()
    dev = onsets.device
    out = {"songs": torch.empty(n * TGRAM_DTYPE.itemsize, dtype=torch.uint8, device=dev),
           "frames": torch.empty(nf * TGRAM_FRAME_DTYPE.itemsize, dtype=torch.uint8, device=dev), "counts": counts}
    if gram:
        out["gram"] = torch.empty((nf, LAGS), dtype=torch.int64, device=dev)
    with _on_device_of(lib, onsets, None) as cur:
        args = (C.c_void_p(onsets.data_ptr()), (C.c_int32 * n)(*hops), n, C.byref(p),
                C.c_void_p(out["songs"].data_ptr()), C.c_void_p(out["frames"].data_ptr()) if nf else None, nf,
                C.c_void_p(out["gram"].data_ptr()) if gram and nf else None, C.c_void_p(cur.cuda_stream))
        if ctx is None:
            check(lib.bl_amd_tgram_device(*args), "bl_amd_tgram_device")
        else:
            check(lib.bl_amd_ctx_tgram_device(ctx.handle, *args), "bl_amd_ctx_tgram_device")
    return out


def tgram_host(onsets_list, p=None, gram=False):
    """Tempograms of onset curves in host memory (bl_amd_tgram_host), blocking: onsets_list as
    bliss_amd.rhythm.rhythm_from_onsets() takes it.  Returns (songs, frames, gram or None): the records as
    tgram_to_numpy() gives them, the frames of all songs one behind the other (songs["frames"] each), gram a uint64 array
    of shape (frames, 512)."""
    p = _params(p)
    curves = _curves_check(onsets_list)
    n = len(curves)
    flat = np.ascontiguousarray(np.concatenate(curves), dtype=np.uint32)
    nf = sum(frames_count(o.size, p) for o in curves)
    songs = (_lib.SongTgram * n)()
    frames = (_lib.TgramFrame * max(nf, 1))()
    rows = np.zeros((nf, LAGS), dtype=np.uint64) if gram else None
    check(_lib.load().bl_amd_tgram_host(C.c_void_p(flat.ctypes.data), (C.c_int32 * n)(*[o.size for o in curves]), n,
                                        C.byref(p), songs, frames,
                                        C.c_void_p(rows.ctypes.data) if gram and nf else None), "bl_amd_tgram_host")
    s, f = tgram_to_numpy(bytes(songs), bytes(frames))
    return s, f[:nf], rows


def from_pcm(pcm_list, channels, p=None, gram=False):
    """(songs, frames, gram or None, per-song hop counts) of songs in host memory: the tempo call with its onset curves
    (bliss_amd.rhythm.rhythm_device) and then this call on them, both on the device; only the records come back."""
    import torch
    import bliss_amd
    from .rhythm import rhythm_device
    p = _params(p)
    arrs = [np.ascontiguousarray(a, dtype=np.int16).reshape(-1) for a in pcm_list]
    corpus = bliss_amd.DeviceCorpus([a.size for a in arrs], channels, 1)
    for i, a in enumerate(arrs):
        corpus.upload(i, a)
    _, ons, _ = rhythm_device(corpus, p.lag_min, p.lag_max, onsets=True)
    lengths, chs = corpus._songs()
    hops = [int(ln) // ch // HOP for ln, ch in zip(lengths, chs)]
    with torch.cuda.device(corpus.device):
        out = tgram_device(ons, hops, p, gram=gram)
        torch.cuda.synchronize(corpus.device)
    s, f = tgram_to_numpy(out["songs"].cpu().numpy().tobytes(), out["frames"].cpu().numpy().tobytes())
    return s, f, (out["gram"].cpu().numpy().view(np.uint64) if gram else None), hops


def _frames_array(frames):
    fr = np.ascontiguousarray(frames)
    if fr.dtype != TGRAM_FRAME_DTYPE or fr.ndim != 1:
        raise ValueError("frames must be a 1-D array of bl_amd_tgram_frame records (tgram_to_numpy)")
    return fr


def bpm(frames, rate=22050):
    """float64 array of the tempo of every frame in beats per minute (bl_amd_tgram_bpm), NaN where lag == 0."""
    fr = _frames_array(frames)
    rate = int_in("rate", rate, 1, 2 ** 31 - 1)
    lib = _lib.load()
    ptr = fr.ctypes.data_as(C.POINTER(_lib.TgramFrame))
    return np.array([lib.bl_amd_tgram_bpm(C.byref(ptr[i]), rate) for i in range(fr.size)], dtype=np.float64)


def seconds(frame, p=None, rate=22050):
    """The time of the centre of a frame's window in seconds (bl_amd_tgram_seconds)."""
    return _lib.load().bl_amd_tgram_seconds(int_in("frame", frame, 0, 2 ** 31 - 1), C.byref(_params(p)),
                                            int_in("rate", rate, 1, 2 ** 31 - 1))


def steadiness(songs):
    """float64 array of n_near / n_tempo per song (bl_amd_tgram_steadiness): the share of the frames whose tempo is the
    song's median tempo; 0 where no frame has a tempo."""
    st = np.ascontiguousarray(songs)
    if st.dtype != TGRAM_DTYPE or st.ndim != 1:
        raise ValueError("songs must be a 1-D array of bl_amd_song_tgram records (tgram_to_numpy)")
    lib = _lib.load()
    ptr = st.ctypes.data_as(C.POINTER(_lib.SongTgram))
    return np.array([lib.bl_amd_tgram_steadiness(C.byref(ptr[i])) for i in range(st.size)], dtype=np.float64)


# ---- beats that follow the tempo over time (bl_amd_tbeats_*) --------------------------------------------------------

SEG_MAX, TIGHT_MAX, FRAMES_MAX = 16384, 4096, 1 << 20


def beats_params(p=None, tight=128, fold=False, seg=None, origin=None):
    """A bl_amd_tbeats_params.  From a tempogram's parameters (bl_amd_tbeats_params_from_tgram): a frame speaks for the
    `stride` hops around the centre of its window, so seg = stride and origin = (blocks - 1) stride / 2.  With `seg`
    (16 .. 16 384) and `origin` (0 .. 2^24 - 1) given, those instead.  tight (0 .. 4096) is that of
    bliss_amd.rhythm.beats_device; with `fold`, a frame whose lag is near half or twice the song's anchor lag is moved
    by an octave towards it."""
    tight = int_in("tight", tight, 0, TIGHT_MAX)
    bp = _lib.TbeatsParams()
    if seg is None and origin is None:
        check(_lib.load().bl_amd_tbeats_params_from_tgram(C.byref(_params(p)), tight, 1 if fold else 0, C.byref(bp)),
              "bl_amd_tbeats_params_from_tgram")
        return bp
    bp.seg, bp.origin = int_in("seg", seg, 16, SEG_MAX), int_in("origin", 0 if origin is None else origin, 0, (1 << 24) - 1)
    bp.tight, bp.fold = tight, 1 if fold else 0
    return bp


def _beats_params(bp):
    if bp is None:
        return beats_params()
    if not isinstance(bp, _lib.TbeatsParams):
        raise ValueError("params must come from bliss_amd.tempogram.beats_params()")
    return bp


def beats_shape():
    """(scores the grid kernel keeps on the chip, frames the track kernel scans at a time) (bl_amd_tbeats_shape)."""
    v = [C.c_int() for _ in range(2)]
    _lib.load().bl_amd_tbeats_shape(*[C.byref(x) for x in v])
    return tuple(x.value for x in v)


def beats_to_numpy(raw_songs):
    """bytes / a uint8 array of bl_amd_song_tbeats records -> a structured numpy array with the header's field names."""
    return np.frombuffer(bytes(raw_songs), dtype=TBEATS_DTYPE).copy()


def beats_device(onsets, hops, tgram, bp=None, anchor=True, links=False, scores=False, track=False, ctx=None):
    """Enqueue the beat grids of n songs (bl_amd_tbeats_device) on torch's current stream, the periods read in place
    from what tgram_device() returned for the same curves: the frames' lags at a stride of 40 bytes and, with `anchor`,
    the songs' median lags at a stride of 56.  Returns a dict of CUDA tensors: "songs" (uint8, 64 bytes per song),
    "flags" (uint8 per hop) and, where asked for, "links" (int16 holding uint16), "scores" (int64) and "track" (int32 per
    frame); beats_to_numpy() reads the records once the stream has been waited for."""
    import torch
    from .queries import _on_device_of
    bp = _beats_params(bp)
    hops = _hops_check(hops)
    n, total = len(hops), sum(hops)
    if onsets.dtype != torch.int32 or not onsets.is_cuda or not onsets.is_contiguous() or onsets.dim() != 1 or \
            onsets.numel() != total:
        raise ValueError(f"onsets must be a contiguous 1-D int32 CUDA tensor of sum(hops) = {total} values")
    counts = [int(x) for x in tgram["counts"]]
    nf = sum(counts)
    for k in ("songs", "frames"):
        t = tgram[k]
        if t.dtype != torch.uint8 or not t.is_cuda or t.device != onsets.device or not t.is_contiguous() or t.dim() != 1:
            raise ValueError(f'tgram["{k}"] must be a contiguous 1-D uint8 CUDA tensor on the device of onsets')
    if len(counts) != n or tgram["songs"].numel() != n * TGRAM_DTYPE.itemsize or \
            tgram["frames"].numel() != nf * TGRAM_FRAME_DTYPE.itemsize:
        raise ValueError("tgram must be what tgram_device() returned for these songs")
    lib = _lib.load()
    dev = onsets.device
    out = {"songs": torch.empty(n * TBEATS_DTYPE.itemsize, dtype=torch.uint8, device=dev),
           "flags": torch.empty(total, dtype=torch.uint8, device=dev)}
    if links:
        out["links"] = torch.empty(total, dtype=torch.int16, device=dev)
    if scores:
        out["scores"] = torch.empty(total, dtype=torch.int64, device=dev)
    if track:
        out["track"] = torch.empty(nf, dtype=torch.int32, device=dev)
    opt = lambda k: C.c_void_p(out[k].data_ptr()) if k in out and out[k].numel() else None
    with _on_device_of(lib, onsets, None) as cur:
        args = (C.c_void_p(onsets.data_ptr()), (C.c_int32 * n)(*hops), (C.c_int32 * n)(*counts), n,
                C.c_void_p(tgram["frames"].data_ptr() + TGRAM_FRAME_DTYPE.fields["lag"][1]) if nf else None,
                TGRAM_FRAME_DTYPE.itemsize,
                C.c_void_p(tgram["songs"].data_ptr() + TGRAM_DTYPE.fields["lag_median"][1]) if anchor else None,
                TGRAM_DTYPE.itemsize, C.byref(bp), C.c_void_p(out["songs"].data_ptr()),
                C.c_void_p(out["flags"].data_ptr()), opt("links"), opt("scores"), opt("track"),
                C.c_void_p(cur.cuda_stream))
        if ctx is None:
            check(lib.bl_amd_tbeats_device(*args), "bl_amd_tbeats_device")
        else:
            check(lib.bl_amd_ctx_tbeats_device(ctx.handle, *args), "bl_amd_ctx_tbeats_device")
    return out


def beats_host(onsets_list, lags_list, anchors=None, bp=None, links=False, scores=False, track=False):
    """Beat grids of onset curves and frame lags in host memory (bl_amd_tbeats_host), blocking.  lags_list: per song a
    sequence of int32 lags (it may be empty); anchors: None or one lag per song.  Returns (songs, flags, links or None,
    scores or None, track or None), the arrays of all songs one behind the other."""
    bp = _beats_params(bp)
    curves = _curves_check(onsets_list)
    n = len(curves)
    if len(lags_list) != n or (anchors is not None and len(anchors) != n):
        raise ValueError("one sequence of lags, and one anchor if any, per song")
    lags = [np.ascontiguousarray(x, dtype=np.int32).reshape(-1) for x in lags_list]
    if any(x.size > FRAMES_MAX for x in lags):
        raise ValueError(f"at most {FRAMES_MAX} frames per song")
    flat = np.ascontiguousarray(np.concatenate(curves), dtype=np.uint32)
    lag = np.ascontiguousarray(np.concatenate(lags + [np.zeros(1, np.int32)]), dtype=np.int32)
    anc = None if anchors is None else np.ascontiguousarray(anchors, dtype=np.int32)
    nh, nf = flat.size, lag.size - 1
    songs = (_lib.SongTbeats * n)()
    flags = np.zeros(nh, np.uint8)
    outs = [np.zeros(k, dt) if want else None for want, k, dt in ((links, nh, np.uint16), (scores, nh, np.int64),
                                                                  (track, max(nf, 1), np.int32))]
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    check(_lib.load().bl_amd_tbeats_host(ptr(flat), (C.c_int32 * n)(*[o.size for o in curves]),
                                         (C.c_int32 * n)(*[x.size for x in lags]), n, ptr(lag), ptr(anc), C.byref(bp),
                                         songs, ptr(flags), *[ptr(a) for a in outs]), "bl_amd_tbeats_host")
    return (beats_to_numpy(bytes(songs)), flags, outs[0], outs[1], None if outs[2] is None else outs[2][:nf])


def beats_from_pcm(pcm_list, channels, p=None, tight=128, fold=False):
    """(beat records, flags of all songs one behind the other, tempogram song records, frame records, per-song hop
    counts) of songs in host memory: the tempo call with its onset curves, the tempogram on them and the grid that
    follows it, all on the device with nothing copied in between."""
    import torch
    import bliss_amd
    from .rhythm import rhythm_device
    p = _params(p)
    arrs = [np.ascontiguousarray(a, dtype=np.int16).reshape(-1) for a in pcm_list]
    corpus = bliss_amd.DeviceCorpus([a.size for a in arrs], channels, 1)
    for i, a in enumerate(arrs):
        corpus.upload(i, a)
    _, ons, _ = rhythm_device(corpus, p.lag_min, p.lag_max, onsets=True)
    lengths, chs = corpus._songs()
    hops = [int(ln) // ch // HOP for ln, ch in zip(lengths, chs)]
    with torch.cuda.device(corpus.device):
        tgram = tgram_device(ons, hops, p)
        out = beats_device(ons, hops, tgram, beats_params(p, tight, fold))
        torch.cuda.synchronize(corpus.device)
    s, f = tgram_to_numpy(tgram["songs"].cpu().numpy().tobytes(), tgram["frames"].cpu().numpy().tobytes())
    return beats_to_numpy(out["songs"].cpu().numpy().tobytes()), out["flags"].cpu().numpy(), s, f, hops


def edge_bpm(flags, n=8, at_end=False, rate=22050):
    """The tempo of one song's grid over its first (or, with at_end, last) min(n, beats) beats in beats per minute
    (bl_amd_tbeats_edge_bpm): the tempo a transition into (out of) the song has to match.  NaN below two beats."""
    fl = np.ascontiguousarray(flags, dtype=np.uint8).reshape(-1)
    return _lib.load().bl_amd_tbeats_edge_bpm(C.c_void_p(fl.ctypes.data), fl.size, int_in("rate", rate, 1, 2 ** 31 - 1),
                                              int_in("n", n, 0, 2 ** 31 - 1), 1 if at_end else 0)
