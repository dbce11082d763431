"""Per-song chroma and musical key (include/bliss_amd.h: bl_amd_song_chroma, bl_amd_frame_chroma, bl_amd_chroma_*): how a
song's energy spreads over the twelve pitch classes, in exact integers, and the major or minor key whose profile fits it.

This module is imported explicitly (`import bliss_amd.chroma`): the package's own namespace is unchanged."""
import ctypes as C

import numpy as np

from . import _lib
from ._args import host_pcm, songs_check
from ._lib import check
from .records import CHROMA_DTYPE, FRAME_CHROMA_DTYPE

FRAME, HOP, PITCHES = 4096, 2048, 48   # BL_AMD_CHROMA_FRAME, BL_AMD_CHROMA_HOP, BL_AMD_CHROMA_PITCHES
_SHORTEST = (1, 2)   # the least interleaved samples of a mono and of a stereo song: one frame of the PCM, Fr >= 1


def _frames(lengths, channels):
    return [max(0, (int(ln) // ch - FRAME) // HOP + 1) for ln, ch in zip(lengths, channels)]


def chroma_to_numpy(raw, frames_raw=None):
    """bytes / uint8 array of bl_amd_song_chroma records -> structured numpy array with the header's field names; with
    frames_raw (bl_amd_frame_chroma records) the pair (songs, frames)."""
    songs = np.frombuffer(bytes(raw), dtype=CHROMA_DTYPE).copy()
    if frames_raw is None:
        return songs
    return songs, np.frombuffer(bytes(frames_raw), dtype=FRAME_CHROMA_DTYPE).copy()


def chroma_device(corpus, frames=False, ctx=None):
    """Enqueue chroma and key of every song of a DeviceCorpus (bl_amd_chroma_batch_device) on torch's current stream;
    returns the CUDA uint8 tensors (song records, frame records or None) the corpus owns; fetch_chroma() reads them.
    ctx: an explicit Context."""
    lengths, channels = corpus._songs()
    total = sum(_frames(lengths, songs_check(lengths, channels, _SHORTEST)))
    torch, n = corpus.torch, corpus.n_songs
    with torch.cuda.device(corpus.device):
        rec = torch.zeros(n * CHROMA_DTYPE.itemsize, dtype=torch.uint8, device=corpus.device)
        fr = torch.zeros(max(total, 1) * FRAME_CHROMA_DTYPE.itemsize, dtype=torch.uint8,
                         device=corpus.device) if frames else None
    corpus._call("chroma_batch_device", ctx, C.c_void_p(corpus.pcm.data_ptr()), corpus.desc, n,
                 C.c_void_p(rec.data_ptr()), C.c_void_p(fr.data_ptr()) if frames else C.c_void_p(), total,
                 corpus._stream())
    corpus.chroma_raw, corpus.chroma_frames_raw, corpus.chroma_total = rec, fr, total
    return rec, fr


def fetch_chroma(corpus):
    """Wait for the device and return what the last chroma_device() call on this corpus computed: (songs, frames)
    structured arrays, frames None unless it was asked for.  Song i's frames start at the sum of the earlier songs'
    `frames`."""
    if getattr(corpus, "chroma_raw", None) is None:
        raise RuntimeError("chroma_device() has not been called on this corpus")
    corpus.torch.cuda.synchronize(corpus.device)
    songs = chroma_to_numpy(corpus.chroma_raw.cpu().numpy().tobytes())
    if corpus.chroma_frames_raw is None:
        return songs, None
    raw = corpus.chroma_frames_raw.cpu().numpy().tobytes()[:corpus.chroma_total * FRAME_CHROMA_DTYPE.itemsize]
    return songs, np.frombuffer(raw, dtype=FRAME_CHROMA_DTYPE).copy()


def chroma_batch_host(pcm_list, channels, frames=False):
    """Chroma and key of songs in host memory (bl_amd_chroma_batch_host): pcm_list a list of 1-D int16 arrays
    (interleaved), channels per song or one for all.  Returns (songs, frames) as fetch_chroma() does."""
    arrs, ptrs, ns = host_pcm(pcm_list, np.int16)
    n = len(arrs)
    sizes = [a.size for a in arrs]
    channels = songs_check(sizes, channels, _SHORTEST)
    chs = (C.c_int32 * n)(*channels)
    out = (_lib.SongChroma * n)()
    total = sum(_frames(sizes, channels))
    fr = (_lib.FrameChroma * max(total, 1))() if frames else None
    check(_lib.load().bl_amd_chroma_batch_host(ptrs, ns, chs, n, out, fr), "bl_amd_chroma_batch_host")
    songs = chroma_to_numpy(bytes(out))
    if not frames:
        return songs, None
    return songs, np.frombuffer(bytes(fr), dtype=FRAME_CHROMA_DTYPE)[:total].copy()


def chroma_table():
    """The constant-Q bank (bl_amd_chroma_table, no device): (re, im) int8 arrays of shape (48, 4096), gain uint32 (48,)
    and len int32 (48,)."""
    re, im = np.zeros((PITCHES, FRAME), np.int8), np.zeros((PITCHES, FRAME), np.int8)
    gain, ln = np.zeros(PITCHES, np.uint32), np.zeros(PITCHES, np.int32)
    check(_lib.load().bl_amd_chroma_table(re.ctypes.data, im.ctypes.data, gain.ctypes.data, ln.ctypes.data),
          "bl_amd_chroma_table")
    return re, im, gain, ln


def key_names(records):
    """The keys of bl_amd_song_chroma records as strings (bl_amd_chroma_key_name): "C", "F#", "A#m"; "" for key -1."""
    rec = np.ascontiguousarray(records)
    if rec.dtype != CHROMA_DTYPE or rec.ndim != 1:
        raise ValueError("records must be a 1-D array of bl_amd_song_chroma records (chroma_to_numpy)")
    lib, buf, names = _lib.load(), C.create_string_buffer(8), []
    for key in rec["key"]:
        lib.bl_amd_chroma_key_name(int(key), buf)
        names.append(buf.value.decode("ascii"))
    return names
