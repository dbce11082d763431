"""Mel bands, cepstrum and flatness per frame and song (include/bliss_amd.h: bl_amd_song_mel, bl_amd_frame_mel,
bl_amd_mel_*): the 32 log-mel band levels of every frame (the log-mel spectrogram), 13 cepstral coefficients (MFCC) and
the spectral flatness, in exact integers, and their sums over the song.

This module is imported explicitly (`import bliss_amd.mel`): the package's own namespace is unchanged."""
import ctypes as C

import numpy as np

from . import _lib
from ._args import host_pcm, int_in, songs_check
from ._lib import check
from .records import FRAME_MEL_DTYPE, MEL_DTYPE

BANDS, COEFFS, FRAME = _lib.BL_AMD_MEL_BANDS, _lib.BL_AMD_MEL_COEFFS, 512
_SHORTEST = (FRAME, 2 * FRAME)   # the least interleaved samples of a mono and of a stereo song: one whole frame
MEL_SUMMARY_DTYPE = np.dtype([("mfcc", "<f8", (COEFFS,)), ("mfcc_std", "<f8", (COEFFS,)), ("flatness_db", "<f8"),
                              ("flatness_std_db", "<f8")])


def _frames(lengths, channels):
    return [(int(ln) // ch) // FRAME for ln, ch in zip(lengths, channels)]


def _min_energy(min_energy):
    return int_in("min_energy", min_energy, 0, 2 ** 64 - 1)


def mel_to_numpy(raw, frames_raw=None, bands_raw=None):
    """bytes / uint8 arrays -> (songs, frames, bands): structured arrays of bl_amd_song_mel and bl_amd_frame_mel records
    with the header's field names and the band levels as uint32 of shape (F, 32); what is not given comes back None."""
    songs = np.frombuffer(bytes(raw), dtype=MEL_DTYPE).copy()
    frames = None if frames_raw is None else np.frombuffer(bytes(frames_raw), dtype=FRAME_MEL_DTYPE).copy()
    bands = None if bands_raw is None else np.frombuffer(bytes(bands_raw), dtype=np.uint32).reshape(-1, BANDS).copy()
    return songs, frames, bands


def mel_device(corpus, frames=False, bands=False, min_energy=0, ctx=None):
    """Enqueue the mel records of every song of a DeviceCorpus (bl_amd_mel_batch_device) on torch's current stream;
    returns the CUDA uint8 tensors (song records, frame records or None, band levels or None) the corpus owns;
    fetch_mel() reads them.  min_energy: a frame enters the song's sums iff its energy is above 0 and at least this.
    ctx: an explicit Context."""
    min_energy = _min_energy(min_energy)
    lengths, channels = corpus._songs()
    total = sum(_frames(lengths, songs_check(lengths, channels, _SHORTEST)))
    torch, n = corpus.torch, corpus.n_songs
    with torch.cuda.device(corpus.device):
        rec = torch.zeros(n * MEL_DTYPE.itemsize, dtype=torch.uint8, device=corpus.device)
        fr = torch.zeros(total * FRAME_MEL_DTYPE.itemsize, dtype=torch.uint8, device=corpus.device) if frames else None
        bd = torch.zeros(total * BANDS * 4, dtype=torch.uint8, device=corpus.device) if bands else None
    corpus._call("mel_batch_device", ctx, C.c_void_p(corpus.pcm.data_ptr()), corpus.desc, n, min_energy,
                 C.c_void_p(rec.data_ptr()), C.c_void_p(fr.data_ptr()) if frames else C.c_void_p(),
                 C.c_void_p(bd.data_ptr()) if bands else C.c_void_p(), total, corpus._stream())
    corpus.mel_raw, corpus.mel_frames_raw, corpus.mel_bands_raw = rec, fr, bd
    return rec, fr, bd


def fetch_mel(corpus):
    """Wait for the device and return what the last mel_device() call on this corpus computed: (songs, frames, bands) as
    mel_to_numpy() gives them, frames and bands None unless they were asked for.  Song i's frames start at the sum of
    the earlier songs' `frames`."""
    if getattr(corpus, "mel_raw", None) is None:
        raise RuntimeError("mel_device() has not been called on this corpus")
    corpus.torch.cuda.synchronize(corpus.device)

    def host(t):
        return None if t is None else t.cpu().numpy().tobytes()
    return mel_to_numpy(host(corpus.mel_raw), host(corpus.mel_frames_raw), host(corpus.mel_bands_raw))


def mel_batch_host(pcm_list, channels, frames=False, bands=False, min_energy=0):
    """The mel records of songs in host memory (bl_amd_mel_batch_host): pcm_list a list of 1-D int16 arrays
    (interleaved), channels per song or one for all.  Returns (songs, frames, bands) as fetch_mel() does."""
    min_energy = _min_energy(min_energy)
    arrs, ptrs, ns = host_pcm(pcm_list, np.int16)
    n = len(arrs)
    sizes = [a.size for a in arrs]
    channels = songs_check(sizes, channels, _SHORTEST)
    chs = (C.c_int32 * n)(*channels)
    out = (_lib.SongMel * n)()
    total = sum(_frames(sizes, channels))
    fr = (_lib.FrameMel * total)() if frames else None
    bd = np.zeros((total, BANDS), dtype=np.uint32) if bands else None
    check(_lib.load().bl_amd_mel_batch_host(ptrs, ns, chs, n, min_energy, out, fr,
                                            bd.ctypes.data_as(C.POINTER(C.c_uint32)) if bands else None),
          "bl_amd_mel_batch_host")
    songs, fr_np, _ = mel_to_numpy(bytes(out), bytes(fr) if frames else None)
    return songs, fr_np, bd


def mel_table():
    """The tables (bl_amd_mel_table, no device): edges int32 (34,) in sixteenths of a bin, weights uint8 (32, 256) and
    the cosine table int32 (13, 32)."""
    edges, weights = np.zeros(BANDS + 2, np.int32), np.zeros((BANDS, 256), np.uint8)
    dct = np.zeros((COEFFS, BANDS), np.int32)
    check(_lib.load().bl_amd_mel_table(edges.ctypes.data, weights.ctypes.data, dct.ctypes.data), "bl_amd_mel_table")
    return edges, weights, dct


def mel_summary(records):
    """What a user reads off the integers (bl_amd_mel_mfcc, bl_amd_mel_flatness_db), as a structured array: `mfcc` and
    `mfcc_std` (13 each: mean and population standard deviation over the used frames, in log2 units), `flatness_db` and
    `flatness_std_db`; NaN where a song has no used frame."""
    rec = np.ascontiguousarray(records)
    if rec.dtype != MEL_DTYPE or rec.ndim != 1 or rec.size < 1:
        raise ValueError("records must be a non-empty 1-D array of bl_amd_song_mel records (mel_to_numpy)")
    lib = _lib.load()
    out = np.empty(rec.size, dtype=MEL_SUMMARY_DTYPE)
    ptr = rec.ctypes.data_as(C.POINTER(_lib.SongMel))
    std = C.c_double()
    for i in range(rec.size):
        for k in range(COEFFS):
            out["mfcc"][i, k] = lib.bl_amd_mel_mfcc(C.byref(ptr[i]), k, C.byref(std))
            out["mfcc_std"][i, k] = std.value
        out["flatness_db"][i] = lib.bl_amd_mel_flatness_db(C.byref(ptr[i]), C.byref(std))
        out["flatness_std_db"][i] = std.value
    return out
