"""Batch helpers over the C-ABI: device-resident corpora (torch owns the memory,
the library owns the arithmetic) and host-pointer conveniences."""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._args import host_pcm, int_in, per_song, songs_check
from ._lib import check, libc_free
from .queries import _on_device_of
from .records import (LEVELS_DTYPE, RESULT_DTYPE, TIMBRE_FRAME_DTYPE, TIMBRE_SONG_DTYPE, levels_to_numpy, results_to_numpy,
                      timbre_to_numpy)

# the least interleaved samples of a mono and of a stereo song: levels want two samples, timbre one frame of 512 per channel
_LEVELS_SHORTEST, _TIMBRE_SHORTEST = (2, 2), (512, 1024)


def _timbre_params_check(pct, min_energy):
    return int_in("pct", pct, 1, 100), int_in("min_energy", min_energy, 0, 2 ** 64 - 1)


def _timbre_frames(lengths, channels):
    return [int(ln) // ch // 512 for ln, ch in zip(lengths, channels)]


class DeviceCorpus:
    """n_songs decoded songs laid out in one int16 arena in HBM.

    lengths: interleaved sample counts; channels / durations: per song (or scalars).
    The arena is a torch int16 CUDA tensor; every song starts at a multiple of 8 samples.
    """

    def __init__(self, lengths, channels, durations, device="cuda:0"):
        import torch
        self.torch = torch
        self.lib = _lib.load()
        self.device = torch.device(device)
        n = len(lengths)
        self.n_songs = n
        self.desc = (_lib.SongDesc * n)()
        off = 0
        for i, (ln, ch, du) in enumerate(zip(lengths, per_song(channels, n), per_song(durations, n))):
            self.desc[i].pcm_offset = off
            self.desc[i].n_samples = int(ln)
            self.desc[i].channels = int(ch)
            self.desc[i].duration = int(du)
            off += (int(ln) + 7) & ~7
        self.total_samples = off
        self.levels_raw = self.timbre_raw = self.timbre_frames_raw = None   # owned outputs, allocated on first use
        idx = self.device.index if self.device.index is not None else 0
        with torch.cuda.device(idx):
            check(self.lib.bl_amd_init(idx), "bl_amd_init")
            self.pcm = torch.zeros(off + 64, dtype=torch.int16, device=self.device)
            self.results = torch.zeros(n * RESULT_DTYPE.itemsize, dtype=torch.uint8, device=self.device)

    @property
    def pcm_bytes(self):
        return 2 * sum(int(d.n_samples) for d in self.desc)

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _call(self, name, ctx, *args):
        """bl_amd_<name>(*args) on the thread's default context, or bl_amd_ctx_<name>(ctx, *args) on an explicit one"""
        if ctx is None:
            name = "bl_amd_" + name
            check(getattr(self.lib, name)(*args), name)
        else:
            name = "bl_amd_ctx_" + name
            check(getattr(self.lib, name)(ctx.handle, *args), name)

    def _songs(self):
        """(interleaved sample counts, channel counts) of the descriptors, read in one pass over them"""
        songs = [(d.n_samples, d.channels) for d in self.desc]
        return [s[0] for s in songs], [s[1] for s in songs]

    def _owned(self, buf, nbytes):
        """buf, or on first use (buf is None) a zeroed uint8 device buffer of nbytes"""
        if buf is None:
            with self.torch.cuda.device(self.device):
                buf = self.torch.zeros(nbytes, dtype=self.torch.uint8, device=self.device)
        return buf

    def synth(self, seed_base, sample_rate):
        check(self.lib.bl_amd_synth_pcm_device(C.c_void_p(self.pcm.data_ptr()), self.desc,
                                               self.n_songs, seed_base, sample_rate,
                                               self._stream()), "bl_amd_synth_pcm_device")

    def upload(self, index, pcm_int16):
        t = self.torch.from_numpy(np.ascontiguousarray(pcm_int16, dtype=np.int16))
        o = int(self.desc[index].pcm_offset)
        assert t.numel() == self.desc[index].n_samples
        self.pcm[o:o + t.numel()].copy_(t)

    def analyze(self, ctx=None):
        """Enqueue the analysis on torch's current stream (asynchronous); ctx: an explicit
        Context instead of the thread's default one."""
        self._call("analyze_batch_device", ctx, C.c_void_p(self.pcm.data_ptr()), self.desc, self.n_songs,
                   C.c_void_p(self.results.data_ptr()), self._stream())

    def upload_s32(self, index, pcm_int32):
        """A 32-bit source: narrowed on the device (>> 16) straight into the song's slot."""
        t = self.torch.from_numpy(np.ascontiguousarray(pcm_int32, dtype=np.int32)).to(self.device)
        o = int(self.desc[index].pcm_offset)
        assert t.numel() == self.desc[index].n_samples
        dst = self.pcm[o:o + t.numel()]
        check(self.lib.bl_amd_narrow_s32_device(C.c_void_p(t.data_ptr()), C.c_void_p(dst.data_ptr()),
                                                t.numel(), self._stream()), "bl_amd_narrow_s32_device")
        self.torch.cuda.current_stream(self.device).synchronize()  # t may be freed on return

    def fetch(self):
        self.torch.cuda.synchronize(self.device)
        return results_to_numpy(self.results.cpu().numpy().tobytes())

    def levels(self, silence=0, ctx=None):
        """Enqueue the signal levels of every song (bl_amd_levels_batch_device) on torch's current stream; returns the
        uint8 CUDA tensor of bl_amd_song_levels records this corpus owns (fetch_levels() reads it).  silence: a frame
        is silent while every channel has |s| <= silence (lead / trail).  ctx: an explicit Context."""
        silence = int_in("silence", silence, 0, 32767)
        songs_check(*self._songs(), _LEVELS_SHORTEST)
        self.levels_raw = self._owned(self.levels_raw, self.n_songs * LEVELS_DTYPE.itemsize)
        self._call("levels_batch_device", ctx, C.c_void_p(self.pcm.data_ptr()), self.desc, self.n_songs, silence,
                   C.c_void_p(self.levels_raw.data_ptr()), self._stream())
        return self.levels_raw

    def fetch_levels(self):
        """Wait for the device and return what the last levels() call computed, as a structured array."""
        if self.levels_raw is None:
            raise RuntimeError("levels() has not been called on this corpus")
        self.torch.cuda.synchronize(self.device)
        return levels_to_numpy(self.levels_raw.cpu().numpy().tobytes())

    def timbre(self, pct=85, min_energy=0, frames=True, ctx=None):
        """Enqueue the spectral timbre of every song (bl_amd_timbre_batch_device) on torch's current stream; returns
        the uint8 CUDA tensors (song records, frame records or None) this corpus owns (fetch_timbre() reads them).
        pct: the rolloff percentage, 1..100; min_energy: a frame enters the song's sums iff its energy is above 0 and
        at least this; frames: also keep every frame's record.  ctx: an explicit Context."""
        pct, min_energy = _timbre_params_check(pct, min_energy)
        lengths, channels = self._songs()
        total = sum(_timbre_frames(lengths, songs_check(lengths, channels, _TIMBRE_SHORTEST)))
        self.timbre_raw = self._owned(self.timbre_raw, self.n_songs * TIMBRE_SONG_DTYPE.itemsize)
        self.timbre_frames_raw = self._owned(self.timbre_frames_raw, total * TIMBRE_FRAME_DTYPE.itemsize) if frames else None
        fr = C.c_void_p(self.timbre_frames_raw.data_ptr()) if frames else C.c_void_p()
        self._call("timbre_batch_device", ctx, C.c_void_p(self.pcm.data_ptr()), self.desc, self.n_songs, pct, min_energy,
                   C.c_void_p(self.timbre_raw.data_ptr()), fr, total, self._stream())
        return self.timbre_raw, self.timbre_frames_raw

    def fetch_timbre(self):
        """Wait for the device and return what the last timbre() call computed: (songs, frames) structured arrays,
        frames None if that call kept none.  Song i's frames start at the sum of the earlier songs' `frames`."""
        if self.timbre_raw is None:
            raise RuntimeError("timbre() has not been called on this corpus")
        self.torch.cuda.synchronize(self.device)
        songs = self.timbre_raw.cpu().numpy().tobytes()
        if self.timbre_frames_raw is None:
            return timbre_to_numpy(songs), None
        return timbre_to_numpy(songs, self.timbre_frames_raw.cpu().numpy().tobytes())

    def force_vectors(self):
        """(n_songs, 4) float32 CUDA tensor view-copy of the force vectors."""
        rec = self.results.view(self.n_songs, RESULT_DTYPE.itemsize)
        return rec[:, :16].contiguous().view(self.torch.float32).view(self.n_songs, 4)


class Context:
    """An explicit library context: one device, its own workspace and internal streams.
    Independent of the default context and of other Contexts (also on the same device)."""

    def __init__(self, device=0):
        self.lib = _lib.load()
        self.handle = C.c_void_p()
        check(self.lib.bl_amd_ctx_create(int(device), C.byref(self.handle)), "bl_amd_ctx_create")

    def close(self):
        if self.handle:
            self.lib.bl_amd_ctx_destroy(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def analyze_batch_host(self, pcm_list, channels, durations):
        args, out, _keep = _host_args(pcm_list, channels, durations, np.int16)
        check(self.lib.bl_amd_ctx_analyze_batch_host(self.handle, *args, out),
              "bl_amd_ctx_analyze_batch_host")
        return results_to_numpy(bytes(out))


def _host_args(pcm_list, channels, durations, dtype):
    arrs, ptrs, ns = host_pcm(pcm_list, dtype)
    n = len(arrs)
    chs = (C.c_int32 * n)(*per_song(channels, n))
    dus = (C.c_uint64 * n)(*per_song(durations, n))
    out = (_lib.SongResult * n)()
    return (ptrs, ns, chs, dus, n), out, arrs


def analyze_batch_host(pcm_list, channels, durations):
    """pcm_list: list of 1-D int16 numpy arrays (interleaved).  Returns structured results."""
    lib = _lib.load()
    args, out, _keep = _host_args(pcm_list, channels, durations, np.int16)
    check(lib.bl_amd_analyze_batch_host(*args, out), "bl_amd_analyze_batch_host")
    return results_to_numpy(bytes(out))


def last_freq_stats():
    """Diagnostic (bl_amd_last_freq_stats): what the frequency and statistics passes of the default context's most
    recent launch group left in the workspace, in the caller's song order.  Returns a dict: n_songs, parts (the
    BL_AMD_PART_* bits of what that group wrote; the rest is left over from earlier calls), spectrum (n, 256) float32
    (bin 0 unspecified), sum (n,) int64, sumsq (n,) uint64, hist (n, 4096) uint32.  Waits for the device."""
    lib = _lib.load()
    parts = C.c_int(0)
    n = lib.bl_amd_last_freq_stats(0, None, None, None, None, C.byref(parts))
    if n < 0:
        raise RuntimeError("bl_amd_last_freq_stats failed; see stderr")
    spectrum = np.zeros((n, 256), dtype=np.float32)
    total = np.zeros(n, dtype=np.int64)
    sumsq = np.zeros(n, dtype=np.uint64)
    hist = np.zeros((n, 4096), dtype=np.uint32)
    if n and lib.bl_amd_last_freq_stats(n, spectrum.ctypes.data_as(C.POINTER(C.c_float)),
                                        total.ctypes.data_as(C.POINTER(C.c_longlong)),
                                        sumsq.ctypes.data_as(C.POINTER(C.c_ulonglong)),
                                        hist.ctypes.data_as(C.POINTER(C.c_uint)), C.byref(parts)) != n:
        raise RuntimeError("bl_amd_last_freq_stats failed; see stderr")
    return dict(n_songs=n, parts=parts.value, spectrum=spectrum, sum=total, sumsq=sumsq, hist=hist)


def tail_from_envelope(n_samples, durations, envelopes):
    """Diagnostic (bl_amd_tail_from_envelope): the envelope tail kernel on compressed envelopes of the caller's, one
    launch group.  n_samples / durations per song; envelopes: per song a float64 array of 2 * (n_samples // 512)
    slots (the last two are never read).  Returns the structured results: nb_frames, n_windows, beat, atk_sum, tempo,
    attack and status are filled, the rest is zero."""
    lib = _lib.load()
    n = len(n_samples)
    desc = (_lib.SongDesc * n)()
    for i, (ln, du) in enumerate(zip(n_samples, per_song(durations, n))):
        desc[i].pcm_offset, desc[i].n_samples, desc[i].channels, desc[i].duration = 0, int(ln), 1, int(du)
    env = np.ascontiguousarray(np.concatenate([np.asarray(e, dtype=np.float64).reshape(-1) for e in envelopes]))
    out = (_lib.SongResult * n)()
    check(lib.bl_amd_tail_from_envelope(desc, n, env.ctypes.data_as(C.POINTER(C.c_double)), env.size, out),
          "bl_amd_tail_from_envelope")
    return results_to_numpy(bytes(out))


def levels_batch_host(pcm_list, channels, silence=0):
    """Signal levels of songs in host memory (bl_amd_levels_batch_host): pcm_list a list of 1-D int16 arrays
    (interleaved), channels per song or one for all.  Returns the structured array of levels_to_numpy()."""
    silence = int_in("silence", silence, 0, 32767)
    arrs, ptrs, ns = host_pcm(pcm_list, np.int16)
    n = len(arrs)
    chs = (C.c_int32 * n)(*songs_check([a.size for a in arrs], channels, _LEVELS_SHORTEST))
    out = (_lib.SongLevels * n)()
    check(_lib.load().bl_amd_levels_batch_host(ptrs, ns, chs, n, silence, out), "bl_amd_levels_batch_host")
    return levels_to_numpy(bytes(out))


def timbre_batch_host(pcm_list, channels, pct=85, min_energy=0, frames=True):
    """Spectral timbre of songs in host memory (bl_amd_timbre_batch_host): pcm_list a list of 1-D int16 arrays
    (interleaved), channels per song or one for all.  Returns (songs, frames): the structured arrays of
    timbre_to_numpy(), frames None unless asked for."""
    pct, min_energy = _timbre_params_check(pct, min_energy)
    arrs, ptrs, ns = host_pcm(pcm_list, np.int16)
    n, sizes = len(arrs), [a.size for a in arrs]
    channels = songs_check(sizes, channels, _TIMBRE_SHORTEST)
    chs = (C.c_int32 * n)(*channels)
    out = (_lib.SongTimbre * n)()
    fout = (_lib.FrameTimbre * sum(_timbre_frames(sizes, channels)))() if frames else None
    check(_lib.load().bl_amd_timbre_batch_host(ptrs, ns, chs, n, pct, min_energy, out, fout), "bl_amd_timbre_batch_host")
    if not frames:
        return timbre_to_numpy(bytes(out)), None
    return timbre_to_numpy(bytes(out), bytes(fout))


def analyze_files(filenames, n_threads=0, keep_pcm=False):
    """`for f in filenames: bl_analyze(f)` as one call (bl_amd_analyze_files): files decoded on host
    threads while earlier ones are transferred and analysed.  Returns (list of dicts with the
    song's fields, or None where the file could not be analysed; array of bl_analyze codes)."""
    lib = _lib.load()
    n = len(filenames)
    names = (C.c_char_p * n)(*[os.fsencode(f) for f in filenames])
    songs = (_lib.BlSong * n)()
    codes = (C.c_int * n)()
    got = lib.bl_amd_analyze_files(names, n, songs, codes, int(n_threads), int(bool(keep_pcm)))
    if got == _lib.BL_UNEXPECTED:
        for sg in songs:
            lib.bl_free_song(C.byref(sg))
        raise RuntimeError("bl_amd_analyze_files failed with BL_UNEXPECTED; see stderr")
    out = []
    for i in range(n):
        sg = songs[i]
        if codes[i] == _lib.BL_UNEXPECTED:
            out.append(None)
        else:
            rec = {k: getattr(sg, k) for k in ("force", "channels", "nSamples", "sample_rate", "bitrate",
                                                 "nb_bytes_per_sample", "calm_or_loud", "resampled", "duration")}
            rec["force_vector"] = {k: getattr(sg.force_vector, k) for k in ("tempo", "amplitude", "frequency", "attack")}
            for k in ("filename", "artist", "title", "album", "tracknumber", "genre"):
                v = getattr(sg, k)
                rec[k] = v.decode("utf-8", "replace") if v is not None else None
            if keep_pcm and sg.sample_array:
                rec["pcm"] = np.ctypeslib.as_array(C.cast(sg.sample_array, C.POINTER(C.c_int16)),
                                                   shape=(sg.nSamples,)).copy()
            out.append(rec)
        lib.bl_free_song(C.byref(sg))
    return out, np.array(list(codes), dtype=np.int32)


def analyze_batch_host_s32(pcm_list, channels, durations):
    """Same for 32-bit sources (1-D int32 arrays): narrowed with >> 16 while they are staged."""
    lib = _lib.load()
    args, out, _keep = _host_args(pcm_list, channels, durations, np.int32)
    check(lib.bl_amd_analyze_batch_host_s32(*args, out), "bl_amd_analyze_batch_host_s32")
    return results_to_numpy(bytes(out))


def analyze_batch_host_rate(pcm_list, channels, durations, sample_rate):
    """Songs at `sample_rate` Hz (1-D int16 or int32 arrays, all of one dtype): each wave is
    converted to 22 050 Hz stereo on the device between its transfer and its analysis."""
    lib = _lib.load()
    dtype = np.asarray(pcm_list[0]).dtype
    if dtype not in (np.int16, np.int32):
        raise TypeError("int16 or int32 PCM expected")
    (ptrs, ns, chs, dus, n), out, _keep = _host_args(pcm_list, channels, durations, dtype)
    check(lib.bl_amd_analyze_batch_host_rate(ptrs, int(dtype == np.int32), ns, chs, dus, n, int(sample_rate), out),
          "bl_amd_analyze_batch_host_rate")
    return results_to_numpy(bytes(out))


def analyze_corpus_multi(pcm_list, channels, durations, devices, gather="rccl", matrix=True):
    """Shard the corpus over `devices` (a rank per entry), analyse, all-gather the force vectors
    and compute the bl_distance matrix by row blocks (bl_amd_analyze_corpus_multi).  Returns
    (results, matrix or None), both in the caller's song order."""
    lib = _lib.load()
    args, out, _keep = _host_args(pcm_list, channels, durations, np.int16)
    n = args[-1]
    devs = (C.c_int * len(devices))(*[int(d) for d in devices])
    flags = {"rccl": 0, "peer": 1}[gather]
    mat = np.empty((n, n), dtype=np.float32) if matrix else None
    mp = mat.ctypes.data_as(C.POINTER(C.c_float)) if matrix else None
    check(lib.bl_amd_analyze_corpus_multi(*args, devs, len(devices), flags, out, mp),
          "bl_amd_analyze_corpus_multi")
    return results_to_numpy(bytes(out)), mat


def analyze_corpus_multi_device(corpora, gather="rccl", matrix=True, keep_rows=False):
    """Resident corpora, one DeviceCorpus per rank (each on its rank's device; several on one
    device with gather="peer"): analyse every shard where it lies, all-gather the force vectors,
    row blocks of the bl_distance matrix (bl_amd_analyze_corpus_multi_device).  Returns
    (results in shard-major order, N x N matrix or None, list of per-shard row-block CUDA tensors
    or None)."""
    lib = _lib.load()
    torch = corpora[0].torch
    n = sum(c.n_songs for c in corpora)
    shards = (_lib.Shard * len(corpora))()
    rows = []
    for r, c in enumerate(corpora):
        c.torch.cuda.synchronize(c.device)   # the arena was filled on torch's stream
        shards[r].device = c.device.index or 0
        shards[r].n_songs = c.n_songs
        shards[r].d_pcm = c.pcm.data_ptr()
        shards[r].h_desc = C.cast(c.desc, C.POINTER(_lib.SongDesc))
        shards[r].d_results = c.results.data_ptr()
        if keep_rows:
            rows.append(torch.empty((c.n_songs, n), dtype=torch.float32, device=c.device))
            shards[r].d_rows = rows[-1].data_ptr()
    out = (_lib.SongResult * n)()
    mat = np.empty((n, n), dtype=np.float32) if matrix else None
    mp = mat.ctypes.data_as(C.POINTER(C.c_float)) if matrix else None
    flags = {"rccl": 0, "peer": 1}[gather]
    check(lib.bl_amd_analyze_corpus_multi_device(shards, len(corpora), flags, out, mp),
          "bl_amd_analyze_corpus_multi_device")
    return results_to_numpy(bytes(out)), mat, (rows if keep_rows else None)


def resample_host(pcm, channels, in_rate):
    """Interleaved int16 / int32 (left-justified) numpy PCM at in_rate Hz -> interleaved stereo int16
    at 22 050 Hz, the conversion bl_audio_decode applies (include/bliss_amd.h)."""
    lib = _lib.load()
    pcm = np.ascontiguousarray(pcm)
    if pcm.dtype not in (np.int16, np.int32):
        raise TypeError("int16 or int32 PCM expected")
    out = C.POINTER(C.c_int16)()
    n = C.c_size_t(0)
    check(lib.bl_amd_resample_host(pcm.ctypes.data, int(pcm.dtype == np.int32), pcm.size // channels,
                                   channels, in_rate, C.byref(out), C.byref(n)), "bl_amd_resample_host")
    try:
        return np.ctypeslib.as_array(out, shape=(2 * n.value,)).copy()
    finally:
        libc_free(out)


def resample_batch_device(d_in, frames, channels, in_rate, stream=None):
    """Songs resident in HBM at in_rate Hz (one torch int16 or int32 CUDA tensor, song i = the next
    frames[i] * channels[i] elements, starts rounded up to 8 elements) -> (int16 CUDA arena at
    22 050 Hz stereo, SongDesc-ready list of (pcm_offset, n_samples)).  Asynchronous on `stream`."""
    import torch
    lib = _lib.load()
    n = len(frames)
    desc = (_lib.ResampleDesc * n)()
    in_off = out_off = 0
    placed = []
    for i, (fr, ch) in enumerate(zip(frames, per_song(channels, n))):
        of = lib.bl_amd_resample_out_frames(int(fr), in_rate)
        desc[i].in_offset, desc[i].out_offset = in_off, out_off
        desc[i].frames, desc[i].channels = int(fr), int(ch)
        placed.append((out_off, 2 * of))
        in_off += (int(fr) * int(ch) + 7) & ~7
        out_off += (2 * of + 7) & ~7
    out = torch.zeros(out_off + 64, dtype=torch.int16, device=d_in.device)
    with _on_device_of(lib, d_in, stream) as cur:
        check(lib.bl_amd_resample_batch_device(d_in.data_ptr(), int(d_in.dtype == torch.int32), desc, n,
                                               in_rate, out.data_ptr(), C.c_void_p(cur.cuda_stream)),
              "bl_amd_resample_batch_device")
    return out, placed
