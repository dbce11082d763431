"""Batch helpers over the C-ABI: device-resident corpora (torch owns the memory,
the library owns the arithmetic) and host-pointer conveniences."""
import contextlib
import ctypes as C
import os

import numpy as np

from . import _lib

RESULT_DTYPE = np.dtype([
    ("tempo", "<f4"), ("amplitude", "<f4"), ("frequency", "<f4"), ("attack", "<f4"),
    ("force", "<f4"), ("calm_or_loud", "<i4"), ("status", "<i4"), ("start", "<i4"),
    ("end", "<i4"), ("mean", "<i4"), ("variance", "<i4"), ("n_frames", "<i4"),
    ("nb_frames", "<i4"), ("n_windows", "<i4"), ("beat", "<i4"), ("hist_integral", "<f4"),
    ("freq_peak", "<f4"), ("atk_sum", "<f8")], align=True)
assert RESULT_DTYPE.itemsize == C.sizeof(_lib.SongResult) == 80


def results_to_numpy(raw_bytes):
    """bytes / uint8 array of bl_amd_song_result records -> structured numpy array."""
    return np.frombuffer(bytes(raw_bytes), dtype=RESULT_DTYPE).copy()


LEVELS_DTYPE = np.dtype([
    ("sum", "<i8", (2,)), ("sum_sq", "<u8", (2,)), ("peak", "<i4", (2,)), ("zero_cross", "<i4", (2,)),
    ("clipped", "<i4", (2,)), ("lead", "<i4"), ("trail", "<i4"), ("frames", "<i4"), ("status", "<i4"),
    ("head", "<i2", (2,)), ("tail", "<i2", (2,))], align=True)
assert LEVELS_DTYPE.itemsize == C.sizeof(_lib.SongLevels) == 80

LEVELS_DB_DTYPE = np.dtype([("peak_db", "<f8", (2,)), ("rms_db", "<f8", (2,)), ("dc", "<f8", (2,)),
                            ("zcr", "<f8", (2,))])


def levels_to_numpy(raw):
    """bytes / uint8 array of bl_amd_song_levels records -> structured numpy array with the header's field names."""
    return np.frombuffer(bytes(raw), dtype=LEVELS_DTYPE).copy()


TIMBRE_FRAME_DTYPE = np.dtype([("energy", "<u8"), ("moment", "<u8"), ("rolloff", "<i4"), ("peak", "<i4")], align=True)
TIMBRE_SONG_DTYPE = np.dtype([
    ("centroid_sum", "<u8"), ("centroid_sumsq", "<u8"), ("rolloff_sum", "<u8"), ("rolloff_sumsq", "<u8"),
    ("peak_sum", "<u8"), ("peak_sumsq", "<u8"), ("energy_max", "<u8"), ("frames", "<i4"), ("used", "<i4"),
    ("status", "<i4"), ("reserved", "<i4")], align=True)
assert TIMBRE_FRAME_DTYPE.itemsize == C.sizeof(_lib.FrameTimbre) == 24
assert TIMBRE_SONG_DTYPE.itemsize == C.sizeof(_lib.SongTimbre) == 72

TIMBRE_HZ_DTYPE = np.dtype([("centroid_hz", "<f8"), ("centroid_std_hz", "<f8"), ("rolloff_hz", "<f8"),
                            ("rolloff_std_hz", "<f8"), ("peak_hz", "<f8"), ("peak_std_hz", "<f8")])


def timbre_to_numpy(raw_songs, raw_frames=None):
    """bytes / uint8 arrays of bl_amd_song_timbre (and bl_amd_frame_timbre) records -> structured numpy arrays with the
    header's field names.  Returns the song array, or (songs, frames) when raw_frames is given."""
    songs = np.frombuffer(bytes(raw_songs), dtype=TIMBRE_SONG_DTYPE).copy()
    if raw_frames is None:
        return songs
    return songs, np.frombuffer(bytes(raw_frames), dtype=TIMBRE_FRAME_DTYPE).copy()


def _timbre_params_check(pct, min_energy):
    if isinstance(pct, bool) or not isinstance(pct, (int, np.integer)) or not 1 <= pct <= 100:
        raise ValueError(f"pct must be an integer in [1, 100], got {pct!r}")
    if isinstance(min_energy, bool) or not isinstance(min_energy, (int, np.integer)) or not 0 <= min_energy < 2 ** 64:
        raise ValueError(f"min_energy must be an integer in [0, 2^64), got {min_energy!r}")
    return int(pct), int(min_energy)


def _timbre_songs_check(lengths, channels):
    """per-song channel list and frame counts, once there is a song and every song has 1 or 2 channels and a frame"""
    n = len(lengths)
    if n < 1:
        raise ValueError("at least one song is needed")
    channels = [channels] * n if np.isscalar(channels) else list(channels)
    if len(channels) != n:
        raise ValueError(f"{n} songs but {len(channels)} channel counts")
    frames = []
    for ln, ch in zip(lengths, channels):
        if isinstance(ch, bool) or not isinstance(ch, (int, np.integer)) or ch not in (1, 2):
            raise ValueError(f"channels must be 1 or 2, got {ch!r}")
        if int(ln) // int(ch) // 512 < 1:
            raise ValueError(f"a song needs at least one frame of 512 samples per channel, got {int(ln)} samples")
        frames.append(int(ln) // int(ch) // 512)
    return [int(ch) for ch in channels], frames


def _silence_check(silence):
    if isinstance(silence, bool) or not isinstance(silence, (int, np.integer)) or not 0 <= silence <= 32767:
        raise ValueError(f"silence must be an integer in [0, 32767], got {silence!r}")
    return int(silence)


def _levels_songs_check(lengths, channels):
    """per-song channel list, once there is a song and every song has 1 or 2 channels and at least 2 samples"""
    n = len(lengths)
    if n < 1:
        raise ValueError("at least one song is needed")
    channels = [channels] * n if np.isscalar(channels) else list(channels)
    if len(channels) != n:
        raise ValueError(f"{n} songs but {len(channels)} channel counts")
    for ln, ch in zip(lengths, channels):
        if isinstance(ch, bool) or not isinstance(ch, (int, np.integer)) or ch not in (1, 2):
            raise ValueError(f"channels must be 1 or 2, got {ch!r}")
        if int(ln) < 2:
            raise ValueError(f"a song needs at least 2 samples, got {int(ln)}")
    return [int(ch) for ch in channels]


def _check(rc, what):
    if rc != _lib.BL_OK:
        raise RuntimeError(f"{what} failed with BL_UNEXPECTED ({rc}); see stderr")


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
        channels = [channels] * n if np.isscalar(channels) else list(channels)
        durations = [durations] * n if np.isscalar(durations) else list(durations)
        self.n_songs = n
        self.desc = (_lib.SongDesc * n)()
        off = 0
        for i, (ln, ch, du) in enumerate(zip(lengths, channels, durations)):
            self.desc[i].pcm_offset = off
            self.desc[i].n_samples = int(ln)
            self.desc[i].channels = int(ch)
            self.desc[i].duration = int(du)
            off += (int(ln) + 7) & ~7
        self.total_samples = off
        idx = self.device.index if self.device.index is not None else 0
        with torch.cuda.device(idx):
            _check(self.lib.bl_amd_init(idx), "bl_amd_init")
            self.pcm = torch.zeros(off + 64, dtype=torch.int16, device=self.device)
            self.results = torch.zeros(n * C.sizeof(_lib.SongResult), dtype=torch.uint8,
                                       device=self.device)

    @property
    def pcm_bytes(self):
        return 2 * sum(int(d.n_samples) for d in self.desc)

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def synth(self, seed_base, sample_rate):
        _check(self.lib.bl_amd_synth_pcm_device(C.c_void_p(self.pcm.data_ptr()), self.desc,
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
        if ctx is None:
            _check(self.lib.bl_amd_analyze_batch_device(C.c_void_p(self.pcm.data_ptr()), self.desc,
                                                        self.n_songs,
                                                        C.c_void_p(self.results.data_ptr()),
                                                        self._stream()), "bl_amd_analyze_batch_device")
        else:
            _check(self.lib.bl_amd_ctx_analyze_batch_device(ctx.handle, C.c_void_p(self.pcm.data_ptr()),
                                                            self.desc, self.n_songs,
                                                            C.c_void_p(self.results.data_ptr()),
                                                            self._stream()),
                   "bl_amd_ctx_analyze_batch_device")

    def upload_s32(self, index, pcm_int32):
        """A 32-bit source: narrowed on the device (>> 16) straight into the song's slot."""
        t = self.torch.from_numpy(np.ascontiguousarray(pcm_int32, dtype=np.int32)).to(self.device)
        o = int(self.desc[index].pcm_offset)
        assert t.numel() == self.desc[index].n_samples
        dst = self.pcm[o:o + t.numel()]
        _check(self.lib.bl_amd_narrow_s32_device(C.c_void_p(t.data_ptr()), C.c_void_p(dst.data_ptr()),
                                                 t.numel(), self._stream()), "bl_amd_narrow_s32_device")
        self.torch.cuda.current_stream(self.device).synchronize()  # t may be freed on return

    def fetch(self):
        self.torch.cuda.synchronize(self.device)
        return results_to_numpy(self.results.cpu().numpy().tobytes())

    def levels(self, silence=0, ctx=None):
        """Enqueue the signal levels of every song (bl_amd_levels_batch_device) on torch's current stream; returns the
        uint8 CUDA tensor of bl_amd_song_levels records this corpus owns (fetch_levels() reads it).  silence: a frame
        is silent while every channel has |s| <= silence (lead / trail).  ctx: an explicit Context."""
        silence = _silence_check(silence)
        _levels_songs_check([d.n_samples for d in self.desc], [d.channels for d in self.desc])
        if getattr(self, "levels_raw", None) is None:
            with self.torch.cuda.device(self.device):
                self.levels_raw = self.torch.zeros(self.n_songs * C.sizeof(_lib.SongLevels), dtype=self.torch.uint8,
                                                   device=self.device)
        args = (C.c_void_p(self.pcm.data_ptr()), self.desc, self.n_songs, silence,
                C.c_void_p(self.levels_raw.data_ptr()), self._stream())
        if ctx is None:
            _check(self.lib.bl_amd_levels_batch_device(*args), "bl_amd_levels_batch_device")
        else:
            _check(self.lib.bl_amd_ctx_levels_batch_device(ctx.handle, *args), "bl_amd_ctx_levels_batch_device")
        return self.levels_raw

    def fetch_levels(self):
        """Wait for the device and return what the last levels() call computed, as a structured array."""
        if getattr(self, "levels_raw", None) is None:
            raise RuntimeError("levels() has not been called on this corpus")
        self.torch.cuda.synchronize(self.device)
        return levels_to_numpy(self.levels_raw.cpu().numpy().tobytes())

    def timbre(self, pct=85, min_energy=0, frames=True, ctx=None):
        """Enqueue the spectral timbre of every song (bl_amd_timbre_batch_device) on torch's current stream; returns
        the uint8 CUDA tensors (song records, frame records or None) this corpus owns (fetch_timbre() reads them).
        pct: the rolloff percentage, 1..100; min_energy: a frame enters the song's sums iff its energy is above 0 and
        at least this; frames: also keep every frame's record.  ctx: an explicit Context."""
        pct, min_energy = _timbre_params_check(pct, min_energy)
        _, nfr = _timbre_songs_check([d.n_samples for d in self.desc], [d.channels for d in self.desc])
        total = sum(nfr)
        with self.torch.cuda.device(self.device):
            if getattr(self, "timbre_raw", None) is None:
                self.timbre_raw = self.torch.zeros(self.n_songs * C.sizeof(_lib.SongTimbre), dtype=self.torch.uint8,
                                                   device=self.device)
            if frames and getattr(self, "timbre_frames_raw", None) is None:
                self.timbre_frames_raw = self.torch.zeros(total * C.sizeof(_lib.FrameTimbre), dtype=self.torch.uint8,
                                                          device=self.device)
        if not frames:
            self.timbre_frames_raw = None
        fr = C.c_void_p(self.timbre_frames_raw.data_ptr()) if frames else C.c_void_p()
        args = (C.c_void_p(self.pcm.data_ptr()), self.desc, self.n_songs, pct, min_energy,
                C.c_void_p(self.timbre_raw.data_ptr()), fr, total, self._stream())
        if ctx is None:
            _check(self.lib.bl_amd_timbre_batch_device(*args), "bl_amd_timbre_batch_device")
        else:
            _check(self.lib.bl_amd_ctx_timbre_batch_device(ctx.handle, *args), "bl_amd_ctx_timbre_batch_device")
        return self.timbre_raw, self.timbre_frames_raw

    def fetch_timbre(self):
        """Wait for the device and return what the last timbre() call computed: (songs, frames) structured arrays,
        frames None if that call kept none.  Song i's frames start at the sum of the earlier songs' `frames`."""
        if getattr(self, "timbre_raw", None) is None:
            raise RuntimeError("timbre() has not been called on this corpus")
        self.torch.cuda.synchronize(self.device)
        songs = timbre_to_numpy(self.timbre_raw.cpu().numpy().tobytes())
        if self.timbre_frames_raw is None:
            return songs, None
        return timbre_to_numpy(self.timbre_raw.cpu().numpy().tobytes(), self.timbre_frames_raw.cpu().numpy().tobytes())

    def force_vectors(self):
        """(n_songs, 4) float32 CUDA tensor view-copy of the force vectors."""
        rec = self.results.view(self.n_songs, C.sizeof(_lib.SongResult))
        return rec[:, :16].contiguous().view(self.torch.float32).view(self.n_songs, 4)


class Context:
    """An explicit library context: one device, its own workspace and internal streams.
    Independent of the default context and of other Contexts (also on the same device)."""

    def __init__(self, device=0):
        self.lib = _lib.load()
        self.handle = C.c_void_p()
        _check(self.lib.bl_amd_ctx_create(int(device), C.byref(self.handle)), "bl_amd_ctx_create")

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
        _check(self.lib.bl_amd_ctx_analyze_batch_host(self.handle, *args, out),
               "bl_amd_ctx_analyze_batch_host")
        return results_to_numpy(bytes(out))


def _host_args(pcm_list, channels, durations, dtype):
    n = len(pcm_list)
    arrs = [np.ascontiguousarray(p, dtype=dtype) for p in pcm_list]
    channels = [channels] * n if np.isscalar(channels) else list(channels)
    durations = [durations] * n if np.isscalar(durations) else list(durations)
    ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
    ns = (C.c_int32 * n)(*[a.size for a in arrs])
    chs = (C.c_int32 * n)(*channels)
    dus = (C.c_uint64 * n)(*durations)
    out = (_lib.SongResult * n)()
    return (ptrs, ns, chs, dus, n), out, arrs


def analyze_batch_host(pcm_list, channels, durations):
    """pcm_list: list of 1-D int16 numpy arrays (interleaved).  Returns structured results."""
    lib = _lib.load()
    args, out, _keep = _host_args(pcm_list, channels, durations, np.int16)
    _check(lib.bl_amd_analyze_batch_host(*args, out), "bl_amd_analyze_batch_host")
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
    durations = [durations] * n if np.isscalar(durations) else list(durations)
    desc = (_lib.SongDesc * n)()
    for i, (ln, du) in enumerate(zip(n_samples, durations)):
        desc[i].pcm_offset, desc[i].n_samples, desc[i].channels, desc[i].duration = 0, int(ln), 1, int(du)
    env = np.ascontiguousarray(np.concatenate([np.asarray(e, dtype=np.float64).reshape(-1) for e in envelopes]))
    out = (_lib.SongResult * n)()
    _check(lib.bl_amd_tail_from_envelope(desc, n, env.ctypes.data_as(C.POINTER(C.c_double)), env.size, out),
           "bl_amd_tail_from_envelope")
    return results_to_numpy(bytes(out))


def levels_batch_host(pcm_list, channels, silence=0):
    """Signal levels of songs in host memory (bl_amd_levels_batch_host): pcm_list a list of 1-D int16 arrays
    (interleaved), channels per song or one for all.  Returns the structured array of levels_to_numpy()."""
    silence = _silence_check(silence)
    arrs = [np.ascontiguousarray(p, dtype=np.int16).reshape(-1) for p in pcm_list]
    channels = _levels_songs_check([a.size for a in arrs], channels)
    lib = _lib.load()
    n = len(arrs)
    ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
    ns = (C.c_int32 * n)(*[a.size for a in arrs])
    chs = (C.c_int32 * n)(*channels)
    out = (_lib.SongLevels * n)()
    _check(lib.bl_amd_levels_batch_host(ptrs, ns, chs, n, silence, out), "bl_amd_levels_batch_host")
    return levels_to_numpy(bytes(out))


def timbre_batch_host(pcm_list, channels, pct=85, min_energy=0, frames=True):
    """Spectral timbre of songs in host memory (bl_amd_timbre_batch_host): pcm_list a list of 1-D int16 arrays
    (interleaved), channels per song or one for all.  Returns (songs, frames): the structured arrays of
    timbre_to_numpy(), frames None unless asked for."""
    pct, min_energy = _timbre_params_check(pct, min_energy)
    arrs = [np.ascontiguousarray(p, dtype=np.int16).reshape(-1) for p in pcm_list]
    channels, nfr = _timbre_songs_check([a.size for a in arrs], channels)
    lib = _lib.load()
    n = len(arrs)
    ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
    ns = (C.c_int32 * n)(*[a.size for a in arrs])
    chs = (C.c_int32 * n)(*channels)
    out = (_lib.SongTimbre * n)()
    fout = (_lib.FrameTimbre * sum(nfr))() if frames else None
    _check(lib.bl_amd_timbre_batch_host(ptrs, ns, chs, n, pct, min_energy, out, fout), "bl_amd_timbre_batch_host")
    if not frames:
        return timbre_to_numpy(bytes(out)), None
    return timbre_to_numpy(bytes(out), bytes(fout))


def timbre_hz(songs, rate=22050):
    """What a user reads off the integers (bl_amd_timbre_centroid_hz, _rolloff_hz, _peak_hz): mean and population
    standard deviation over the used frames, in Hz, as a structured array; NaN where a song has no used frame."""
    st = np.ascontiguousarray(songs)
    if st.dtype != TIMBRE_SONG_DTYPE or st.ndim != 1 or st.size < 1:
        raise ValueError("songs must be a non-empty 1-D array of bl_amd_song_timbre records (timbre_to_numpy)")
    lib = _lib.load()
    out = np.empty(st.size, dtype=TIMBRE_HZ_DTYPE)
    recs = st.ctypes.data_as(C.POINTER(_lib.SongTimbre))
    std = C.c_double()
    for i in range(st.size):
        for name, fn in (("centroid", lib.bl_amd_timbre_centroid_hz), ("rolloff", lib.bl_amd_timbre_rolloff_hz),
                         ("peak", lib.bl_amd_timbre_peak_hz)):
            out[name + "_hz"][i] = fn(C.byref(recs[i]), int(rate), C.byref(std))
            out[name + "_std_hz"][i] = std.value
    return out


def _levels_array(levels):
    lv = np.ascontiguousarray(levels)
    if lv.dtype != LEVELS_DTYPE or lv.ndim != 1 or lv.size < 1:
        raise ValueError("levels must be a non-empty 1-D array of bl_amd_song_levels records (levels_to_numpy)")
    return lv


def gapless_links(levels):
    """bool array of n - 1 entries: song i runs into song i + 1 (bl_amd_gapless_host: the rule of the reference's
    examples/detect-gapless.c on the last two samples of one song and the first two of the next)."""
    lv = _levels_array(levels)
    lib = _lib.load()
    linked = np.zeros(max(lv.size - 1, 1), dtype=np.uint8)
    _check(lib.bl_amd_gapless_host(lv.ctypes.data_as(C.POINTER(_lib.SongLevels)), lv.size,
                                   linked.ctypes.data_as(C.POINTER(C.c_uint8))), "bl_amd_gapless_host")
    return linked[:lv.size - 1].astype(bool)


def levels_db(levels):
    """What a player reads off the integers, per channel, as a structured array: peak_db = 20 log10(peak / 32768),
    rms_db = 10 log10(sum_sq / (frames 2^30)) (-inf for silence and for channel 1 of a mono song), dc = sum / frames
    and zcr = zero_cross / max(frames - 1, 1)."""
    lv = _levels_array(levels)
    out = np.empty(lv.size, dtype=LEVELS_DB_DTYPE)
    frames = lv["frames"].astype(np.float64)[:, None]
    with np.errstate(divide="ignore"):
        out["peak_db"] = 20.0 * np.log10(lv["peak"].astype(np.float64) / 32768.0)
        out["rms_db"] = 10.0 * np.log10(lv["sum_sq"].astype(np.float64) / (frames * 2.0 ** 30))
    out["dc"] = lv["sum"].astype(np.float64) / frames
    out["zcr"] = lv["zero_cross"].astype(np.float64) / np.maximum(frames - 1.0, 1.0)
    return out


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
    _check(lib.bl_amd_analyze_batch_host_s32(*args, out), "bl_amd_analyze_batch_host_s32")
    return results_to_numpy(bytes(out))


def analyze_batch_host_rate(pcm_list, channels, durations, sample_rate):
    """Songs at `sample_rate` Hz (1-D int16 or int32 arrays, all of one dtype): each wave is
    converted to 22 050 Hz stereo on the device between its transfer and its analysis."""
    lib = _lib.load()
    dtype = np.asarray(pcm_list[0]).dtype
    if dtype not in (np.int16, np.int32):
        raise TypeError("int16 or int32 PCM expected")
    (ptrs, ns, chs, dus, n), out, _keep = _host_args(pcm_list, channels, durations, dtype)
    _check(lib.bl_amd_analyze_batch_host_rate(ptrs, int(dtype == np.int32), ns, chs, dus, n, int(sample_rate), out),
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
    _check(lib.bl_amd_analyze_corpus_multi(*args, devs, len(devices), flags, out, mp),
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
    _check(lib.bl_amd_analyze_corpus_multi_device(shards, len(corpora), flags, out, mp),
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
    _check(lib.bl_amd_resample_host(pcm.ctypes.data, int(pcm.dtype == np.int32), pcm.size // channels,
                                    channels, in_rate, C.byref(out), C.byref(n)), "bl_amd_resample_host")
    try:
        return np.ctypeslib.as_array(out, shape=(2 * n.value,)).copy()
    finally:
        _libc_free(out)


def _libc_free(ptr):
    C.CDLL(None).free(C.cast(ptr, C.c_void_p))


def resample_batch_device(d_in, frames, channels, in_rate, stream=None):
    """Songs resident in HBM at in_rate Hz (one torch int16 or int32 CUDA tensor, song i = the next
    frames[i] * channels[i] elements, starts rounded up to 8 elements) -> (int16 CUDA arena at
    22 050 Hz stereo, SongDesc-ready list of (pcm_offset, n_samples)).  Asynchronous on `stream`."""
    import torch
    lib = _lib.load()
    n = len(frames)
    channels = [channels] * n if np.isscalar(channels) else list(channels)
    desc = (_lib.ResampleDesc * n)()
    in_off = out_off = 0
    placed = []
    for i, (fr, ch) in enumerate(zip(frames, channels)):
        of = lib.bl_amd_resample_out_frames(int(fr), in_rate)
        desc[i].in_offset, desc[i].out_offset = in_off, out_off
        desc[i].frames, desc[i].channels = int(fr), int(ch)
        placed.append((out_off, 2 * of))
        in_off += (int(fr) * int(ch) + 7) & ~7
        out_off += (2 * of + 7) & ~7
    out = torch.zeros(out_off + 64, dtype=torch.int16, device=d_in.device)
    with _on_device_of(lib, d_in, stream) as cur:
        _check(lib.bl_amd_resample_batch_device(d_in.data_ptr(), int(d_in.dtype == torch.int32), desc, n,
                                                in_rate, out.data_ptr(), C.c_void_p(cur.cuda_stream)),
               "bl_amd_resample_batch_device")
    return out, placed


def _matrix(fn_name, vecs):
    lib = _lib.load()
    v = np.ascontiguousarray(vecs, dtype=np.float32).reshape(-1, 4)
    n = v.shape[0]
    out = np.empty((n, n), dtype=np.float32)
    rc = getattr(lib, fn_name)(v.ctypes.data_as(C.POINTER(_lib.ForceVector)), n,
                               out.ctypes.data_as(C.POINTER(C.c_float)))
    _check(rc, fn_name)
    return out


def distance_matrix(vecs):
    """N x N bl_distance matrix (ref src/analyze.c:96-100) of (N, 4) force vectors."""
    return _matrix("bl_amd_distance_matrix_host", vecs)


def cosine_matrix(vecs):
    """N x N bl_cosine_similarity matrix (ref src/analyze.c:135-140)."""
    return _matrix("bl_amd_cosine_matrix_host", vecs)


def playlist(vecs, seed_index):
    """Song indices ordered by increasing bl_distance from song `seed_index`, and the
    distances (ref python/examples/make_m3u_playlist.py:62-72).  Stable for ties.  NaN distances after every
    number, in index order: numpy's stable argsort."""
    lib = _lib.load()
    v = np.ascontiguousarray(vecs, dtype=np.float32).reshape(-1, 4)
    n = v.shape[0]
    order = np.empty(n, dtype=np.int32)
    dist = np.empty(n, dtype=np.float32)
    rc = lib.bl_amd_playlist_host(v.ctypes.data_as(C.POINTER(_lib.ForceVector)), n, int(seed_index),
                                  order.ctypes.data_as(C.POINTER(C.c_int32)),
                                  dist.ctypes.data_as(C.POINTER(C.c_float)))
    _check(rc, "bl_amd_playlist_host")
    return order, dist


_KNN_METRICS = {"distance": _lib.BL_AMD_KNN_DISTANCE, "cosine": _lib.BL_AMD_KNN_COSINE}


def _metric_check(metric, shape):
    """the metric's code, for a known metric over (n, 4) force vectors"""
    if metric not in _KNN_METRICS:
        raise ValueError(f"metric must be one of {sorted(_KNN_METRICS)}, got {metric!r}")
    if len(shape) != 2 or shape[1] != 4 or shape[0] < 1:
        raise ValueError(f"force vectors must have shape (n, 4) with n >= 1, got {tuple(shape)}")
    return _KNN_METRICS[metric]


def _device_vecs_check(d_vecs):
    import torch
    if d_vecs.dtype != torch.float32 or not d_vecs.is_cuda or not d_vecs.is_contiguous():
        raise ValueError("d_vecs must be a contiguous float32 CUDA tensor")


def _rows_check(n, row_begin, n_rows):
    """n_rows (None: all rows from row_begin) once [row_begin, row_begin + n_rows) lies inside [0, n)"""
    if n_rows is None:
        n_rows = n - row_begin
    if not (0 <= row_begin < n and 1 <= n_rows <= n - row_begin):
        raise ValueError(f"rows [{row_begin}, {row_begin + n_rows}) are not inside [0, {n})")
    return n_rows


@contextlib.contextmanager
def _on_device_of(lib, tensor, stream):
    """The tensor's device current and the library initialised on it; yields the torch stream to launch on (`stream`,
    else that device's current one) without entering it: the caller decides under which stream it allocates."""
    import torch
    cur = stream if stream is not None else torch.cuda.current_stream(tensor.device)
    idx = tensor.device.index or 0
    with torch.cuda.device(idx):
        _check(lib.bl_amd_init(idx), "bl_amd_init")
        yield cur


def _knn_check(k, metric, shape):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= _lib.BL_AMD_KNN_MAX_K:
        raise ValueError(f"k must be an integer in [1, {_lib.BL_AMD_KNN_MAX_K}], got {k!r}")
    return _metric_check(metric, shape)


def _knn_host_call(name, args, rows, k):
    """(index, value) of shape (rows, k) from the kNN host entry point `name`, called with `args` and the two outputs"""
    lib = _lib.load()
    index = np.empty((rows, k), dtype=np.int32)
    value = np.empty((rows, k), dtype=np.float32)
    rc = getattr(lib, name)(*args, index.ctypes.data_as(C.POINTER(C.c_int32)), value.ctypes.data_as(C.POINTER(C.c_float)))
    _check(rc, name)
    return index, value


def _knn_device_call(name, args, v, rows, k, stream):
    """The same for a device entry point, on the device of the library tensor v and on `stream`"""
    import torch
    lib = _lib.load()
    index = torch.empty((rows, k), dtype=torch.int32, device=v.device)
    value = torch.empty((rows, k), dtype=torch.float32, device=v.device)
    with _on_device_of(lib, v, stream) as cur:
        _check(getattr(lib, name)(*args, index.data_ptr(), value.data_ptr(), C.c_void_p(cur.cuda_stream)), name)
    return index, value


def knn(vecs, k, metric="distance"):
    """The k nearest songs of every song of (n, 4) force vectors: (index (n, k) int32, value (n, k) float32).
    Values have the bits of bl_distance ("distance", nearest = smallest) or bl_cosine_similarity ("cosine",
    nearest = largest); ties go to the smaller index and the song itself is never listed
    (ref python/examples/make_m3u_playlist.py:62-72 for every seed).  Slots past n - 1 hold -1 and NaN."""
    v = np.ascontiguousarray(vecs, dtype=np.float32)
    m = _knn_check(k, metric, v.shape)
    n = v.shape[0]
    return _knn_host_call("bl_amd_knn_host", (v.ctypes.data_as(C.POINTER(_lib.ForceVector)), n, int(k), m), n, k)


def knn_device(d_vecs, k, metric="distance", row_begin=0, n_rows=None, stream=None):
    """knn() for the queries d_vecs[row_begin:row_begin + n_rows] against all of d_vecs, a float32 (n, 4) CUDA
    tensor; returns (index, value) CUDA tensors of shape (n_rows, k) on its device, asynchronously on `stream`
    (default: the current stream of that device)."""
    m = _knn_check(k, metric, tuple(d_vecs.shape))
    _device_vecs_check(d_vecs)
    n = d_vecs.shape[0]
    n_rows = _rows_check(n, row_begin, n_rows)
    return _knn_device_call("bl_amd_knn_device", (d_vecs.data_ptr(), n, int(row_begin), int(n_rows), int(k), m), d_vecs,
                            n_rows, k, stream)


def _chain_check(seeds, length, metric, shape, n_limit):
    """(metric code, seeds as a contiguous 1-D int32 numpy array or None for a tensor); n_limit: reject seeds outside
    [0, n_limit) (None: leave them to the device, which answers with a -1 / NaN row)"""
    if isinstance(length, bool) or not isinstance(length, (int, np.integer)) or length < 1:
        raise ValueError(f"length must be an integer >= 1, got {length!r}")
    m = _metric_check(metric, shape)
    if hasattr(seeds, "is_cuda"):   # a torch tensor: chain_device checks it
        return m, None
    s = np.asarray(seeds)
    if s.dtype == np.bool_ or not np.issubdtype(s.dtype, np.integer):
        raise ValueError(f"seeds must be integers, got dtype {s.dtype}")
    if s.ndim > 1 or s.size < 1:
        raise ValueError(f"seeds must be a scalar or a non-empty 1-D sequence, got shape {s.shape}")
    s = s.reshape(-1)
    if n_limit is not None and (s.min() < 0 or s.max() >= n_limit):
        raise ValueError(f"seeds must lie in [0, {n_limit})")
    if s.min() < -2 ** 31 or s.max() >= 2 ** 31:
        raise ValueError("seeds do not fit 32 bits")
    return m, np.ascontiguousarray(s, dtype=np.int32)


def chain(vecs, seeds, length, metric="distance"):
    """Song-to-song chains over (n, 4) force vectors, one per seed (a scalar seed gives one chain): slot 0 is the
    seed and every next slot the song nearest to the previous one that the chain has not played yet, nearest as in
    knn().  Returns (order (n_chains, length) int32, value (n_chains, length) float32); value[c, t] has the bits of
    bl_distance / bl_cosine_similarity between the songs of slots t - 1 and t (slot 0: the seed with itself).
    Slots past n hold -1 and NaN."""
    v = np.ascontiguousarray(vecs, dtype=np.float32)
    m, s = _chain_check(seeds, length, metric, v.shape, v.shape[0] if v.ndim == 2 else 0)
    lib = _lib.load()
    order = np.empty((s.size, length), dtype=np.int32)
    value = np.empty((s.size, length), dtype=np.float32)
    rc = lib.bl_amd_chain_host(v.ctypes.data_as(C.POINTER(_lib.ForceVector)), v.shape[0],
                               s.ctypes.data_as(C.POINTER(C.c_int32)), s.size, int(length), m,
                               order.ctypes.data_as(C.POINTER(C.c_int32)), value.ctypes.data_as(C.POINTER(C.c_float)))
    _check(rc, "bl_amd_chain_host")
    return order, value


def chain_device(d_vecs, d_seeds, length, metric="distance", stream=None):
    """chain() on the device: d_vecs a contiguous float32 (n, 4) CUDA tensor, d_seeds an int32 CUDA tensor on the same
    device (0-D or 1-D) or host integers, which are uploaded.  Returns (order, value) CUDA tensors of shape
    (n_chains, length), asynchronously on `stream` (default: the current stream of that device).  A seed outside
    [0, n) gives a row of -1 / NaN."""
    import torch
    m, s = _chain_check(d_seeds, length, metric, tuple(d_vecs.shape), None)
    _device_vecs_check(d_vecs)
    if s is None:
        if d_seeds.dtype != torch.int32 or d_seeds.dim() > 1 or d_seeds.numel() < 1:
            raise ValueError("d_seeds must be an int32 tensor with 0 or 1 dimensions and at least one element")
        if not d_seeds.is_cuda or d_seeds.device != d_vecs.device:
            raise ValueError("d_seeds must be on the device of d_vecs")
    lib = _lib.load()
    v = d_vecs
    n = v.shape[0]
    with _on_device_of(lib, v, stream) as cur, torch.cuda.stream(cur):
        sd = torch.from_numpy(s).to(v.device) if s is not None else d_seeds.reshape(-1).contiguous()
        n_chains = sd.numel()
        order = torch.empty((n_chains, length), dtype=torch.int32, device=v.device)
        value = torch.empty((n_chains, length), dtype=torch.float32, device=v.device)
        _check(lib.bl_amd_chain_device(v.data_ptr(), n, sd.data_ptr(), n_chains, int(length), m, order.data_ptr(),
                                       value.data_ptr(), C.c_void_p(cur.cuda_stream)), "bl_amd_chain_device")
        if s is not None:
            sd.record_stream(cur)   # the uploaded seeds are freed when this returns
    return order, value


def _mix_gap_check(gap, tags):
    if isinstance(gap, bool) or not isinstance(gap, (int, np.integer)) or not 0 <= gap <= _lib.BL_AMD_MIX_MAX_GAP:
        raise ValueError(f"gap must be an integer in [0, {_lib.BL_AMD_MIX_MAX_GAP}], got {gap!r}")
    if gap > 0 and tags is None:
        raise ValueError("gap > 0 needs tags")
    return int(gap)


def _mix_seeds_check(seeds, seed_vecs):
    if (seeds is None) == (seed_vecs is None):
        raise ValueError("exactly one of seeds and seed_vecs must be given")


def mix(vecs, seeds, length, metric="distance", tags=None, gap=0, exclude=None, seed_vecs=None):
    """chain() under rules.  tags: n integers (artist, album ...; negative = untagged) of which no value may repeat
    within `gap` slots (0 <= gap <= 16; 0 ignores the tags).  exclude: n bools or bytes, non-zero = never picked.
    seed_vecs: (m, 4) float32 vectors instead of seeds (pass seeds=None): slot 0 is the song nearest to the vector
    among the songs not excluded.  An index seed takes slot 0 even if it is excluded.  A chain with no allowed song
    left ends: the rest of its row holds -1 and NaN.  To continue a chain, call again with seed = its last song and
    exclude = everything played so far.  Returns (order, value) as chain() does."""
    v = np.ascontiguousarray(vecs, dtype=np.float32)
    _mix_seeds_check(seeds, seed_vecs)
    gap = _mix_gap_check(gap, tags)
    n = v.shape[0] if v.ndim == 2 else 0
    q = None
    if seed_vecs is not None:
        if hasattr(seed_vecs, "dtype") and seed_vecs.dtype != np.float32:
            raise ValueError(f"seed_vecs must be float32, got {seed_vecs.dtype}")
        q = np.ascontiguousarray(seed_vecs, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != 4 or q.shape[0] < 1:
            raise ValueError(f"seed_vecs must have shape (m, 4) with m >= 1, got {q.shape}")
        m, s = _chain_check(0, length, metric, v.shape, None)[0], None
    else:
        m, s = _chain_check(seeds, length, metric, v.shape, n)
    tg = None
    if tags is not None:
        tg = np.asarray(tags)
        if tg.dtype == np.bool_ or not np.issubdtype(tg.dtype, np.integer) or tg.shape != (n,):
            raise ValueError(f"tags must be {n} integers, got dtype {tg.dtype} and shape {tg.shape}")
        if tg.size and (tg.min() < -2 ** 31 or tg.max() >= 2 ** 31):
            raise ValueError("tags do not fit 32 bits")
        tg = np.ascontiguousarray(tg, dtype=np.int32)
    ex = None
    if exclude is not None:
        ex = np.asarray(exclude)
        if ex.dtype not in (np.bool_, np.uint8) or ex.shape != (n,):
            raise ValueError(f"exclude must be {n} bools or uint8, got dtype {ex.dtype} and shape {ex.shape}")
        ex = np.ascontiguousarray(ex).view(np.uint8)
    lib = _lib.load()
    n_chains = q.shape[0] if q is not None else s.size
    order = np.empty((n_chains, length), dtype=np.int32)
    value = np.empty((n_chains, length), dtype=np.float32)
    fv, i32 = C.POINTER(_lib.ForceVector), C.POINTER(C.c_int32)
    rc = lib.bl_amd_mix_host(v.ctypes.data_as(fv), n, s.ctypes.data_as(i32) if s is not None else None,
                             q.ctypes.data_as(fv) if q is not None else None, n_chains, int(length), m,
                             tg.ctypes.data_as(i32) if tg is not None else None, gap,
                             ex.ctypes.data_as(C.POINTER(C.c_uint8)) if ex is not None else None,
                             order.ctypes.data_as(i32), value.ctypes.data_as(C.POINTER(C.c_float)))
    _check(rc, "bl_amd_mix_host")
    return order, value


def mix_device(d_vecs, d_seeds, length, metric="distance", tags=None, gap=0, exclude=None, seed_vecs=None, stream=None):
    """mix() on the device: d_vecs as chain_device() takes it, d_seeds as chain_device() takes them or None with
    seed_vecs, a contiguous, 16-byte aligned float32 (m, 4) CUDA tensor that may be a view into d_vecs.  tags: an
    int32 CUDA tensor of n entries; exclude: a bool or uint8 CUDA tensor of n entries; both contiguous and on the
    device of d_vecs.
    Returns (order, value) CUDA tensors of shape (n_chains, length), asynchronously on `stream`."""
    import torch
    _mix_seeds_check(d_seeds, seed_vecs)
    gap = _mix_gap_check(gap, tags)
    shape = tuple(d_vecs.shape)
    if seed_vecs is not None:
        m, s = _chain_check(0, length, metric, shape, None)[0], None
        if not isinstance(seed_vecs, torch.Tensor) or seed_vecs.dtype != torch.float32 or seed_vecs.dim() != 2 or \
                seed_vecs.shape[1] != 4 or seed_vecs.shape[0] < 1:
            raise ValueError("seed_vecs must be a float32 tensor of shape (m, 4) with m >= 1")
    else:
        m, s = _chain_check(d_seeds, length, metric, shape, None)
    n = shape[0]
    for name, t, kinds in (("tags", tags, (torch.int32,)), ("exclude", exclude, (torch.bool, torch.uint8))):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype not in kinds or tuple(t.shape) != (n,)):
            raise ValueError(f"{name} must be a tensor of {n} entries of {' or '.join(str(k) for k in kinds)}")
    _device_vecs_check(d_vecs)
    if seed_vecs is None and s is None:
        if d_seeds.dtype != torch.int32 or d_seeds.dim() > 1 or d_seeds.numel() < 1:
            raise ValueError("d_seeds must be an int32 tensor with 0 or 1 dimensions and at least one element")
    for name, t in (("d_seeds", d_seeds if s is None else None), ("seed_vecs", seed_vecs), ("tags", tags),
                    ("exclude", exclude)):
        if t is not None and (not t.is_cuda or t.device != d_vecs.device or
                              (name != "d_seeds" and not t.is_contiguous())):
            raise ValueError(f"{name} must be a contiguous tensor on the device of d_vecs")
    if seed_vecs is not None and seed_vecs.data_ptr() % 16:   # a view such as flat[1:9].view(2, 4) is contiguous
        raise ValueError("seed_vecs must be 16-byte aligned")
    lib = _lib.load()
    v = d_vecs
    with _on_device_of(lib, v, stream) as cur, torch.cuda.stream(cur):
        sd = None
        if seed_vecs is None:
            sd = torch.from_numpy(s).to(v.device) if s is not None else d_seeds.reshape(-1).contiguous()
        n_chains = seed_vecs.shape[0] if seed_vecs is not None else sd.numel()
        order = torch.empty((n_chains, length), dtype=torch.int32, device=v.device)
        value = torch.empty((n_chains, length), dtype=torch.float32, device=v.device)
        _check(lib.bl_amd_mix_device(v.data_ptr(), n, sd.data_ptr() if sd is not None else None,
                                     seed_vecs.data_ptr() if seed_vecs is not None else None, n_chains, int(length), m,
                                     tags.data_ptr() if tags is not None else None, gap,
                                     exclude.data_ptr() if exclude is not None else None, order.data_ptr(),
                                     value.data_ptr(), C.c_void_p(cur.cuda_stream)), "bl_amd_mix_device")
        if s is not None:
            sd.record_stream(cur)   # the uploaded seeds are freed when this returns
    return order, value


def _radius_check(r, metric, shape):
    """(metric code, the radius as a Python float that is an exact f32)"""
    if isinstance(r, bool) or not isinstance(r, (int, float, np.integer, np.floating)):
        raise ValueError(f"the radius must be a real number, got {r!r}")
    m = _metric_check(metric, shape)
    with np.errstate(over="ignore"):
        r32 = np.float32(r)
    if np.isnan(r32):
        raise ValueError("the radius must not be NaN")
    return m, float(r32)


def _radius_host_call(name, args, rows):
    """(offsets, index, value) of `rows` queries from the radius host entry point `name`, called with `args` and the
    three outputs; the two blocks the library allocates are copied and freed"""
    lib = _lib.load()
    offsets = np.empty(rows + 1, dtype=np.int64)
    p_index, p_value = C.POINTER(C.c_int32)(), C.POINTER(C.c_float)()
    rc = getattr(lib, name)(*args, offsets.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(p_index), C.byref(p_value))
    _check(rc, name)
    try:
        total = int(offsets[rows])
        index = np.ctypeslib.as_array(p_index, shape=(total,)).copy() if total else np.empty(0, dtype=np.int32)
        value = np.ctypeslib.as_array(p_value, shape=(total,)).copy() if total else np.empty(0, dtype=np.float32)
    finally:
        _libc_free(p_index)
        _libc_free(p_value)
    return offsets, index, value


def _radius_device_call(count, fill, args, v, rows, values, stream):
    """The same from the device entry points `count` and `fill`, both called with `args` and their outputs on the
    device of the library tensor v: count, read the total back (the one synchronisation), fill"""
    import torch
    lib = _lib.load()
    with _on_device_of(lib, v, stream) as cur, torch.cuda.stream(cur):
        s = C.c_void_p(cur.cuda_stream)
        offsets = torch.empty(rows + 1, dtype=torch.int64, device=v.device)
        _check(getattr(lib, count)(*args, offsets.data_ptr(), s), count)
        total = int(offsets[-1].item())
        # one slot at least: an empty result still goes through the fill call, which then writes nothing
        index = torch.empty(max(total, 1), dtype=torch.int32, device=v.device)
        value = torch.empty(max(total, 1), dtype=torch.float32, device=v.device) if values else None
        _check(getattr(lib, fill)(*args, offsets.data_ptr(), index.data_ptr(), value.data_ptr() if values else None, s),
               fill)
    return offsets, index[:total], value[:total] if values else None


def radius(vecs, r, metric="distance"):
    """The songs within radius r of every song of (n, 4) force vectors, as compressed sparse row lists:
    (offsets int64 (n + 1,), index int32 (total,), value float32 (total,)); row i is index[offsets[i]:offsets[i + 1]],
    in ascending song index, and never lists i.  Within means bl_distance <= r ("distance") or bl_cosine_similarity
    >= r ("cosine") on the f32 matrix entry, whose bits `value` holds; a NaN entry is never within."""
    v = np.ascontiguousarray(vecs, dtype=np.float32)
    m, r = _radius_check(r, metric, v.shape)
    n = v.shape[0]
    return _radius_host_call("bl_amd_radius_host", (v.ctypes.data_as(C.POINTER(_lib.ForceVector)), n, m, r), n)


def radius_device(d_vecs, r, metric="distance", row_begin=0, n_rows=None, values=True, stream=None):
    """radius() for the queries d_vecs[row_begin:row_begin + n_rows] against all of d_vecs, a contiguous float32
    (n, 4) CUDA tensor.  Returns (offsets int64 (n_rows + 1,), index int32 (total,), value float32 (total,) or None
    without `values`) as CUDA tensors on its device.  Count and fill run on `stream` (default: the current stream of
    that device); between them the total is read back, which is the one synchronisation."""
    m, r = _radius_check(r, metric, tuple(d_vecs.shape))
    _device_vecs_check(d_vecs)
    n = d_vecs.shape[0]
    n_rows = _rows_check(n, row_begin, n_rows)
    return _radius_device_call("bl_amd_radius_count_device", "bl_amd_radius_fill_device",
                               (d_vecs.data_ptr(), n, int(row_begin), int(n_rows), m, r), d_vecs, n_rows, values, stream)


def duplicate_groups(vecs, r, metric="distance"):
    """A group label per song of (n, 4) force vectors, int32 (n,): the smallest song index among the songs connected
    to it by steps of at most radius r (bl_distance <= r, or bl_cosine_similarity >= r), as radius() defines "within".
    The same recording under two names gets one label; a song with no neighbour is its own group."""
    v = np.ascontiguousarray(vecs, dtype=np.float32)
    m, r = _radius_check(r, metric, v.shape)
    lib = _lib.load()
    n = v.shape[0]
    group = np.empty(n, dtype=np.int32)
    rc = lib.bl_amd_groups_host(v.ctypes.data_as(C.POINTER(_lib.ForceVector)), n, m, r,
                                group.ctypes.data_as(C.POINTER(C.c_int32)))
    _check(rc, "bl_amd_groups_host")
    return group


def duplicate_groups_device(d_vecs, r, metric="distance", stream=None):
    """duplicate_groups() on the device: d_vecs a contiguous float32 (n, 4) CUDA tensor; returns an int32 (n,) CUDA
    tensor on its device, asynchronously on `stream` (default: the current stream of that device)."""
    import torch
    m, r = _radius_check(r, metric, tuple(d_vecs.shape))
    _device_vecs_check(d_vecs)
    lib = _lib.load()
    v = d_vecs
    n = v.shape[0]
    with _on_device_of(lib, v, stream) as cur, torch.cuda.stream(cur):
        group = torch.empty(n, dtype=torch.int32, device=v.device)
        _check(lib.bl_amd_groups_device(v.data_ptr(), n, m, r, group.data_ptr(), C.c_void_p(cur.cuda_stream)),
               "bl_amd_groups_device")
    return group


def _cross_shapes_check(q_shape, v_shape):
    for name, shape in (("queries", q_shape), ("vecs", v_shape)):
        if len(shape) != 2 or shape[1] != 4 or shape[0] < 1:
            raise ValueError(f"{name} must have shape (m, 4) with m >= 1, got {tuple(shape)}")


def _cross_host_vecs(queries, vecs):
    """(queries, vecs) as contiguous float32 numpy arrays.  Plain sequences are converted; an array that says what it
    holds must hold float32, so that the two sides cannot silently differ in precision."""
    for name, x in (("queries", queries), ("vecs", vecs)):
        if hasattr(x, "dtype") and x.dtype != np.float32:
            raise ValueError(f"{name} must be float32, got {x.dtype}")
    q, v = np.ascontiguousarray(queries, dtype=np.float32), np.ascontiguousarray(vecs, dtype=np.float32)
    _cross_shapes_check(q.shape, v.shape)
    return q, v


def _cross_device_check(d_queries, d_vecs):
    import torch
    for name, t in (("d_queries", d_queries), ("d_vecs", d_vecs)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch tensor")
    _cross_shapes_check(tuple(d_queries.shape), tuple(d_vecs.shape))
    if d_queries.dtype != torch.float32 or d_vecs.dtype != torch.float32:
        raise ValueError(f"d_queries and d_vecs must both be float32, got {d_queries.dtype} and {d_vecs.dtype}")
    if d_queries.device != d_vecs.device:
        raise ValueError(f"d_queries ({d_queries.device}) and d_vecs ({d_vecs.device}) must be on the same device")
    if not d_vecs.is_cuda:
        raise ValueError("d_queries and d_vecs must be CUDA tensors")
    if not d_queries.is_contiguous() or not d_vecs.is_contiguous():
        raise ValueError("d_queries and d_vecs must be contiguous")


def knn_cross(queries, vecs, k, metric="distance"):
    """The k nearest songs of the library `vecs` (n, 4) to each of `queries` (m, 4), vectors that need not be songs of
    it: (index (m, k) int32, value (m, k) float32), ordered and valued as knn() does.  Unlike knn() nothing is left
    out: a query equal to library song 7 lists song 7 first, at distance 0.  Slots past n hold -1 and NaN."""
    m_code = _knn_check(k, metric, (1, 4))   # the shapes are checked per side below
    q, v = _cross_host_vecs(queries, vecs)
    m = q.shape[0]
    fv = C.POINTER(_lib.ForceVector)
    return _knn_host_call("bl_amd_cross_knn_host",
                          (q.ctypes.data_as(fv), m, v.ctypes.data_as(fv), v.shape[0], int(k), m_code), m, k)


def knn_cross_device(d_queries, d_vecs, k, metric="distance", stream=None):
    """knn_cross() on the device: d_queries (m, 4) and d_vecs (n, 4) contiguous float32 CUDA tensors on one device;
    d_queries may be a view into d_vecs and needs 16-byte alignment only.  Returns (index, value) CUDA tensors of
    shape (m, k), asynchronously on `stream` (default: the current stream of that device).  Queries are independent:
    shard by slicing d_queries."""
    m_code = _knn_check(k, metric, (1, 4))
    _cross_device_check(d_queries, d_vecs)
    q, v = d_queries, d_vecs
    m = q.shape[0]
    return _knn_device_call("bl_amd_cross_knn_device", (q.data_ptr(), m, v.data_ptr(), v.shape[0], int(k), m_code), v, m,
                            k, stream)


def _radius_cross_check(r, metric):
    return _radius_check(r, metric, (1, 4))   # the shapes are checked per side


def radius_cross(queries, vecs, r, metric="distance"):
    """The songs of the library `vecs` (n, 4) within radius r of each of `queries` (m, 4), as compressed sparse row
    lists: (offset int64 (m + 1,), index int32 (total,), value float32 (total,)), as radius() defines "within" and
    orders a row.  Unlike radius() nothing is left out: with r = 0 a query that is in the library finds its copy."""
    m_code, r = _radius_cross_check(r, metric)
    q, v = _cross_host_vecs(queries, vecs)
    m = q.shape[0]
    fv = C.POINTER(_lib.ForceVector)
    return _radius_host_call("bl_amd_cross_radius_host",
                             (q.ctypes.data_as(fv), m, v.ctypes.data_as(fv), v.shape[0], m_code, r), m)


def radius_cross_device(d_queries, d_vecs, r, metric="distance", values=True, stream=None):
    """radius_cross() on the device, tensors as for knn_cross_device().  Returns (offset int64 (m + 1,), index int32
    (total,), value float32 (total,) or None without `values`) as CUDA tensors.  Count and fill run on `stream`;
    between them the total is read back, which is the one synchronisation."""
    m_code, r = _radius_cross_check(r, metric)
    _cross_device_check(d_queries, d_vecs)
    q, v = d_queries, d_vecs
    m, n = q.shape[0], v.shape[0]
    return _radius_device_call("bl_amd_cross_radius_count_device", "bl_amd_cross_radius_fill_device",
                               (q.data_ptr(), m, v.data_ptr(), n, m_code, r), v, m, values, stream)


def playlist_vec(vecs, seed_vec):
    """playlist() from a seed that need not be a song of `vecs`: the song indices by increasing bl_distance from the
    4-component `seed_vec`, and the distances.  Stable for ties; a seed equal to a song lists it at distance 0.  NaN
    distances after every number, in index order: numpy's stable argsort."""
    v = np.ascontiguousarray(vecs, dtype=np.float32)
    if v.ndim != 2 or v.shape[1] != 4 or v.shape[0] < 1:
        raise ValueError(f"force vectors must have shape (n, 4) with n >= 1, got {v.shape}")
    sv = np.asarray(seed_vec, dtype=np.float32)
    if sv.shape != (4,):
        raise ValueError(f"the seed must be one force vector of 4 components, got shape {sv.shape}")
    lib = _lib.load()
    n = v.shape[0]
    order = np.empty(n, dtype=np.int32)
    dist = np.empty(n, dtype=np.float32)
    seed = _lib.ForceVector(*(float(x) for x in sv))
    rc = lib.bl_amd_playlist_vec_host(v.ctypes.data_as(C.POINTER(_lib.ForceVector)), n, seed,
                                      order.ctypes.data_as(C.POINTER(C.c_int32)),
                                      dist.ctypes.data_as(C.POINTER(C.c_float)))
    _check(rc, "bl_amd_playlist_vec_host")
    return order, dist
