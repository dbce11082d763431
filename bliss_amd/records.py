"""The records of the C-ABI as numpy structured arrays, and the readers that work on records alone (no device)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check

# bl_amd_song_result with its leading force vector `v` flattened into four fields
RESULT_DTYPE = np.dtype([
    ("tempo", "<f4"), ("amplitude", "<f4"), ("frequency", "<f4"), ("attack", "<f4"),
    ("force", "<f4"), ("calm_or_loud", "<i4"), ("status", "<i4"), ("start", "<i4"),
    ("end", "<i4"), ("mean", "<i4"), ("variance", "<i4"), ("n_frames", "<i4"),
    ("nb_frames", "<i4"), ("n_windows", "<i4"), ("beat", "<i4"), ("hist_integral", "<f4"),
    ("freq_peak", "<f4"), ("atk_sum", "<f8")], align=True)
_R, _V = _lib.SongResult, _lib.ForceVector
assert [(k, RESULT_DTYPE.fields[k][1], RESULT_DTYPE.fields[k][0]) for k in RESULT_DTYPE.names] == \
    [(k, _R.v.offset + getattr(_V, k).offset, np.dtype(t)) for k, t in _V._fields_] + \
    [(k, getattr(_R, k).offset, np.dtype(t)) for k, t in _R._fields_[1:]]
assert RESULT_DTYPE.itemsize == C.sizeof(_R) == 80

# the other records have the header's field names: taken from the ctypes structures
LEVELS_DTYPE = np.dtype(_lib.SongLevels)
TIMBRE_SONG_DTYPE = np.dtype(_lib.SongTimbre)
TIMBRE_FRAME_DTYPE = np.dtype(_lib.FrameTimbre)
RHYTHM_DTYPE = np.dtype(_lib.SongRhythm)
BEATS_DTYPE = np.dtype(_lib.SongBeats)
LOUD_DTYPE = np.dtype(_lib.SongLoud)
TPEAK_DTYPE = np.dtype(_lib.SongTpeak)
FPRINT_MATCH_DTYPE = np.dtype(_lib.FprintMatch)
FORM_DTYPE = np.dtype(_lib.SongForm)
COVER_MATCH_DTYPE = np.dtype(_lib.CoverMatch)
CHORDS_DTYPE = np.dtype(_lib.SongChords)
TGRAM_DTYPE = np.dtype(_lib.SongTgram)
TGRAM_FRAME_DTYPE = np.dtype(_lib.TgramFrame)
TBEATS_DTYPE = np.dtype(_lib.SongTbeats)
CHROMA_DTYPE = np.dtype(_lib.SongChroma)
FRAME_CHROMA_DTYPE = np.dtype(_lib.FrameChroma)
MEL_DTYPE = np.dtype(_lib.SongMel)
FRAME_MEL_DTYPE = np.dtype(_lib.FrameMel)

LEVELS_DB_DTYPE = np.dtype([("peak_db", "<f8", (2,)), ("rms_db", "<f8", (2,)), ("dc", "<f8", (2,)),
                            ("zcr", "<f8", (2,))])
TIMBRE_HZ_DTYPE = np.dtype([("centroid_hz", "<f8"), ("centroid_std_hz", "<f8"), ("rolloff_hz", "<f8"),
                            ("rolloff_std_hz", "<f8"), ("peak_hz", "<f8"), ("peak_std_hz", "<f8")])


def results_to_numpy(raw_bytes):
    """bytes / uint8 array of bl_amd_song_result records -> structured numpy array."""
    return np.frombuffer(bytes(raw_bytes), dtype=RESULT_DTYPE).copy()


def levels_to_numpy(raw):
    """bytes / uint8 array of bl_amd_song_levels records -> structured numpy array with the header's field names."""
    return np.frombuffer(bytes(raw), dtype=LEVELS_DTYPE).copy()


def timbre_to_numpy(raw_songs, raw_frames=None):
    """bytes / uint8 arrays of bl_amd_song_timbre (and bl_amd_frame_timbre) records -> structured numpy arrays with the
    header's field names.  Returns the song array, or (songs, frames) when raw_frames is given."""
    songs = np.frombuffer(bytes(raw_songs), dtype=TIMBRE_SONG_DTYPE).copy()
    if raw_frames is None:
        return songs
    return songs, np.frombuffer(bytes(raw_frames), dtype=TIMBRE_FRAME_DTYPE).copy()


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
    check(lib.bl_amd_gapless_host(lv.ctypes.data_as(C.POINTER(_lib.SongLevels)), lv.size,
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
