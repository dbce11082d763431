"""ctypes binding of libbliss_amd.so (the C-ABI of include/bliss.h + include/bliss_amd.h).

This mirrors what the reference's cffi module `bliss._bliss` exposes
(ref python/build_bliss.py:35-38: cdef = include/bliss.h minus '#' lines) plus the
batch extension.  The shared object is built in-tree by `__graft_entry__.build()`
(make -C bliss_amd/csrc) and loaded from this directory; there is no fallback:
a missing library raises ImportError.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# BLISS_AMD_LIB: load another build of the same C-ABI (A/B measurements of kernel variants)
LIB_PATH = os.environ.get("BLISS_AMD_LIB") or os.path.join(_HERE, "libbliss_amd.so")

BL_LOUD, BL_CALM, BL_UNKNOWN, BL_UNEXPECTED, BL_OK = 0, 1, 2, -2, 0
BL_AMD_KNN_DISTANCE, BL_AMD_KNN_COSINE, BL_AMD_KNN_MAX_K = 0, 1, 128  # include/bliss_amd.h
BL_AMD_CHAIN_AUTO, BL_AMD_CHAIN_PER_CHAIN, BL_AMD_CHAIN_SPLIT = 0, 1, 2  # include/bliss_amd.h
BL_AMD_MIX_MAX_GAP = 16  # include/bliss_amd.h
BL_AMD_PART_SPECTRUM, BL_AMD_PART_SUMS, BL_AMD_PART_HIST = 1, 2, 4  # include/bliss_amd.h
BL_AMD_DESC_DIMS, BL_AMD_DESC_SCALE_MAX = 32, 32512  # include/bliss_amd.h
BL_AMD_MEL_BANDS, BL_AMD_MEL_COEFFS = 32, 13  # include/bliss_amd.h
BL_AMD_HMIX_KEY, BL_AMD_HMIX_TEMPO, BL_AMD_HMIX_HALF_DOUBLE = 1, 2, 4  # include/bliss_amd.h


class ForceVector(C.Structure):  # ref include/bliss.h:26-31
    _fields_ = [("tempo", C.c_float), ("amplitude", C.c_float),
                ("frequency", C.c_float), ("attack", C.c_float)]


class EnvelopeResult(C.Structure):  # ref include/bliss.h:34-37
    _fields_ = [("tempo", C.c_float), ("attack", C.c_float)]


class BlSong(C.Structure):  # ref include/bliss.h:49-67
    _fields_ = [("force", C.c_float), ("force_vector", ForceVector),
                ("sample_array", C.c_void_p), ("channels", C.c_int), ("nSamples", C.c_int),
                ("sample_rate", C.c_int), ("bitrate", C.c_int),
                ("nb_bytes_per_sample", C.c_int), ("calm_or_loud", C.c_int),
                ("resampled", C.c_int), ("duration", C.c_uint64),
                ("filename", C.c_char_p), ("artist", C.c_char_p), ("title", C.c_char_p),
                ("album", C.c_char_p), ("tracknumber", C.c_char_p), ("genre", C.c_char_p)]


class SongDesc(C.Structure):  # include/bliss_amd.h bl_amd_song_desc
    _fields_ = [("pcm_offset", C.c_uint64), ("n_samples", C.c_int32),
                ("channels", C.c_int32), ("duration", C.c_uint64)]


class ResampleDesc(C.Structure):  # include/bliss_amd.h bl_amd_resample_desc
    _fields_ = [("in_offset", C.c_uint64), ("out_offset", C.c_uint64), ("frames", C.c_int32),
                ("channels", C.c_int32)]


class SongResult(C.Structure):  # include/bliss_amd.h bl_amd_song_result
    _fields_ = [("v", ForceVector), ("force", C.c_float), ("calm_or_loud", C.c_int32),
                ("status", C.c_int32), ("start", C.c_int32), ("end", C.c_int32),
                ("mean", C.c_int32), ("variance", C.c_int32), ("n_frames", C.c_int32),
                ("nb_frames", C.c_int32), ("n_windows", C.c_int32), ("beat", C.c_int32),
                ("hist_integral", C.c_float), ("freq_peak", C.c_float),
                ("atk_sum", C.c_double)]


class SongLevels(C.Structure):  # include/bliss_amd.h bl_amd_song_levels
    _fields_ = [("sum", C.c_int64 * 2), ("sum_sq", C.c_uint64 * 2), ("peak", C.c_int32 * 2),
                ("zero_cross", C.c_int32 * 2), ("clipped", C.c_int32 * 2), ("lead", C.c_int32), ("trail", C.c_int32),
                ("frames", C.c_int32), ("status", C.c_int32), ("head", C.c_int16 * 2), ("tail", C.c_int16 * 2)]


class FrameTimbre(C.Structure):  # include/bliss_amd.h bl_amd_frame_timbre
    _fields_ = [("energy", C.c_uint64), ("moment", C.c_uint64), ("rolloff", C.c_int32), ("peak", C.c_int32)]


class SongTimbre(C.Structure):  # include/bliss_amd.h bl_amd_song_timbre
    _fields_ = [("centroid_sum", C.c_uint64), ("centroid_sumsq", C.c_uint64), ("rolloff_sum", C.c_uint64),
                ("rolloff_sumsq", C.c_uint64), ("peak_sum", C.c_uint64), ("peak_sumsq", C.c_uint64),
                ("energy_max", C.c_uint64), ("frames", C.c_int32), ("used", C.c_int32), ("status", C.c_int32),
                ("reserved", C.c_int32)]


class SongRhythm(C.Structure):  # include/bliss_amd.h bl_amd_song_rhythm
    _fields_ = [("r0", C.c_uint64), ("r_prev", C.c_uint64), ("r_lag", C.c_uint64), ("r_next", C.c_uint64),
                ("r_peak", C.c_uint64), ("onset_sum", C.c_uint64), ("onset_max", C.c_uint32), ("hops", C.c_int32),
                ("terms", C.c_int32), ("lag", C.c_int32), ("lag_peak", C.c_int32), ("status", C.c_int32)]


class SongBeats(C.Structure):  # include/bliss_amd.h bl_amd_song_beats
    _fields_ = [("score", C.c_int64), ("pen_scale", C.c_uint64), ("hops", C.c_int32), ("period", C.c_int32),
                ("n_beats", C.c_int32), ("first", C.c_int32), ("last", C.c_int32), ("status", C.c_int32)]


class LoudParams(C.Structure):  # include/bliss_amd.h bl_amd_loud_params
    _fields_ = [("s1_b", C.c_double * 3), ("s1_a", C.c_double * 2), ("s2_a", C.c_double * 2), ("hop", C.c_int32),
                ("warm", C.c_int32), ("abs_gate", C.c_uint64)]


class SongLoud(C.Structure):  # include/bliss_amd.h bl_amd_song_loud
    _fields_ = [("gated_sum", C.c_uint64 * 2), ("abs_sum", C.c_uint64 * 2), ("momentary_max", C.c_uint64),
                ("st_max", C.c_uint64), ("lra_lo", C.c_uint64), ("lra_hi", C.c_uint64), ("gated_count", C.c_int32),
                ("abs_count", C.c_int32), ("st_gated", C.c_int32), ("hops", C.c_int32), ("blocks", C.c_int32),
                ("status", C.c_int32)]


class SongTpeak(C.Structure):  # include/bliss_amd.h bl_amd_song_tpeak
    _fields_ = [("at", C.c_int64 * 2), ("overs", C.c_int64 * 2), ("tpeak", C.c_uint32 * 2), ("peak", C.c_int32 * 2),
                ("frames", C.c_int32), ("status", C.c_int32)]


class FprintMatch(C.Structure):  # include/bliss_amd.h bl_amd_fprint_match
    _fields_ = [("errors", C.c_uint32), ("overlap", C.c_uint32), ("offset", C.c_int32), ("score", C.c_uint32),
                ("status", C.c_int32), ("reserved", C.c_int32)]


class FormParams(C.Structure):  # include/bliss_amd.h bl_amd_form_params
    _fields_ = [("pool", C.c_int32), ("seg", C.c_int32), ("min_lag", C.c_int32), ("nov", C.c_int32),
                ("peak_num", C.c_int32), ("peak_den", C.c_int32), ("reserved", C.c_int32)]


class SongForm(C.Structure):  # include/bliss_amd.h bl_amd_song_form
    _fields_ = [("units", C.c_int32), ("status", C.c_int32), ("thumb_start", C.c_int32), ("thumb_lag", C.c_int32),
                ("thumb_score", C.c_uint32), ("thumb_self", C.c_uint32), ("boundaries", C.c_int32),
                ("nov_max_unit", C.c_int32), ("nov_max", C.c_uint64), ("reserved", C.c_uint64)]


class CoverParams(C.Structure):  # include/bliss_amd.h bl_amd_cover_params
    _fields_ = [("thr", C.c_int32), ("gap", C.c_int32), ("transpose", C.c_int32), ("reserved", C.c_int32)]


class CoverMatch(C.Structure):  # include/bliss_amd.h bl_amd_cover_match
    _fields_ = [("score", C.c_uint32), ("a_start", C.c_int32), ("a_end", C.c_int32), ("b_start", C.c_int32),
                ("b_end", C.c_int32), ("transpose", C.c_int32), ("units_a", C.c_int32), ("units_b", C.c_int32),
                ("status", C.c_int32), ("reserved", C.c_int32)]


class ChordsParams(C.Structure):  # include/bliss_amd.h bl_amd_chords_params
    _fields_ = [("none", C.c_int32), ("reserved", C.c_int32), ("cost", C.c_uint16 * 625), ("pad", C.c_uint16 * 3)]


class SongChords(C.Structure):  # include/bliss_amd.h bl_amd_song_chords
    _fields_ = [("units", C.c_int32), ("status", C.c_int32), ("score", C.c_int32), ("changes", C.c_int32),
                ("top", C.c_int32), ("top_units", C.c_int32), ("none_units", C.c_int32), ("reserved", C.c_int32)]


class TgramParams(C.Structure):  # include/bliss_amd.h bl_amd_tgram_params
    _fields_ = [("stride", C.c_int32), ("blocks", C.c_int32), ("lag_min", C.c_int32), ("lag_max", C.c_int32),
                ("tol", C.c_int32), ("octaves", C.c_int32), ("reserved", C.c_int32 * 2)]


class TgramFrame(C.Structure):  # include/bliss_amd.h bl_amd_tgram_frame
    _fields_ = [("r0", C.c_uint64), ("r_prev", C.c_uint64), ("r_lag", C.c_uint64), ("r_next", C.c_uint64),
                ("lag", C.c_int32), ("lag_peak", C.c_int32)]


class SongTgram(C.Structure):  # include/bliss_amd.h bl_amd_song_tgram
    _fields_ = [("hops", C.c_int32), ("frames", C.c_int32), ("n_tempo", C.c_int32), ("status", C.c_int32),
                ("frame_first", C.c_int32), ("frame_last", C.c_int32), ("lag_first", C.c_int32),
                ("lag_last", C.c_int32), ("lag_low", C.c_int32), ("lag_high", C.c_int32), ("lag_median", C.c_int32),
                ("n_near", C.c_int32), ("n_jumps", C.c_int32), ("reserved", C.c_int32)]


class TbeatsParams(C.Structure):  # include/bliss_amd.h bl_amd_tbeats_params
    _fields_ = [("seg", C.c_int32), ("origin", C.c_int32), ("tight", C.c_int32), ("fold", C.c_int32),
                ("reserved", C.c_int32 * 4)]


class SongTbeats(C.Structure):  # include/bliss_amd.h bl_amd_song_tbeats
    _fields_ = [("score", C.c_int64), ("pen_scale", C.c_uint64), ("hops", C.c_int32), ("frames", C.c_int32),
                ("n_beats", C.c_int32), ("first", C.c_int32), ("last", C.c_int32), ("status", C.c_int32),
                ("period_first", C.c_int32), ("period_last", C.c_int32), ("n_runs", C.c_int32),
                ("n_filled", C.c_int32), ("n_folded", C.c_int32), ("reserved", C.c_int32)]


class FrameChroma(C.Structure):  # include/bliss_amd.h bl_amd_frame_chroma
    _fields_ = [("x", C.c_uint64 * 12)]


class SongChroma(C.Structure):  # include/bliss_amd.h bl_amd_song_chroma
    _fields_ = [("chroma", C.c_uint64 * 12), ("score", C.c_int64), ("score_next", C.c_int64), ("frames", C.c_int32),
                ("key", C.c_int32), ("status", C.c_int32), ("reserved", C.c_int32)]


class FrameMel(C.Structure):  # include/bliss_amd.h bl_amd_frame_mel
    _fields_ = [("mfcc", C.c_int32 * 13), ("flat", C.c_int32)]


class SongMel(C.Structure):  # include/bliss_amd.h bl_amd_song_mel
    _fields_ = [("mfcc_sum", C.c_int64 * 13), ("mfcc_sumsq", C.c_uint64 * 13), ("flat_sum", C.c_int64),
                ("flat_sumsq", C.c_uint64), ("band_sum", C.c_uint64 * 32), ("frames", C.c_int32), ("used", C.c_int32),
                ("status", C.c_int32), ("reserved", C.c_int32)]


class Desc(C.Structure):  # include/bliss_amd.h bl_amd_desc
    _fields_ = [("q", C.c_int16 * 32)]


class DescRange(C.Structure):  # include/bliss_amd.h bl_amd_desc_range
    _fields_ = [("lo", C.c_float * 32), ("hi", C.c_float * 32), ("n_finite", C.c_uint32 * 32)]


class HmixAttr(C.Structure):  # include/bliss_amd.h bl_amd_hmix_attr
    _fields_ = [("tempo", C.c_uint16), ("key", C.c_uint8), ("reserved", C.c_uint8)]


class HmixRule(C.Structure):  # include/bliss_amd.h bl_amd_hmix_rule
    _fields_ = [("key_ok", C.c_uint32 * 24), ("tempo_tol", C.c_uint32), ("flags", C.c_uint32)]


class Shard(C.Structure):  # include/bliss_amd.h bl_amd_shard
    _fields_ = [("device", C.c_int32), ("n_songs", C.c_int32), ("d_pcm", C.c_void_p),
                ("h_desc", C.POINTER(SongDesc)), ("d_results", C.c_void_p), ("d_rows", C.c_void_p)]


# every symbol include/*.h declares: name -> (restype, argtypes)
_P = C.POINTER
SYMBOLS = {
    # include/bliss.h
    "bl_analyze": (C.c_int, [C.c_char_p, _P(BlSong)]),
    "bl_distance_file": (C.c_float, [C.c_char_p, C.c_char_p, _P(BlSong), _P(BlSong)]),
    "bl_distance": (C.c_float, [ForceVector, ForceVector]),
    "bl_cosine_similarity_file": (C.c_float, [C.c_char_p, C.c_char_p, _P(BlSong), _P(BlSong)]),
    "bl_cosine_similarity": (C.c_float, [ForceVector, ForceVector]),
    "bl_envelope_sort": (None, [_P(BlSong), _P(EnvelopeResult)]),
    "bl_amplitude_sort": (C.c_float, [_P(BlSong)]),
    "bl_frequency_sort": (C.c_float, [_P(BlSong)]),
    "bl_audio_decode": (C.c_int, [C.c_char_p, _P(BlSong)]),
    "bl_free_song": (None, [_P(BlSong)]),
    "bl_version": (C.c_float, []),
    "bl_initialize_song": (None, [_P(BlSong)]),
    "bl_mean": (C.c_int, [_P(C.c_int16), C.c_int]),
    "bl_variance": (C.c_int, [_P(C.c_int16), C.c_int, C.c_int]),
    "bl_rectangular_filter": (None, [_P(C.c_double), _P(C.c_double), C.c_int, C.c_int]),
    # include/bliss_amd.h
    "bl_amd_init": (C.c_int, [C.c_int]),
    "bl_amd_device_count": (C.c_int, []),
    "bl_amd_ctx_create": (C.c_int, [C.c_int, _P(C.c_void_p)]),
    "bl_amd_ctx_destroy": (None, [C.c_void_p]),
    "bl_amd_ctx_device": (C.c_int, [C.c_void_p]),
    "bl_amd_analyze_batch_device": (C.c_int, [C.c_void_p, _P(SongDesc), C.c_int, C.c_void_p, C.c_void_p]),
    "bl_amd_ctx_analyze_batch_device": (C.c_int, [C.c_void_p, C.c_void_p, _P(SongDesc), C.c_int, C.c_void_p,
                                                  C.c_void_p]),
    "bl_amd_ctx_analyze_batch_host": (C.c_int, [C.c_void_p, _P(C.c_void_p), _P(C.c_int32), _P(C.c_int32),
                                                _P(C.c_uint64), C.c_int, _P(SongResult)]),
    "bl_amd_analyze_files": (C.c_int, [_P(C.c_char_p), C.c_int, _P(BlSong), _P(C.c_int), C.c_int, C.c_int]),
    "bl_amd_set_host_transfer": (C.c_int, [C.c_int]),
    "bl_amd_analyze_batch_host_s32": (C.c_int, [_P(C.c_void_p), _P(C.c_int32), _P(C.c_int32),
                                                _P(C.c_uint64), C.c_int, _P(SongResult)]),
    "bl_amd_analyze_batch_host_rate": (C.c_int, [_P(C.c_void_p), C.c_int, _P(C.c_int32), _P(C.c_int32),
                                                 _P(C.c_uint64), C.c_int, C.c_int, _P(SongResult)]),
    "bl_amd_narrow_s32_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "bl_amd_resample_out_frames": (C.c_size_t, [C.c_size_t, C.c_int]),
    "bl_amd_resample_host": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_int, C.c_int,
                                       _P(_P(C.c_int16)), _P(C.c_size_t)]),
    "bl_amd_resample_batch_device": (C.c_int, [C.c_void_p, C.c_int, _P(ResampleDesc), C.c_int, C.c_int,
                                               C.c_void_p, C.c_void_p]),
    "bl_amd_ctx_resample_batch_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, _P(ResampleDesc), C.c_int,
                                                   C.c_int, C.c_void_p, C.c_void_p]),
    "bl_amd_analyze_corpus_multi": (C.c_int, [_P(C.c_void_p), _P(C.c_int32), _P(C.c_int32), _P(C.c_uint64),
                                              C.c_int, _P(C.c_int), C.c_int, C.c_int, _P(SongResult),
                                              _P(C.c_float)]),
    "bl_amd_analyze_corpus_multi_device": (C.c_int, [_P(Shard), C.c_int, C.c_int, _P(SongResult), _P(C.c_float)]),
    "bl_amd_decode_allow_native_rate": (None, [C.c_int]),
    "bl_amd_flac_verify": (C.c_int, [C.c_char_p, _P(C.c_uint8), _P(C.c_uint8)]),
    "bl_amd_analyze_batch_host": (C.c_int, [_P(C.c_void_p), _P(C.c_int32), _P(C.c_int32),
                                            _P(C.c_uint64), C.c_int, _P(SongResult)]),
    "bl_amd_distance_matrix_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "bl_amd_cosine_matrix_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "bl_amd_distance_matrix_host": (C.c_int, [_P(ForceVector), C.c_int, _P(C.c_float)]),
    "bl_amd_cosine_matrix_host": (C.c_int, [_P(ForceVector), C.c_int, _P(C.c_float)]),
    "bl_amd_selftest_sqrt": (C.c_int, [_P(C.c_uint64)]),
    "bl_amd_selftest_cos": (C.c_int, [_P(C.c_uint64), C.c_uint64]),
    "bl_amd_playlist_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bl_amd_playlist_host": (C.c_int, [_P(ForceVector), C.c_int, C.c_int, _P(C.c_int32), _P(C.c_float)]),
    "bl_amd_playlist_vec_device": (C.c_int, [C.c_void_p, C.c_int, ForceVector, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bl_amd_playlist_vec_host": (C.c_int, [_P(ForceVector), C.c_int, ForceVector, _P(C.c_int32), _P(C.c_float)]),
    "bl_amd_knn_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                    C.c_void_p]),
    "bl_amd_knn_host": (C.c_int, [_P(ForceVector), C.c_int, C.c_int, C.c_int, _P(C.c_int32), _P(C.c_float)]),
    "bl_amd_cross_knn_device": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                          C.c_void_p, C.c_void_p]),
    "bl_amd_cross_knn_host": (C.c_int, [_P(ForceVector), C.c_int, _P(ForceVector), C.c_int, C.c_int, C.c_int,
                                        _P(C.c_int32), _P(C.c_float)]),
    "bl_amd_chain_device": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                      C.c_void_p, C.c_void_p]),
    "bl_amd_ctx_chain_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "bl_amd_chain_host": (C.c_int, [_P(ForceVector), C.c_int, _P(C.c_int32), C.c_int, C.c_int, C.c_int, _P(C.c_int32),
                                    _P(C.c_float)]),
    "bl_amd_chain_shape": (C.c_int, [C.c_int, C.c_int]),
    "bl_amd_chain_force_shape": (C.c_int, [C.c_int]),
    "bl_amd_mix_device": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                    C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bl_amd_ctx_mix_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                        C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bl_amd_mix_host": (C.c_int, [_P(ForceVector), C.c_int, _P(C.c_int32), _P(ForceVector), C.c_int, C.c_int, C.c_int,
                                  _P(C.c_int32), C.c_int, _P(C.c_uint8), _P(C.c_int32), _P(C.c_float)]),
    "bl_amd_radius_bound": (C.c_float, [C.c_float]),
    "bl_amd_radius_count_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p,
                                             C.c_void_p]),
    "bl_amd_ctx_radius_count_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                                 C.c_void_p, C.c_void_p]),
    "bl_amd_radius_fill_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p]),
    "bl_amd_ctx_radius_fill_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bl_amd_radius_host": (C.c_int, [_P(ForceVector), C.c_int, C.c_int, C.c_float, _P(C.c_int64), _P(_P(C.c_int32)),
                                     _P(_P(C.c_float))]),
    "bl_amd_cross_radius_count_device": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float,
                                                   C.c_void_p, C.c_void_p]),
    "bl_amd_ctx_cross_radius_count_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                       C.c_float, C.c_void_p, C.c_void_p]),
    "bl_amd_cross_radius_fill_device": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bl_amd_ctx_cross_radius_fill_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                      C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bl_amd_cross_radius_host": (C.c_int, [_P(ForceVector), C.c_int, _P(ForceVector), C.c_int, C.c_int, C.c_float,
                                           _P(C.c_int64), _P(_P(C.c_int32)), _P(_P(C.c_float))]),
    "bl_amd_groups_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "bl_amd_ctx_groups_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p,
                                           C.c_void_p]),
    "bl_amd_groups_host": (C.c_int, [_P(ForceVector), C.c_int, C.c_int, C.c_float, _P(C.c_int32)]),
    "bl_amd_levels_batch_device": (C.c_int, [C.c_void_p, _P(SongDesc), C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "bl_amd_ctx_levels_batch_device": (C.c_int, [C.c_void_p, C.c_void_p, _P(SongDesc), C.c_int, C.c_int, C.c_void_p,
                                                 C.c_void_p]),
    "bl_amd_levels_batch_host": (C.c_int, [_P(C.c_void_p), _P(C.c_int32), _P(C.c_int32), C.c_int, C.c_int,
                                           _P(SongLevels)]),
    "bl_amd_gapless_host": (C.c_int, [_P(SongLevels), C.c_int, _P(C.c_uint8)]),
    "bl_amd_levels_peak_db": (C.c_double, [_P(SongLevels), C.c_int]),
    "bl_amd_levels_rms_db": (C.c_double, [_P(SongLevels), C.c_int]),
    "bl_amd_timbre_frames": (C.c_int, [C.c_int, C.c_int]),
    "bl_amd_timbre_batch_device": (C.c_int, [C.c_void_p, _P(SongDesc), C.c_int, C.c_int, C.c_uint64, C.c_void_p,
                                             C.c_void_p, C.c_longlong, C.c_void_p]),
    "bl_amd_ctx_timbre_batch_device": (C.c_int, [C.c_void_p, C.c_void_p, _P(SongDesc), C.c_int, C.c_int, C.c_uint64,
                                                 C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]),
    "bl_amd_timbre_batch_host": (C.c_int, [_P(C.c_void_p), _P(C.c_int32), _P(C.c_int32), C.c_int, C.c_int, C.c_uint64,
                                           _P(SongTimbre), _P(FrameTimbre)]),
    "bl_amd_timbre_centroid_hz": (C.c_double, [_P(SongTimbre), C.c_int, _P(C.c_double)]),
    "bl_amd_timbre_rolloff_hz": (C.c_double, [_P(SongTimbre), C.c_int, _P(C.c_double)]),
    "bl_amd_timbre_peak_hz": (C.c_double, [_P(SongTimbre), C.c_int, _P(C.c_double)]),
    "bl_amd_rhythm_hops": (C.c_int, [C.c_int, C.c_int]),
    "bl_amd_rhythm_batch_device": (C.c_int, [C.c_void_p, _P(SongDesc), C.c_int, C.c_int, C.c_int, C.c_void_p,
                                             C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]),
    "bl_amd_ctx_rhythm_batch_device": (C.c_int, [C.c_void_p, C.c_void_p, _P(SongDesc), C.c_int, C.c_int, C.c_int,
                                                 C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]),
    "bl_amd_rhythm_batch_host": (C.c_int, [_P(C.c_void_p), _P(C.c_int32), _P(C.c_int32), C.c_int, C.c_int, C.c_int,
                                           _P(SongRhythm), _P(C.c_uint32), _P(C.c_uint64)]),
    "bl_amd_rhythm_from_onsets": (C.c_int, [_P(C.c_uint32), _P(C.c_int32), C.c_int, C.c_int, C.c_int, _P(SongRhythm),
                                            _P(C.c_uint64)]),
    "bl_amd_rhythm_bpm": (C.c_double, [_P(SongRhythm), C.c_int]),
    "bl_amd_rhythm_strength": (C.c_double, [_P(SongRhythm)]),
    "bl_amd_selftest_isqrt": (C.c_int, [_P(C.c_uint64)]),
    "bl_amd_beats_device": (C.c_int, [C.c_void_p, _P(C.c_int32), C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bl_amd_ctx_beats_device": (C.c_int, [C.c_void_p, C.c_void_p, _P(C.c_int32), C.c_int, C.c_void_p, C.c_int, C.c_int,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bl_amd_beats_host": (C.c_int, [_P(C.c_uint32), _P(C.c_int32), C.c_int, _P(C.c_int32), C.c_int, _P(SongBeats),
                                    _P(C.c_uint8), _P(C.c_uint16), _P(C.c_int64)]),
    "bl_amd_beats_list": (C.c_int, [_P(C.c_uint8), C.c_int, C.c_int, _P(C.c_int32), _P(C.c_double), C.c_int]),
    "bl_amd_beats_bpm": (C.c_double, [_P(SongBeats), C.c_int]),
    "bl_amd_loud_batch_device": (C.c_int, [C.c_void_p, _P(SongDesc), C.c_int, _P(LoudParams), C.c_void_p, C.c_void_p,
                                           C.c_longlong, C.c_void_p]),
    "bl_amd_ctx_loud_batch_device": (C.c_int, [C.c_void_p, C.c_void_p, _P(SongDesc), C.c_int, _P(LoudParams), C.c_void_p,
                                               C.c_void_p, C.c_longlong, C.c_void_p]),
    "bl_amd_loud_batch_host": (C.c_int, [_P(C.c_void_p), _P(C.c_int32), _P(C.c_int32), C.c_int, _P(LoudParams),
                                         _P(SongLoud), _P(C.c_uint64)]),
    "bl_amd_loud_from_hops": (C.c_int, [_P(C.c_uint64), _P(C.c_int32), C.c_int, _P(LoudParams), _P(SongLoud)]),
    "bl_amd_loud_kweight": (C.c_int, [C.c_int, _P(LoudParams)]),
    "bl_amd_loud_lufs": (C.c_double, [_P(SongLoud), C.c_int]),
    "bl_amd_loud_momentary_max_lufs": (C.c_double, [_P(SongLoud), C.c_int]),
    "bl_amd_loud_short_max_lufs": (C.c_double, [_P(SongLoud), C.c_int]),
    "bl_amd_loud_range_lu": (C.c_double, [_P(SongLoud)]),
    "bl_amd_loud_gain_db": (C.c_double, [_P(SongLoud), C.c_int, C.c_double]),
    "bl_amd_loud_profile_ms": (C.c_double, [C.c_char_p, _P(C.c_int)]),
    "bl_amd_tpeak_batch_device": (C.c_int, [C.c_void_p, _P(SongDesc), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                            C.c_longlong, C.c_void_p]),
    "bl_amd_ctx_tpeak_batch_device": (C.c_int, [C.c_void_p, C.c_void_p, _P(SongDesc), C.c_int, C.c_int, C.c_int,
                                                C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]),
    "bl_amd_tpeak_batch_host": (C.c_int, [_P(C.c_void_p), _P(C.c_int32), _P(C.c_int32), C.c_int, C.c_int, C.c_int,
                                          _P(SongTpeak), _P(C.c_uint32)]),
    "bl_amd_tpeak_table": (None, [_P(C.c_int32)]),
    "bl_amd_tpeak_shape": (None, [_P(C.c_int), _P(C.c_int)]),
    "bl_amd_tpeak_dbtp": (C.c_double, [_P(SongTpeak), C.c_int]),
    "bl_amd_tpeak_song_dbtp": (C.c_double, [_P(SongTpeak)]),
    "bl_amd_tpeak_gain_db": (C.c_double, [_P(SongLoud), C.c_int, C.c_double, _P(SongTpeak), C.c_double]),
    "bl_amd_tpeak_profile_ms": (C.c_double, [C.c_char_p, _P(C.c_int)]),
    "bl_amd_fprint_words": (C.c_int, [C.c_int]),
    "bl_amd_fprint_words_device": (C.c_int, [C.c_void_p, _P(C.c_int32), C.c_int, C.c_void_p, C.c_longlong, C.c_void_p]),
    "bl_amd_ctx_fprint_words_device": (C.c_int, [C.c_void_p, C.c_void_p, _P(C.c_int32), C.c_int, C.c_void_p,
                                                 C.c_longlong, C.c_void_p]),
    "bl_amd_fprint_words_host": (C.c_int, [C.c_void_p, _P(C.c_int32), C.c_int, C.c_void_p]),
    "bl_amd_fprint_match_device": (C.c_int, [C.c_void_p, _P(C.c_int32), C.c_int, C.c_void_p, _P(C.c_int32), C.c_int,
                                             C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                             C.c_void_p]),
    "bl_amd_ctx_fprint_match_device": (C.c_int, [C.c_void_p, C.c_void_p, _P(C.c_int32), C.c_int, C.c_void_p,
                                                 _P(C.c_int32), C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                 C.c_void_p, C.c_void_p, C.c_void_p]),
    "bl_amd_fprint_match_host": (C.c_int, [C.c_void_p, _P(C.c_int32), C.c_int, C.c_void_p, _P(C.c_int32), C.c_int,
                                           C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "bl_amd_fprint_shape": (None, [C.c_int, _P(C.c_int), _P(C.c_int), _P(C.c_int), _P(C.c_int)]),
    "bl_amd_fprint_ber": (C.c_double, [_P(FprintMatch)]),
    "bl_amd_fprint_offset_seconds": (C.c_double, [_P(FprintMatch), C.c_int]),
    "bl_amd_fprint_profile_ms": (C.c_double, [C.c_char_p, _P(C.c_int)]),
    "bl_amd_form_device": (C.c_int, [C.c_void_p, _P(C.c_int32), C.c_int, _P(FormParams), C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]),
    "bl_amd_ctx_form_device": (C.c_int, [C.c_void_p, C.c_void_p, _P(C.c_int32), C.c_int, _P(FormParams), C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]),
    "bl_amd_form_host": (C.c_int, [C.c_void_p, _P(C.c_int32), C.c_int, _P(FormParams), C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p]),
    "bl_amd_form_units": (C.c_int, [C.c_int, C.c_int]),
    "bl_amd_form_seconds": (C.c_double, [C.c_int, C.c_int, C.c_int]),
    "bl_amd_form_score": (C.c_double, [_P(SongForm)]),
    "bl_amd_form_shape": (None, [_P(C.c_int), _P(C.c_int)]),
    "bl_amd_form_profile_ms": (C.c_double, [C.c_char_p, _P(C.c_int)]),
    "bl_amd_cover_units_device": (C.c_int, [C.c_void_p, _P(C.c_int32), C.c_int, C.c_int, C.c_void_p, C.c_longlong,
                                            C.c_void_p]),
    "bl_amd_ctx_cover_units_device": (C.c_int, [C.c_void_p, C.c_void_p, _P(C.c_int32), C.c_int, C.c_int, C.c_void_p,
                                                C.c_longlong, C.c_void_p]),
    "bl_amd_cover_units_host": (C.c_int, [C.c_void_p, _P(C.c_int32), C.c_int, C.c_int, C.c_void_p]),
    "bl_amd_cover_match_device": (C.c_int, [C.c_void_p, _P(C.c_int32), C.c_int, C.c_void_p, _P(C.c_int32), C.c_int,
                                            C.c_void_p, C.c_int, _P(CoverParams), C.c_void_p, C.c_void_p]),
    "bl_amd_ctx_cover_match_device": (C.c_int, [C.c_void_p, C.c_void_p, _P(C.c_int32), C.c_int, C.c_void_p,
                                                _P(C.c_int32), C.c_int, C.c_void_p, C.c_int, _P(CoverParams),
                                                C.c_void_p, C.c_void_p]),
    "bl_amd_cover_match_host": (C.c_int, [C.c_void_p, _P(C.c_int32), C.c_int, C.c_void_p, _P(C.c_int32), C.c_int,
                                          C.c_void_p, C.c_int, _P(CoverParams), C.c_void_p]),
    "bl_amd_cover_score": (C.c_double, [_P(CoverMatch), C.c_int]),
    "bl_amd_cover_seconds": (C.c_double, [C.c_int, C.c_int, C.c_int]),
    "bl_amd_cover_tempo_ratio": (C.c_double, [_P(CoverMatch)]),
    "bl_amd_cover_shape": (None, [_P(C.c_int), _P(C.c_int)]),
    "bl_amd_cover_profile_ms": (C.c_double, [C.c_char_p, _P(C.c_int)]),
    "bl_amd_chords_device": (C.c_int, [C.c_void_p, _P(C.c_int32), C.c_int, C.c_longlong, _P(ChordsParams), C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    "bl_amd_ctx_chords_device": (C.c_int, [C.c_void_p, C.c_void_p, _P(C.c_int32), C.c_int, C.c_longlong,
                                           _P(ChordsParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bl_amd_chords_host": (C.c_int, [C.c_void_p, _P(C.c_int32), C.c_int, _P(ChordsParams), C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "bl_amd_chords_costs": (C.c_int, [C.c_int, C.c_int, _P(C.c_uint16)]),
    "bl_amd_chords_name": (C.c_char_p, [C.c_int]),
    "bl_amd_chords_segments": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]),
    "bl_amd_chords_shape": (None, [_P(C.c_int), _P(C.c_int), _P(C.c_int)]),
    "bl_amd_chords_profile_ms": (C.c_double, [C.c_char_p, _P(C.c_int)]),
    "bl_amd_tgram_frames": (C.c_int, [C.c_int, _P(TgramParams)]),
    "bl_amd_tgram_device": (C.c_int, [C.c_void_p, _P(C.c_int32), C.c_int, _P(TgramParams), C.c_void_p, C.c_void_p,
                                      C.c_longlong, C.c_void_p, C.c_void_p]),
    "bl_amd_ctx_tgram_device": (C.c_int, [C.c_void_p, C.c_void_p, _P(C.c_int32), C.c_int, _P(TgramParams), C.c_void_p,
                                          C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]),
    "bl_amd_tgram_host": (C.c_int, [C.c_void_p, _P(C.c_int32), C.c_int, _P(TgramParams), C.c_void_p, C.c_void_p,
                                    C.c_void_p]),
    "bl_amd_tgram_bpm": (C.c_double, [_P(TgramFrame), C.c_int]),
    "bl_amd_tgram_seconds": (C.c_double, [C.c_int, _P(TgramParams), C.c_int]),
    "bl_amd_tgram_steadiness": (C.c_double, [_P(SongTgram)]),
    "bl_amd_tgram_shape": (None, [_P(C.c_int), _P(C.c_int)]),
    "bl_amd_tgram_profile_ms": (C.c_double, [C.c_char_p, _P(C.c_int)]),
    "bl_amd_tbeats_device": (C.c_int, [C.c_void_p, _P(C.c_int32), _P(C.c_int32), C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                       C.c_int, _P(TbeatsParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "bl_amd_ctx_tbeats_device": (C.c_int, [C.c_void_p, C.c_void_p, _P(C.c_int32), _P(C.c_int32), C.c_int, C.c_void_p,
                                           C.c_int, C.c_void_p, C.c_int, _P(TbeatsParams), C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bl_amd_tbeats_host": (C.c_int, [C.c_void_p, _P(C.c_int32), _P(C.c_int32), C.c_int, C.c_void_p, C.c_void_p,
                                     _P(TbeatsParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bl_amd_tbeats_params_from_tgram": (C.c_int, [_P(TgramParams), C.c_int, C.c_int, _P(TbeatsParams)]),
    "bl_amd_tbeats_edge_bpm": (C.c_double, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "bl_amd_tbeats_shape": (None, [_P(C.c_int), _P(C.c_int)]),
    "bl_amd_tbeats_profile_ms": (C.c_double, [C.c_char_p, _P(C.c_int)]),
    "bl_amd_chroma_frames": (C.c_int, [C.c_int, C.c_int]),
    "bl_amd_chroma_batch_device": (C.c_int, [C.c_void_p, _P(SongDesc), C.c_int, C.c_void_p, C.c_void_p, C.c_longlong,
                                             C.c_void_p]),
    "bl_amd_ctx_chroma_batch_device": (C.c_int, [C.c_void_p, C.c_void_p, _P(SongDesc), C.c_int, C.c_void_p, C.c_void_p,
                                                 C.c_longlong, C.c_void_p]),
    "bl_amd_chroma_batch_host": (C.c_int, [_P(C.c_void_p), _P(C.c_int32), _P(C.c_int32), C.c_int, _P(SongChroma),
                                           _P(FrameChroma)]),
    "bl_amd_chroma_table": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bl_amd_chroma_key_name": (C.c_int, [C.c_int, C.c_char_p]),
    "bl_amd_mel_frames": (C.c_int, [C.c_int, C.c_int]),
    "bl_amd_mel_batch_device": (C.c_int, [C.c_void_p, _P(SongDesc), C.c_int, C.c_uint64, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_longlong, C.c_void_p]),
    "bl_amd_ctx_mel_batch_device": (C.c_int, [C.c_void_p, C.c_void_p, _P(SongDesc), C.c_int, C.c_uint64, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]),
    "bl_amd_mel_batch_host": (C.c_int, [_P(C.c_void_p), _P(C.c_int32), _P(C.c_int32), C.c_int, C.c_uint64, _P(SongMel),
                                        _P(FrameMel), _P(C.c_uint32)]),
    "bl_amd_mel_table": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "bl_amd_mel_mfcc": (C.c_double, [_P(SongMel), C.c_int, _P(C.c_double)]),
    "bl_amd_mel_flatness_db": (C.c_double, [_P(SongMel), _P(C.c_double)]),
    "bl_amd_selftest_ilog2": (C.c_int, [_P(C.c_uint64)]),
    "bl_amd_desc_range_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "bl_amd_desc_quantize_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, _P(C.c_uint16), C.c_void_p,
                                              C.c_void_p]),
    "bl_amd_desc_knn_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
    "bl_amd_desc_cross_knn_device": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                               C.c_void_p, C.c_void_p]),
    "bl_amd_ctx_desc_knn_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                             C.c_void_p, C.c_void_p]),
    "bl_amd_ctx_desc_cross_knn_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                   C.c_void_p, C.c_void_p, C.c_void_p]),
    "bl_amd_desc_build_host": (C.c_int, [_P(C.c_float), C.c_int, C.c_int, _P(C.c_uint16), C.c_int, _P(DescRange),
                                         _P(Desc)]),
    "bl_amd_desc_knn_host": (C.c_int, [_P(Desc), C.c_int, _P(Desc), C.c_int, C.c_int, _P(C.c_int32), _P(C.c_uint64)]),
    "bl_amd_desc_knn_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "bl_amd_desc_chain_device": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                           C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bl_amd_ctx_desc_chain_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                               C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bl_amd_desc_chain_host": (C.c_int, [_P(Desc), C.c_int, _P(C.c_int32), _P(Desc), C.c_int, C.c_int, _P(C.c_int32),
                                         C.c_int, _P(C.c_uint8), _P(C.c_int32), _P(C.c_uint64)]),
    "bl_amd_desc_chain_shape": (C.c_int, [C.c_int, C.c_int]),
    "bl_amd_desc_hmix_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, _P(HmixRule), C.c_void_p, C.c_void_p, C.c_int,
                                          C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bl_amd_ctx_desc_hmix_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, _P(HmixRule), C.c_void_p,
                                              C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p]),
    "bl_amd_desc_hmix_host": (C.c_int, [_P(Desc), _P(HmixAttr), C.c_int, _P(HmixRule), _P(C.c_int32), _P(Desc), C.c_int,
                                        C.c_int, _P(C.c_int32), C.c_int, _P(C.c_uint8), _P(C.c_int32), _P(C.c_uint64)]),
    "bl_amd_hmix_rule_camelot": (C.c_int, [_P(HmixRule), C.c_int, C.c_int]),
    "bl_amd_hmix_attrs": (C.c_int, [_P(SongRhythm), _P(SongChroma), C.c_int, C.c_int, _P(HmixAttr)]),
    "bl_amd_synth_pcm_device": (C.c_int, [C.c_void_p, _P(SongDesc), C.c_int, C.c_uint32, C.c_uint32, C.c_void_p]),
    "bl_amd_set_fir_mode": (C.c_int, [C.c_int]),
    "bl_amd_fir_mode": (C.c_int, []),
    "bl_amd_profile": (None, [C.c_int]),
    "bl_amd_profile_reset": (None, []),
    "bl_amd_profile_ms": (C.c_double, [C.c_char_p, _P(C.c_int)]),
    "bl_amd_last_energies": (C.c_longlong, [_P(C.c_float), C.c_longlong]),
    "bl_amd_last_freq_stats": (C.c_int, [C.c_int, _P(C.c_float), _P(C.c_longlong), _P(C.c_ulonglong), _P(C.c_uint),
                                         _P(C.c_int)]),
    "bl_amd_tail_from_envelope": (C.c_int, [_P(SongDesc), C.c_int, _P(C.c_double), C.c_longlong, _P(SongResult)]),
    "bl_amd_shutdown": (None, []),
}

_lib = None


def load():
    """Load libbliss_amd.so (once) and attach prototypes.  Raises ImportError if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(make -C bliss_amd/csrc). bliss_amd has no pure-Python or CPU fallback.")
    try:  # share torch's HIP runtime (same SONAME) when torch is in the process
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is optional for the C-ABI
        pass
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError -> missing export
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what):
    """Raise for the return code rc of the entry point `what` unless it is BL_OK."""
    if rc != BL_OK:
        raise RuntimeError(f"{what} failed with BL_UNEXPECTED ({rc}); see stderr")


def libc_free(ptr):
    """free() a block the library handed to the caller."""
    C.CDLL(None).free(C.cast(ptr, C.c_void_p))
