"""bliss_amd — MI355X-native implementation of the bliss per-song analysis hot path.

Python surface mirrors the reference's `bliss` package (ref python/bliss/__init__.py:7-12)
for the analysis path and adds the batch entry points of include/bliss_amd.h.
All computation happens in libbliss_amd.so (hand-written HIP kernels for gfx950).
"""
from . import _lib
from ._lib import (BL_CALM, BL_LOUD, BL_OK, BL_UNEXPECTED, BL_UNKNOWN, BlSong, EnvelopeResult,
                   ForceVector, FrameTimbre, SongDesc, SongLevels, SongResult, SongTimbre, load)
from . import distance, version
from .batch import (Context, DeviceCorpus, analyze_batch_host, analyze_files, analyze_batch_host_rate, analyze_batch_host_s32,
                    analyze_corpus_multi, analyze_corpus_multi_device, chain, chain_device, mix, mix_device, cosine_matrix, distance_matrix, knn, knn_device,
                    playlist, knn_cross, knn_cross_device, playlist_vec, radius_cross, radius_cross_device,
                    duplicate_groups, duplicate_groups_device, radius, radius_device,
                    resample_batch_device,
                    resample_host, results_to_numpy,
                    gapless_links, levels_batch_host, levels_db, levels_to_numpy, last_freq_stats, tail_from_envelope,
                    timbre_batch_host, timbre_hz, timbre_to_numpy)
from .bl_song import bl_song

__all__ = ["_lib", "load", "BlSong", "ForceVector", "EnvelopeResult", "SongDesc", "SongResult",
           "BL_LOUD", "BL_CALM", "BL_UNKNOWN", "BL_UNEXPECTED", "BL_OK", "DeviceCorpus",
           "analyze_batch_host", "analyze_files", "analyze_batch_host_rate", "analyze_batch_host_s32", "analyze_corpus_multi", "analyze_corpus_multi_device", "Context",
           "distance_matrix", "cosine_matrix", "results_to_numpy", "playlist", "knn", "knn_device", "chain", "chain_device", "mix", "mix_device",
           "radius", "radius_device", "knn_cross", "knn_cross_device", "radius_cross", "radius_cross_device", "playlist_vec",
           "duplicate_groups", "duplicate_groups_device",
           "SongLevels", "levels_batch_host", "levels_to_numpy", "levels_db", "gapless_links",
           "SongTimbre", "FrameTimbre", "timbre_batch_host", "timbre_to_numpy", "timbre_hz",
           "last_freq_stats", "tail_from_envelope", "resample_host", "resample_batch_device", "bl_song", "distance", "version"]


def __getattr__(name):
    """`bliss_amd.lib`: the loaded C library, the counterpart of the reference's `bliss.lib`
    (ref python/bliss/__init__.py:5) — e.g. `bliss_amd.lib.bl_version()`.  Loaded on first use."""
    if name == "lib":
        return load()
    raise AttributeError(f"module 'bliss_amd' has no attribute {name!r}")
