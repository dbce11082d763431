"""bliss_amd — MI355X-native implementation of the bliss per-song analysis hot path.

Python surface mirrors the reference's `bliss` package (ref python/bliss/__init__.py:7-12)
for the analysis path and adds the batch entry points of include/bliss_amd.h.
All computation happens in libbliss_amd.so (hand-written HIP kernels for gfx950).
"""
from . import _lib
from ._lib import (BL_CALM, BL_LOUD, BL_OK, BL_UNEXPECTED, BL_UNKNOWN, BlSong, EnvelopeResult,
                   ForceVector, FrameTimbre, SongDesc, SongLevels, SongResult, SongTimbre, load)
from . import distance, version
from .batch import (Context, DeviceCorpus, analyze_batch_host, analyze_batch_host_rate, analyze_batch_host_s32,
                    analyze_corpus_multi, analyze_corpus_multi_device, analyze_files, last_freq_stats, levels_batch_host,
                    resample_batch_device, resample_host, tail_from_envelope, timbre_batch_host)
from .queries import (chain, chain_device, cosine_matrix, distance_matrix, duplicate_groups, duplicate_groups_device, knn,
                      knn_cross, knn_cross_device, knn_device, mix, mix_device, playlist, playlist_vec, radius,
                      radius_cross, radius_cross_device, radius_device)
from .records import gapless_links, levels_db, levels_to_numpy, results_to_numpy, timbre_hz, timbre_to_numpy
from .bl_song import bl_song

__all__ = [
    # the C library, its structures and constants
    "_lib", "load", "BlSong", "ForceVector", "EnvelopeResult", "SongDesc", "SongResult", "SongLevels", "SongTimbre",
    "FrameTimbre", "BL_LOUD", "BL_CALM", "BL_UNKNOWN", "BL_UNEXPECTED", "BL_OK",
    # the reference's surface
    "bl_song", "distance", "version",
    # batch: resident corpora, contexts, host batches, rate conversion, diagnostics
    "DeviceCorpus", "Context", "analyze_batch_host", "analyze_batch_host_s32", "analyze_batch_host_rate", "analyze_files",
    "analyze_corpus_multi", "analyze_corpus_multi_device", "levels_batch_host", "timbre_batch_host", "resample_host",
    "resample_batch_device", "last_freq_stats", "tail_from_envelope",
    # records
    "results_to_numpy", "levels_to_numpy", "timbre_to_numpy", "levels_db", "timbre_hz", "gapless_links",
    # queries
    "distance_matrix", "cosine_matrix", "playlist", "playlist_vec", "knn", "knn_device", "knn_cross", "knn_cross_device",
    "chain", "chain_device", "mix", "mix_device", "radius", "radius_device", "radius_cross", "radius_cross_device",
    "duplicate_groups", "duplicate_groups_device"]


def __getattr__(name):
    """`bliss_amd.lib`: the loaded C library, the counterpart of the reference's `bliss.lib`
    (ref python/bliss/__init__.py:5) — e.g. `bliss_amd.lib.bl_version()`.  Loaded on first use."""
    if name == "lib":
        return load()
    raise AttributeError(f"module 'bliss_amd' has no attribute {name!r}")
