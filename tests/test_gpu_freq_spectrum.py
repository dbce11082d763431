"""The frequency pass where its claim is made: every bin of the summed power spectrum, and the raw statistics that ride
along with it, bit for bit — not only the one f32 per song that `frequency` is (tests/test_gpu_parity.py), in which
most one-ulp errors of a bin vanish and which never reads bins 1, 3, 5, 7, 9 and 235..255 except as peak candidates.

Read through bl_amd_last_freq_stats from the workspace, compared with tests/freq_reference.py (a per-bin numpy
restatement of the oracle, proved in tests/test_freq_reference_host.py) on stereo songs of every n_frames in 5..136 and
mono songs of every n_frames in 10..136: every remainder of the 64-frame iteration of k_freq_scan and of the 32-frame
one of k_freq_frames, one to five iterations, every number of live frames in the last iteration on every wave, idle
waves and lane groups, odd and even counts, and a different number of samples behind the last frame for every song.
All comparisons are of integers or of f32 bit patterns; there is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import bliss_amd
from bliss_amd import _lib
from tests import freq_reference as fr
from tests.test_gpu_parity import check_song

pytestmark = pytest.mark.gpu

ALL = _lib.BL_AMD_PART_SPECTRUM | _lib.BL_AMD_PART_SUMS | _lib.BL_AMD_PART_HIST


def where(sg, i, path):
    nf = sg["n_frames"]
    return (f"song {i}: {sg['channels']} ch, n_frames {nf} (mod 64: {nf % 64}, mod 32: {nf % 32}, mod 8: {nf % 8}, "
            f"mod 2: {nf % 2}), {sg['extra']} samples behind, {path}")


def assert_spectrum(got, want, sg, i, path):
    g, w = got.view(np.uint32)[1:], want.view(np.uint32)[1:]   # bin 0 is unspecified
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (f"{where(sg, i, path)}: {bad.size} bins differ, first bin {bad[0] + 1}: got {g[bad[0]]:#010x} "
                           f"({float(got[bad[0] + 1])!r}), want {w[bad[0]]:#010x} ({float(want[bad[0] + 1])!r}); "
                           f"bins {[int(b) + 1 for b in bad[:12]]}")


def assert_statistics(st, k, want, sg, i, path):
    _, total, sumsq, hist = want
    assert int(st["sum"][k]) == total, f"{where(sg, i, path)}: sum {int(st['sum'][k]):#x}, want {total:#x}"
    assert int(st["sumsq"][k]) == sumsq, f"{where(sg, i, path)}: sumsq {int(st['sumsq'][k]):#x}, want {sumsq:#x}"
    bad = np.flatnonzero(st["hist"][k].astype(np.int64) != hist)
    assert bad.size == 0, (f"{where(sg, i, path)}: {bad.size} histogram counts differ, first at value {bad[0] - 2048}: "
                           f"got {int(st['hist'][k][bad[0]]):#x}, want {int(hist[bad[0]]):#x}")


def run_batch(songs):
    corpus = bliss_amd.DeviceCorpus([s["pcm"].size for s in songs], [s["channels"] for s in songs],
                                    [s["duration"] for s in songs])
    for i, s in enumerate(songs):
        corpus.upload(i, np.array(s["pcm"]))   # a writable copy: the shared material is read-only
    corpus.analyze()
    return corpus.fetch(), bliss_amd.last_freq_stats()


@pytest.fixture(scope="module")
def songs(oracle):
    return fr.song_set(oracle)


@pytest.fixture(scope="module")
def reference(oracle):
    return fr.reference(oracle)


@pytest.fixture(scope="module")
def fused(gpu_lib, songs):
    """the whole set in one batch of mixed lengths: k_freq_scan, records length-sorted inside"""
    return run_batch(songs)


def test_fused_pass_spectrum_bits(fused, songs, reference):
    _, st = fused
    assert st["n_songs"] == len(songs) == 259 and st["parts"] == ALL
    for i, (sg, want) in enumerate(zip(songs, reference)):
        assert_spectrum(st["spectrum"][i], want[0], sg, i, "k_freq_scan")


def test_fused_pass_statistics(fused, songs, reference):
    _, st = fused
    for i, (sg, want) in enumerate(zip(songs, reference)):
        assert_statistics(st, i, want, sg, i, "k_freq_scan")


def test_fused_pass_records_still_match_the_oracle(fused, songs, oracle, reference):
    got, _ = fused
    assert np.all(got["status"] == 0)
    assert [int(x) for x in got["n_frames"]] == [s["n_frames"] for s in songs]
    for i in range(0, len(songs), 20):
        sg = songs[i]
        check_song(got[i], oracle.analyze(sg["pcm"], sg["channels"], sg["duration"]), where(sg, i, "batch"))
    for i, (sg, want) in enumerate(zip(songs, reference)):   # and the finish, from the reference's spectrum
        freq, peak = fr.finish(want[0])
        assert np.float32(got[i]["frequency"]).view(np.uint32) == freq.view(np.uint32), where(sg, i, "k_freq_finish")
        assert np.float32(got[i]["freq_peak"]).view(np.uint32) == peak.view(np.uint32), where(sg, i, "k_freq_finish")


def test_equal_lengths_batch_and_the_diagnostics_arguments(gpu_lib, oracle):
    """a batch the runtime does not sort; then the diagnostic with some and with none of its outputs"""
    songs, want = fr.equal_length_set(oracle), fr.reference(oracle, "equal")
    got, st = run_batch(songs)
    assert st["n_songs"] == len(songs) and st["parts"] == ALL and np.all(got["status"] == 0)
    for i, sg in enumerate(songs):
        assert_spectrum(st["spectrum"][i], want[i][0], sg, i, "k_freq_scan, equal lengths")
        assert_statistics(st, i, want[i], sg, i, "k_freq_scan, equal lengths")
    n = len(songs)
    assert gpu_lib.bl_amd_last_freq_stats(0, None, None, None, None, None) == n
    spectrum = np.full((n, 256), np.float32(-1))
    total = np.full(n, -1, dtype=np.int64)
    parts = C.c_int(-1)
    assert gpu_lib.bl_amd_last_freq_stats(3, spectrum.ctypes.data_as(C.POINTER(C.c_float)),
                                          total.ctypes.data_as(C.POINTER(C.c_longlong)), None, None, C.byref(parts)) == n
    assert parts.value == ALL
    assert np.array_equal(spectrum[:3].view(np.uint32), st["spectrum"][:3].view(np.uint32)) and np.all(spectrum[3:] == -1)
    assert list(total[:3]) == [w[1] for w in want[:3]] and np.all(total[3:] == -1)


def one_per_remainder(songs):
    """(song index, song) for every n_frames mod 32 of both channel counts, spread over the iteration counts"""
    picks = []
    for ch in (2, 1):
        for r in range(32):
            mine = [i for i, s in enumerate(songs) if s["channels"] == ch and s["n_frames"] % 32 == r]
            picks.append(mine[r % len(mine)])
    assert len(picks) == 64 and len(set(picks)) == 64
    return [(i, songs[i]) for i in picks]


def as_song(sg):
    song = _lib.BlSong()
    song.sample_array = sg["pcm"].ctypes.data
    song.channels, song.nSamples, song.sample_rate = sg["channels"], sg["pcm"].size, fr.RATE
    song.nb_bytes_per_sample, song.duration = 2, sg["duration"]
    return song


def test_frequency_kernel_alone(gpu_lib, fused, songs, reference):
    """bl_frequency_sort runs k_freq_frames (four waves, 32 frames per iteration): the same bits as the reference and
    as the fused pass, for every remainder of its iteration.  Consecutive calls are on different songs, so nothing
    left over from the call before can pass."""
    _, batch = fused
    for i, sg in one_per_remainder(songs):
        song = as_song(sg)
        frq = gpu_lib.bl_frequency_sort(C.byref(song))
        st = bliss_amd.last_freq_stats()
        path = "bl_frequency_sort (k_freq_frames)"
        # the frequency analysis reads no statistics: no statistics pass runs, and the diagnostic claims the spectrum alone
        assert st["n_songs"] == 1 and st["parts"] == _lib.BL_AMD_PART_SPECTRUM, where(sg, i, path)
        assert_spectrum(st["spectrum"][0], reference[i][0], sg, i, path)
        assert_spectrum(st["spectrum"][0], batch["spectrum"][i], sg, i, path + " against k_freq_scan")
        assert np.float32(frq).view(np.uint32) == fr.finish(reference[i][0])[0].view(np.uint32), where(sg, i, path)


def test_statistics_kernel_alone(gpu_lib, fused, songs, reference):
    """bl_amplitude_sort runs k_pcm_scan: the same integers as numpy and as the fused pass; no frequency pass runs, and
    the diagnostic does not call the spectrum written"""
    _, batch = fused
    for i, sg in one_per_remainder(songs):
        song = as_song(sg)
        amp = gpu_lib.bl_amplitude_sort(C.byref(song))
        st = bliss_amd.last_freq_stats()
        path = "bl_amplitude_sort (k_pcm_scan)"
        assert np.isfinite(amp), where(sg, i, path)
        assert st["n_songs"] == 1 and st["parts"] == _lib.BL_AMD_PART_SUMS | _lib.BL_AMD_PART_HIST, where(sg, i, path)
        assert_statistics(st, 0, reference[i], sg, i, path)
        assert int(st["sum"][0]) == int(batch["sum"][i]) and int(st["sumsq"][0]) == int(batch["sumsq"][i])
        assert np.array_equal(st["hist"][0], batch["hist"][i]), where(sg, i, path + " against k_freq_scan")
