"""The derived statistics where they are made: k_pcm_scan's steady-state loop, k_trim, k_song_prep, k_variance_wrap and
its finish, k_amp_finish, k_force and the stand-alone bl_mean / bl_variance, held to tests/stats_reference.py (numpy and
Python integers by the reference's definitions, proved in tests/test_stats_reference_host.py) and to the oracle.  Every
comparison is of integers or of f32 / f64 bit patterns; the only bound is the one tests/test_gpu_windows.py already
applies to the window energies of FIR modes 1 and 2, through its own helpers.

1. Long songs through the single-song entry points: the only launches in which a lane of k_pcm_scan takes two vectors
   together are those of one song of more than 8 * n_cu * 2048 samples (tests/stats_reference.py::scan_geometry).
   Among them the two songs with more than 2^24 equal samples.
2. The designed songs (wrapped sums, truncated quotients, means on the closed form's limit, negative and huge
   variances, variance 0, histograms at the edges of the integral window, one and two samples, force 0) through the
   device batch, the host batch and the single analyzers.
3. The songs with |mean| > 13 571, negative variances among them, through the window kernel in the three FIR modes.
4. bl_variance with means that are not the song's."""
import ctypes as C

import numpy as np
import pytest

import bliss_amd
from bliss_amd import _lib
from tests import stats_reference as sr
from tests.test_gpu_parity import check_song
from tests.test_gpu_windows import _check_exact, _check_mode0, _check_modes12, _reference, _run
from tests.test_stats_reference_host import CALLER_SONGS, caller_means

pytestmark = pytest.mark.gpu

STATS_ONLY = _lib.BL_AMD_PART_SUMS | _lib.BL_AMD_PART_HIST


def _i16p(pcm):
    return pcm.ctypes.data_as(C.POINTER(C.c_int16))


def as_song(pcm, channels, duration):
    song = _lib.BlSong()
    song.sample_array = pcm.ctypes.data
    song.channels, song.nSamples, song.sample_rate = channels, pcm.size, sr.RATE
    song.nb_bytes_per_sample, song.duration = 2, duration
    return song


def _bytes(rec):
    """the bytes of every field of a record, NaN payloads included; the padding in front of atk_sum is nobody's"""
    return b"".join(np.ascontiguousarray(rec[k]).view(np.uint8).tobytes() for k in rec.dtype.names)


def _f32(x):
    return np.float32(x).view(np.uint32)


@pytest.fixture(scope="module")
def n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- 1. the single-song path on long songs ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def long_songs(n_cu):
    return sr.long_songs(n_cu)


def test_the_long_songs_reach_every_class_of_the_scan_loop(oracle, long_songs, n_cu):
    reached = {name: sr.scan_geometry(s.size, 1, n_cu) for name, s in long_songs.items()}
    for name, got in reached.items():
        print(f"{name:10s} {long_songs[name].size:9d} samples on {n_cu} CUs: {sorted(got)}")
    loop = set().union(*reached.values())
    # a song of more than one stride leaves no lane idle: that class, and the tails of 4 and 6, are the designed songs'
    designed = set().union(*[sr.scan_geometry(s["pcm"].size, 1, n_cu) for s in sr.song_set(oracle)])
    assert loop >= sr.PAIRED | {"single_only"}, sorted((sr.PAIRED | {"single_only"}) - loop)
    assert not designed & sr.PAIRED, sorted(designed)
    assert loop | designed == sr.ALL_CLASSES, sorted(sr.ALL_CLASSES - (loop | designed))


@pytest.mark.parametrize("name", ("1.5g", "2g", "2g+1", "2.5g", "3.5g", "sat_value", "sat_zero"))
def test_single_song_path_on_a_long_song(gpu_lib, long_songs, name):
    pcm = long_songs[name]
    exp = sr.expected(pcm)
    n = pcm.size
    song = as_song(pcm, 1, sr.duration_of(n, 1))
    amp = np.float32(gpu_lib.bl_amplitude_sort(C.byref(song)))
    st = bliss_amd.last_freq_stats()
    assert st["n_songs"] == 1 and st["parts"] == STATS_ONLY, (name, st["n_songs"], st["parts"])
    assert int(st["sum"][0]) == exp["sum"], (name, "sum", int(st["sum"][0]), exp["sum"])
    assert int(st["sumsq"][0]) == exp["sumsq"], (name, "sumsq", int(st["sumsq"][0]), exp["sumsq"])
    bad = np.flatnonzero(st["hist"][0].astype(np.int64) != exp["hist"])
    assert bad.size == 0, (name, f"{bad.size} histogram counts differ, first at value {bad[0] - 2048}: got "
                                 f"{int(st['hist'][0][bad[0]])}, want {int(exp['hist'][bad[0]])}")
    # the entry point returns the amplitude alone; the integral is a step on the way to it
    assert sr.same_bits(amp, exp["amplitude"]), (name, "amplitude", float(amp), float(exp["amplitude"]))
    own = sr.amplitude(st["hist"][0], exp["start"], exp["end"], n)[1]   # k_amp_finish alone, from the GPU's counts
    assert sr.same_bits(amp, own), (name, "amplitude from the GPU's own counts", float(amp), float(own))
    mean = gpu_lib.bl_mean(_i16p(pcm), n)
    assert mean == exp["mean"], (name, "bl_mean", mean, exp["mean"])
    var = gpu_lib.bl_variance(_i16p(pcm), n, mean)
    assert var == exp["variance"], (name, "bl_variance", var, exp["variance"])


def test_envelope_of_a_long_song_has_the_oracles_bits(gpu_lib, oracle, long_songs):
    pcm = long_songs["2.5g"]
    duration = sr.duration_of(pcm.size, 1)
    want, _ = oracle.envelope(pcm, duration)
    env = _lib.EnvelopeResult()
    song = as_song(pcm, 1, duration)
    gpu_lib.bl_envelope_sort(C.byref(song), C.byref(env))
    assert np.isfinite(want["tempo"]) and np.isfinite(want["attack"])
    assert _f32(env.tempo) == _f32(want["tempo"]), (env.tempo, want["tempo"])
    assert _f32(env.attack) == _f32(want["attack"]), (env.attack, want["attack"])


# ---- 2. the designed songs by three routes ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def songs(oracle):
    return sr.song_set(oracle)


@pytest.fixture(scope="module")
def ref(oracle):
    return sr.reference(oracle)


def _device_batch(songs):
    corpus = bliss_amd.DeviceCorpus([s["pcm"].size for s in songs], [s["channels"] for s in songs],
                                    [s["duration"] for s in songs])
    for i, s in enumerate(songs):
        corpus.upload(i, np.array(s["pcm"]))   # a writable copy: the shared material is read-only
    corpus.analyze()
    return corpus.fetch()


@pytest.fixture(scope="module")
def device_batch(gpu_lib, songs):
    """one batch of mixed lengths, which the runtime sorts: k_freq_scan, songs that take the wrap pass between songs
    that do not"""
    lengths = [s["pcm"].size for s in songs]
    assert lengths != sorted(lengths, reverse=True)
    return _device_batch(songs)


@pytest.fixture(scope="module")
def host_batch(gpu_lib, songs):
    return bliss_amd.analyze_batch_host([s["pcm"] for s in songs], [s["channels"] for s in songs],
                                        [s["duration"] for s in songs])


def _check_against_the_reference(rec, exp, tag):
    for k in ("start", "end", "mean", "variance", "status"):
        assert int(rec[k]) == exp[k], (tag, k, int(rec[k]), exp[k])
    for k in ("hist_integral", "amplitude"):
        assert sr.same_bits(rec[k], exp[k]), (tag, k, float(rec[k]), float(exp[k]))


def _check_record(rec, sg, exp, full, tag):
    _check_against_the_reference(rec, exp, tag)
    if sg["var0"]:
        assert int(rec["status"]) == _lib.BL_UNEXPECTED, tag
    elif sg["one_sample"]:
        assert np.isnan(rec["amplitude"]) and np.isnan(rec["force"]) and int(rec["calm_or_loud"]) == _lib.BL_UNKNOWN, tag
        assert int(rec["status"]) == 0, tag
    else:
        check_song(rec, full, tag)


@pytest.mark.parametrize("route", ("device batch", "host batch"))
def test_designed_songs_in_a_batch(device_batch, host_batch, songs, ref, route):
    got = device_batch if route == "device batch" else host_batch
    assert len(got) == len(songs)
    wrap = [s["name"] for s in songs if abs(ref[s["name"]][0]["mean"]) > sr.CLOSED_FORM_LIMIT]
    at = [i for i, s in enumerate(songs) if s["name"] in wrap]
    assert len(wrap) >= 4 and any(b - a > 1 for a, b in zip(at, at[1:]))   # the wrap pass, between songs without it
    for i, sg in enumerate(songs):
        exp, full = ref[sg["name"]]
        _check_record(got[i], sg, exp, full, f"{route}: {sg['name']}")
    zero = got[[s["name"] for s in songs].index("zero_force")]
    assert _f32(zero["force"]) == 0 and int(zero["calm_or_loud"]) == _lib.BL_UNKNOWN   # +0.0, neither LOUD nor CALM


def test_the_routes_give_identical_bytes(gpu_lib, device_batch, host_batch, songs, ref):
    for i, sg in enumerate(songs):
        name = sg["name"]
        assert _bytes(device_batch[i]) == _bytes(host_batch[i]), (name, device_batch[i], host_batch[i])
        rec, pcm = device_batch[i], sg["pcm"]
        song = as_song(pcm, sg["channels"], sg["duration"])
        amp = gpu_lib.bl_amplitude_sort(C.byref(song))
        st = bliss_amd.last_freq_stats()
        exp = ref[name][0]
        assert st["parts"] == STATS_ONLY and int(st["sum"][0]) == exp["sum"] and int(st["sumsq"][0]) == exp["sumsq"], name
        assert np.array_equal(st["hist"][0].astype(np.int64), exp["hist"]), (name, "k_pcm_scan's counts")
        env = _lib.EnvelopeResult()
        gpu_lib.bl_envelope_sort(C.byref(song), C.byref(env))
        for k, v in (("amplitude", amp), ("tempo", env.tempo), ("attack", env.attack)):
            assert sr.same_bits(v, rec[k]), (name, k, "single analyzer", float(v), "batch", float(rec[k]))
        mean = gpu_lib.bl_mean(_i16p(pcm), pcm.size)
        assert mean == int(rec["mean"]) == exp["mean"], (name, "bl_mean", mean, exp["mean"])
        var = gpu_lib.bl_variance(_i16p(pcm), pcm.size, mean)
        assert var == int(rec["variance"]) == exp["variance"], (name, "bl_variance", var, exp["variance"])


def test_a_flagged_song_alone_gives_the_bytes_of_the_batch(gpu_lib, device_batch, songs, ref):
    """the songs that take the wrap pass and the songs the analysis refuses, each as a batch of its own"""
    flagged = [i for i, s in enumerate(songs)
               if abs(ref[s["name"]][0]["mean"]) > sr.CLOSED_FORM_LIMIT or s["var0"] or s["one_sample"]]
    assert len(flagged) >= 10
    for i in flagged:
        alone = _device_batch([songs[i]])[0]
        assert _bytes(alone) == _bytes(device_batch[i]), (songs[i]["name"], alone, device_batch[i])


# ---- 3. negative and huge variances through the window kernel -----------------------------------------------------

@pytest.fixture(scope="module")
def beyond(oracle, songs, ref):
    """name -> (pcm, channels) of the designed songs with |mean| > 13 571"""
    out = {s["name"]: (s["pcm"], s["channels"]) for s in songs if abs(ref[s["name"]][0]["mean"]) > sr.CLOSED_FORM_LIMIT}
    assert sum(ref[n][0]["variance"] < 0 for n in out) >= 2 and "large_variance" in out
    return out


@pytest.fixture(scope="module")
def beyond_runs(gpu_lib, beyond):
    return _run(gpu_lib, beyond, list(beyond))


@pytest.fixture(scope="module")
def beyond_ref(oracle, beyond, ref):
    out = _reference(oracle, beyond)
    for name, (full, _, _) in out.items():
        assert (full["mean"], full["variance"]) == (ref[name][0]["mean"], ref[name][0]["variance"]), name
    return out


def test_fir_mode0_energies_are_the_oracles_bits_under_any_variance(beyond_runs, beyond_ref):
    _check_mode0(beyond_runs, beyond_ref, "beyond")


def test_fir_modes_1_and_2_stay_mode0s_under_any_variance(beyond_runs):
    moved = _check_modes12(beyond_runs, "beyond")
    for mode in (1, 2):
        print(f"mode {mode}: {len(moved[mode])} energies differ from mode 0's (by one ulp): {moved[mode]}")
        assert len(moved[mode]) <= 2, (mode, moved[mode])


def test_every_energy_lies_within_the_derived_bound_under_any_variance(beyond_runs, beyond_ref):
    _check_exact(beyond_runs, beyond_ref, "beyond")


# ---- 4. bl_variance with a caller's mean --------------------------------------------------------------------------

def test_bl_variance_with_a_callers_mean(gpu_lib, songs, ref):
    by_name = {s["name"]: s for s in songs}
    for name in CALLER_SONGS:
        pcm = by_name[name]["pcm"]
        for m in caller_means(ref[name][0]["mean"]):
            got = gpu_lib.bl_variance(_i16p(pcm), pcm.size, m)
            assert got == sr.variance_wrapped(pcm, m), (name, m, got, sr.variance_wrapped(pcm, m))
