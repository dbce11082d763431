"""tests/stats_reference.py is what tests/test_gpu_stats.py holds the statistics kernels to, so it is proved here,
without a device: on every designed song and on the two saturation songs its mean, variance, trim, histogram integral,
amplitude and force are the oracle's, integers exact and floats bit for bit.  Then the errors a kernel can make are made
in the reference itself, and each of them must change the result of at least one song, named here: a floor for C's
truncation, a sum or a square that does not wrap, the closed form of the variance used beyond its limit, a histogram
that does not saturate or saturates before the silence is taken off, a smoothing loop pruned one bin or three too far,
and >= for > in calm_or_loud.  Last, the facts the GPU test relies on are checked where no device is needed: which
classes of k_pcm_scan's loop which songs reach, and that the designed songs are what their names say.  What each
mutation changes is printed (pytest -s)."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import freq_reference as fr
from tests import stats_reference as sr
from tests.oracle_py import OrcResult

N_CU = 256   # the compute units of an MI355X; the GPU test reads the device's
CALLER_MEANS = (0, 13571, 13572, -20000, 2 ** 20, -2 ** 30)   # and the song's own mean and mean +- 1
CALLER_SONGS = ("wrap_up", "floor", "large_variance", "mean+13572", "zeros_inside")


def caller_means(mean):
    return (mean, mean + 1, mean - 1) + CALLER_MEANS


def oracle_amplitude(oracle, pcm):
    r = OrcResult()
    pcm = np.ascontiguousarray(pcm)
    amp = oracle.lib.orc_amplitude(pcm.ctypes.data_as(C.POINTER(C.c_int16)), pcm.size, C.byref(r))
    return r.start, r.end, np.float32(r.hist_integral), np.float32(amp)


@pytest.fixture(scope="module")
def songs(oracle):
    return {s["name"]: s for s in sr.song_set(oracle)}


@pytest.fixture(scope="module")
def ref(oracle):
    return sr.reference(oracle)


@pytest.fixture(scope="module")
def saturation(oracle):
    """name -> (pcm, expected, the oracle's start, end, integral, amplitude)"""
    def one(item):
        return item[0], (item[1], sr.expected(item[1]), oracle_amplitude(oracle, item[1]))
    with ThreadPoolExecutor(2) as pool:
        return dict(pool.map(one, sr.saturation_songs().items()))


def test_the_reference_is_the_oracle_on_every_designed_song(oracle, songs, ref):
    for name, sg in songs.items():
        exp, full = ref[name]
        pcm = sg["pcm"]
        assert exp["mean"] == oracle.mean(pcm) == full["mean"], (name, exp["mean"], full["mean"])
        assert exp["variance"] == oracle.variance(pcm, exp["mean"]) == full["variance"], (name, exp["variance"], full["variance"])
        assert (exp["start"], exp["end"]) == (full["start"], full["end"]), name
        assert sr.same_bits(exp["hist_integral"], full["hist_integral"]), (name, float(exp["hist_integral"]), full["hist_integral"])
        assert sr.same_bits(exp["amplitude"], full["amplitude"]), (name, float(exp["amplitude"]), full["amplitude"])
        force, col = sr.force_of(full["tempo"], full["amplitude"], full["frequency"], full["attack"])
        assert sr.same_bits(force, full["force"]) and col == full["calm_or_loud"], (name, float(force), full["force"], col)
        # the other two statements of the same integral: tests/freq_reference.py's, and the pruned loop of the kernel
        n = pcm.size
        assert sr.same_bits(fr.hist_integral(exp["hist"], exp["start"], exp["end"], n), exp["hist_integral"]), name
        assert sr.same_bits(sr.amplitude(exp["hist"], exp["start"], exp["end"], n, reach_short=0)[0], exp["hist_integral"]), name
        if abs(exp["mean"]) <= sr.CLOSED_FORM_LIMIT:
            assert fr.mean_variance(exp["sum"], exp["sumsq"], n) == (exp["mean"], exp["variance"]), name


def test_the_reference_is_the_oracle_on_the_saturation_songs(oracle, saturation):
    for name, (pcm, exp, (start, end, integral, amp)) in saturation.items():
        assert exp["mean"] == oracle.mean(pcm) and exp["variance"] == oracle.variance(pcm, exp["mean"]), name
        assert (exp["start"], exp["end"]) == (start, end), name
        assert np.isfinite(integral) and sr.same_bits(exp["hist_integral"], integral), (name, float(exp["hist_integral"]), float(integral))
        assert sr.same_bits(exp["amplitude"], amp), (name, float(exp["amplitude"]), float(amp))
        assert sr.same_bits(fr.hist_integral(exp["hist"], start, end, pcm.size), integral), name
        assert sr.same_bits(sr.amplitude(exp["hist"], start, end, pcm.size, reach_short=0)[0], integral), name
    raw = {name: int(s[1]["hist"].max()) for name, s in saturation.items()}
    assert raw["sat_value"] == 2 ** 24 + 5000 and raw["sat_zero"] == 2 ** 24 - 10 + 5000, raw
    exp = saturation["sat_zero"][1]
    assert exp["start"] + (saturation["sat_zero"][0].size - 1 - exp["end"]) == 5000


def test_variance_with_a_callers_mean(oracle, songs, ref):
    for name in CALLER_SONGS:
        pcm = songs[name]["pcm"]
        for m in caller_means(ref[name][0]["mean"]):
            assert sr.variance_wrapped(pcm, m) == oracle.variance(pcm, m), (name, m)


def test_every_mutation_changes_a_named_song(oracle, songs, ref, saturation):
    exp = {name: e for name, (e, _) in ref.items()}
    full = {name: f for name, (_, f) in ref.items()}
    stats = dict(exp)
    stats.update({name: s[1] for name, s in saturation.items()})
    pcm_of = {name: s["pcm"] for name, s in songs.items()}

    def integral_changed(names, **switch):
        hit = []
        for name in names:
            e = stats[name]
            n = pcm_of[name].size if name in pcm_of else saturation[name][0].size
            got = sr.amplitude(e["hist"], e["start"], e["end"], n, **switch)[0]
            if not sr.same_bits(got, e["hist_integral"]):
                hit.append(name)
        return hit

    def own_variance(name, **switch):
        return sr.variance_wrapped(pcm_of[name], exp[name]["mean"], **switch)

    everything = list(songs) + list(saturation)
    # mutation -> (the songs whose result it changes, the songs that must be among them)
    found = {
        "floor instead of truncation in the mean":
            ([n for n in songs if sr.mean_wrapped(pcm_of[n], floor=True) != exp[n]["mean"]],
             {"wrap_up", "quotient_-0", "quotient_-1-", "wrapped_mean-13571", "mean-13572"}),
        "an unwrapped sum":
            ([n for n in songs if sr.mean_wrapped(pcm_of[n], wrap=False) != exp[n]["mean"]],
             {"wrap_up", "wrap_down", "wrap_twice", "quotient_-1", "wrapped_mean+13572", "floor", "ceiling"}),
        "floor instead of truncation in the variance":
            ([n for n in songs if own_variance(n, floor=True) != exp[n]["variance"]], {"floor_noisy"}),
        "an unwrapped square":
            ([n for n in songs if own_variance(n, wrap=False) != exp[n]["variance"]], {"floor", "floor_noisy", "ceiling"}),
        "the closed form used beyond 13 571":
            ([n for n in songs if own_variance(n, closed_form=True) != exp[n]["variance"]], {"floor", "floor_noisy", "ceiling"}),
        "saturate=False": (integral_changed(everything, saturate=False), {"sat_value"}),
        "saturate_before_trim=True": (integral_changed(everything, saturate_before_trim=True), {"sat_zero"}),
        "reach_short=1": (integral_changed(everything, reach_short=1), {"edge_spikes", "constant-1002", "constant+1000"}),
        "reach_short=3": (integral_changed(everything, reach_short=3), {"edge_spikes", "constant-1002", "constant+1000"}),
        ">= for > in calm_or_loud":
            ([n for n in songs if sr.force_of(full[n]["tempo"], full[n]["amplitude"], full[n]["frequency"],
                                              full[n]["attack"], ge=True)[1] != full[n]["calm_or_loud"]], {"zero_force"}),
    }
    print("\nerror made in the reference: the songs whose result changes")
    for name, (hit, _) in found.items():
        print(f"  {name:44s} {len(hit):2d}: {', '.join(hit)}")
    for name, (hit, must) in found.items():
        assert must <= set(hit), (name, "not detected by", sorted(must - set(hit)))
    # what the mutations of the smoothing do NOT change: ordinary material, which is why the songs above exist
    assert "zeros_inside" not in found["reach_short=3"][0] and "sat_zero" not in found["saturate=False"][0]


def test_which_songs_reach_which_class_of_the_scan_loop(oracle, songs):
    """today's gap as a fact of the geometry: analysed one at a time, no designed song makes a lane of k_pcm_scan take
    two vectors together; the long songs reach every class of the loop, and with the designed songs every tail"""
    designed = {name: sr.scan_geometry(s["pcm"].size, 1, N_CU) for name, s in songs.items()}
    for name, got in designed.items():
        assert not got & sr.PAIRED and "single_only" in got, (name, sorted(got))
    long_ = {name: sr.scan_geometry(s.size, 1, N_CU) for name, s in sr.long_songs(N_CU).items()}
    for name, got in long_.items():
        print(f"{name:10s} {sr.long_songs(N_CU)[name].size:9d} samples: {sorted(got)}")
    g = 8 * N_CU * 256
    assert [s.size for s in sr.long_songs(N_CU).values()][:5] == [12 * g, 16 * g + 1, 16 * g + 8 + 5, 20 * g + 7, 28 * g + 3]
    assert long_["1.5g"] == {"single_only", "paired_no_leftover", "tail_0"}
    assert long_["2g"] == {"paired_no_leftover", "tail_1"}
    assert long_["2g+1"] == {"paired_no_leftover", "paired_leftover", "tail_5"}
    assert long_["2.5g"] == {"paired_no_leftover", "paired_leftover", "tail_7"}
    assert long_["3.5g"] == {"paired_twice", "paired_no_leftover", "paired_leftover", "tail_3"}
    assert "paired_twice" in long_["sat_value"] and "paired_twice" in long_["sat_zero"]
    reached = set().union(*long_.values())
    # a song of more than one stride has no idle lane: that class is the short songs'
    assert reached >= set(sr.STRUCTURAL) - {"idle_block_lanes"}, sorted(set(sr.STRUCTURAL) - reached)
    assert reached | set().union(*designed.values()) == sr.ALL_CLASSES
    # a batch shares the grid among its songs: there a lane of a designed song does pair
    batch_max = max(s["pcm"].size for s in songs.values())
    in_batch = set().union(*[sr.scan_geometry(s["pcm"].size, len(songs), N_CU, batch_max) for s in songs.values()])
    assert in_batch & sr.PAIRED


def test_the_designed_songs_are_what_their_names_say(oracle, songs, ref):
    assert 24 <= len(songs) <= 40
    assert {s["pcm"].size & 7 for s in songs.values()} == set(range(8))
    assert {s["channels"] for s in songs.values()} == {1, 2}
    assert all(sr.SHORTEST <= s["pcm"].size <= 300002 for s in songs.values())
    exp = {name: e for name, (e, _) in ref.items()}
    for name, sg in songs.items():
        full = ref[name][1]
        ratings = [full[k] for k in ("tempo", "amplitude", "frequency", "attack", "force")]
        assert sg["var0"] == (exp[name]["variance"] == 0), name
        assert sg["one_sample"] == (exp[name]["start"] == exp[name]["end"]), name
        if sg["var0"]:
            assert exp[name]["status"] == sr.BL_UNEXPECTED and np.isfinite(full["amplitude"]), name
        elif sg["one_sample"]:
            assert np.isnan(full["amplitude"]) and np.isnan(full["force"]) and full["calm_or_loud"] == sr.UNKNOWN, name
        else:
            assert np.all(np.isfinite(ratings)), (name, ratings)
    assert exp["two_samples"]["start"] - exp["two_samples"]["end"] == -1
    assert exp["zeros_inside"]["start"] > 0 and exp["zeros_inside"]["hist"][2048] > exp["zeros_inside"]["start"] + 2050
    for m in (13571, 13572, -13571, -13572):
        assert exp[f"wrapped_mean{m:+d}"]["mean"] == m and exp[f"mean{m:+d}"]["mean"] == m
    assert [exp[k]["mean"] for k in ("quotient_-0", "quotient_-1", "quotient_-1-")] == [0, -1, -1]
    assert (exp["floor"]["mean"], exp["floor"]["variance"]) == (28588, -530408560)
    assert exp["wrap_up"]["mean"] < -10000 and exp["wrap_down"]["mean"] > 10000
    assert abs(exp["wrap_twice"]["sum"]) > 2 * 2 ** 32 - 2 ** 31
    assert exp["large_variance"]["variance"] > 2 ** 30 and abs(exp["large_variance"]["mean"]) > sr.CLOSED_FORM_LIMIT
    beyond = [n for n, e in exp.items() if abs(e["mean"]) > sr.CLOSED_FORM_LIMIT]
    negative = [n for n, e in exp.items() if e["variance"] < 0]
    opposite = [n for n, e in exp.items() if abs(e["sum"]) >= 2 ** 31 and e["sum"] * e["mean"] < 0]
    print(f"\n|mean| > 13571: {beyond}\nnegative variance: {negative}\nwrapped to the opposite sign: {opposite}")
    assert len(beyond) >= 4 and len(negative) >= 2 and len(opposite) >= 3
    for name in CALLER_SONGS:
        assert name in songs
