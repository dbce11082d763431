"""FIR mode 2 of the window kernel transforms the unscaled integer filter sums and applies the song's scale, squared, to
the power terms (bl_fft512_power1_sq in bliss_amd/csrc/bl_fft_tan.h; kappa from k_song_prep).  On short songs at the
edges of that arithmetic the integers must stay mode 0's and the oracle's, the bits must not depend on the launch
geometry or the run, and the window energies must stay mode 0's up to the project's allowance: at most two per batch,
each one ulp off.

Songs (44.1 kHz, mono): 18 windows (the shortest input the library takes), 20 and 22 windows (n_windows mod 4 = 2, 0, 2:
a last round of two windows and a full one); a 20-s song, analysed alone and beside a 60-s one (other run boundaries:
blocks filtered in front of a run here are main-loop blocks there); samples within +-3 (variance 4: close to the largest
scale, kappa ~ 1e-6); a full-scale square wave (the smallest scale of real material); means of +-32 000 with a few LSB of
noise (the largest constant in the matrix products' initial values, the variance from the wrap pass); and a constant
song, which keeps its status."""
import numpy as np
import pytest

from bliss_amd import _lib
from tests.test_gpu_parity import check_song
from tests.window_reference import analyze as _analyze_songs, grid_x as _grid_x, run_starts as _run_starts

pytestmark = pytest.mark.gpu

RATE = 44100
I_20S = 3       # position of the 20-s song in _songs()


def _songs(oracle):
    rng = np.random.default_rng(92001)
    out = [oracle.synth(92001, RATE, 1, 5120), oracle.synth(92002, RATE, 1, 5700), oracle.synth(92003, RATE, 1, 6200),
           oracle.synth(92004, RATE, 1, RATE * 20), oracle.synth(92005, RATE, 1, RATE * 60),
           rng.integers(-3, 4, RATE * 2).astype(np.int16)]
    t = np.arange(RATE * 2)
    sq = np.where((t // 37) % 2 == 0, 32767, -32768).astype(np.int16)
    sq[::1001] = 0   # a few quiet samples: the reference's histogram needs its central bins non-empty
    out.append(sq)
    # 60 000 samples: the reference's int32 sum of the samples does not wrap, so the mean is the offset itself
    out.append((32000 + rng.integers(-20, 21, 60000)).astype(np.int16))
    out.append((-32000 + rng.integers(-20, 21, 60000)).astype(np.int16))
    return out


def _secs(pcm):
    return max(1, len(pcm) // RATE)


def _analyze(lib, songs, mode):
    return _analyze_songs(lib, [(p, 1) for p in songs], mode)


@pytest.fixture(scope="module")
def runs(gpu_lib, oracle):
    songs = _songs(oracle)
    ref = [oracle.analyze(p, 1, _secs(p)) for p in songs]
    return {"songs": songs, "ref": ref, "m0": _analyze(gpu_lib, songs, 0), "m2": _analyze(gpu_lib, songs, 2),
            "m2_again": _analyze(gpu_lib, songs, 2), "alone": _analyze(gpu_lib, [songs[I_20S]], 2)}


def test_the_integers_equal_mode0s_and_the_oracles(runs):
    got0, _ = runs["m0"]
    got2, _ = runs["m2"]
    for i, full in enumerate(runs["ref"]):
        check_song(got0[i], full, f"env_unscaled[{i}] mode 0")
        for k in got2.dtype.names:
            if got2.dtype[k].kind == "i":
                assert int(got2[i][k]) == int(got0[i][k]), (i, k, "mode 2 vs mode 0")
                if k in full:
                    assert int(got2[i][k]) == int(full[k]), (i, k, "mode 2 vs the oracle")
    assert [int(g["n_windows"]) for g in got2[:3]] == [18, 20, 22]
    assert int(got2[5]["variance"]) <= 4
    assert int(got2[7]["mean"]) == 32000 and int(got2[8]["mean"]) == -32000


def test_mode2_energies_are_mode0s_up_to_one_ulp(runs):
    _, en0 = runs["m0"]
    _, en2 = runs["m2"]
    moved = 0
    for i, (a, b) in enumerate(zip(en2, en0)):
        d = np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
        for w in np.nonzero(d)[0]:
            print(f"song {i} window {int(w)}: mode 2 {a[w]!r}, mode 0 {b[w]!r}, {int(d[w])} ulp")
        print(f"song {i}: {len(a)} windows, {int(np.count_nonzero(d))} energies moved")
        assert d.max() <= 1, (i, int(d.max()))
        moved += int(np.count_nonzero(d))
    assert moved <= 2, moved   # the project's allowance for a batch


def test_the_20s_song_alone_and_beside_the_60s_one_gives_the_same_bits(runs):
    import torch
    got, en = runs["m2"]
    one, en1 = runs["alone"]
    assert np.array_equal(en1[0].view(np.uint32), en[I_20S].view(np.uint32)), "window energies, alone vs in the batch"
    for k in got.dtype.names:
        assert one[0][k] == got[I_20S][k] or (one[0][k] != one[0][k] and got[I_20S][k] != got[I_20S][k]), k
    # the runs begin at other rounds in the two launches: that is the case this test is about
    lengths = [len(p) for p in runs["songs"]]
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    nw = int(got[I_20S]["n_windows"])
    assert _run_starts(nw, _grid_x(lengths[I_20S], 1, n_cu)) != _run_starts(nw, _grid_x(max(lengths), len(lengths), n_cu))


def test_two_runs_give_identical_records_and_energies(runs):
    (a, ea), (b, eb) = runs["m2"], runs["m2_again"]
    for k in a.dtype.names:
        assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)), k
    for x, y in zip(ea, eb):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def test_a_constant_song_keeps_its_status(gpu_lib):
    """Variance 0: kappa is not a number, as the scale was; the library flags the song in mode 2 as in mode 0, with the
    same integers."""
    song = [np.full(RATE * 2, 1000, dtype=np.int16)]
    got0, _ = _analyze(gpu_lib, song, 0)
    got2, _ = _analyze(gpu_lib, song, 2)
    assert int(got0[0]["status"]) == _lib.BL_UNEXPECTED and int(got2[0]["status"]) == _lib.BL_UNEXPECTED
    assert int(got2[0]["variance"]) == 0 and int(got2[0]["mean"]) == 1000
    for k in got2.dtype.names:
        if got2.dtype[k].kind == "i":
            assert int(got2[0][k]) == int(got0[0][k]), k
