"""FIR mode 2 of the window kernel as exact int8 matrix products (bliss_amd/csrc/bl_fir_int.h) on short songs: the
three paths that filter — the main loop, the block in front of a run, the zero-state heads — must give one set of bits
whatever the launch geometry, and stay mode 0's result up to its own rounding noise.

Songs (44.1 kHz): five of the synthetic generator, mono and stereo, 2-6 s and the shortest input the library takes
(5 120 samples: 18 windows are 5 rounds, fewer than the 7 compute waves of a workgroup, so some runs are empty); a
full-scale square wave; a song with a DC offset beyond |mean| = 13 571.  n_windows = 2 * floor(n / 512) - 2 is even, so
n_windows mod 4 takes its two possible values, 0 and 2; a song with fewer than four windows is below the shortest
input.  The seeds are the ones tests/host/test_fir_int_host.cpp runs on the CPU: no energy moves against the oracle
there."""
import numpy as np
import pytest

from bliss_amd import _lib
from tests.test_gpu_parity import check_song
from tests.window_reference import analyze as _analyze, grid_x as _grid_x, run_starts as _run_starts

pytestmark = pytest.mark.gpu

RATE = 44100
SYNTH = [(81001, 2, 176400), (81002, 1, 132812), (81003, 2, 529200), (81004, 1, 5120), (81005, 2, 265134)]


def _songs(oracle):
    out = [(oracle.synth(seed, RATE, ch, n), ch) for seed, ch, n in SYNTH]
    dc = (oracle.synth(81006, RATE, 1, 88533).astype(np.int32) // 2 + 15000).astype(np.int16)
    out.append((dc, 1))
    t = np.arange(176400)
    sq = np.where((t // 37) % 2 == 0, 32767, -32768).astype(np.int16)
    sq[::1001] = 0   # a few quiet samples: the reference's histogram needs its central bins non-empty
    out.append((sq, 2))
    return out


def _secs(pcm, ch):
    return max(1, len(pcm) // (RATE * ch))


@pytest.fixture(scope="module")
def runs(gpu_lib, oracle):
    songs = _songs(oracle)
    ref = [(oracle.analyze(p, c, _secs(p, c)), oracle.envelope(p, _secs(p, c))[1]) for p, c in songs]
    return {"songs": songs, "ref": ref, "m0": _analyze(gpu_lib, songs, 0), "m2": _analyze(gpu_lib, songs, 2),
            "m2_again": _analyze(gpu_lib, songs, 2), "alone": [_analyze(gpu_lib, [s], 2) for s in songs]}


def _same_records(a, b):
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8))
               for k in a.dtype.names)


def test_mode0_and_the_integers_equal_the_oracle(runs):
    got0, en0 = runs["m0"]
    got2, _ = runs["m2"]
    for i, (full, ref_en) in enumerate(runs["ref"]):
        check_song(got0[i], full, f"fir_int[{i}] mode 0")
        nw = int(got0[i]["n_windows"])
        assert nw == len(en0[i]) and nw % 4 in (0, 2)
        assert np.array_equal(en0[i].view(np.uint32), ref_en[:nw].view(np.uint32)), (i, "window energies, mode 0")
        for k in got2.dtype.names:
            if got2.dtype[k].kind == "i":
                assert int(got2[i][k]) == int(got0[i][k]), (i, k, "mode 2 vs mode 0")
                if k in full:
                    assert int(got2[i][k]) == int(full[k]), (i, k, "mode 2 vs the oracle")
    assert {int(g["n_windows"]) % 4 for g in got0} == {0, 2}
    assert abs(int(got0[5]["mean"])) > 13571


def test_mode2_energies_are_mode0s_up_to_one_ulp(runs):
    _, en0 = runs["m0"]
    _, en2 = runs["m2"]
    moved = 0
    for i, (a, b) in enumerate(zip(en2, en0)):
        d = np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
        print(f"song {i}: {len(a)} windows, {int(np.count_nonzero(d))} energies moved, largest step {int(d.max())} ulp")
        assert d.max() <= 1, (i, int(d.max()))
        moved += int(np.count_nonzero(d))
    assert moved <= 2, moved   # the project's cap for a file; the CPU run of the same songs shows none


def test_a_song_alone_and_in_the_batch_gives_the_same_bits(runs):
    import torch
    got, en = runs["m2"]
    lengths = [len(p) for p, _ in runs["songs"]]
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    differ = 0
    for i, (one, en1) in enumerate(runs["alone"]):
        assert np.array_equal(en1[0].view(np.uint32), en[i].view(np.uint32)), (i, "window energies, alone vs in the batch")
        for k in got.dtype.names:
            assert one[0][k] == got[i][k] or (one[0][k] != one[0][k] and got[i][k] != got[i][k]), (i, k)
        nw = int(got[i]["n_windows"])
        differ += _run_starts(nw, _grid_x(lengths[i], 1, n_cu)) != _run_starts(nw, _grid_x(max(lengths), len(lengths), n_cu))
    # the case this test is about: runs that begin at other rounds beside a longer song than alone (the 2-s stereo
    # song: 6 blocks alone, 18 in the batch), so blocks filtered in front of a run here are main-loop blocks there
    assert differ >= 2, differ


def test_two_runs_give_identical_records_and_energies(runs):
    (a, ea), (b, eb) = runs["m2"], runs["m2_again"]
    assert _same_records(a, b)
    for x, y in zip(ea, eb):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def test_a_constant_song_keeps_its_status(gpu_lib):
    """Variance 0: the reference divides by zero, the library flags the song — in mode 2 as in mode 0, with the same
    integers."""
    song = [(np.full(RATE * 2, 1000, dtype=np.int16), 1)]
    got0, _ = _analyze(gpu_lib, song, 0)
    got2, _ = _analyze(gpu_lib, song, 2)
    assert int(got0[0]["status"]) == _lib.BL_UNEXPECTED and int(got2[0]["status"]) == _lib.BL_UNEXPECTED
    assert int(got2[0]["variance"]) == 0 and int(got2[0]["mean"]) == 1000
    for k in got2.dtype.names:
        if got2.dtype[k].kind == "i":
            assert int(got2[0][k]) == int(got0[0][k]), k
