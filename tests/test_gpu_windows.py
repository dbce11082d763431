"""k_env_windows3 (bliss_amd/csrc/bl_env_kernels.hip) at every round count from 5 to 65, in launches of 1, 2, 5 and 57
workgroups per song and in the three FIR modes, held per window to the oracle (mode 0: bit for bit), to mode 0 (modes 1
and 2: the project's allowance of two energies one ulp off) and to the exact energies of tests/window_reference.py, a
reference that shares no transform with the oracle.  Only the GPU runs the kernel's orchestration: the split of a
song's rounds over the compute waves, waves whose run is shorter or empty, the five-block ring, the block in front of a
run, the zero-state heads, the range-checked loads, the hand-over of the two halves of the ordered sum one step apart.

The sweep batches (tests/window_reference.py names the geometry classes; the test asserts that they are reached with
the device's CU count):
    A  sweep songs shorter than 57 344 samples, alone          1 workgroup per song
    B  the whole sweep                                         2
    C  the whole sweep beside one 10-second song               5
    D  the eight shortest sweep songs beside a 45-second song  57 on 256 CUs: most workgroups of a short song have no round
The designed songs (a tone per term around the place where the halves of the sum meet, byte-plane edges, alternating
full scale, the mean classes of the matrix products' constant) run alone and beside the 10-second song; the split
corpus runs as the one batch the launcher splits into a head and a rest launch."""
import ctypes as C
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import window_reference as wr
from tests.test_fir_int_host import build_program, run_files
from tests.test_gpu_parity import check_song

pytestmark = pytest.mark.gpu

MODES = (0, 1, 2)


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    """not a check: prints what the file took, oracle and fixtures included"""
    t0 = time.perf_counter()
    yield
    print(f"\ntests/test_gpu_windows.py: {time.perf_counter() - t0:.1f} s")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


def _same_record(a, b):
    return all(_bits(a[k]) == _bits(b[k]) for k in a.dtype.names)


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _reference(oracle, songs):
    """name -> (the oracle's full record, the oracle's energies, the exact energies), the oracle's runs side by side"""
    names = list(songs)
    oracle.analyze(*songs[names[0]], 1)   # the oracle's tables are built by its first call

    def one(name):
        pcm, ch = songs[name]
        full = oracle.analyze(pcm, ch, wr.secs(pcm, ch))
        rec, en = oracle.envelope(pcm, wr.secs(pcm, ch))
        return full, en[:rec["n_windows"]].copy()
    with ThreadPoolExecutor(8) as pool:
        res = list(pool.map(one, names))
    out = {}
    for name, (full, en) in zip(names, res):
        mean, var = wr.mean_variance(oracle, songs[name][0])
        assert (mean, var) == (full["mean"], full["variance"]), name
        exact = wr.exact_energies(songs[name][0], mean, var)
        assert wr.within_bound(en, exact).all(), name
        exact.setflags(write=False)
        en.setflags(write=False)
        out[name] = (full, en, exact)
    return out


def _run(lib, songs, names):
    """mode -> name -> (record, energies) of the songs `names` analysed as one batch"""
    out = {}
    for mode in MODES:
        got, en = wr.analyze(lib, [songs[n] for n in names], mode)
        out[mode] = {n: (got[i], en[i]) for i, n in enumerate(names)}
    return out


@pytest.fixture(scope="module")
def n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def sweep_songs(oracle):
    songs = {f"sweep{i}": s for i, s in enumerate(wr.sweep(oracle))}
    songs["companion10"], songs["companion45"] = wr.companion(oracle, 10), wr.companion(oracle, 45)
    return songs


@pytest.fixture(scope="module")
def sweep_batches(sweep_songs):
    sweep = [n for n in sweep_songs if n.startswith("sweep")]
    return {"A": [n for n in sweep if len(sweep_songs[n][0]) < wr.A_LIMIT], "B": sweep, "C": sweep + ["companion10"],
            "D": sorted(sweep, key=lambda n: len(sweep_songs[n][0]))[:8] + ["companion45"]}


@pytest.fixture(scope="module")
def sweep_ref(oracle, sweep_songs):
    return _reference(oracle, sweep_songs)


@pytest.fixture(scope="module")
def sweep_runs(gpu_lib, sweep_songs, sweep_batches):
    return {b: _run(gpu_lib, sweep_songs, names) for b, names in sweep_batches.items()}


def _check_mode0(runs, ref, tag):
    """(b): every energy bit-identical to the oracle's, every record passes check_song"""
    for name, (rec, en) in runs[0].items():
        full, ref_en, _ = ref[name]
        check_song(rec, full, f"{tag} {name} mode 0")
        assert int(rec["n_windows"]) == len(en) == len(ref_en), (tag, name)
        bad = np.flatnonzero(en.view(np.uint32) != ref_en.view(np.uint32))
        assert bad.size == 0, (tag, name, "mode 0 vs the oracle, windows", bad[:8].tolist(), en[bad[:4]], ref_en[bad[:4]])


def _check_modes12(runs, tag):
    """(c) within one batch: integer fields mode 0's, every energy within one ulp of mode 0's; returns
    mode -> [(name, window)] of the energies that differ"""
    moved = {}
    for mode in (1, 2):
        moved[mode] = []
        for name, (rec, en) in runs[mode].items():
            rec0, en0 = runs[0][name]
            for k in rec.dtype.names:
                if rec.dtype[k].kind == "i":
                    assert int(rec[k]) == int(rec0[k]), (tag, name, k, f"mode {mode} vs mode 0")
            d = _ulps(en, en0)
            assert d.max() <= 1, (tag, name, f"mode {mode}", np.flatnonzero(d > 1)[:8].tolist(), int(d.max()))
            moved[mode] += [(name, int(w)) for w in np.flatnonzero(d)]
    return moved


def _check_exact(runs, ref, tag):
    """(d): every energy of every mode within the derived bound of the exact reference"""
    for mode in MODES:
        for name, (_, en) in runs[mode].items():
            exact = ref[name][2]
            ok = wr.within_bound(en, exact)
            assert ok.all(), (tag, name, f"mode {mode}", np.flatnonzero(~ok)[:8].tolist(),
                              float((np.abs(en - exact) / exact).max()), wr.BOUND)


def test_the_batches_reach_every_geometry_class(sweep_songs, sweep_batches, n_cu):
    gx, reached = {}, set()
    for b, names in sweep_batches.items():
        lengths = [len(sweep_songs[n][0]) for n in names]
        gx[b] = wr.grid_x(max(lengths), len(lengths), n_cu)
        got = wr.geometry_classes([wr.n_windows_of(n) for n in lengths], gx[b])
        print(f"batch {b}: {len(names)} songs, {gx[b]} workgroups per song on {n_cu} CUs, {len(got)} classes; "
              f"misses {sorted(wr.ALL_CLASSES - got)}")
        reached |= got
    assert gx["A"] == 1 and len(set(gx.values())) == 4, gx
    assert reached == wr.ALL_CLASSES, sorted(wr.ALL_CLASSES - reached)


@pytest.mark.parametrize("batch", "ABCD")
def test_mode0_is_the_oracle_bit_for_bit(sweep_runs, sweep_ref, batch):
    _check_mode0(sweep_runs[batch], sweep_ref, f"batch {batch}")


def test_modes_1_and_2_do_not_depend_on_the_geometry_and_stay_mode0s(sweep_runs):
    moved = {b: _check_modes12(sweep_runs[b], f"batch {b}") for b in "ABCD"}
    for mode in (1, 2):
        first = {}   # name -> (batch, record, energies) of the song's first appearance
        for b in "BCDA":
            for name, (rec, en) in sweep_runs[b][mode].items():
                b0, rec0, en0 = first.setdefault(name, (b, rec, en))
                assert np.array_equal(en.view(np.uint32), en0.view(np.uint32)), (name, f"mode {mode}", "batch", b, "vs", b0)
                assert _same_record(rec, rec0), (name, f"mode {mode}", "records, batch", b, "vs", b0)
        once = sorted(set().union(*[moved[b][mode] for b in "ABCD"]))   # the batches agree bit for bit: count once
        print(f"mode {mode}: {len(once)} of {sum(len(v[2]) for v in first.values())} energies differ from mode 0's "
              f"(by one ulp): {once}")
        assert len(once) <= 2, (mode, once)


@pytest.mark.parametrize("batch", "ABCD")
def test_every_energy_lies_within_the_derived_bound_of_the_exact_one(sweep_runs, sweep_ref, batch):
    _check_exact(sweep_runs[batch], sweep_ref, f"batch {batch}")


@pytest.fixture(scope="module")
def designed(gpu_lib, oracle, tmp_path_factory):
    """the designed songs alone and beside the 10-second companion, their references, and what the CPU emulation of
    mode 2 (the shipped route of tests/host/test_fir_int_host.cpp) counted on them"""
    tmp = tmp_path_factory.mktemp("designed")
    songs = dict(wr.designed())
    cpu = run_files(build_program(tmp), tmp, songs, jobs=8)
    songs["companion10"] = wr.companion(oracle, 10)
    own = [n for n in songs if n != "companion10"]
    return {"ref": _reference(oracle, songs), "own": own, "cpu_moved": sum(v[1] for v in cpu.values()),
            "runs": {"alone": _run(gpu_lib, songs, own), "beside": _run(gpu_lib, songs, own + ["companion10"])}}


def test_the_designed_songs_in_mode0_are_the_oracle_bit_for_bit(designed):
    for tag, r in designed["runs"].items():
        _check_mode0(r, designed["ref"], tag)


def test_the_designed_songs_in_modes_1_and_2_stay_mode0s_whatever_the_geometry(designed):
    runs = designed["runs"]
    for tag, r in runs.items():
        moved = _check_modes12(r, tag)
        for mode in (1, 2):
            print(f"designed songs {tag}, mode {mode}: {len(moved[mode])} energies differ from mode 0's: {moved[mode]}")
            assert len(moved[mode]) <= 2, (tag, mode, moved[mode])
        own_moved = [m for m in moved[2] if m[0] != "companion10"]
        print(f"designed songs {tag}, mode 2: {len(own_moved)} moved on the GPU, {designed['cpu_moved']} in the CPU emulation")
        assert len(own_moved) <= designed["cpu_moved"], (tag, own_moved, designed["cpu_moved"])
    for mode in (1, 2):
        for name in designed["own"]:
            (ra, ea), (rb, eb) = runs["alone"][mode][name], runs["beside"][mode][name]
            assert np.array_equal(ea.view(np.uint32), eb.view(np.uint32)) and _same_record(ra, rb), (name, mode)


def test_the_designed_songs_lie_within_the_derived_bound_of_the_exact_energies(designed):
    for tag, r in designed["runs"].items():
        _check_exact(r, designed["ref"], tag)


def _launches(lib, songs, mode):
    """wr.analyze with the profile counter around it: (records, energies, env_windows launches)"""
    lib.bl_amd_profile_reset()
    lib.bl_amd_profile(1)
    try:
        got, en = wr.analyze(lib, songs, mode)
    finally:
        lib.bl_amd_profile(0)
    n = C.c_int(0)
    lib.bl_amd_profile_ms(b"env_windows", C.byref(n))
    return got, en, n.value


def test_the_head_rest_split_gives_the_bits_of_unsplit_batches(gpu_lib, oracle):
    songs = list(wr.split_corpus(oracle))
    got0, en0, launches0 = _launches(gpu_lib, songs, 0)
    got2, en2, launches2 = _launches(gpu_lib, songs, 2)
    assert launches0 == 2 and launches2 == 2, (launches0, launches2)   # the split happened
    for i, (pcm, ch) in enumerate(songs):
        rec, ref_en = oracle.envelope(pcm, wr.secs(pcm, ch))
        nw = rec["n_windows"]
        assert int(got0[i]["n_windows"]) == nw == len(en0[i]), i
        assert np.array_equal(en0[i].view(np.uint32), ref_en[:nw].view(np.uint32)), (i, "mode 0 vs the oracle")
    parts = {}
    for mode in (0, 2):
        head, en_head, l_head = _launches(gpu_lib, songs[:wr.SPLIT_HEAD], mode)
        rest, en_rest, l_rest = _launches(gpu_lib, songs[wr.SPLIT_HEAD:], mode)
        assert l_head == 1 and l_rest == 1, (mode, l_head, l_rest)   # too small to split
        parts[mode] = (np.concatenate([head, rest]), en_head + en_rest)
    for mode, got, en in ((0, got0, en0), (2, got2, en2)):
        recs, ens = parts[mode]
        for i in range(len(songs)):
            assert np.array_equal(en[i].view(np.uint32), ens[i].view(np.uint32)), (i, f"mode {mode}", "split vs unsplit")
            assert _same_record(got[i], recs[i]), (i, f"mode {mode}", "records, split vs unsplit")
    assert all(int(g["status"]) == 0 for g in got2)
