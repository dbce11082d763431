"""Parity at the sizes BASELINE.json quotes: the full configs[1] count (1 024 x 30 s) and the
metric's own song shape (S180 = 3 min, 44.1 kHz, stereo) in a resident batch — HIP path vs the
CPU oracle on the same bytes (the device generator is byte-identical to oracle/orc_synth.c)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bliss_amd
from tests.test_gpu_parity import check_song

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _driver_tail(stdout, stderr, keep=2000):
    """What the driver keeps of a bench run (BENCH_r*.json `tail`): the last `keep` bytes of stdout followed by its
    stderr section."""
    return (stdout + "\n---- stderr ----\n" + stderr)[-keep:]


def _run_bench(cmd, tmp_path, env=None, timeout=900):
    """bench.py as a child process.  Returns (line, details): the ONE compact stdout line — which must survive the
    driver's 2 000-byte tail whole (round 5's 21 KB line did not: BENCH_r05.json `parsed: null`) — and the full record
    it wrote to --details-out."""
    det = os.path.join(str(tmp_path), "bench_details.json")
    r = subprocess.run(cmd + ["--details-out", det], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env,
                       timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    assert len(lines[0]) <= 1700, len(lines[0])
    tail = _driver_tail(r.stdout, r.stderr)
    kept = [l for l in tail.splitlines() if l.startswith("{")]
    assert kept and kept[-1] == lines[0], "the JSON line does not fit in the last 2 000 bytes of stdout + stderr"
    line = json.loads(kept[-1])
    assert line["details"] == "bench_details.json"
    return line, json.load(open(det))


def _energies(lib, got):
    total = int(sum(int(g["nb_frames"]) for g in got))
    en = np.zeros(total, dtype=np.float32)
    assert lib.bl_amd_last_energies(en.ctypes.data_as(C.POINTER(C.c_float)), total) == total
    offs = np.concatenate([[0], np.cumsum(got["nb_frames"].astype(np.int64))])
    return en, offs


def _check_sample(lib, oracle, corpus, got, picks, rate, channels, seconds, seed_base, tag):
    """`got`: the batch as the default FIR mode analysed it (the library's last batch).  Features and
    integers are held against the oracle as they are; the window energies of the default mode may
    sit one f32 ulp off the reference arithmetic in about one window per 10^8 (bl_amd_set_fir_mode),
    so they are compared with that allowance and then — after a second analysis in mode 0, the
    reference's own FIR — bit for bit."""
    en, offs = _energies(lib, got)
    try:
        assert lib.bl_amd_set_fir_mode(0) == 0
        corpus.analyze()
        got0 = corpus.fetch()
        en0, _ = _energies(lib, got0)
    finally:
        lib.bl_amd_set_fir_mode(-1)
    # default mode vs mode 0 over the whole batch: every integer identical.  The default mode moves about one window
    # energy per 10^8 by one f32 ulp — at 8 192 S180 songs that is a handful of the 508 million
    # energies, each of which shows in its song's f64 onset sum (atk_sum, ~1e-12 relative) and, rarely, in the last
    # bit of an f32 feature; small batches see none of it
    for k in got.dtype.names:
        if got.dtype[k].kind == "i":
            assert np.array_equal(got[k], got0[k]), (tag, "default FIR mode vs mode 0", k)
        elif got.dtype[k].itemsize == 8:
            differ = np.flatnonzero(got[k] != got0[k])
            assert len(differ) <= max(2, len(got) // 512), (tag, "default FIR mode vs mode 0", k, len(differ))
            assert np.allclose(got[k], got0[k], rtol=1e-9, atol=0), (tag, k)
        else:
            d = np.abs(got[k].view(np.int32).astype(np.int64) - got0[k].view(np.int32).astype(np.int64))
            assert d.max() <= 1 and np.count_nonzero(d) <= max(1, len(got) // 2048), (tag, "default FIR mode vs mode 0", k,
                                                                                     int(d.max()), int(np.count_nonzero(d)))
    n = rate * channels * seconds
    pcm = corpus.pcm
    moved = 0
    for i in picks:
        o = int(corpus.desc[i].pcm_offset)
        song = pcm[o:o + n].cpu().numpy()
        # the generator is a pure function of (seed, index): spot-check the bytes, then let the
        # oracle analyse exactly what the kernels read
        assert np.array_equal(song[:65536], oracle.synth(seed_base + i, rate, channels, 65536))
        _, ref_en = oracle.envelope(song, seconds)
        full = oracle.analyze(song, channels, seconds)
        check_song(got[i], full, f"{tag}[{i}]")
        nw = int(got[i]["n_windows"])
        assert np.array_equal(en0[offs[i]:offs[i] + nw].view(np.uint32), ref_en[:nw].view(np.uint32)), \
            (tag, i, "window energies, mode 0")
        d = np.abs(en[offs[i]:offs[i] + nw].view(np.int32).astype(np.int64) - ref_en[:nw].view(np.int32).astype(np.int64))
        assert d.max() <= 1, (tag, i, "window energies, default mode: more than one ulp", int(d.max()))
        moved += int(np.count_nonzero(d))
    assert moved <= 2, (tag, "window energies, default mode", moved)   # <= 1e6 windows compared: none expected


def test_configs1_full_count(gpu_lib, oracle):
    """BASELINE configs[1]: 1 024 synthetic 30-s 44.1 kHz stereo buffers on one GPU; every song's
    integers checked for plausibility, 8 of them against the oracle (ints exact, floats 1e-4
    relative, all 10 332 window energies bit-identical)."""
    n = 44100 * 2 * 30
    corpus = bliss_amd.DeviceCorpus([n] * 1024, 2, 30)
    corpus.synth(seed_base=20000, sample_rate=44100)
    corpus.analyze()
    got = corpus.fetch()
    assert np.all(got["status"] == 0) and np.all(got["n_windows"] == 10332)
    assert np.all(got["n_frames"] == 2583) and np.all(got["nb_frames"] == 10334)
    assert np.all(got["start"] < 8) and np.all(got["end"] > n - 9)   # the generator may emit a 0 at an end
    assert np.all(np.isfinite(got["force"])) and len(np.unique(got["force"])) > 900
    _check_sample(gpu_lib, oracle, corpus, got, (0, 1, 255, 256, 511, 700, 1022, 1023), 44100, 2, 30, 20000,
                  "s30x1024")


def test_s180_resident_batch(gpu_lib, oracle):
    """The headline shape: 256 resident S180 songs (8.1 GB of PCM), 8 of them against the oracle
    including beat / tempo and all 62 012 window energies."""
    n = 44100 * 2 * 180
    corpus = bliss_amd.DeviceCorpus([n] * 256, 2, 180)
    corpus.synth(seed_base=30000, sample_rate=44100)
    corpus.analyze()
    got = corpus.fetch()
    assert np.all(got["status"] == 0) and np.all(got["n_windows"] == 62012)
    assert np.all(got["n_frames"] == 15503) and np.all(got["beat"] > 100)
    _check_sample(gpu_lib, oracle, corpus, got, (0, 1, 63, 64, 127, 128, 200, 255), 44100, 2, 180, 30000, "s180x256")


def test_configs2_shard_resident_headline_shape(gpu_lib, oracle):
    """BASELINE configs[2]'s per-GPU shard as bench.py holds it: 8 192 resident S180 songs (260 GB of PCM; the largest
    power of two that fits if the box has less free HBM).  Every song: status 0 and the integer geometry of the shape
    (62 012 windows, 15 503 frames); the default FIR mode and mode 0 agree in every field of every song; 16 songs
    spread over the batch against the oracle — integers exact, floats 1e-4 relative, all 62 012 window energies of
    each bit-identical in mode 0.  Until round 6 this shape was only checked inside bench.py."""
    import torch
    n = 44100 * 2 * 180
    free_b, _ = torch.cuda.mem_get_info(0)
    per_song = 2 * n + 12 * (2 * (n // 512)) + 4 * 4096 + 4096
    fit = int((free_b - (10 << 30)) // per_song)
    songs = 8192 if fit >= 8192 else 1 << (max(fit, 1).bit_length() - 1)
    assert songs >= 256, (songs, free_b)
    corpus = bliss_amd.DeviceCorpus([n] * songs, 2, 180)
    corpus.synth(seed_base=40000, sample_rate=44100)
    corpus.analyze()
    got = corpus.fetch()
    assert np.all(got["status"] == 0) and np.all(got["n_windows"] == 62012) and np.all(got["nb_frames"] == 62014)
    assert np.all(got["n_frames"] == 15503) and np.all(got["beat"] > 100)
    assert np.all(got["start"] < 8) and np.all(got["end"] > n - 9)
    assert np.all(np.isfinite(got["force"])) and len(np.unique(got["force"])) > 0.9 * songs
    picks = sorted(set(int(round(j * (songs - 1) / 15)) for j in range(16)))
    _check_sample(gpu_lib, oracle, corpus, got, picks, 44100, 2, 180, 40000, f"s180x{songs}")
    del corpus
    torch.cuda.empty_cache()


def test_bench_under_torchrun_runs_rccl_and_verifies(gpu_lib, tmp_path):
    """bench.py as the driver launches it for N > 1 (torch.distributed.run, one rank per GPU, RCCL
    group) at world size 1 and a small batch: process-group init, the all-gather of the force
    vectors and the row-block matrix run, and the line reports oracle-verified songs."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
           "--master-addr", "127.0.0.1", "--master-port", "29611", os.path.join(ROOT, "bench.py"),
           "--gpus", "1", "--steps", "1", "--warmup", "1", "--songs-per-gpu", "16", "--seconds", "20",
           "--full", "--no-cpu-baseline", "--verify", "4"]
    line, det = _run_bench(cmd, tmp_path, env=env)
    assert line["n_gpus"] == 1 and line["results_ok"] is True and line["verified_songs"] == 4
    assert line["collective"] == "nccl" and det["collective"]["all_gather_calls"] >= 2
    assert line["roofline"]["kernel"] and line["value"] > 0
    # both contract objects stand on the compact line
    assert line["roofline"]["frac"] > 0 and line["roofline"]["bound"] == "hbm" and line["roofline"]["peak"] == 8000.0
    assert {"value", "unit", "cores", "kind", "sample"} <= set(line["cpu_baseline"])
    # both f64 floors: at the clock the power cap leaves and at the specified 2.4 GHz
    assert 0 < line["roofline"]["frac_of_f64_floor_nominal"] < line["roofline"]["frac_of_f64_floor"] < 1.2
    # the strict-order figures (real steps in FIR mode 0) and the literal north_star bar
    # (a 16-song batch is launch-bound: the two modes time alike there, mode 0 is 19 % slower at the real size)
    assert 0 < line["value_fir_mode0"] <= line["value"] * 1.5 and line["roofline"]["frac_fir_mode0"] > 0
    assert det["fir_modes"]["mode0_steps"] >= 1 and det["fir_modes"]["songs_with_an_integer_differing_from_mode0"] == 0
    assert line["strict_1e-4_rel_failures"] == 0
    assert set(det["verification"]["n_failing_strict_1e-4_rel"]) == {"tempo", "amplitude", "frequency", "attack", "force"}
    assert det["device_state"]["samples"] >= 0 and "pci" in det["device_state"] and "sclk_mhz" in line["device_state"]
    oc = det["other_configs"]
    assert oc["configs1"]["results_ok"] is True and oc["configs4_mixed"]["results_ok"] is True
    assert oc["configs1"]["songs_per_s"] > 0 and oc["configs4_mixed"]["verified_songs"] >= 3
    assert line["other_configs"]["ok"] is True and line["other_configs"]["configs1_songs_per_s"] > 0
    # roofline.traffic: collected in the run itself when rocprofv3 and the counters are there (two --pmc passes in
    # child processes), else the committed profile's figure — either way the line says which
    rf = det["roofline"]
    if "live_collection_error" in rf["traffic_source"]:
        assert line["roofline"]["traffic_src"].startswith("profiles/") and rf["traffic"] > 0
    else:
        assert line["roofline"]["traffic_src"] == "live_pmc" and rf["traffic_source"]["what"].startswith("collected in this run")
        # a 16-song batch: L2 / MALL hits can take a little off FETCH_SIZE
        assert 0.8 < rf["traffic"] / rf["algorithmic_bytes_per_launch"] < 1.3, rf["traffic"]


def test_bench_self_launch(gpu_lib, tmp_path):
    """The driver's own command form, `python bench.py --gpus N ...` with no launcher around it:
    --launch takes the N = 1 case through the same self-launch path N > 1 uses (ranks started
    under torch.distributed.run on 127.0.0.1, RCCL process group, one JSON line on stdout)."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--launch", "--steps", "2", "--warmup", "1",
           "--songs-per-gpu", "16", "--seconds", "20", "--full", "--no-cpu-baseline", "--verify", "4", "--no-live-traffic"]
    line, det = _run_bench(cmd, tmp_path)
    assert line["n_gpus"] == 1 and line["steps"] == 2 and line["results_ok"] is True
    assert line["collective"] == "nccl" and det["collective"]["all_gather_calls"] >= 2
    assert line["verified_songs"] == 4 and line["roofline"]["frac"] > 0
    assert line["roofline"]["traffic_src"] is None or line["roofline"]["traffic_src"].startswith("profiles/")   # --no-live-traffic
    # more ranks than devices: refused before anything is launched, and the message says why
    import torch
    if torch.cuda.device_count() == 1:
        r2 = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], stdout=subprocess.PIPE,
                            stderr=subprocess.PIPE, text=True, timeout=300)
        assert r2.returncode == 2 and r2.stdout.strip() == ""
        assert "1 HIP device(s)" in r2.stderr and "WORLD_SIZE" not in r2.stderr


def test_bench_plain_run_dumps_what_the_timed_step_computed(gpu_lib, oracle, tmp_path):
    """A plain run (no --full) times the steps and leaves every leg beside them out; --dump-outputs writes what the last
    timed step computed: the song records (checked against the oracle on two songs), the gathered force vectors and the
    row block of the distance matrix (the oracle's matrix of those vectors, bit for bit), all float32 / float64."""
    dump = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--songs-per-gpu", "16", "--seconds", "20", "--dump-outputs", str(dump)]
    line, det = _run_bench(cmd, tmp_path)
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "songs/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["results_ok"] is True and line["verified_songs"] == 0 and "value_fir_mode0" not in line
    assert det["other_configs"] is None and det["distance_matrix_10k_s"] is None and det["cpu_baseline"]["value"] is None
    assert "mode0_steps" not in det["fir_modes"] and det["kernels_ms"]["env_windows"]["launches"] == 2
    files = {p.stem: np.load(p) for p in dump.glob("*.npy")}
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(p.stat().st_size for p in dump.glob("*.npy")) < 64 << 20
    assert set(bliss_amd.batch.RESULT_DTYPE.names) < set(files)
    assert np.array_equal(files["song_index"], np.arange(16))
    fv = np.stack([files[k] for k in ("tempo", "amplitude", "frequency", "attack")], axis=1)
    assert np.array_equal(files["force_vectors"], fv) and np.array_equal(files["force_vectors_index"], np.arange(16))
    assert np.array_equal(files["distance_rows_index"], np.arange(16)) and files["distance_rows"].shape == (16, 16)
    assert np.array_equal(files["distance_rows"], oracle.distance_matrix(fv))
    n = 44100 * 2 * 20
    for i in (0, 15):
        got = np.zeros(1, dtype=bliss_amd.batch.RESULT_DTYPE)
        for k in got.dtype.names:
            got[k] = files[k][i]
        check_song(got[0], oracle.analyze(oracle.synth(i, 44100, 2, n), 2, 20), f"dump[{i}]")


def test_bench_on_every_gpu_of_the_box(gpu_lib, tmp_path):
    """`python bench.py --gpus <all>` on a box with more than one HIP device: N ranks under torch.distributed.run, an
    RCCL group of N, the all-gather of the force vectors across xGMI, every rank's row block and its share of the
    oracle check.  Skipped on a one-GPU box (there test_bench_two_ranks_rehearsal_on_one_gpu runs the N-rank code
    over gloo); on the first multi-GPU lease it runs as it stands."""
    import torch
    n = torch.cuda.device_count()
    if n < 2:
        pytest.skip("one HIP device on this box")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--steps", "2", "--warmup", "1",
           "--songs-per-gpu", "64", "--seconds", "30", "--full", "--cpu-ladder", "1,8", "--verify", str(4 * n), "--no-other-configs"]
    line, det = _run_bench(cmd, tmp_path, timeout=1500)
    assert line["n_gpus"] == n and line["results_ok"] is True and line["verified_songs"] == 4 * n
    assert line["collective"] == "nccl" and det["collective"]["all_gather_calls"] >= 3
    assert line["config"]["parallelism"] == f"shard{n}" and f"{64 * n} total" in line["config"]["workload"]
    assert len(line["per_rank_ms"]) == n
    pr = det["per_rank"]
    assert len(pr["ms_per_step"]) == n == len(pr["env_windows_ms"]) and min(pr["env_windows_ms"]) > 0
    assert len(det["device_state"]["per_rank_sclk_mhz"]) == n
    assert det["rehearsal"] is None and "rehearsal" not in line and line["scaling"] == "weak" and line["value"] > 0


def test_fir_modes_agree(gpu_lib, oracle):
    """The three forms of the envelope FIR (bl_amd_set_fir_mode): mode 0 is the reference's
    arithmetic and must give the oracle's window energies bit for bit; modes 1 and 2 may move an
    energy by one f32 ulp about once per 10^8 windows — here: every integer equal, every float
    feature equal, at most 2 of the ~2.6 million energies one ulp apart."""
    n = 44100 * 2 * 30
    corpus = bliss_amd.DeviceCorpus([n] * 256, 2, 30)
    corpus.synth(seed_base=52000, sample_rate=44100)
    try:
        out = {}
        for mode in (0, 1, 2):
            assert gpu_lib.bl_amd_set_fir_mode(mode) == 0 and gpu_lib.bl_amd_fir_mode() == mode
            corpus.analyze()
            got = corpus.fetch()
            en, offs = _energies(gpu_lib, got)
            out[mode] = (got, en.copy())
        g0, e0 = out[0]
        song = corpus.pcm[int(corpus.desc[7].pcm_offset):int(corpus.desc[7].pcm_offset) + n].cpu().numpy()
        _, ref_en = oracle.envelope(song, 30)
        nw = int(g0[7]["n_windows"])
        assert np.array_equal(e0[offs[7]:offs[7] + nw].view(np.uint32), ref_en[:nw].view(np.uint32))
        for mode in (1, 2):
            g, e = out[mode]
            for k in g.dtype.names:
                assert np.array_equal(g[k], g0[k]), (mode, k)
            d = np.abs(e.view(np.int32).astype(np.int64) - e0.view(np.int32).astype(np.int64))
            assert d.max() <= 1 and np.count_nonzero(d) <= 2, (mode, int(d.max()), int(np.count_nonzero(d)))
    finally:
        gpu_lib.bl_amd_set_fir_mode(-1)
    assert gpu_lib.bl_amd_set_fir_mode(3) == bliss_amd.BL_UNEXPECTED


def test_bench_two_ranks_rehearsal_on_one_gpu(gpu_lib, tmp_path):
    """The N = 2 job of bench.py on a one-GPU box: --share-device puts both ranks on device 0 with a
    gloo group (RCCL refuses two ranks per device).  Everything but the transport is the N-rank code:
    the ranks' shards and seeds (rank 1 analyses songs 24..47), the gather order, row blocks that
    start at row 24, the oracle check shared out over the ranks, results_ok reduced over both."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--share-device", "--steps", "1", "--warmup", "1",
           "--songs-per-gpu", "24", "--seconds", "20", "--full", "--cpu-ladder", "1,8", "--verify", "8", "--no-live-traffic"]
    line, det = _run_bench(cmd, tmp_path)
    assert line["n_gpus"] == 2 and line["results_ok"] is True and line["verified_songs"] == 8
    assert line["collective"] == "gloo" and det["collective"]["all_gather_calls"] >= 2
    assert line["config"]["songs_per_gpu"] == 24 and line["config"]["parallelism"] == "shard2"
    assert "48 total" in line["config"]["workload"] and line["rehearsal"] and det["rehearsal"]
    # an N > 1 line carries what a scaling run needs to be read: the CPU baseline (rank 0, after the timed region)
    # and every rank's own clock (the dominant-kernel times are in the details file)
    assert line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["kind"] == "port" and "rank 0 of 2" in line["cpu_baseline"]["sample"]
    assert len(line["per_rank_ms"]) == 2 and max(line["per_rank_ms"]) <= line["ms_per_step"] * 1.001
    pr = det["per_rank"]
    assert len(pr["ms_per_step"]) == 2 == len(pr["env_windows_ms"]) and min(pr["env_windows_ms"]) > 0
    assert pr["ms_per_step_min"] <= pr["ms_per_step_max"] <= det["ms_per_step"] * 1.001
