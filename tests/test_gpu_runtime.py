"""Runtime behaviour of the C-ABI: explicit contexts driven from two host threads, launch
groups, the asynchronous enqueue, registered vs staged host transfer, 32-bit sources, and the
multi-device corpus entry point (RCCL gather at world size 1, peer gather with two ranks on one
device)."""
import ctypes as C
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

import bliss_amd
from bliss_amd import _lib
from tests.test_gpu_parity import check_song

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _songs(oracle, seed0, count, rate=22050):
    out = []
    for i in range(count):
        ch = 1 + (i % 2)
        secs = 6 + (i * 5) % 9
        out.append((oracle.synth(seed0 + i, rate, ch, rate * ch * secs + 8 * (i % 3)), ch, secs))
    return out


def _same(a, b):
    for k in a.dtype.names:
        assert np.array_equal(a[k], b[k]), k


def test_two_contexts_from_two_threads(gpu_lib, oracle):
    """Two explicit contexts on device 0, each driven by its own host thread on its own stream,
    several rounds concurrently: each keeps its own workspace, results match the oracle."""
    import torch
    dev = torch.device("cuda", 0)
    sets = [_songs(oracle, 4000, 6), _songs(oracle, 4100, 7)]
    out, err = [None, None], []

    def work(t):
        try:
            torch.cuda.set_device(0)
            with bliss_amd.Context(0) as ctx:
                assert gpu_lib.bl_amd_ctx_device(ctx.handle) == 0
                pcms = [p for p, _, _ in sets[t]]
                corpus = bliss_amd.DeviceCorpus([p.size for p in pcms], [c for _, c, _ in sets[t]],
                                                [d for _, _, d in sets[t]])
                for i, p in enumerate(pcms):
                    corpus.upload(i, p)
                stream = torch.cuda.Stream(dev)
                with torch.cuda.stream(stream):
                    for _ in range(5):
                        corpus.analyze(ctx=ctx)
                stream.synchronize()
                out[t] = corpus.fetch()
        except Exception as e:  # surfaced below
            err.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not err, err
    for t in range(2):
        for i, (p, c, d) in enumerate(sets[t]):
            check_song(out[t][i], oracle.analyze(p, c, d), ("ctx", t, i))


def test_entry_points_interleaved_on_two_streams_without_host_sync(gpu_lib, oracle):
    """Synthesis, analysis, levels and timbre of two corpora on the default context, issued twice in a row with the
    stream alternating from call to call and no host synchronisation but the last: twelve record uploads through the
    four pinned slots, and every call takes the workspace over from a call on the other stream.  Every output equals
    what the same calls give with a device synchronisation after each."""
    import torch
    dev = torch.device("cuda", 0)
    xs = _songs(oracle, 4500, 9)
    X = bliss_amd.DeviceCorpus([p.size for p, _, _ in xs], [c for _, c, _ in xs], [d for _, _, d in xs])
    for i, (p, _, _) in enumerate(xs):
        X.upload(i, p)
    ych = [1 + i % 2 for i in range(7)]
    ysec = [6 + (i * 2) % 5 for i in range(7)]
    Y = bliss_amd.DeviceCorpus([22050 * c * s + 8 * (i % 3) for i, (c, s) in enumerate(zip(ych, ysec))], ych, ysec)
    calls = [lambda: Y.synth(seed_base=4600, sample_rate=22050), X.analyze, X.levels, X.timbre, Y.analyze, Y.levels]

    def outputs():
        return [Y.pcm, X.results, X.levels_raw, X.timbre_raw, X.timbre_frames_raw, Y.results, Y.levels_raw]

    def fetch():
        torch.cuda.synchronize()
        y_pcm = Y.pcm.cpu().numpy()   # the songs, not the gaps between them: nothing writes those
        y_pcm = np.concatenate([y_pcm[int(d.pcm_offset):int(d.pcm_offset) + d.n_samples] for d in Y.desc])
        ts, tf = X.fetch_timbre()
        return {"Y.pcm": y_pcm, "X.levels": X.fetch_levels(), "X.timbre": ts, "X.frames": tf,
                "Y.levels": Y.fetch_levels()}, {"X": X.fetch(), "Y": Y.fetch()}

    for f in calls:
        f()
        torch.cuda.synchronize()
    want, want_res = fetch()
    for t in outputs():
        t.view(torch.uint8).fill_(0xAB)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    for k, f in enumerate(calls + calls):
        with torch.cuda.stream(streams[k % 2]):
            f()
    got, got_res = fetch()
    for name in want:
        assert got[name].tobytes() == want[name].tobytes(), name
    for name in want_res:   # field by field: the analysis records carry padding nothing writes
        for k in want_res[name].dtype.names:
            assert got_res[name][k].tobytes() == want_res[name][k].tobytes(), (name, k)
    assert int(want_res["Y"]["status"].max()) == 0 and int(want["Y.levels"]["frames"].min()) > 0
    check_song(got_res["X"][0], oracle.analyze(*xs[0]), "X, song 0")


def test_corpus_owned_outputs(gpu_lib):
    """The output buffers a DeviceCorpus owns, on three short songs: not there before the first call, allocated by it,
    the frame records dropped by timbre(frames=False) and allocated again, and the same bytes from the default context
    and from an explicit one, for levels, timbre and the analysis."""
    corpus = bliss_amd.DeviceCorpus([5120, 5633, 6144], [1, 2, 1], 1)
    corpus.synth(seed_base=8100, sample_rate=22050)
    assert corpus.levels_raw is None and corpus.timbre_raw is None and corpus.timbre_frames_raw is None
    with pytest.raises(RuntimeError):
        corpus.fetch_levels()
    with pytest.raises(RuntimeError):
        corpus.fetch_timbre()
    with bliss_amd.Context(0) as ctx:
        assert corpus.levels() is corpus.levels_raw
        levels = corpus.fetch_levels()
        assert levels["frames"].tolist() == [5120, 2816, 6144] and int(levels["status"].max()) == 0
        corpus.levels_raw.fill_(0xAB)
        corpus.levels(ctx=ctx)
        assert corpus.fetch_levels().tobytes() == levels.tobytes()

        raw_songs, raw_frames = corpus.timbre(frames=True)
        assert raw_songs is corpus.timbre_raw and raw_frames is corpus.timbre_frames_raw
        songs, frames = corpus.fetch_timbre()
        assert songs["frames"].tolist() == [10, 5, 12] and frames.shape == (27,)
        raw_songs, raw_frames = corpus.timbre(frames=False)
        assert raw_songs is corpus.timbre_raw and raw_frames is None and corpus.timbre_frames_raw is None
        only_songs, none = corpus.fetch_timbre()
        assert none is None and only_songs.tobytes() == songs.tobytes()
        for kw in ({}, {"ctx": ctx}):   # the frame records are allocated again, then written over through the context
            corpus.timbre_raw.fill_(0xAB)
            if corpus.timbre_frames_raw is not None:
                corpus.timbre_frames_raw.fill_(0xAB)
            corpus.timbre(frames=True, **kw)
            again_songs, again_frames = corpus.fetch_timbre()
            assert again_songs.tobytes() == songs.tobytes() and again_frames.tobytes() == frames.tobytes(), kw

        corpus.analyze()
        plain = corpus.fetch()
        corpus.results.fill_(0xAB)
        corpus.analyze(ctx=ctx)
        again = corpus.fetch()
        for k in plain.dtype.names:   # field by field: bytes 68..71 of an analysis record are padding, whose value is not defined
            assert again[k].tobytes() == plain[k].tobytes(), k
        assert not (again["status"].view(np.uint32) == 0xABABABAB).any()   # the second call wrote every record


def test_launch_groups_and_async_enqueue(oracle, tmp_path):
    """More songs than one launch group holds (group size lowered through the environment for a
    fresh process) give the same records as a single group; and the device entry point returns
    long before the GPU is done."""
    code = r'''
import sys, time, json
import numpy as np
sys.path.insert(0, %r)
import torch, bliss_amd
n = 22050 * 2 * 7
c = bliss_amd.DeviceCorpus([n + 8 * (i %% 4) for i in range(13)], 2, 7)
c.synth(seed_base=5000, sample_rate=22050)
c.analyze(); r = c.fetch()
big = bliss_amd.DeviceCorpus([44100 * 2 * 30] * 256, 2, 30)
big.synth(seed_base=1, sample_rate=44100)
big.analyze(); torch.cuda.synchronize()
t0 = time.perf_counter(); big.analyze(); t1 = time.perf_counter(); torch.cuda.synchronize(); t2 = time.perf_counter()
np.save(sys.argv[1], r)
print(json.dumps({"enqueue": t1 - t0, "total": t2 - t0}))
''' % ROOT
    outs = {}
    for tag, env in (("one", {}), ("five", {"BL_AMD_GROUP_SONGS": "5"})):
        f = str(tmp_path / f"{tag}.npy")
        r = subprocess.run([sys.executable, "-c", code, f], env=dict(os.environ, **env), text=True,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[tag] = (np.load(f), __import__("json").loads(r.stdout.strip().splitlines()[-1]))
    _same(outs["one"][0], outs["five"][0])
    ref = oracle.analyze(oracle.synth(5012, 22050, 2, 22050 * 2 * 7), 2, 7)
    check_song(outs["five"][0][12], ref, "group-of-5, last song")
    t = outs["one"][1]
    assert t["enqueue"] < 0.5 * t["total"], t     # ~14 ms of kernels behind a sub-millisecond enqueue


_WAVE_SECS = [1, 1, 2, 1, 3, 1, 1, 2, 1, 1, 3, 1, 1]


def _wave_lengths(rate):
    return [rate * (1 + i % 2) * s + 8 * (i % 3) for i, s in enumerate(_WAVE_SECS)]


def _wave_split(lengths, budget):
    """the rule of bl_waves.h: songs in order, padded to 8, as many as fit `budget` samples but at least one"""
    waves, total = [[]], 0
    for i, n in enumerate(lengths):
        padded = (n + 7) & ~7
        if waves[-1] and total + padded > budget:
            waves.append([])
            total = 0
        waves[-1].append(i)
        total += padded
    return waves


def test_host_batch_over_many_waves(oracle, tmp_path):
    """The host batch, staged and registered, from 16- and 32-bit sources, with and without rate conversion, and the
    host forms of levels and timbre, on thirteen songs of 1-3 s: a fresh process whose wave budget is lowered to
    300 000 bytes (6, 9 and 13 waves: both pinned buffers, both arenas and both registration lists are reused, waves of
    several songs and single songs above the budget both occur) gives what a process with the default budget (one wave)
    gives, and what the oracle gives."""
    code = r'''
import sys
import numpy as np
sys.path.insert(0, %r)
import bliss_amd
from tests.oracle_py import Oracle
orc = Oracle()
secs = %r
chans = [1 + i %% 2 for i in range(13)]
def songs(rate):
    return [orc.synth(7000 + i, rate, chans[i], rate * chans[i] * s + 8 * (i %% 3)) for i, s in enumerate(secs)]
def mark(name):
    print("== " + name, file=sys.stderr, flush=True)
lo, hi = songs(22050), songs(44100)
rng = np.random.default_rng(5)
wide = lambda ps: [(p.astype(np.int32) << 16) | rng.integers(0, 65536, p.size, dtype=np.int32) for p in ps]
out = {}
mark("staged"); out["staged"] = bliss_amd.analyze_batch_host(lo, chans, secs)
lib = bliss_amd.load()
assert lib.bl_amd_set_host_transfer(1) == 0
mark("registered"); out["registered"] = bliss_amd.analyze_batch_host(lo, chans, secs)
assert lib.bl_amd_set_host_transfer(0) == 0
mark("s32"); out["s32"] = bliss_amd.analyze_batch_host_s32(wide(lo), chans, secs)
mark("rate16"); out["rate16"] = bliss_amd.analyze_batch_host_rate(hi, chans, secs, 44100)
mark("rate32"); out["rate32"] = bliss_amd.analyze_batch_host_rate(wide(hi), chans, secs, 44100)
mark("levels"); out["levels"] = bliss_amd.levels_batch_host(hi, chans)
mark("timbre"); out["timbre"], out["frames"] = bliss_amd.timbre_batch_host(hi, chans, frames=True)
mark("end")
for k in ("staged", "registered", "s32", "rate16", "rate32"):
    assert int(out[k]["status"].max()) == 0, k
np.savez(sys.argv[1], **out)
''' % (ROOT, _WAVE_SECS)
    budget = 300000
    # the split the lowered process must make: reaches buffer reuse (a slot's third wave is wave 4) and both branches
    split = {name: _wave_split(_wave_lengths(rate), budget // esz)
             for name, rate, esz in (("staged", 22050, 2), ("rate16", 44100, 2), ("rate32", 44100, 4))}
    assert [len(w) for w in split["staged"]] == [3, 2, 2, 2, 2, 2]
    assert [len(w) for w in split["rate16"]] == [2, 1, 1, 1, 2, 1, 2, 1, 2]
    assert [len(w) for w in split["rate32"]] == [1] * 13
    hi = _wave_lengths(44100)
    assert len(split["rate16"]) >= 5 and any(len(w) >= 2 for w in split["rate16"])
    assert any(len(w) == 1 and ((hi[w[0]] + 7) & ~7) > budget // 2 for w in split["rate16"])
    outs, errs = {}, {}
    for tag, env in (("plain", {}), ("waves", {"BL_AMD_HOST_WAVE_BYTES": str(budget), "BL_AMD_HOST_TRACE": "1"})):
        f = str(tmp_path / f"{tag}.npz")
        r = subprocess.run([sys.executable, "-c", code, f], env=dict(os.environ, **env), text=True,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[tag], errs[tag] = np.load(f), r.stderr
    for k in ("staged", "registered", "s32", "rate16", "rate32"):
        _same(outs["plain"][k], outs["waves"][k])
    for k in ("levels", "timbre", "frames"):
        assert outs["plain"][k].tobytes() == outs["waves"][k].tobytes(), k
    _same(outs["waves"]["staged"], outs["waves"]["registered"])
    _same(outs["waves"]["staged"], outs["waves"]["s32"])
    for i in (0, 12):
        ch = 1 + i % 2
        ref = oracle.analyze(oracle.synth(7000 + i, 22050, ch, _wave_lengths(22050)[i]), ch, _WAVE_SECS[i])
        check_song(outs["waves"]["staged"][i], ref, f"song {i}, six waves")
    # the trace lines of each call of the lowered process (the registered form and the levels and timbre print none)
    traced, call = {}, None
    for line in errs["waves"].splitlines():
        if line.startswith("== "):
            call = line[3:]
        elif line.startswith("wave "):
            traced.setdefault(call, []).append(int(line[5:line.index(":")]))
    assert traced["staged"] == list(range(6)), traced
    assert traced["s32"] == list(range(6)), traced
    assert traced["rate16"] == list(range(9)), traced
    assert traced["rate32"] == list(range(13)), traced
    assert set(traced) == {"staged", "s32", "rate16", "rate32"}, traced
    assert "wave 1:" not in errs["plain"]


def test_mixed_batch_with_early_tail_equals_the_plain_path(oracle, tmp_path):
    """A mixed-length group of >= 1 024 songs gives its longest songs their own window launch and starts their serial
    tail under the window kernel of the rest (blk_analyze, n_head).  Same records as the same corpus analysed in
    launch groups too small to be split (fresh process, BL_AMD_GROUP_SONGS=500), and a sample of them against the
    oracle."""
    code = r'''
import sys
import numpy as np
sys.path.insert(0, %r)
import torch, bliss_amd
rng = np.random.default_rng(77)
lengths = np.floor(np.exp(rng.uniform(np.log(6000), np.log(260000), 1400))).astype(np.int64)
chans = rng.integers(1, 3, 1400)
lengths = (lengths // chans) * chans
c = bliss_amd.DeviceCorpus(lengths.tolist(), chans.tolist(), [3] * 1400)
c.synth(seed_base=31000, sample_rate=22050)
c.analyze(); r = c.fetch()
assert int(r["status"].max()) == 0
np.save(sys.argv[1], r)
np.save(sys.argv[1] + ".len.npy", np.stack([lengths, chans]))
''' % ROOT
    outs = {}
    for tag, env in (("split", {}), ("groups", {"BL_AMD_GROUP_SONGS": "500"})):
        f = str(tmp_path / f"{tag}.npy")
        r = subprocess.run([sys.executable, "-c", code, f], env=dict(os.environ, **env), text=True,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[tag] = np.load(f)
    _same(outs["split"], outs["groups"])
    lengths, chans = np.load(str(tmp_path / "split.npy.len.npy"))
    order = np.argsort(-lengths)
    for i in [int(order[0]), int(order[255]), int(order[256]), int(order[700]), int(order[-1])]:
        ref = oracle.analyze(oracle.synth(31000 + i, 22050, int(chans[i]), int(lengths[i])), int(chans[i]), 3)
        check_song(outs["split"][i], ref, f"song {i} of the split batch ({lengths[i]} samples)")


def test_measurement_switches_are_ignored_by_the_product_build(tmp_path):
    """The result-invalidating measurement aids (BL_AMD_SQRT_VARIANT=3: the distance kernel's store stream alone,
    BL_AMD_NO_SIDE, BL_AMD_FUSED_SCAN, and the round-3 switches BL_AMD_ENV_DBG / BL_AMD_ENV_OLD, whose code is gone) only exist in `make measure` builds
    (-DBL_AMD_MEASURE); the shipped library must give the same records, window energies and distance matrix
    whether those variables are set or not."""
    code = r'''
import sys, hashlib
import numpy as np
sys.path.insert(0, %r)
import torch, bliss_amd
lengths = [22050 * 2 * 9 + 8 * i for i in range(5)] + [5120, 6000, 22050 * 1 * 40, 44100 * 2 * 33]
chans = [2, 2, 2, 2, 2, 2, 1, 1, 2]
c = bliss_amd.DeviceCorpus(lengths, chans, 9)
c.synth(seed_base=900, sample_rate=22050)
c.analyze(); r = c.fetch()
np.save(sys.argv[1], r)
lib = bliss_amd.load()
import ctypes as C
buf = (C.c_float * 400000)()
n = lib.bl_amd_last_energies(buf, 400000)
e = np.frombuffer(bytes(buf), dtype=np.float32)[: max(n, 0)]
# a song owns nb_frames slots and fills the first n_windows of them; the other two are never written
valid, off = [], 0
for nb, nw in zip(r["nb_frames"], r["n_windows"]):
    valid.append(e[off:off + int(nw)]); off += int(nb)
assert off == n
vecs = np.stack([r["tempo"], r["amplitude"], r["frequency"], r["attack"]], axis=1).astype(np.float32)
d = bliss_amd.distance_matrix(vecs)
print(n, hashlib.md5(np.concatenate(valid).tobytes()).hexdigest(), hashlib.md5(np.ascontiguousarray(d).tobytes()).hexdigest())
''' % ROOT
    outs = {}
    switches = {"BL_AMD_SQRT_VARIANT": "3", "BL_AMD_ENV_DBG": "3", "BL_AMD_ENV_OLD": "1", "BL_AMD_NO_SIDE": "1",
                "BL_AMD_FUSED_SCAN": "0"}
    for tag, env in (("plain", {}), ("switches", switches)):
        f = str(tmp_path / f"{tag}.npy")
        r = subprocess.run([sys.executable, "-c", code, f], env=dict(os.environ, **env), text=True,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[tag] = (np.load(f), r.stdout.strip().splitlines()[-1])
    _same(outs["plain"][0], outs["switches"][0])
    assert outs["plain"][1] == outs["switches"][1] and not outs["plain"][1].startswith("0 "), outs


def test_host_transfer_modes_and_s32(gpu_lib, oracle):
    songs = _songs(oracle, 4300, 9)
    pcms, chans, durs = [p for p, _, _ in songs], [c for _, c, _ in songs], [d for _, _, d in songs]
    staged = bliss_amd.analyze_batch_host(pcms, chans, durs)
    assert gpu_lib.bl_amd_set_host_transfer(1) == 0            # hipHostRegister on the caller's buffers
    try:
        reg = bliss_amd.analyze_batch_host(pcms, chans, durs)
    finally:
        assert gpu_lib.bl_amd_set_host_transfer(0) == 0
    _same(staged, reg)
    assert pcms[0][0] == oracle.synth(4300, 22050, 1, 1)[0]    # the caller's memory is still its own
    # 32-bit sources: narrowed by the library (host staging and device kernel), oracle gets numpy's >> 16
    rng = np.random.default_rng(2)
    s32 = [(p.astype(np.int32) << 16) | rng.integers(0, 65536, p.size, dtype=np.int32) for p in pcms]
    got = bliss_amd.analyze_batch_host_s32(s32, chans, durs)
    _same(staged, got)
    corpus = bliss_amd.DeviceCorpus([p.size for p in pcms], chans, durs)
    for i, q in enumerate(s32):
        corpus.upload_s32(i, q)
    corpus.analyze()
    _same(staged, corpus.fetch())
    for i in (0, 4, 8):
        check_song(got[i], oracle.analyze((s32[i] >> 16).astype(np.int16), chans[i], durs[i]), ("s32", i))
    odd = np.arange(-70000, 70001, 7, dtype=np.int32) * 30011   # unaligned views through the scalar path
    import torch
    t = torch.from_numpy(odd).cuda()
    o = torch.zeros(odd.size + 3, dtype=torch.int16, device="cuda")
    assert gpu_lib.bl_amd_narrow_s32_device(C.c_void_p(t.data_ptr() + 4), C.c_void_p(o.data_ptr() + 2),
                                            odd.size - 1, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(o.cpu().numpy()[1:odd.size], (odd[1:] >> 16).astype(np.int16))


def test_invalid_host_descriptors_fail_before_staging(gpu_lib):
    good = np.ones(8192, dtype=np.int16)
    ptrs = (C.c_void_p * 2)(good.ctypes.data, None)
    ns = (C.c_int32 * 2)(8192, 8192)
    ch = (C.c_int32 * 2)(1, 1)
    du = (C.c_uint64 * 2)(1, 1)
    out = (_lib.SongResult * 2)()
    assert gpu_lib.bl_amd_analyze_batch_host(ptrs, ns, ch, du, 2, out) == _lib.BL_UNEXPECTED   # NULL buffer
    ptrs[1] = good.ctypes.data
    ns[1] = -5
    assert gpu_lib.bl_amd_analyze_batch_host(ptrs, ns, ch, du, 2, out) == _lib.BL_UNEXPECTED   # negative length


def _all_devices():
    import torch
    return list(range(torch.cuda.device_count()))


def _check_corpus_multi(oracle, devices, gather):
    songs = _songs(oracle, 4500, 11)
    for equal in (False, True):
        use = songs if not equal else [(oracle.synth(4600 + i, 22050, 2, 22050 * 2 * 6), 2, 6) for i in range(7)]
        pcms, chans, durs = [p for p, _, _ in use], [c for _, c, _ in use], [d for _, _, d in use]
        res, mat = bliss_amd.analyze_corpus_multi(pcms, chans, durs, devices, gather=gather)
        single = bliss_amd.analyze_batch_host(pcms, chans, durs)
        _same(single, res)
        fv = np.stack([single[k] for k in ("tempo", "amplitude", "frequency", "attack")], axis=1)
        assert np.array_equal(mat, bliss_amd.distance_matrix(fv))
        assert np.array_equal(mat, oracle.distance_matrix(fv))
    res2, none = bliss_amd.analyze_corpus_multi(pcms, chans, durs, devices, gather=gather, matrix=False)
    _same(res, res2)
    assert none is None


@pytest.mark.parametrize("devices,gather", [([0], "rccl"), ([0], "peer"), ([0, 0], "peer"), ([0, 0, 0], "peer")])
def test_corpus_multi(gpu_lib, oracle, devices, gather):
    """The C-ABI batch-of-songs mode.  RCCL (ncclCommInitAll + ncclAllGather) runs at world size
    1; the peer gather also takes several ranks on one device, which exercises the sharding, the
    per-rank contexts and threads, the exchange and the row-block matrix with W = 2, 3."""
    _check_corpus_multi(oracle, devices, gather)


@pytest.mark.parametrize("gather", ["rccl", "peer"])
def test_corpus_multi_on_every_device(gpu_lib, oracle, gather):
    """The same on every HIP device the box has, one rank per device: ncclCommInitAll over N devices and an
    ncclAllGather that crosses xGMI, or hipMemcpyPeerAsync between devices.  Skipped on a one-GPU box; on an N-GPU
    box it runs without an edit."""
    devices = _all_devices()
    if len(devices) < 2:
        pytest.skip("one HIP device on this box: W > 1 is covered on device 0 by test_corpus_multi")
    _check_corpus_multi(oracle, devices, gather)
    _check_corpus_multi(oracle, devices[::-1], gather)     # rank r need not sit on device r


def _check_corpus_multi_device_resident(oracle, counts, gather, devices=None):
    import torch
    devices = devices or [0] * len(counts)
    songs = _songs(oracle, 4700, sum(counts))
    pcms, chans, durs = [p for p, _, _ in songs], [c for _, c, _ in songs], [d for _, _, d in songs]
    whole = bliss_amd.DeviceCorpus([p.size for p in pcms], chans, durs)
    for i, p in enumerate(pcms):
        whole.upload(i, p)
    whole.analyze()
    single = whole.fetch()
    fv = np.stack([single[k] for k in ("tempo", "amplitude", "frequency", "attack")], axis=1)
    want = bliss_amd.distance_matrix(fv)
    corpora, first = [], 0
    for cnt, d in zip(counts, devices):
        part = range(first, first + cnt)
        c = bliss_amd.DeviceCorpus([pcms[i].size for i in part] or [8], [chans[i] for i in part] or [1],
                                   [durs[i] for i in part] or [1], device=f"cuda:{d}")
        if cnt == 0:
            c.n_songs = 0          # an empty shard: the arena exists, nothing to analyse
        for k, i in enumerate(part):
            c.upload(k, pcms[i])
        corpora.append(c)
        first += cnt
    for _ in range(2):             # second call: the contexts' exchange buffers are reused
        res, mat, rows = bliss_amd.analyze_corpus_multi_device(corpora, gather=gather, keep_rows=True)
        _same(single, res)
        assert np.array_equal(mat, want) and np.array_equal(mat, oracle.distance_matrix(fv))
        for d in set(devices):
            torch.cuda.synchronize(d)
        assert np.array_equal(np.concatenate([r.cpu().numpy() for r in rows], axis=0), want)
    # the shard's own device records are the same records
    off = 0
    for c in corpora:
        if c.n_songs:
            _same(single[off:off + c.n_songs], c.fetch()[:c.n_songs])
        off += c.n_songs
    res2, none, _ = bliss_amd.analyze_corpus_multi_device(corpora, gather=gather, matrix=False)
    _same(single, res2)
    assert none is None


@pytest.mark.parametrize("counts,gather", [((5,), "rccl"), ((4, 3), "peer"), ((3, 0, 4), "peer"), ((2, 3, 2), "peer")])
def test_corpus_multi_device_resident(gpu_lib, oracle, counts, gather):
    """bl_amd_analyze_corpus_multi_device: the corpus already resident, one arena per rank (here
    all on device 0, separate contexts and host threads; an empty shard included).  Records and
    matrix must equal the single-context path bit for bit, the row blocks left in HBM too."""
    _check_corpus_multi_device_resident(oracle, counts, gather)


@pytest.mark.parametrize("gather", ["rccl", "peer"])
def test_corpus_multi_device_resident_on_every_device(gpu_lib, oracle, gather):
    """One resident shard per HIP device of the box (uneven counts, the last but one empty when there are more than
    two): the vectors cross xGMI by RCCL or by peer copies, every device computes its own row block.  Skipped on a
    one-GPU box."""
    devices = _all_devices()
    if len(devices) < 2:
        pytest.skip("one HIP device on this box: W > 1 is covered on device 0 by test_corpus_multi_device_resident")
    counts = [3 + (d % 3) for d in devices]
    if len(devices) > 2:
        counts[-2] = 0
    _check_corpus_multi_device_resident(oracle, tuple(counts), gather, devices)


def test_scalar_helpers_match_the_kernels(gpu_lib):
    """bl_distance / bl_cosine_similarity of one pair are host arithmetic (bl_api.c): the same
    bits as the all-pairs kernels."""
    rng = np.random.default_rng(31)
    v = (rng.standard_normal((300, 4)) * 9).astype(np.float32)
    dm, cm = bliss_amd.distance_matrix(v), bliss_amd.cosine_matrix(v)
    for i, j in rng.integers(0, 300, (400, 2)):
        a, b = _lib.ForceVector(*v[i]), _lib.ForceVector(*v[j])
        assert gpu_lib.bl_distance(a, b) == dm[i, j]
        assert gpu_lib.bl_cosine_similarity(a, b) == cm[i, j]


def test_analyze_files_equals_the_per_file_loop(gpu_lib, oracle, tmp_path):
    """bl_amd_analyze_files(filenames, ...) is `for f: bl_analyze(f, &song)` with the decoding on host
    threads and the songs batched to the GPU: every song struct — force vector, force, calm_or_loud,
    metadata — equals what the one-file call gives, bit for bit; a missing file and a clip that is
    too short are reported per file and do not stop the rest."""
    import shutil
    from tests.test_ingest import write_flac_verbatim, _write_wav16
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    files = []
    for name in ("song.flac", "song_s32.flac", "song_s32_mono.flac"):
        dst = tmp_path / name
        shutil.copy(os.path.join(gold, name), dst)
        files.append(str(dst))
    for i in range(9):
        rate, ch, secs = (22050, 44100, 48000)[i % 3], 1 + (i % 2), 5 + i % 5   # the test FLAC writer stops at 128 frames of 4096
        pcm = oracle.synth(6100 + i, rate, ch, rate * ch * secs)
        f = tmp_path / f"synth{i}.{'flac' if i % 2 else 'wav'}"
        if i % 2:
            write_flac_verbatim(f, pcm, ch, rate, 16)
        else:
            _write_wav16(f, pcm, ch, rate)
        files.append(str(f))
    missing = str(tmp_path / "missing.flac")
    short = tmp_path / "short.wav"
    _write_wav16(short, oracle.synth(1, 22050, 2, 3000), 2, 22050)
    order = files[:5] + [missing] + files[5:9] + [str(short)] + files[9:]
    recs, codes = bliss_amd.analyze_files(order, n_threads=4)
    assert len(recs) == len(order) == 14
    n_ok = 0
    for f, rec, code in zip(order, recs, codes):
        song = _lib.BlSong()
        rc = gpu_lib.bl_analyze(f.encode(), C.byref(song))
        assert rc == code, f
        if rc == _lib.BL_UNEXPECTED:
            assert rec is None and f in (missing, str(short))
            gpu_lib.bl_free_song(C.byref(song))   # bl_analyze leaves a decoded-but-unanalysable song allocated
            continue
        n_ok += 1
        for k in ("tempo", "amplitude", "frequency", "attack"):
            assert rec["force_vector"][k] == getattr(song.force_vector, k), (f, k)
        assert rec["force"] == song.force and rec["calm_or_loud"] == song.calm_or_loud
        for k in ("channels", "nSamples", "sample_rate", "bitrate", "nb_bytes_per_sample", "resampled", "duration"):
            assert rec[k] == getattr(song, k), (f, k)
        assert rec["title"] == song.title.decode() and rec["filename"] == f
        gpu_lib.bl_free_song(C.byref(song))
    assert n_ok == 12
    # keep_pcm: the decoded samples stay with the song
    recs2, _ = bliss_amd.analyze_files(order[:2], n_threads=1, keep_pcm=True)
    assert recs2[0]["pcm"].size == recs2[0]["nSamples"] == 488138
    # a NULL name among the files, song structs full of garbage (callers pass uninitialised structs, ref
    # tests/test_analyze.c:27-28): reported for that file only, every pointer field NULL afterwards
    names = (C.c_char_p * 3)(order[0].encode(), None, order[1].encode())
    songs = (_lib.BlSong * 3)()
    C.memset(songs, 0xAB, C.sizeof(songs))
    codes3 = (C.c_int * 3)()
    assert gpu_lib.bl_amd_analyze_files(names, 3, songs, codes3, 2, 0) == 2
    assert codes3[1] == _lib.BL_UNEXPECTED and codes3[0] == codes[0] and codes3[2] == codes[1]
    assert not songs[1].sample_array and songs[1].title is None and songs[1].filename is None
    assert songs[0].force_vector.tempo == recs[0]["force_vector"]["tempo"]
    for sg in songs:
        gpu_lib.bl_free_song(C.byref(sg))
