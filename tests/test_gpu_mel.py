"""Mel bands, cepstrum and flatness on the GPU (bl_amd_mel_batch_device, bl_amd_ctx_mel_batch_device,
bl_amd_mel_batch_host, bl_amd_selftest_ilog2, bliss_amd.mel): every field of bl_amd_frame_mel and bl_amd_song_mel and
every band level is an exact integer and is compared with == against tests/mel_reference.py, the Python-int restatement
of the header's definitions on top of tests/freq_reference.py's per-frame power values.  There is no tolerance anywhere.

A wave takes 8 frames per iteration and a workgroup 32, so the songs are 1, 7, 8, 9, 31, 32, 33, 64, 65 and 100 frames
long, mono and stereo, in one mixed batch.  Every arena is filled with 32767 before the songs are placed and the
outputs with 0xA5 before the call, with 64 more bytes behind each, so a read outside a song's whole frames, a field the
kernel does not write and a write behind an output all show."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import bliss_amd
import bliss_amd.descriptor
import bliss_amd.mel as M
from bliss_amd import _lib
from bliss_amd.records import FRAME_MEL_DTYPE, MEL_DTYPE, RESULT_DTYPE
from tests import freq_reference as fr
from tests import mel_reference as mr
from tests import timbre_reference as tr

pytestmark = pytest.mark.gpu

U = _lib.BL_UNEXPECTED
W = 512
SENTINEL = 0xA5
TAIL = 64
LENGTHS = (1, 7, 8, 9, 31, 32, 33, 64, 65, 100)
SONG_LISTS = ("mfcc_sum", "mfcc_sumsq", "band_sum")
SONG_SCALARS = ("flat_sum", "flat_sumsq", "frames", "used", "status", "reserved")


# ---- running the library -----------------------------------------------------------------------------------------

def frames_of(n, ch):
    return (n // ch) // W


def place(songs, offsets=None):
    """(torch int16 arena filled with 32767, list of (pcm_offset, n_samples, channels)): the songs at multiples of 8
    samples one behind the other, or at `offsets`"""
    import torch
    items, off = [], 0
    for i, (pcm, ch) in enumerate(songs):
        at = offsets[i] if offsets is not None else off
        items.append((at, pcm.size, ch))
        off = at + ((pcm.size + 7) & ~7)
    end = max(at + n for at, n, _ in items)
    host = np.full(end + 64, 32767, dtype=np.int16)
    for (at, n, _), (pcm, _) in zip(items, songs):
        host[at:at + n] = pcm
    return torch.from_numpy(host).cuda(), items


def call(lib, arena, items, min_energy=0, want_frames=True, want_bands=True, ctx=None, n_records=None, fill=SENTINEL):
    """(return code, song records, frame records or None, band levels or None) of one call whose outputs, and TAIL
    bytes behind each, were filled with `fill`; the tails are checked here"""
    import torch
    n = len(items)
    desc = (_lib.SongDesc * max(n, 1))()
    for i, (at, ns, ch) in enumerate(items):
        desc[i].pcm_offset, desc[i].n_samples, desc[i].channels, desc[i].duration = at, ns, ch, 77 + i
    total = sum(max(frames_of(ns, ch), 0) if ch in (1, 2) else 0 for _, ns, ch in items)
    sizes = (max(n, 1) * 496, max(total, 1) * 56, max(total, 1) * 128)
    so, fo, bo = (torch.full((sz + TAIL,), fill, dtype=torch.uint8, device="cuda") for sz in sizes)
    args = (C.c_void_p(arena.data_ptr()), desc, n, min_energy, C.c_void_p(so.data_ptr()),
            C.c_void_p(fo.data_ptr()) if want_frames else None, C.c_void_p(bo.data_ptr()) if want_bands else None,
            total if n_records is None else n_records, None)
    rc = (lib.bl_amd_mel_batch_device(*args) if ctx is None else lib.bl_amd_ctx_mel_batch_device(ctx.handle, *args))
    torch.cuda.synchronize()
    raw = [t.cpu().numpy().tobytes() for t in (so, fo, bo)]
    for r, sz, wanted in zip(raw, sizes, (True, want_frames, want_bands)):
        assert r[sz:] == bytes([fill]) * TAIL, "a write behind an output"
        assert wanted or r == bytes([fill]) * (sz + TAIL), "a write into an output that was not passed"
    songs = np.frombuffer(raw[0], dtype=MEL_DTYPE, count=max(n, 1))[:n]
    frames = np.frombuffer(raw[1], dtype=FRAME_MEL_DTYPE, count=max(total, 1))[:total] if want_frames else None
    bands = np.frombuffer(raw[2], dtype=np.uint32, count=max(total, 1) * 32).reshape(-1, 32)[:total] if want_bands else None
    return rc, songs, frames, bands


def run(lib, songs, **kw):
    arena, items = place(songs)
    rc, so, fo, bo = call(lib, arena, items, **kw)
    assert rc == 0
    return so, fo, bo


# ---- the reference, computed once per song and shared ------------------------------------------------------------

class Reference:
    """the frames of a song by tests/mel_reference.py, cached by the song's bytes; song records for any min_energy"""

    def __init__(self, oracle):
        self.oracle = oracle
        self.frames = {}

    def records(self, pcm, ch, min_energy=0):
        k = (np.asarray(pcm).tobytes()[:frames_of(pcm.size, ch) * W * ch * 2], ch)
        if k not in self.frames:
            self.frames[k] = [mr.frame_record(row) for row in tr.power_of(self.oracle, pcm, ch)]
        return self.frames[k], mr.song_record(self.frames[k], min_energy)


@pytest.fixture(scope="module")
def ref(oracle):
    return Reference(oracle)


def assert_equal(got, songs, ref, min_energy=0, what=""):
    so, fo, bo = got
    at = 0
    for i, (pcm, ch) in enumerate(songs):
        frames, rec = ref.records(pcm, ch, min_energy)
        F = len(frames)
        where = f"{what} song {i} ({ch} ch, F {F}, min_energy {min_energy})"
        for name in SONG_LISTS:
            g = [int(x) for x in so[name][i]]
            assert g == rec[name], f"{where}: {name} {g}, want {rec[name]}"
        for name in SONG_SCALARS:
            assert int(so[name][i]) == rec[name], f"{where}: {name} {int(so[name][i])}, want {rec[name]}"
        for arr, key in ((None if fo is None else fo["mfcc"], "mfcc"), (None if fo is None else fo["flat"], "flat"),
                         (bo, "E")):
            if arr is None:
                continue
            g = np.asarray(arr[at:at + F]).astype(np.int64).reshape(F, -1)
            want = np.array([f[key] for f in frames], dtype=np.int64).reshape(F, -1)
            if not np.array_equal(g, want):
                t, k = (int(v[0]) for v in np.nonzero(g != want))
                raise AssertionError(f"{where}: frame {t} (mod 32: {t % 32}, mod 8: {t % 8}) {key}[{k}] {g[t, k]}, want "
                                     f"{want[t, k]}; {int((g != want).any(axis=1).sum())} frames differ")
        at += F
    for arr in (fo, bo):
        assert arr is None or at == arr.shape[0]


# ---- material ----------------------------------------------------------------------------------------------------

def noise(rng, n, amp):
    return rng.integers(-amp, amp + 1, n).astype(np.int16)


@functools.lru_cache(maxsize=None)
def standard_songs():
    """mono and stereo at every length that matters, noise at amplitudes 1, 30 and 30 000 (small S, where S + 1 matters,
    and negative coefficients, where the floor of the shift matters), with 0, 1 or 511 samples behind the last frame"""
    rng = np.random.default_rng(61)
    out = []
    for i, F in enumerate(LENGTHS):
        for ch in (1, 2):
            extra = (0, 1, W * ch - 1)[(i + ch) % 3]
            out.append((noise(rng, F * W * ch + extra, (1, 30, 30000)[(i + ch) % 3]), ch))
    return tuple(out)


def band_tone(b, level, n_frames=1):
    """a sine at the centre of band b (edge b + 1, in sixteenths of a bin)"""
    n = np.arange(n_frames * W)
    return np.rint(level * np.sin(2 * np.pi * (mr.EDGES[b + 1] / 16.0) * n / W))


@functools.lru_cache(maxsize=None)
def tone_ladder():
    """mono, F = 100: frame t a sine at the centre of band t mod 32 whose level cycles over 30, 1 000 and 32 767; stereo,
    F = 33: the same tone on both channels, bands downwards"""
    mono = np.concatenate([band_tone(t % 32, (30, 1000, 32767)[t % 3]) for t in range(100)])
    both = np.concatenate([band_tone(31 - t % 32, (32767, 1000)[t % 2]) for t in range(33)])
    return ((mono.astype(np.int16), 1), (np.repeat(both.astype(np.int16), 2), 2))


@functools.lru_cache(maxsize=None)
def extremes():
    rng = np.random.default_rng(63)
    F = 9
    n = np.arange(F * W)
    square = np.where(n % 128 < 64, 32767, -32768).astype(np.int16)
    gap = noise(rng, 33 * W * 2 + 5, 3000)
    gap[10 * W * 2:20 * W * 2] = 0
    return (
        (np.zeros(F * W, np.int16), 1),                                # silence: every field 0
        (np.zeros(F * W * 2 + 3, np.int16), 2),
        (square, 1),                                                   # energy ~ 2^49.6: the largest S
        (np.repeat(square, 2), 2),
        (np.full(F * W, -32768, np.int16), 1),                         # 2^48 in bin 1, which no band takes
        (np.full(F * W * 2, -32768, np.int16), 2),
        (rng.choice(np.array([-1, 1], np.int16), F * W), 1),           # +-1 noise
        (gap, 2),                                                      # used < frames
    )


def everything():
    return list(standard_songs()) + list(extremes()) + list(tone_ladder())


# ---- tests -------------------------------------------------------------------------------------------------------

def test_every_length_mono_and_stereo_in_one_mixed_batch(gpu_lib, ref):
    songs = list(standard_songs())
    got = run(gpu_lib, songs)
    assert_equal(got, songs, ref, what="standard")
    so, fo, bo = got
    assert [int(x) for x in so["frames"]] == [F for F in LENGTHS for _ in (1, 2)]
    assert int(fo["mfcc"].min()) < 0 and int(so["mfcc_sum"].min()) < 0      # the floor of a negative sum was compared
    plus1 = [f for pcm, ch in songs for f in ref.records(pcm, ch)[0]
             if any(mr.ilog2(s + 1) != mr.ilog2(s) for s in f["S"] if s > 0)]
    assert len(plus1) > 20                                                  # frames on which S + 1 for S shows
    assert int(so["used"].min()) > 0


def test_silence_square_wave_and_constant_minus_32768(gpu_lib, ref):
    songs = list(extremes())
    got = run(gpu_lib, songs)
    assert_equal(got, songs, ref, what="extremes")
    so, fo, bo = got
    for i in (0, 1):                                                        # silence
        assert so[i].tobytes()[:480] == bytes(480) and int(so["used"][i]) == 0 and int(so["frames"][i]) == 9
    assert fo[:18].tobytes() == bytes(18 * 56) and bo[:18].tobytes() == bytes(18 * 128)
    loud = ref.records(*songs[2])[0]
    assert 2 ** 49 < max(f["energy"] for f in loud) < 2 ** 50 and 2 ** 53 < max(max(f["S"]) for f in loud) < 2 ** 56
    const = ref.records(*songs[4])[0]
    assert max(f["energy"] for f in const) > 2 ** 47 and int(so["used"][4]) == 9     # used although no band takes bin 1
    assert 0 < int(so["used"][7]) == int(so["frames"][7]) - 10


def test_tone_ladder_makes_every_band_the_strongest_of_some_frame(gpu_lib, ref):
    songs = list(tone_ladder())
    got = run(gpu_lib, songs)
    assert_equal(got, songs, ref, what="ladder")
    for (pcm, ch), F in zip(songs, (100, 33)):
        frames = ref.records(pcm, ch)[0]
        strongest = [f["E"].index(max(f["E"])) for f in frames]
        assert len(frames) == F and set(strongest) == set(range(32)), sorted(set(range(32)) - set(strongest))
    mono = ref.records(*songs[0])[0]
    assert [f["E"].index(max(f["E"])) for f in mono] == [t % 32 for t in range(100)]      # a pure tone does it
    bo = got[2]
    assert [int(np.argmax(row)) for row in bo[:100]] == [t % 32 for t in range(100)]


def test_min_energy_between_two_frames_and_exactly_on_one(gpu_lib, ref):
    songs = [standard_songs()[18], standard_songs()[13], extremes()[7], tone_ladder()[0]]
    energies = sorted({f["energy"] for pcm, ch in songs for f in ref.records(pcm, ch)[0] if f["energy"] > 0})
    lo, hi = energies[len(energies) // 2], energies[len(energies) // 2 + 1]
    assert lo + 1 < hi
    used = {}
    for min_energy in (0, 1, lo, lo + 1, hi, 2 ** 63):
        got = run(gpu_lib, songs, min_energy=min_energy)
        assert_equal(got, songs, ref, min_energy=min_energy, what="min_energy")
        used[min_energy] = int(got[0]["used"].sum())
    assert used[0] == used[1] > used[lo] == used[lo + 1] + 1 == used[hi] + 1 and used[2 ** 63] == 0


def test_one_song_alone_equals_the_same_song_in_a_batch_of_37_and_in_reversed_order(gpu_lib, ref):
    pool = (everything() * 2)[:36]
    for song in (tone_ladder()[1], standard_songs()[5], extremes()[7]):
        alone = run(gpu_lib, [song])
        for pos in (0, 17, 36):
            batch = pool[:pos] + [song] + pool[pos:]
            assert len(batch) == 37
            for order in (batch, batch[::-1]):
                so, fo, bo = run(gpu_lib, order)
                p = pos if order is batch else 36 - pos
                at = sum(frames_of(q.size, c) for q, c in order[:p])
                assert so[p].tobytes() == alone[0][0].tobytes()
                assert fo[at:at + alone[1].size].tobytes() == alone[1].tobytes()
                assert bo[at:at + alone[1].size].tobytes() == alone[2].tobytes()
    assert_equal((so, fo, bo), order, ref, what="batch of 37, reversed")


def test_pcm_offsets_8_and_4104(gpu_lib, ref):
    song = standard_songs()[11]
    got = []
    for off in (8, 4104):
        arena, items = place([song], offsets=[off])
        rc, so, fo, bo = call(gpu_lib, arena, items)
        assert rc == 0
        assert_equal((so, fo, bo), [song], ref, what=f"offset {off}")
        got.append((so.tobytes(), fo.tobytes(), bo.tobytes()))
    assert got[0] == got[1]


def test_every_combination_of_the_frame_outputs_gives_the_same_song_records(gpu_lib, ref):
    songs = everything()
    so, fo, bo = run(gpu_lib, songs)
    assert_equal((so, fo, bo), songs, ref, what="everything")
    for wf, wb in ((True, False), (False, True), (False, False)):
        so2, fo2, bo2 = run(gpu_lib, songs, want_frames=wf, want_bands=wb)
        assert so2.tobytes() == so.tobytes()
        assert (fo2 is None) == (not wf) and (bo2 is None) == (not wb)
        assert fo2 is None or fo2.tobytes() == fo.tobytes()
        assert bo2 is None or bo2.tobytes() == bo.tobytes()
    # n_frame_records is ignored without a frame output
    arena, items = place(songs)
    rc, so3, _, _ = call(gpu_lib, arena, items, want_frames=False, want_bands=False, n_records=-5)
    assert rc == 0 and so3.tobytes() == so.tobytes()


def test_second_context_equals_the_default_one(gpu_lib, ref):
    songs = everything()
    so, fo, bo = run(gpu_lib, songs)
    with bliss_amd.Context(0) as ctx:
        so2, fo2, bo2 = run(gpu_lib, songs, ctx=ctx)
        got3 = run(gpu_lib, songs[:8], ctx=ctx, min_energy=1000)
    assert so2.tobytes() == so.tobytes() and fo2.tobytes() == fo.tobytes() and bo2.tobytes() == bo.tobytes()
    assert_equal(got3, songs[:8], ref, min_energy=1000, what="ctx")


def test_outputs_are_fully_overwritten(gpu_lib):
    songs = everything()
    so, fo, bo = run(gpu_lib, songs)        # all three were filled with 0xA5, and call() looked behind them
    assert int(so["reserved"].max()) == 0 and int(so["status"].max()) == 0
    so0, fo0, bo0 = run(gpu_lib, songs, fill=0x00)
    assert so0.tobytes() == so.tobytes() and fo0.tobytes() == fo.tobytes() and bo0.tobytes() == bo.tobytes()


def test_rejections_write_nothing(gpu_lib):
    rng = np.random.default_rng(67)
    songs = [(noise(rng, 2048, 3000), 2), (noise(rng, 1030, 3000), 1)]
    arena, items = place(songs)
    assert call(gpu_lib, arena, items)[0] == 0
    bad = [
        dict(n_records=3), dict(n_records=5), dict(n_records=3, want_frames=False), dict(n_records=5, want_bands=False),
        dict(items=[(0, 2048, 3), items[1]]),                       # channels 3
        dict(items=[items[0], (2048, 511, 1)]),                     # F = 0
        dict(items=[items[0], (2049, 1030, 1)]),                    # an odd pcm_offset
        dict(items=[items[0], (2052, 1030, 1)]),
        dict(items=[]),                                             # n_songs = 0
    ]
    for kw in bad:
        kw = dict(kw)
        its = kw.pop("items", items)
        if "n_records" not in kw:
            kw["n_records"] = sum(frames_of(n, c) for _, n, c in its if c in (1, 2))
        rc, so, fo, bo = call(gpu_lib, arena, its, **kw)
        assert rc == U, kw
        for t in (so, fo, bo):
            assert t is None or t.tobytes() == bytes([SENTINEL]) * t.nbytes, kw
    # NULL pointers and a misaligned arena
    import torch
    desc = (_lib.SongDesc * 2)()
    for i, (at, ns, ch) in enumerate(items):
        desc[i].pcm_offset, desc[i].n_samples, desc[i].channels = at, ns, ch
    so = torch.full((2 * 496,), SENTINEL, dtype=torch.uint8, device="cuda")
    fo = torch.full((4 * 56,), SENTINEL, dtype=torch.uint8, device="cuda")
    bo = torch.full((4 * 128,), SENTINEL, dtype=torch.uint8, device="cuda")
    p, s, f, b = arena.data_ptr(), so.data_ptr(), fo.data_ptr(), bo.data_ptr()
    fn = gpu_lib.bl_amd_mel_batch_device
    assert fn(None, desc, 2, 0, s, f, b, 4, None) == U
    assert fn(p, None, 2, 0, s, f, b, 4, None) == U
    assert fn(p, desc, 2, 0, None, f, b, 4, None) == U
    assert fn(p + 8, desc, 2, 0, s, f, b, 4, None) == U
    assert fn(p, desc, 2, 0, s + 4, f, b, 4, None) == U
    assert fn(p, desc, 2, 0, s, f + 2, b, 4, None) == U
    assert fn(p, desc, 2, 0, s, f, b + 2, 4, None) == U
    assert gpu_lib.bl_amd_ctx_mel_batch_device(None, p, desc, 2, 0, s, f, b, 4, None) == U
    torch.cuda.synchronize()
    for t in (so, fo, bo):
        assert bytes(t.cpu().numpy()) == bytes([SENTINEL]) * t.numel()


def test_selftest_ilog2(gpu_lib):
    counts = (C.c_uint64 * 2)(7, 7)
    assert gpu_lib.bl_amd_selftest_ilog2(counts) == 0
    assert list(counts) == [192 + 2 ** 17 - 1, 0]
    assert gpu_lib.bl_amd_selftest_ilog2(None) == 0


def test_host_form_and_python_wrappers(gpu_lib, ref):
    songs = everything()
    so, fo, bo = run(gpu_lib, songs, min_energy=1000)
    n = len(songs)
    ptrs = (C.c_void_p * n)(*[p.ctypes.data for p, _ in songs])
    ns = (C.c_int32 * n)(*[p.size for p, _ in songs])
    chs = (C.c_int32 * n)(*[c for _, c in songs])
    hs, hf, hb = (_lib.SongMel * n)(), (_lib.FrameMel * fo.size)(), (C.c_uint32 * (32 * fo.size))()
    for buf in (hs, hf, hb):
        C.memset(buf, SENTINEL, C.sizeof(buf))
    assert gpu_lib.bl_amd_mel_batch_host(ptrs, ns, chs, n, 1000, hs, hf, hb) == 0
    assert bytes(hs) == so.tobytes() and bytes(hf) == fo.tobytes() and bytes(hb) == bo.tobytes()
    C.memset(hs, SENTINEL, C.sizeof(hs))
    assert gpu_lib.bl_amd_mel_batch_host(ptrs, ns, chs, n, 1000, hs, None, None) == 0
    assert bytes(hs) == so.tobytes()
    # Python: the host form and the corpus functions
    pcms, chans = [p for p, _ in songs], [c for _, c in songs]
    ps, pf, pb = M.mel_batch_host(pcms, chans, frames=True, bands=True, min_energy=1000)
    assert ps.tobytes() == so.tobytes() and pf.tobytes() == fo.tobytes() and pb.tobytes() == bo.tobytes()
    ps2, none, pb2 = M.mel_batch_host(pcms, chans, bands=True, min_energy=1000)
    assert none is None and ps2.tobytes() == so.tobytes() and pb2.tobytes() == bo.tobytes()
    corpus = bliss_amd.DeviceCorpus([p.size for p in pcms], chans, 1)
    corpus.pcm.fill_(32767)
    for i, p in enumerate(pcms):
        corpus.upload(i, p)
    M.mel_device(corpus, frames=True, bands=True, min_energy=1000)
    cs, cf, cb = M.fetch_mel(corpus)
    assert cs.tobytes() == so.tobytes() and cf.tobytes() == fo.tobytes() and cb.tobytes() == bo.tobytes()
    with bliss_amd.Context(0) as ctx:
        M.mel_device(corpus, min_energy=1000, ctx=ctx)
        cs2, none, none2 = M.fetch_mel(corpus)
    assert none is None and none2 is None and cs2.tobytes() == so.tobytes()
    # the figures a user reads, from the exact integers
    summary = M.mel_summary(ps)
    for i, (pcm, ch) in enumerate(songs):
        frames, _ = ref.records(pcm, ch)
        used = [f for f in frames if f["energy"] >= 1000]
        if not used:
            assert np.isnan(summary["mfcc"][i]).all() and np.isnan(summary["flatness_std_db"][i])
            continue
        m = np.array([f["mfcc"] for f in used], dtype=np.float64) / 4096
        fl = np.array([f["flat"] for f in used], dtype=np.float64) * (10 * np.log10(2.0) / 131072)
        assert summary["mfcc"][i] == pytest.approx(m.mean(axis=0), rel=1e-12, abs=1e-12)
        assert summary["mfcc_std"][i] == pytest.approx(m.std(axis=0), rel=1e-9, abs=1e-9 * abs(m).max())
        assert summary["flatness_db"][i] == pytest.approx(-fl.mean(), rel=1e-12, abs=1e-12)
    x, names = bliss_amd.descriptor.features(np.zeros(n, RESULT_DTYPE), mel=ps)
    assert x.shape == (n, 11) and names[4] == "flatness_db"


def test_host_form_over_two_upload_waves(gpu_lib, tmp_path):
    """BL_AMD_HOST_WAVE_BYTES is read when the default context is created, so the waves need a process of their own:
    64 KiB per wave cuts these songs into several waves, whose frame records and band levels must still follow each
    other"""
    songs = list(standard_songs())
    want = run(gpu_lib, songs)
    code = ("import sys, numpy as np, bliss_amd.mel as M\n"
            "from tests import test_gpu_mel as t\n"
            "songs = list(t.standard_songs())\n"
            "s, f, b = M.mel_batch_host([p for p, _ in songs], [c for _, c in songs], frames=True, bands=True)\n"
            "np.savez(sys.argv[1], s=np.frombuffer(s.tobytes(), np.uint8), f=np.frombuffer(f.tobytes(), np.uint8),\n"
            "         b=np.frombuffer(b.tobytes(), np.uint8))\n")
    out = str(tmp_path / "waves.npz")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code, out], cwd=root, text=True, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300,
                       env=dict(os.environ, BL_AMD_HOST_WAVE_BYTES=str(64 * 1024), PYTHONPATH=root))
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    assert got["s"].tobytes() == want[0].tobytes() and got["f"].tobytes() == want[1].tobytes()
    assert got["b"].tobytes() == want[2].tobytes()


def _last_energies(lib, total):
    en = np.zeros(total, dtype=np.float32)
    assert lib.bl_amd_last_energies(en.ctypes.data_as(C.POINTER(C.c_float)), total) == total
    return en


def test_the_analysis_and_the_timbre_are_untouched(gpu_lib, oracle):
    songs = fr.song_set(oracle)[:12]
    corpus = bliss_amd.DeviceCorpus([s["pcm"].size for s in songs], [s["channels"] for s in songs],
                                    [s["duration"] for s in songs])
    for i, s in enumerate(songs):
        corpus.upload(i, np.array(s["pcm"]))
    total = sum(2 * (s["pcm"].size // W) for s in songs)
    corpus.analyze()
    res = corpus.fetch().tobytes()
    en, st = _last_energies(gpu_lib, total), bliss_amd.last_freq_stats()
    corpus.timbre()
    ts, tf = (a.tobytes() for a in corpus.fetch_timbre())
    run(gpu_lib, everything())
    run(gpu_lib, everything(), want_frames=False, min_energy=50)
    M.mel_device(corpus, frames=True, bands=True)
    M.fetch_mel(corpus)
    en2, st2 = _last_energies(gpu_lib, total), bliss_amd.last_freq_stats()
    assert en2.tobytes() == en.tobytes()
    assert st2["n_songs"] == st["n_songs"] == len(songs) and st2["parts"] == st["parts"]
    for name in ("spectrum", "sum", "sumsq", "hist"):
        assert st2[name].tobytes() == st[name].tobytes(), name
    corpus.timbre()
    ts2, tf2 = (a.tobytes() for a in corpus.fetch_timbre())
    assert ts2 == ts and tf2 == tf
    corpus.analyze()
    assert corpus.fetch().tobytes() == res
