"""Per-frame spectral timbre on the GPU (bl_amd_timbre_batch_device, bl_amd_ctx_timbre_batch_device,
bl_amd_timbre_batch_host, DeviceCorpus.timbre): every field of bl_amd_frame_timbre and bl_amd_song_timbre is an exact
integer and is compared with == against tests/timbre_reference.py, the Python-int restatement of the header's
definitions on top of tests/freq_reference.py's per-frame power values.  There is no tolerance anywhere.

Every arena is filled with 32767 before the songs are placed and the outputs with 0xA5 before the call, so a read
outside a song's whole frames and a field the kernel does not write both show."""
import ctypes as C
import functools

import numpy as np
import pytest

import bliss_amd
from bliss_amd import _lib
from bliss_amd.batch import TIMBRE_FRAME_DTYPE, TIMBRE_SONG_DTYPE
from tests import freq_reference as fr
from tests import timbre_reference as tr

pytestmark = pytest.mark.gpu

U = _lib.BL_UNEXPECTED
W = 512
SONG_FIELDS = ("centroid_sum", "centroid_sumsq", "rolloff_sum", "rolloff_sumsq", "peak_sum", "peak_sumsq",
               "energy_max", "frames", "used", "status", "reserved")
FRAME_FIELDS = ("energy", "moment", "rolloff", "peak")
SENTINEL = 0xA5


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


def call(lib, arena, items, pct=85, min_energy=0, want_frames=True, ctx=None, n_records=None, fill=SENTINEL):
    """(return code, song records, frame records or None) of one call whose outputs were filled with `fill`"""
    import torch
    n = len(items)
    desc = (_lib.SongDesc * n)()
    for i, (at, ns, ch) in enumerate(items):
        desc[i].pcm_offset, desc[i].n_samples, desc[i].channels, desc[i].duration = at, ns, ch, 77 + i
    total = sum(max(frames_of(ns, ch), 0) if ch in (1, 2) else 0 for _, ns, ch in items)
    so = torch.full((max(n, 1) * 72,), fill, dtype=torch.uint8, device="cuda")
    fo = torch.full((max(total, 1) * 24,), fill, dtype=torch.uint8, device="cuda") if want_frames else None
    args = (C.c_void_p(arena.data_ptr()), desc, n, pct, min_energy, C.c_void_p(so.data_ptr()),
            C.c_void_p(fo.data_ptr()) if want_frames else None, total if n_records is None else n_records, None)
    rc = (lib.bl_amd_timbre_batch_device(*args) if ctx is None
          else lib.bl_amd_ctx_timbre_batch_device(ctx.handle, *args))
    torch.cuda.synchronize()
    songs = np.frombuffer(so.cpu().numpy().tobytes(), dtype=TIMBRE_SONG_DTYPE)[:n]
    frames = np.frombuffer(fo.cpu().numpy().tobytes(), dtype=TIMBRE_FRAME_DTYPE)[:total] if want_frames else None
    return rc, songs, frames


def run(lib, songs, **kw):
    arena, items = place(songs)
    rc, so, fo = call(lib, arena, items, **kw)
    assert rc == 0
    return so, fo


# ---- the reference, computed once per song and shared ------------------------------------------------------------

class Reference:
    """per-frame power values of a song, cached by the song's bytes; records for any (pct, min_energy)"""

    def __init__(self, oracle):
        self.oracle = oracle
        self.power = {}
        self.frames = {}

    def key(self, pcm, ch):
        return (np.asarray(pcm).tobytes()[:frames_of(pcm.size, ch) * W * ch * 2], ch)

    def records(self, pcm, ch, pct=85, min_energy=0):
        k = self.key(pcm, ch)
        if k not in self.power:
            self.power[k] = tr.power_of(self.oracle, pcm, ch)
        if (k, pct) not in self.frames:
            self.frames[(k, pct)] = [tr.frame_record(row, pct) for row in self.power[k]]
        frames = self.frames[(k, pct)]
        return frames, tr.song_record(frames, min_energy)


@pytest.fixture(scope="module")
def ref(oracle):
    return Reference(oracle)


def assert_equal(so, fo, songs, ref, pct=85, min_energy=0, what=""):
    at = 0
    for i, (pcm, ch) in enumerate(songs):
        frames, rec = ref.records(pcm, ch, pct, min_energy)
        where = f"{what} song {i} ({ch} ch, F {len(frames)}, pct {pct}, min_energy {min_energy})"
        for name in SONG_FIELDS:
            assert int(so[name][i]) == rec[name], f"{where}: {name} {int(so[name][i])}, want {rec[name]}"
        if fo is not None:
            got = fo[at:at + len(frames)]
            for k, name in enumerate(FRAME_FIELDS):
                want = [f[k] for f in frames]
                g = [int(x) for x in got[name]]
                if g != want:
                    t = next(j for j in range(len(want)) if g[j] != want[j])
                    raise AssertionError(f"{where}: frame {t} (mod 32: {t % 32}, mod 8: {t % 8}) {name} {g[t]}, "
                                         f"want {want[t]}; {sum(a != b for a, b in zip(g, want))} frames differ")
        at += len(frames)
    if fo is not None:
        assert at == fo.size


# ---- material ----------------------------------------------------------------------------------------------------

def noise(rng, n, amp=3000):
    return rng.integers(-amp, amp + 1, n).astype(np.int16)


@functools.lru_cache(maxsize=None)
def short_songs():
    """mono and stereo at F = 1 .. 65 with 0, 1 and 512 channels - 1 samples behind the last frame"""
    rng = np.random.default_rng(41)
    out = []
    for F in (1, 2, 3, 4, 7, 8, 9, 63, 64, 65):
        for ch in (1, 2):
            for extra in (0, 1, W * ch - 1):
                out.append((noise(rng, F * W * ch + extra, 200 << (F % 7)), ch))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def tone_ladder():
    """F = 300, frame t a sine at bin (t mod 255) + 1 whose level cycles over 1, 30, 1 000, 32 767; mono, and stereo
    with another tone on the right"""
    n = np.arange(W)
    levels = (1, 30, 1000, 32767)
    mono = np.concatenate([np.rint(levels[t % 4] * np.sin(2 * np.pi * ((t % 255) + 1) * n / W)) for t in range(300)])
    right = np.concatenate([np.rint(levels[(t + 1) % 4] * np.cos(2 * np.pi * (255 - t % 255) * n / W)) for t in range(300)])
    stereo = np.empty(2 * mono.size)
    stereo[0::2], stereo[1::2] = mono, right
    return ((mono.astype(np.int16), 1), (stereo.astype(np.int16), 2))


@functools.lru_cache(maxsize=None)
def extremes():
    rng = np.random.default_rng(43)
    F = 9
    n = np.arange(F * W)
    square = np.where(n % 128 < 64, 32767, -32768).astype(np.int16)
    impulse = np.zeros(F * W, np.int16)
    impulse[256::W] = 32767
    impulse[3 * W + 256] = -32768
    left = rng.integers(-32767, 32768, 12 * W).astype(np.int16)
    anti = np.empty(2 * left.size, np.int16)
    anti[0::2], anti[1::2] = left, -left
    gap = noise(rng, 30 * W * 2 + 5)
    gap[10 * W * 2:20 * W * 2] = 0
    gap_mono = noise(rng, 33 * W + 100)
    gap_mono[11 * W:22 * W] = 0
    return (
        (square, 1),                                                   # energy ~ 2^49.6
        (np.repeat(square, 2), 2),
        (np.full(F * W, 32767, np.int16), 1),                          # 2^48 in bin 1
        (np.full(F * W, -32768, np.int16), 1),
        (np.full(F * W * 2, -32768, np.int16), 2),
        (np.where(n % 2 == 0, 32767, -32768).astype(np.int16), 1),     # everything at the top: rolloff and peak 255
        (impulse, 1),
        (rng.choice(np.array([-1, 1], np.int16), F * W), 1),           # +-1 noise
        (rng.choice(np.array([-1, 1], np.int16), F * W * 2), 2),
        (np.zeros(F * W, np.int16), 1),
        (np.zeros(F * W * 2 + 3, np.int16), 2),
        (anti, 2),                                                     # L = -R: zero after the average
        (gap, 2),                                                      # used < frames
        (gap_mono, 1),
    )


# ---- tests -------------------------------------------------------------------------------------------------------

def test_song_set_in_one_mixed_batch(gpu_lib, oracle, ref):
    songs = [(np.array(s["pcm"]), s["channels"]) for s in fr.song_set(oracle)]
    assert len(songs) == 259
    so, fo = run(gpu_lib, songs)
    assert_equal(so, fo, songs, ref, what="song_set")
    assert [int(x) for x in so["frames"]] == [s["n_frames"] for s in fr.song_set(oracle)]
    assert len({int(x) for x in fo["rolloff"]}) > 20 and int(so["used"].min()) > 0


def test_very_short_songs(gpu_lib, ref):
    songs = list(short_songs())
    so, fo = run(gpu_lib, songs)
    assert_equal(so, fo, songs, ref, what="short")
    assert sorted({int(x) for x in so["frames"]}) == [1, 2, 3, 4, 7, 8, 9, 63, 64, 65]


def test_tone_ladder_reaches_every_peak_bin(gpu_lib, ref):
    songs = list(tone_ladder())
    so, fo = run(gpu_lib, songs)
    assert_equal(so, fo, songs, ref, what="ladder")
    loud = [int(fo["peak"][t]) for t in range(300) if t % 4 >= 1]
    assert loud == [(t % 255) + 1 for t in range(300) if t % 4 >= 1]
    assert {int(x) for x in fo["peak"][:300]} >= set(range(1, 256))


def test_extremes(gpu_lib, ref):
    songs = list(extremes())
    so, fo = run(gpu_lib, songs)
    assert_equal(so, fo, songs, ref, what="extremes")
    # what the material was designed to reach
    assert 2 ** 49 < int(so["energy_max"][0]) < 2 ** 50 and int(fo["peak"][0]) == 4
    assert 2 ** 47 < int(fo["energy"][2 * 9]) and int(fo["peak"][2 * 9]) == 1
    assert int(fo["rolloff"][5 * 9]) == 255 and int(fo["peak"][5 * 9]) == 255
    for i in (9, 10, 11):     # silence, and L = -R
        assert int(so["used"][i]) == 0 and int(so["energy_max"][i]) == 0 and int(so["centroid_sum"][i]) == 0
    off11 = sum(frames_of(p.size, c) for p, c in songs[:11])
    assert {(int(f["energy"]), int(f["rolloff"]), int(f["peak"])) for f in fo[off11:off11 + 12]} == {(0, 1, 1)}
    assert 0 < int(so["used"][12]) == int(so["frames"][12]) - 10 and int(so["used"][13]) == int(so["frames"][13]) - 11


@pytest.fixture(scope="module")
def parameter_songs():
    return list(extremes()) + list(short_songs())[:24] + [tone_ladder()[0]]


@pytest.mark.parametrize("pct", [1, 50, 85, 99, 100])
def test_rolloff_percentages(gpu_lib, ref, parameter_songs, pct):
    so, fo = run(gpu_lib, parameter_songs, pct=pct)
    assert_equal(so, fo, parameter_songs, ref, pct=pct, what="pct")


def test_min_energy(gpu_lib, ref, parameter_songs):
    energies = sorted(f[0] for pcm, ch in parameter_songs for f in ref.records(pcm, ch)[0])
    median = energies[len(energies) // 2]
    assert 1 < median < 2 ** 63
    for min_energy in (0, 1, median, median + 1, 2 ** 63):
        so, fo = run(gpu_lib, parameter_songs, min_energy=min_energy)
        assert_equal(so, fo, parameter_songs, ref, min_energy=min_energy, what="min_energy")
    assert int(so["used"].max()) == 0 and int(so["rolloff_sumsq"].max()) == 0 and int(so["energy_max"].max()) > 2 ** 49
    # the threshold is the frame's own energy: used exactly from there on
    pcm, ch = parameter_songs[0]
    e = ref.records(pcm, ch)[0][0][0]
    (a, _), (b, _) = run(gpu_lib, [(pcm, ch)], min_energy=e), run(gpu_lib, [(pcm, ch)], min_energy=e + 1)
    assert int(a["used"][0]) > int(b["used"][0])


def test_one_song_alone_equals_the_same_song_in_a_batch_of_37(gpu_lib, oracle, ref):
    pool = [(np.array(s["pcm"]), s["channels"]) for s in fr.song_set(oracle)[:36]]
    for song in (tone_ladder()[1], short_songs()[5], extremes()[12]):
        alone_s, alone_f = run(gpu_lib, [song])
        for pos in (0, 17, 36):
            batch = pool[:pos] + [song] + pool[pos:]
            assert len(batch) == 37
            so, fo = run(gpu_lib, batch)
            at = sum(frames_of(p.size, c) for p, c in batch[:pos])
            assert so[pos].tobytes() == alone_s[0].tobytes()
            assert fo[at:at + alone_f.size].tobytes() == alone_f.tobytes()
    assert_equal(so, fo, batch, ref, what="batch of 37")


def test_pcm_offsets_8_and_4104(gpu_lib, ref):
    song = short_songs()[40]
    got = []
    for off in (8, 4104):
        arena, items = place([song], offsets=[off])
        rc, so, fo = call(gpu_lib, arena, items)
        assert rc == 0
        assert_equal(so, fo, [song], ref, what=f"offset {off}")
        got.append((so.tobytes(), fo.tobytes()))
    assert got[0] == got[1]


def test_no_frame_output_gives_the_same_song_records(gpu_lib, ref, parameter_songs):
    so, _ = run(gpu_lib, parameter_songs)
    so2, none = run(gpu_lib, parameter_songs, want_frames=False)
    assert none is None and so2.tobytes() == so.tobytes()
    # n_frame_records is ignored without a frame output
    arena, items = place(parameter_songs)
    rc, so3, _ = call(gpu_lib, arena, items, want_frames=False, n_records=-5)
    assert rc == 0 and so3.tobytes() == so.tobytes()


def test_second_context_equals_the_default_one(gpu_lib, ref, parameter_songs):
    so, fo = run(gpu_lib, parameter_songs)
    with bliss_amd.Context(0) as ctx:
        so2, fo2 = run(gpu_lib, parameter_songs, ctx=ctx)
        so3, fo3 = run(gpu_lib, parameter_songs, ctx=ctx, pct=50)
    assert so2.tobytes() == so.tobytes() and fo2.tobytes() == fo.tobytes()
    assert_equal(so3, fo3, parameter_songs, ref, pct=50, what="ctx")


def test_outputs_are_fully_overwritten(gpu_lib, parameter_songs):
    so, fo = run(gpu_lib, parameter_songs)      # both were filled with 0xA5
    assert int(so["reserved"].max()) == 0 and int(so["status"].max()) == 0
    so0, fo0 = run(gpu_lib, parameter_songs, fill=0x00)
    assert so0.tobytes() == so.tobytes() and fo0.tobytes() == fo.tobytes()


def test_rejections_write_nothing(gpu_lib):
    rng = np.random.default_rng(47)
    songs = [(noise(rng, 2048), 2), (noise(rng, 1030), 1)]
    arena, items = place(songs)
    assert call(gpu_lib, arena, items)[0] == 0
    bad = [
        dict(pct=0), dict(pct=101), dict(n_records=3), dict(n_records=5),
        dict(items=[(0, 2048, 3), items[1]]),                       # channels 3
        dict(items=[items[0], (2048, 511, 1)]),                     # F = 0
        dict(items=[items[0], (2049, 1030, 1)]),                    # an odd pcm_offset
        dict(items=[items[0], (2052, 1030, 1)]),
        dict(items=[]),                                             # n_songs = 0
    ]
    for kw in bad:
        kw = dict(kw)
        its = kw.pop("items", items)
        if "n_records" not in kw and its is not items:
            kw["n_records"] = sum(frames_of(n, c) for _, n, c in its if c in (1, 2))
        rc, so, fo = call(gpu_lib, arena, its, **kw)
        assert rc == U, kw
        assert so.tobytes() == bytes([SENTINEL]) * so.nbytes and fo.tobytes() == bytes([SENTINEL]) * fo.nbytes, kw
    # NULL pointers and a misaligned arena
    import torch
    desc = (_lib.SongDesc * 2)()
    for i, (at, ns, ch) in enumerate(items):
        desc[i].pcm_offset, desc[i].n_samples, desc[i].channels = at, ns, ch
    so = torch.full((2 * 72,), SENTINEL, dtype=torch.uint8, device="cuda")
    fo = torch.full((4 * 24,), SENTINEL, dtype=torch.uint8, device="cuda")
    p, s, f = arena.data_ptr(), so.data_ptr(), fo.data_ptr()
    fn = gpu_lib.bl_amd_timbre_batch_device
    assert fn(None, desc, 2, 85, 0, s, f, 4, None) == U
    assert fn(p, None, 2, 85, 0, s, f, 4, None) == U
    assert fn(p, desc, 2, 85, 0, None, f, 4, None) == U
    assert fn(p + 8, desc, 2, 85, 0, s, f, 4, None) == U
    assert gpu_lib.bl_amd_ctx_timbre_batch_device(None, p, desc, 2, 85, 0, s, f, 4, None) == U
    torch.cuda.synchronize()
    assert bytes(so.cpu().numpy()) == bytes([SENTINEL]) * 144 and bytes(fo.cpu().numpy()) == bytes([SENTINEL]) * 96


def _last_energies(lib, total):
    en = np.zeros(total, dtype=np.float32)
    assert lib.bl_amd_last_energies(en.ctypes.data_as(C.POINTER(C.c_float)), total) == total
    return en


def test_the_analysis_is_untouched(gpu_lib, oracle, parameter_songs):
    songs = fr.song_set(oracle)[:12]
    corpus = bliss_amd.DeviceCorpus([s["pcm"].size for s in songs], [s["channels"] for s in songs],
                                    [s["duration"] for s in songs])
    for i, s in enumerate(songs):
        corpus.upload(i, np.array(s["pcm"]))
    total = sum(2 * (s["pcm"].size // W) for s in songs)
    corpus.analyze()
    res = corpus.fetch().tobytes()
    en, st = _last_energies(gpu_lib, total), bliss_amd.last_freq_stats()
    run(gpu_lib, parameter_songs)
    run(gpu_lib, parameter_songs, want_frames=False, pct=50)
    en2, st2 = _last_energies(gpu_lib, total), bliss_amd.last_freq_stats()
    assert en2.tobytes() == en.tobytes()
    assert st2["n_songs"] == st["n_songs"] == len(songs) and st2["parts"] == st["parts"]
    for name in ("spectrum", "sum", "sumsq", "hist"):
        assert st2[name].tobytes() == st[name].tobytes(), name
    corpus.analyze()
    assert corpus.fetch().tobytes() == res


def test_host_form_and_python_wrappers(gpu_lib, ref, parameter_songs):
    so, fo = run(gpu_lib, parameter_songs, pct=70, min_energy=1000)
    n = len(parameter_songs)
    ptrs = (C.c_void_p * n)(*[p.ctypes.data for p, _ in parameter_songs])
    ns = (C.c_int32 * n)(*[p.size for p, _ in parameter_songs])
    chs = (C.c_int32 * n)(*[c for _, c in parameter_songs])
    hs, hf = (_lib.SongTimbre * n)(), (_lib.FrameTimbre * fo.size)()
    C.memset(hs, SENTINEL, C.sizeof(hs))
    C.memset(hf, SENTINEL, C.sizeof(hf))
    assert gpu_lib.bl_amd_timbre_batch_host(ptrs, ns, chs, n, 70, 1000, hs, hf) == 0
    assert bytes(hs) == so.tobytes() and bytes(hf) == fo.tobytes()
    C.memset(hs, SENTINEL, C.sizeof(hs))
    assert gpu_lib.bl_amd_timbre_batch_host(ptrs, ns, chs, n, 70, 1000, hs, None) == 0
    assert bytes(hs) == so.tobytes()
    # Python: the host form and the corpus method
    ps, pf = bliss_amd.timbre_batch_host([p for p, _ in parameter_songs], [c for _, c in parameter_songs], pct=70,
                                         min_energy=1000)
    assert ps.tobytes() == so.tobytes() and pf.tobytes() == fo.tobytes()
    ps2, none = bliss_amd.timbre_batch_host([p for p, _ in parameter_songs], [c for _, c in parameter_songs], pct=70,
                                            min_energy=1000, frames=False)
    assert none is None and ps2.tobytes() == so.tobytes()
    corpus = bliss_amd.DeviceCorpus([p.size for p, _ in parameter_songs], [c for _, c in parameter_songs], 1)
    corpus.pcm.fill_(32767)
    for i, (p, _) in enumerate(parameter_songs):
        corpus.upload(i, p)
    corpus.timbre(pct=70, min_energy=1000)
    cs, cf = corpus.fetch_timbre()
    assert cs.tobytes() == so.tobytes() and cf.tobytes() == fo.tobytes()
    corpus.timbre(pct=70, min_energy=1000, frames=False)
    cs2, none = corpus.fetch_timbre()
    assert none is None and cs2.tobytes() == so.tobytes()
    # the Hz figures from the exact integers
    hz = bliss_amd.timbre_hz(ps, rate=22050)
    for i, (pcm, ch) in enumerate(parameter_songs):
        frames, rec = ref.records(pcm, ch, 70, 1000)
        used = [f for f in frames if f[0] > 0 and f[0] >= 1000]
        if not used:
            assert np.isnan(hz["centroid_hz"][i]) and np.isnan(hz["peak_std_hz"][i])
            continue
        c = np.array([tr.centroid(f[0], f[1]) for f in used], dtype=np.float64) / 4096 * 22050 / 512
        r = np.array([f[2] for f in used], dtype=np.float64) * 22050 / 512
        assert hz["centroid_hz"][i] == pytest.approx(c.mean(), rel=1e-12)
        assert hz["centroid_std_hz"][i] == pytest.approx(c.std(), rel=1e-9, abs=1e-9 * c.mean())
        assert hz["rolloff_hz"][i] == pytest.approx(r.mean(), rel=1e-12)
        assert hz["rolloff_std_hz"][i] == pytest.approx(r.std(), rel=1e-9, abs=1e-9 * r.mean())


def test_host_form_over_two_waves(gpu_lib, ref):
    """timbre_batch_host uploads at most 2^27 samples at a time, every song at a multiple of 8.  Padded, the first two
    songs come to 125 829 128 <= 2^27 and the third passes it: the waves are songs {0, 1} and song {2}, and the frame
    output advances from one wave to the next.  Equal to one device call on one corpus, which is never split.  Each song
    is a block of 65 536 random samples of its own seed tiled to length, so a swapped or shifted wave shows; the block
    is 128 frames mono and 64 stereo, and the first period of every song is held against the reference."""
    lengths, chans = (62_914_563, 62_914_560, 20_971_527), (1, 2, 1)
    padded = [(n + 7) & ~7 for n in lengths]
    assert padded[0] + padded[1] <= 1 << 27 < sum(padded)
    blocks = [np.random.default_rng(9200 + i).integers(-32768, 32768, 65536).astype(np.int16) for i in range(3)]
    pcms = [np.resize(b, n) for b, n in zip(blocks, lengths)]
    corpus = bliss_amd.DeviceCorpus(lengths, chans, 1)
    corpus.pcm.fill_(32767)
    for i, p in enumerate(pcms):
        corpus.upload(i, p)
    corpus.timbre()
    cs, cf = corpus.fetch_timbre()
    hs, hf = bliss_amd.timbre_batch_host(pcms, chans)
    assert hs.tobytes() == cs.tobytes() and hf.tobytes() == cf.tobytes()
    hs2, none = bliss_amd.timbre_batch_host(pcms, chans, frames=False)
    assert none is None and hs2.tobytes() == cs.tobytes()
    at = 0
    for i, (block, n, ch) in enumerate(zip(blocks, lengths, chans)):
        period = 65536 // (W * ch)
        frames, _ = ref.records(block, ch)
        assert len(frames) == period and int(hs["frames"][i]) == frames_of(n, ch) >= 2 * period
        for k, name in enumerate(FRAME_FIELDS):
            assert [int(x) for x in hf[name][at:at + period]] == [f[k] for f in frames], (i, name)
            assert np.array_equal(hf[name][at + period:at + 2 * period], hf[name][at:at + period]), (i, name)
        at += frames_of(n, ch)
    assert at == hf.size
