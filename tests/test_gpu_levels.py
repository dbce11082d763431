"""Per-song signal levels on the GPU (bl_amd_levels_batch_device, DeviceCorpus.levels, levels_batch_host,
gapless_links): every field of bl_amd_song_levels is an exact integer and is compared by equality with the numpy oracle
below.  The arena is filled with 32767 before the songs are uploaded, so a read outside a song shows up in `peak`,
`clipped` and `sum`.  The sizes sit around the kernel's seams: 8 samples per 16-byte vector, 2 048 per workgroup step,
the samples behind the last whole vector, one frame, and two lengths at which several workgroups share a song and the
counts pass 65 536."""
import ctypes as C

import numpy as np
import pytest

import bliss_amd
from bliss_amd import _lib
from bliss_amd.batch import LEVELS_DTYPE

pytestmark = pytest.mark.gpu

SIZES = [2, 3, 4, 7, 8, 9, 15, 16, 17, 2047, 2048, 2049, 4095, 4096, 4097, 4103]
LONG = [(1_000_003, 1), (600_006, 2)]
SILENCES = (0, 100)
FIELDS = ("sum", "sum_sq", "peak", "zero_cross", "clipped", "lead", "trail", "frames", "status", "head", "tail")


def oracle_levels(pcm, ch, silence):
    """bl_amd_song_levels of one song by its definition in include/bliss_amd.h"""
    pcm = np.asarray(pcm, dtype=np.int16)
    n = pcm.size
    F = n // ch
    x = pcm[:F * ch].astype(np.int64).reshape(F, ch)
    rec = np.zeros((), dtype=LEVELS_DTYPE)
    for c in range(ch):
        s = x[:, c]
        neg = s < 0
        rec["sum"][c] = s.sum()
        rec["sum_sq"][c] = (s * s).sum()
        rec["peak"][c] = np.abs(s).max()
        rec["zero_cross"][c] = np.count_nonzero(neg[1:] != neg[:-1])
        rec["clipped"][c] = np.count_nonzero((s == 32767) | (s == -32768))
    loud = np.flatnonzero((np.abs(x) > silence).any(axis=1))
    rec["lead"] = loud[0] if loud.size else F
    rec["trail"] = F - 1 - loud[-1] if loud.size else F
    rec["frames"] = F
    rec["status"] = _lib.BL_OK
    rec["head"] = pcm[:2]
    rec["tail"] = pcm[n - 2:]
    return rec


def _frames(kind, F, rng):
    """F + 1 values of one channel's pattern (channel 1 takes them one frame later)"""
    t = np.arange(F + 1)
    if kind == "random":
        return rng.integers(-32768, 32768, F + 1)
    if kind == "alt1":        # a crossing at every frame: catches every seam
        return np.where(t % 2 == 0, 1, -1)
    if kind == "tri":         # 1, 0, -1, 0, ...: zero is non-negative
        return np.array([1, 0, -1, 0])[t % 4]
    if kind == "floor":       # sum_sq = F * 2^30, peak 32768, clipped F
        return np.full(F + 1, -32768)
    if kind == "rails":
        return np.where(t % 2 == 0, 32767, -32768)
    if kind == "zero":
        return np.zeros(F + 1, dtype=np.int64)
    where, value = kind       # one non-zero sample
    v = np.zeros(F + 1, dtype=np.int64)
    at = {"mid": F // 2}.get(where, where if not isinstance(where, str) else None)
    if at is not None and at < 0:
        at += F
    if at is not None and 0 <= at < F:
        v[at] = value
    return v


# the values 100 and -100 are loud for silence 0 and exactly not loud for silence 100
PATTERNS = ["random", "alt1", "tri", "floor", "rails", "zero", (0, 100), (7, -100), (8, 101), ("mid", -32768),
            (-9, 100), (-8, -101), (-1, 32767)]


def make_song(kind, n, ch, rng):
    F = n // ch
    f = _frames(kind, F, rng)
    pcm = np.empty(n, dtype=np.int16)
    if ch == 1:
        pcm[:] = f[:n]
    else:
        pcm[0:2 * F:2] = f[:F]
        pcm[1:2 * F:2] = f[1:F + 1] if isinstance(kind, str) else -f[:F]
        if n > 2 * F:
            pcm[-1] = -32768   # behind the last frame: shows up in `tail` only
    return pcm


@pytest.fixture(scope="module")
def batch(gpu_lib):
    """(songs, channels, corpus, {silence: fetched levels}, {silence: oracle}) — computed once, left unchanged"""
    rng = np.random.default_rng(20261018)
    songs, chans = [], []
    for n in SIZES:
        for ch in (1, 2):
            for kind in PATTERNS:
                songs.append(make_song(kind, n, ch, rng))
                chans.append(ch)
    for (n, ch), kinds in zip(LONG, (("alt1", "random"), ("rails", "random"))):
        for kind in kinds:
            songs.append(make_song(kind, n, ch, rng))
            chans.append(ch)
    corpus = bliss_amd.DeviceCorpus([s.size for s in songs], chans, 1)
    corpus.pcm.fill_(32767)
    for i, s in enumerate(songs):
        corpus.upload(i, s)
    got, want = {}, {}
    for sil in SILENCES:
        corpus.levels(silence=sil)
        got[sil] = corpus.fetch_levels()
        want[sil] = np.array([oracle_levels(s, ch, sil) for s, ch in zip(songs, chans)], dtype=LEVELS_DTYPE)
    return songs, chans, corpus, got, want


@pytest.mark.parametrize("silence", SILENCES)
def test_every_field_equals_the_oracle(batch, silence):
    songs, chans, _, got, want = batch
    g, w = got[silence], want[silence]
    assert g.shape == w.shape == (len(songs),)
    for f in FIELDS:
        bad = np.flatnonzero((g[f] != w[f]).reshape(len(songs), -1).any(axis=1))
        assert bad.size == 0, (f, [(int(i), songs[i].size, chans[i], g[f][i].tolist(), w[f][i].tolist())
                                   for i in bad[:8]])
    assert g.tobytes() == w.tobytes()
    # what the long songs are there for
    assert w["zero_cross"].max() > 65536 and w["clipped"].max() > 65536
    assert (w["peak"][np.array(chans) == 1][:, 1] == 0).all()   # mono: every [1] entry is 0


def test_silence_equal_to_the_loudest_sample_is_silent(batch):
    songs, chans, _, got, _ = batch
    n_checked = 0
    for i, s in enumerate(songs):
        peak = int(np.abs(s[:s.size // chans[i] * chans[i]].astype(np.int64)).max())
        if peak == 100:
            assert got[0][i]["lead"] < got[0][i]["frames"]
            assert got[100][i]["lead"] == got[100][i]["trail"] == got[100][i]["frames"]
            n_checked += 1
    assert n_checked >= 8


def test_a_song_alone_gives_the_bytes_it_got_in_the_batch(batch):
    """independent of the other songs, of n_songs and of the grid: alone a long song gets many more workgroups"""
    songs, chans, _, got, _ = batch
    n_long = 2 * len(LONG)
    with bliss_amd.Context(0) as ctx:
        for i in range(len(songs) - n_long, len(songs)):
            one = bliss_amd.DeviceCorpus([songs[i].size], chans[i], 1)
            one.pcm.fill_(32767)
            one.upload(0, songs[i])
            for sil in SILENCES:
                one.levels(silence=sil)
                assert one.fetch_levels().tobytes() == got[sil][i:i + 1].tobytes(), (i, sil)
                one.levels(silence=sil, ctx=ctx)
                assert one.fetch_levels().tobytes() == got[sil][i:i + 1].tobytes(), (i, sil, "ctx")


def test_output_need_not_be_zeroed_and_a_context_gives_the_same(batch):
    _, _, corpus, got, _ = batch
    corpus.levels_raw.fill_(0xAB)
    with bliss_amd.Context(0) as ctx:
        corpus.levels(silence=100, ctx=ctx)
        assert corpus.fetch_levels().tobytes() == got[100].tobytes()
    corpus.levels_raw.fill_(0xCD)
    corpus.levels(silence=0)
    assert corpus.fetch_levels().tobytes() == got[0].tobytes()


def test_host_form_equals_the_device_form(batch):
    songs, chans, _, got, _ = batch
    for sil in SILENCES:
        assert bliss_amd.levels_batch_host(songs, chans, silence=sil).tobytes() == got[sil].tobytes()


def test_host_form_over_two_waves(gpu_lib):
    """levels_batch_host uploads at most 2^27 samples at a time, every song at a multiple of 8.  Padded, the first two
    songs come to 125 829 128 <= 2^27 and the third passes it: the waves are songs {0, 1} and song {2}.  Byte for byte
    the records of one device call on one corpus, which is never split; each song is a block of 65 536 random samples
    of its own seed tiled to length, so a swapped or shifted wave shows."""
    lengths, chans = (62_914_563, 62_914_560, 20_971_527), (1, 2, 1)
    padded = [(n + 7) & ~7 for n in lengths]
    assert padded[0] + padded[1] <= 1 << 27 < sum(padded)
    songs = [np.resize(np.random.default_rng(9100 + i).integers(-32768, 32768, 65536).astype(np.int16), n)
             for i, n in enumerate(lengths)]
    corpus = bliss_amd.DeviceCorpus(lengths, chans, 1)
    corpus.pcm.fill_(32767)
    for i, s in enumerate(songs):
        corpus.upload(i, s)
    for sil in SILENCES:
        corpus.levels(silence=sil)
        want = corpus.fetch_levels()
        assert bliss_amd.levels_batch_host(songs, chans, silence=sil).tobytes() == want.tobytes(), sil
    for i, (s, ch) in enumerate(zip(songs, chans)):   # the device call itself, by what numpy gives without 64-bit copies
        F = s.size // ch
        assert want["frames"][i] == F and want["status"][i] == _lib.BL_OK
        assert want["head"][i].tolist() == s[:2].tolist() and want["tail"][i].tolist() == s[-2:].tolist()
        for c in range(2):
            v = s[c:F * ch:ch] if c < ch else s[:0]
            assert want["sum"][i][c] == int(v.sum(dtype=np.int64)), (i, c)
            assert want["peak"][i][c] == (max(int(v.max()), -int(v.min())) if c < ch else 0), (i, c)


def test_lead_and_trail_agree_with_the_trim_of_the_analysis(gpu_lib):
    """for songs the analysers accept and silence 0: lead = start // channels, trail = F - 1 - end // channels"""
    rng = np.random.default_rng(5)
    songs, chans = [], []
    for n, ch, a, b in ((6000, 1, 0, 6000), (8192, 2, 1001, 8000), (5121, 2, 16, 5100), (5120, 1, 2049, 5119),
                        (7000, 2, 3, 6990)):
        s = np.zeros(n, dtype=np.int16)
        s[a:b] = rng.integers(1, 3000, b - a) * rng.choice([-1, 1], b - a)
        songs.append(s)
        chans.append(ch)
    corpus = bliss_amd.DeviceCorpus([s.size for s in songs], chans, 1)
    for i, s in enumerate(songs):
        corpus.upload(i, s)
    corpus.analyze()
    res = corpus.fetch()
    corpus.levels(silence=0)
    lv = corpus.fetch_levels()
    for i, ch in enumerate(chans):
        F = songs[i].size // ch
        assert lv["lead"][i] == res["start"][i] // ch, i
        assert lv["trail"][i] == F - 1 - res["end"][i] // ch, i
        assert lv[i].tobytes() == oracle_levels(songs[i], ch, 0).tobytes()


def test_gapless_links_of_a_batch(gpu_lib):
    """songs 0 -> 1 link (slot 0: 1000 against 1100), 1 -> 2 do not (slot 0 differs by 2000, slot 1 is below 5)"""
    rng = np.random.default_rng(6)
    songs = [rng.integers(-20000, 20000, n).astype(np.int16) for n in (4001, 3000, 5000)]
    songs[0][-2:] = (1000, -2000)
    songs[1][:2] = (1100, 500)
    songs[1][-2:] = (3000, 4)
    songs[2][:2] = (5000, 4)
    lv = bliss_amd.levels_batch_host(songs, [1, 2, 2])
    assert lv["tail"][0].tolist() == [1000, -2000] and lv["head"][1].tolist() == [1100, 500]
    assert bliss_amd.gapless_links(lv).tolist() == [True, False]


def test_rejected_calls_write_nothing(gpu_lib):
    import torch
    lib = gpu_lib
    n = 4
    pcm = torch.zeros(4096, dtype=torch.int16, device="cuda:0")
    out = torch.full((n * C.sizeof(_lib.SongLevels),), 0xAB, dtype=torch.uint8, device="cuda:0")

    def call(silence=0, ctx=None, **bad):
        desc = (_lib.SongDesc * n)()
        for i in range(n):
            desc[i].pcm_offset, desc[i].n_samples, desc[i].channels, desc[i].duration = 1024 * i, 1000, 1 + i % 2, 1
        for k, v in bad.items():
            setattr(desc[2], k, v)
        args = (C.c_void_p(pcm.data_ptr()), desc, n, silence, C.c_void_p(out.data_ptr()), None)
        return lib.bl_amd_levels_batch_device(*args) if ctx is None else \
            lib.bl_amd_ctx_levels_batch_device(ctx.handle, *args)

    with bliss_amd.Context(0) as ctx:
        for c in (None, ctx):
            assert call(silence=-1, ctx=c) == _lib.BL_UNEXPECTED
            assert call(silence=32768, ctx=c) == _lib.BL_UNEXPECTED
            assert call(channels=3, ctx=c) == _lib.BL_UNEXPECTED
            assert call(channels=0, ctx=c) == _lib.BL_UNEXPECTED
            assert call(n_samples=1, ctx=c) == _lib.BL_UNEXPECTED
            assert call(pcm_offset=2052, ctx=c) == _lib.BL_UNEXPECTED
    desc = (_lib.SongDesc * 1)()
    desc[0].n_samples, desc[0].channels = 1000, 1
    assert lib.bl_amd_levels_batch_device(C.c_void_p(pcm.data_ptr()), desc, 0, 0, C.c_void_p(out.data_ptr()),
                                          None) == _lib.BL_UNEXPECTED
    torch.cuda.synchronize()
    assert bool((out == 0xAB).all())
    assert call() == _lib.BL_OK   # the same call with nothing wrong goes through
    torch.cuda.synchronize()
    assert not bool((out == 0xAB).all())
