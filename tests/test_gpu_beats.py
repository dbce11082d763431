"""Per-song beat grids on the GPU (bl_amd_beats_device, bl_amd_ctx_beats_device, bl_amd_beats_host, bliss_amd.rhythm):
every field of bl_amd_song_beats, every flag, every link P and every score C is an exact integer and is compared with ==
against tests/beat_reference.py.  There is no tolerance anywhere.

The outputs are filled with 0xA5 before the call, so an element the kernel does not write shows.  The shapes are the
smallest at which the kernel takes another path: lo = (L + 1) >> 1 of 1, below, at and above a row of 16 lanes, a wave
and the workgroup, and the largest ring (L = 510); lengths around lo, 2 L and the ring's 2 048 entries.  The reference of
a (curve, period, tight) is computed once per session and shared."""
import ctypes as C

import numpy as np
import pytest

import bliss_amd
import bliss_amd.rhythm as rh
from bliss_amd import _lib
from bliss_amd.records import BEATS_DTYPE
from tests import beat_reference as br
from tests import rhythm_reference as rr

pytestmark = pytest.mark.gpu

U = _lib.BL_UNEXPECTED
SENTINEL = 0xA5
_REF = {}


def reference(o, L, tight):
    key = (o.tobytes(), L, tight)
    if key not in _REF:
        _REF[key] = br.track_blocks(o, L, tight)
    return _REF[key]


# ---- running the library -----------------------------------------------------------------------------------------

class Call:
    """one call on `songs` = [(curve, L)] whose outputs were filled with 0xA5; read() waits for the device"""

    def __init__(self, lib, songs, tight, links=True, scores=True, ctx=None, period=None, stride=4, hops=None, n=None,
                 onsets=True, out=True, flags=True, shift=(0, 0, 0, 0, 0)):
        import torch
        self.hops = [int(o.size) for o, _ in songs] if hops is None else hops
        self.n = len(songs) if n is None else n
        self.total = sum(int(o.size) for o, _ in songs)
        flat = np.concatenate([np.asarray(o, dtype=np.int64) for o, _ in songs]).astype(np.uint32)
        self.keep = [torch.from_numpy(flat.view(np.int32)).cuda(),
                     torch.from_numpy(np.array([L for _, L in songs], dtype=np.int32)).cuda()]

        def fill(nbytes):
            return torch.full((nbytes + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.so, self.fo = fill(len(songs) * 40), fill(self.total)
        self.lo = fill(self.total * 2) if links else None
        self.co = fill(self.total * 8) if scores else None
        per = self.keep[1].data_ptr() if period is None else period
        args = ((C.c_int32 * len(self.hops))(*self.hops), self.n, C.c_void_p(per + shift[1]), stride, tight,
                C.c_void_p(self.so.data_ptr() + shift[2]) if out else None,
                C.c_void_p(self.fo.data_ptr()) if flags else None,
                C.c_void_p(self.lo.data_ptr() + shift[3]) if links else None,
                C.c_void_p(self.co.data_ptr() + shift[4]) if scores else None, None)
        ons = C.c_void_p(self.keep[0].data_ptr() + shift[0]) if onsets else None
        self.rc = (lib.bl_amd_beats_device(ons, *args) if ctx is None
                   else lib.bl_amd_ctx_beats_device(ctx.handle, ons, *args))

    def _host(self, t, nbytes):
        raw = t.cpu().numpy()
        assert (raw[nbytes:] == SENTINEL).all(), "written past the end"
        return raw[:nbytes].tobytes()

    def read(self):
        import torch
        torch.cuda.synchronize()
        rec = np.frombuffer(self._host(self.so, self.n * 40), dtype=BEATS_DTYPE)
        fl = np.frombuffer(self._host(self.fo, self.total), dtype=np.uint8)
        lk = None if self.lo is None else np.frombuffer(self._host(self.lo, self.total * 2), dtype=np.uint16)
        sc = None if self.co is None else np.frombuffer(self._host(self.co, self.total * 8), dtype=np.int64)
        return rec, fl, lk, sc

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return all(t is None or bool((t == SENTINEL).all()) for t in (self.so, self.fo, self.lo, self.co))


def run(lib, songs, tight, **kw):
    c = Call(lib, songs, tight, **kw)
    assert c.rc == 0
    return c.read()


def assert_equal(got, songs, tight, what=""):
    rec, fl, lk, sc = got
    at = 0
    for i, (o, L) in enumerate(songs):
        want = reference(o, L, tight)
        H = int(o.size)
        where = f"{what} song {i} (H {H}, L {L}, tight {tight})"
        for f in br.FIELDS:
            assert int(rec[f][i]) == want["rec"][f], f"{where}: {f} {int(rec[f][i])}, want {want['rec'][f]}"
        for name, g, w in (("score", sc, want["scores"]), ("link", lk, want["links"]), ("flag", fl, want["flags"])):
            if g is None:
                continue
            g = g[at:at + H]
            if not np.array_equal(g, w):
                h = int(np.flatnonzero(g != w)[0])
                raise AssertionError(f"{where}: {name} of hop {h} {int(g[h])}, want {int(w[h])}; "
                                     f"{int((g != w).sum())} hops differ")
        at += H
    assert at == fl.size


def same_bytes(a, b):
    return all((x is None and y is None) or x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- material -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def grid():
    """a random curve for every period and length"""
    rng = np.random.default_rng(8400)
    return [(rng.integers(0, 1 << 18, H).astype(np.int64), L) for L in br.PERIODS for H in br.lengths_for(L)]


@pytest.fixture(scope="module")
def mixed():
    """about 60 songs of mixed H and L: random, sparse and click curves, two of them without a tempo"""
    rng = np.random.default_rng(8500)
    songs = []
    for k in range(60):
        L = int(rng.choice(br.PERIODS)) if k % 3 else int(rng.integers(20, 200))
        H = int(rng.integers(1, 3000))
        kind = k % 4
        if kind == 0:
            o = rng.integers(0, 1 << 18, H)
        elif kind == 1:
            o = rng.integers(0, 1 << 18, H) * (rng.integers(0, 6, H) == 0)
        elif kind == 2:
            o = br.jitter_clicks(max(L, 2), H, k) if H > 2 else rng.integers(0, 9, H)
        else:
            o = rng.integers(0, 1000, H)
        songs.append((np.asarray(o, dtype=np.int64), L))
    songs[17] = (songs[17][0], 0)
    songs[41] = (songs[41][0], 511)
    return songs


# ---- tests --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tight", br.TIGHTS)
def test_random_curves_at_every_period_and_length(gpu_lib, grid, tight):
    assert_equal(run(gpu_lib, grid, tight), grid, tight, what="grid")


def test_special_curves_at_every_period(gpu_lib):
    for tight in (0, 16, 4096):
        songs = []
        for L in br.PERIODS:
            lo = (L + 1) >> 1
            for H in (2 * L + lo, 2049):
                songs.append((np.zeros(H, np.int64), L))
                songs.append((np.full(H, 1000, np.int64), L))
                songs.append((np.full(H, br.OMAX, np.int64), L))
                for at in (0, H // 2, H - 1):
                    songs.append((br.spikes(H, [at]), L))
        got = run(gpu_lib, songs, tight)
        assert_equal(got, songs, tight, what="special")
        rec = got[0]
        zeros = [i for i, (o, _) in enumerate(songs) if not o.any()]
        assert all(int(rec["n_beats"][i]) == 0 and int(rec["first"][i]) == -1 and int(rec["last"][i]) == -1 and
                   int(rec["score"][i]) == 0 and int(rec["status"][i]) == 0 for i in zeros)
        assert int(rec["pen_scale"].max()) == tight * br.OMAX


def test_named_corpus_of_the_reference(gpu_lib):
    """the curves that tests/test_beat_reference_host.py shows to catch every deliberate mistake of the reference"""
    corpus = br.corpus()
    for tight in sorted({t for _, _, t in corpus.values()}):
        songs = [(o, L) for o, L, t in corpus.values() if t == tight]
        assert_equal(run(gpu_lib, songs, tight), songs, tight, what="corpus")
    assert int(reference(*corpus["bounds_long_L2"])["rec"]["score"]) > 1 << 32


def test_long_curve_wraps_the_ring_many_times(gpu_lib):
    rng = np.random.default_rng(8600)
    long_random = (rng.integers(0, 1 << 18, br.LONG_HOPS).astype(np.int64), br.LONG_PERIOD)
    long_clicks = (br.jitter_clicks(br.LONG_PERIOD, br.LONG_HOPS, 5), br.LONG_PERIOD)
    small = (rng.integers(0, 1 << 18, 300).astype(np.int64), 7)
    alone = run(gpu_lib, [long_random], 128)
    assert_equal(alone, [long_random], 128, what="long alone")
    songs = [small, long_clicks, long_random]
    got = run(gpu_lib, songs, 128)
    assert_equal(got, songs, 128, what="long mixed")
    assert got[1][-br.LONG_HOPS:].tobytes() == alone[1].tobytes()
    clicks = [int(h) for h in np.flatnonzero(long_clicks[0] >= 40000)]
    assert br.beat_hops(got[1][300:300 + br.LONG_HOPS]) == clicks


def test_songs_without_a_tempo_among_valid_ones(gpu_lib):
    rng = np.random.default_rng(8700)
    songs = []
    for L in br.BAD_PERIODS:
        songs.append((rng.integers(1, 1 << 18, 700).astype(np.int64), L))
        songs.append((rng.integers(0, 1 << 18, 500).astype(np.int64), 31))
    songs.append((rng.integers(1, 1 << 18, 1).astype(np.int64), 0))
    for links, scores in ((True, True), (False, False)):
        got = run(gpu_lib, songs, 16, links=links, scores=scores)
        assert_equal(got, songs, 16, what="no tempo")
        rec, fl = got[0], got[1]
        for i, (o, L) in enumerate(songs):
            if L in br.BAD_PERIODS:
                assert rec[i].tobytes() == np.array([(0, 0, o.size, L, 0, 0, 0, U)], dtype=BEATS_DTYPE).tobytes()
        assert not fl[:700].any() and fl[700:1200].any()


def test_mixed_call_is_each_song_alone_in_any_order_on_any_context(gpu_lib, mixed):
    full = run(gpu_lib, mixed, 128)
    assert_equal(full, mixed, 128, what="mixed")
    # links and scores asked for or not: the same records and flags
    for links, scores in ((False, False), (True, False), (False, True)):
        got = run(gpu_lib, mixed, 128, links=links, scores=scores)
        assert (got[2] is None) == (not links) and (got[3] is None) == (not scores)
        assert same_bytes(got[:2], full[:2])
        assert_equal(got, mixed, 128, what=f"links {links} scores {scores}")
    # reversed order
    rev = run(gpu_lib, mixed[::-1], 128)
    assert rev[0][::-1].tobytes() == full[0].tobytes()
    assert_equal(rev, mixed[::-1], 128, what="reversed")
    # through a context, twice on the same workspace
    with bliss_amd.Context(0) as ctx:
        for links in (False, True):
            got = run(gpu_lib, mixed, 128, ctx=ctx, links=links)
            assert same_bytes(got[:2], full[:2]) and got[3].tobytes() == full[3].tobytes()
    # each song alone
    at = 0
    for i, song in enumerate(mixed):
        H = song[0].size
        one = run(gpu_lib, [song], 128)
        assert one[0][0].tobytes() == full[0][i].tobytes(), i
        for a, b in zip(one[1:], full[1:]):
            assert a.tobytes() == b[at:at + H].tobytes(), i
        at += H


def test_launch_groups_of_seven_songs(gpu_lib, mixed, monkeypatch):
    """A context reads BL_AMD_GROUP_SONGS when it is created: with 7 the call runs as launch groups that follow each other
    on the stream and share the link scratch"""
    full = run(gpu_lib, mixed, 16)
    monkeypatch.setenv("BL_AMD_GROUP_SONGS", "7")
    with bliss_amd.Context(0) as ctx:
        for links in (False, True):
            got = run(gpu_lib, mixed, 16, ctx=ctx, links=links, scores=True)
            assert same_bytes(got[:2], full[:2]) and got[3].tobytes() == full[3].tobytes()


def test_rhythm_then_beats_straight_from_the_device_records(gpu_lib):
    """End to end on the click corpus of the tempo tests: bl_amd_rhythm_batch_device with onsets, then
    bl_amd_beats_device reading the lags in place (stride 72); the same bytes as from a packed copy of the lags
    (stride 4), the reference on the reference's own curve, and exactly the clicks."""
    import torch
    tracks = [(rr.click_track(period, hops, ch, seed=period), ch) for period, hops, ch in rr.CLICKS]
    tracks.append((np.zeros(600 * rr.HOP, np.int16), 1))          # silence: lag 0, no tempo
    corpus = bliss_amd.DeviceCorpus([p.size for p, _ in tracks], [ch for _, ch in tracks], 1)
    for d, (pcm, _) in zip(corpus.desc, tracks):
        corpus.pcm[d.pcm_offset:d.pcm_offset + pcm.size] = torch.from_numpy(pcm).cuda()
    rec_t, ons_t, _ = rh.rhythm_device(corpus, rr.LAG_MIN, rr.LAG_MAX)
    hops = [rr.hops_of(p.size, ch) for p, ch in tracks]
    got72 = rh.beats_device(ons_t, hops, rec_t, tight=128, links=True, scores=True)
    records, onsets, _ = rh.fetch_rhythm(corpus)
    lags = torch.from_numpy(records["lag"].astype(np.int32)).cuda()
    got4 = rh.beats_device(ons_t, hops, lags, tight=128, links=True, scores=True)
    torch.cuda.synchronize()
    for a, b in zip(got72, got4):
        assert bytes(a.cpu().numpy()) == bytes(b.cpu().numpy())
    assert [int(x) for x in records["lag"]] == [p for p, _, _ in rr.CLICKS] + [0]
    songs = [(rr.onsets(p, ch), int(lag)) for (p, ch), lag in zip(tracks, records["lag"])]
    assert np.array_equal(np.concatenate([o for o, _ in songs]), onsets.astype(np.int64))
    got = (rh.beats_to_numpy(got72[0].cpu().numpy()), got72[1].cpu().numpy(),
           got72[2].cpu().numpy().view(np.uint16), got72[3].cpu().numpy())
    assert_equal(got, songs, 128, what="end to end")
    at = 0
    for (period, H, _), n_beats in zip(rr.CLICKS, (26, 16, 13, 10)):
        want = list(range(period // 2, H, period))
        assert len(want) == n_beats
        assert br.beat_hops(got[1][at:at + H]) == want
        hop, sec = rh.beat_list(got[1][at:at + H])
        assert list(hop) == want and list(sec) == [128.0 * h / 22050 for h in want]
        at += H
    bpm = rh.beats_bpm(got[0])
    assert list(bpm[:4]) == [60.0 * 22050 / (128.0 * p) for p, _, _ in rr.CLICKS] and np.isnan(bpm[4])
    assert int(got[0]["status"][4]) == U and not got[1][at:].any()


def test_rejected_calls_write_nothing(gpu_lib):
    rng = np.random.default_rng(8800)
    songs = [(rng.integers(0, 1 << 18, 300).astype(np.int64), 20), (rng.integers(0, 1 << 18, 200).astype(np.int64), 9)]
    bad = [dict(onsets=False), dict(out=False), dict(flags=False), dict(n=0), dict(n=-1), dict(hops=[300, 0]),
           dict(hops=[300, 1 << 24]), dict(hops=[-1, 200]), dict(stride=0), dict(stride=2), dict(stride=6),
           dict(stride=-4), dict(tight=-1), dict(tight=4097), dict(shift=(2, 0, 0, 0, 0)), dict(shift=(0, 2, 0, 0, 0)),
           dict(shift=(0, 0, 4, 0, 0)), dict(shift=(0, 0, 0, 1, 0)), dict(shift=(0, 0, 0, 0, 4))]
    for kw in bad:
        tight = kw.pop("tight", 16)
        c = Call(gpu_lib, songs, tight, **kw)
        assert c.rc == U and c.untouched(), kw
    import torch
    c = Call(gpu_lib, songs, 16, period=0)
    assert c.rc == U and c.untouched()
    hops = (C.c_int32 * 2)(300, 200)
    assert gpu_lib.bl_amd_beats_device(C.c_void_p(c.keep[0].data_ptr()), None, 2, C.c_void_p(c.keep[1].data_ptr()), 4, 16,
                                       C.c_void_p(c.so.data_ptr()), C.c_void_p(c.fo.data_ptr()), None, None, None) == U
    assert gpu_lib.bl_amd_ctx_beats_device(None, C.c_void_p(c.keep[0].data_ptr()), hops, 2,
                                           C.c_void_p(c.keep[1].data_ptr()), 4, 16, C.c_void_p(c.so.data_ptr()),
                                           C.c_void_p(c.fo.data_ptr()), None, None, None) == U
    assert c.untouched()
    # the same arguments, valid: the call goes through
    good = Call(gpu_lib, songs, 16)
    assert good.rc == 0
    assert_equal(good.read(), songs, 16, what="valid")
    torch.cuda.synchronize()


def test_host_form_equals_the_device_form(gpu_lib, mixed):
    songs = mixed[:24]
    dev = run(gpu_lib, songs, 128)
    for links, scores in ((True, True), (False, False)):
        rec, fl, lk, sc = rh.beats_host([o for o, _ in songs], [L for _, L in songs], tight=128, links=links,
                                        scores=scores)
        assert rec.tobytes() == dev[0].tobytes() and fl.tobytes() == dev[1].tobytes()
        assert (lk is None) == (not links) and (sc is None) == (not scores)
        if links:
            assert lk.tobytes() == dev[2].tobytes() and sc.tobytes() == dev[3].tobytes()
    # the host form rejects what the device form cannot check: an onset value of 2^18
    o = np.array([1, 1 << 18, 3], dtype=np.uint32)
    rec, fl = (_lib.SongBeats * 1)(), np.full(3, SENTINEL, np.uint8)
    assert gpu_lib.bl_amd_beats_host(o.ctypes.data_as(C.POINTER(C.c_uint32)), (C.c_int32 * 1)(3), 1, (C.c_int32 * 1)(2),
                                     16, rec, fl.ctypes.data_as(C.POINTER(C.c_uint8)), None, None) == U
    assert (fl == SENTINEL).all()


def test_profile_counts_one_launch_per_group(gpu_lib, mixed):
    gpu_lib.bl_amd_profile(1)
    gpu_lib.bl_amd_profile_reset()
    try:
        run(gpu_lib, mixed, 16)
        n = C.c_int(0)
        ms = gpu_lib.bl_amd_profile_ms(b"beats", C.byref(n))
    finally:
        gpu_lib.bl_amd_profile(0)
    assert ms > 0.0 and n.value == 1
