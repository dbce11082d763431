"""Per-song tempo on the GPU (bl_amd_rhythm_batch_device, bl_amd_ctx_rhythm_batch_device, bl_amd_rhythm_batch_host,
bl_amd_rhythm_from_onsets, bl_amd_selftest_isqrt, bliss_amd.rhythm): the onset curve of every hop, all 512 lag products
and every field of bl_amd_song_rhythm are exact integers and are compared with == against tests/rhythm_reference.py.
There is no tolerance anywhere.

Every arena is filled with 32767 before the songs are placed and the outputs with 0xA5 before the call, so a read outside
a song's whole frames and a byte the kernels do not write both show.  The corpus is tests/rhythm_reference.py's, whose
deliberate mistakes tests/test_rhythm_reference_host.py shows to change a named song of it.  The reference of each song
is computed once per session and shared."""
import ctypes as C

import numpy as np
import pytest

import bliss_amd
import bliss_amd.rhythm as rh
from bliss_amd import _lib
from bliss_amd.records import RHYTHM_DTYPE
from tests import rhythm_reference as rr

pytestmark = pytest.mark.gpu

U = _lib.BL_UNEXPECTED
SENTINEL = 0xA5
LO, HI = rr.LAG_MIN, rr.LAG_MAX
_REF = {}


def reference(name, pcm, ch, lo=LO, hi=HI):
    """(record, onsets, R) of a named song; the curve and the lag products are kept, the pick is redone per range"""
    if name not in _REF:
        o = rr.onsets(pcm, ch)
        _REF[name] = (o, rr.lag_products(o))
    o, R = _REF[name]
    if o.size < rr.LAGS:
        return rr.record_from_onsets(o, lo, hi)[0], o, R
    lag, lag_peak, r_peak = rr.pick(R, lo, hi)
    rec = dict(r0=R[0], r_prev=R[lag - 1] if lag else 0, r_lag=R[lag] if lag else 0, r_next=R[lag + 1] if lag else 0,
               r_peak=r_peak, onset_sum=int(o.sum()), onset_max=int(o.max()), hops=int(o.size), terms=int(o.size) - 511,
               lag=lag, lag_peak=lag_peak, status=0)
    return rec, o, R


# ---- running the library -----------------------------------------------------------------------------------------

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
    host = np.full(end + 64, rr.ARENA_FILL, dtype=np.int16)
    for (at, n, _), (pcm, _) in zip(items, songs):
        host[at:at + n] = pcm
    return torch.from_numpy(host).cuda(), items


class Call:
    """one call whose outputs were filled with `fill`; read() waits for the device"""

    def __init__(self, lib, arena, items, lo=LO, hi=HI, onsets=True, acf=True, ctx=None, n_onsets=None, fill=SENTINEL,
                 stream=None, defer=False):
        import torch
        n = len(items)
        desc = (_lib.SongDesc * max(n, 1))()
        for i, (at, ns, ch) in enumerate(items):
            desc[i].pcm_offset, desc[i].n_samples, desc[i].channels, desc[i].duration = at, ns, ch, 0
        self.n = n
        self.total = sum(max(rr.hops_of(ns, ch), 0) if ch in (1, 2) else 0 for _, ns, ch in items)
        self.so = torch.full((max(n, 1) * 72,), fill, dtype=torch.uint8, device="cuda")
        self.oo = torch.full((max(self.total, 1) * 4,), fill, dtype=torch.uint8, device="cuda") if onsets else None
        self.ao = torch.full((max(n, 1) * 4096,), fill, dtype=torch.uint8, device="cuda") if acf else None
        args = (C.c_void_p(arena.data_ptr()), desc, n, lo, hi, C.c_void_p(self.so.data_ptr()),
                C.c_void_p(self.oo.data_ptr()) if onsets else None, self.total if n_onsets is None else n_onsets,
                C.c_void_p(self.ao.data_ptr()) if acf else None,
                C.c_void_p(stream.cuda_stream) if stream is not None else None)
        self.enqueue = ((lambda: lib.bl_amd_rhythm_batch_device(*args)) if ctx is None
                        else (lambda: lib.bl_amd_ctx_rhythm_batch_device(ctx.handle, *args)))
        self.rc = None if defer else self.enqueue()

    def read(self):
        import torch
        torch.cuda.synchronize()
        so = np.frombuffer(self.so.cpu().numpy().tobytes(), dtype=RHYTHM_DTYPE)[:self.n]
        oo = None if self.oo is None else np.frombuffer(self.oo.cpu().numpy().tobytes(), dtype=np.uint32)[:self.total]
        ao = None if self.ao is None else np.frombuffer(self.ao.cpu().numpy().tobytes(),
                                                        dtype=np.uint64).reshape(-1, 512)[:self.n]
        return so, oo, ao

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return all(t is None or bytes(t.cpu().numpy()) == bytes([SENTINEL]) * t.numel() for t in (self.so, self.oo, self.ao))


def run(lib, songs, **kw):
    arena, items = place(songs)
    c = Call(lib, arena, items, **kw)
    assert c.rc == 0
    return c.read()


def assert_equal(got, named, lo=LO, hi=HI, what=""):
    """got: (records, onsets or None, rows or None); named: [(name, pcm, ch)] in the call's order"""
    so, oo, ao = got
    at = 0
    for i, (name, pcm, ch) in enumerate(named):
        rec, o, R = reference(name, pcm, ch, lo, hi)
        where = f"{what} song {i} {name} ({ch} ch, H {o.size})"
        for f in rr.FIELDS:
            assert int(so[f][i]) == rec[f], f"{where}: {f} {int(so[f][i])}, want {rec[f]}"
        if oo is not None:
            g = oo[at:at + o.size].astype(np.int64)
            if not np.array_equal(g, o):
                h = int(np.flatnonzero(g != o)[0])
                raise AssertionError(f"{where}: onset of hop {h} (mod 64: {h % 64}) {int(g[h])}, want {int(o[h])}; "
                                     f"{int((g != o).sum())} hops differ")
        if ao is not None:
            g = [int(x) for x in ao[i]]
            if g != R:
                t = next(t for t in range(512) if g[t] != R[t])
                raise AssertionError(f"{where}: R[{t}] {g[t]}, want {R[t]}; {sum(a != b for a, b in zip(g, R))} lags differ")
        at += o.size
    if oo is not None:
        assert at == oo.size


@pytest.fixture(scope="module")
def corpus():
    return [(name, pcm, ch) for name, (pcm, ch) in rr.corpus().items()]


@pytest.fixture(scope="module")
def long_songs():
    return [(f"long_{ch}ch", rr.long_song(ch), ch) for ch in (1, 2)]


def pairs(named):
    return [(pcm, ch) for _, pcm, ch in named]


# ---- tests -------------------------------------------------------------------------------------------------------

def test_isqrt_selftest(gpu_lib):
    counts = (C.c_uint64 * 2)(5, 5)
    assert gpu_lib.bl_amd_selftest_isqrt(counts) == 0
    assert list(counts) == [3 * 2 ** 17 + 1, 0]
    assert gpu_lib.bl_amd_selftest_isqrt(None) == U


def test_corpus_in_one_mixed_batch(gpu_lib, corpus):
    got = run(gpu_lib, pairs(corpus))
    assert_equal(got, corpus, what="corpus")
    so = got[0]
    by_name = {name: i for i, (name, _, _) in enumerate(corpus)}
    assert sorted({int(h) for h in so["hops"][:2 * len(rr.SHAPES)]}) == sorted(rr.SHAPES)
    for period, _, _ in rr.CLICKS:
        assert int(so["lag"][by_name[f"click_{period}"]]) == period
    for name in ("noise_H1_1ch", "noise_H19_2ch", "noise_H511_1ch", "noise_H511_2ch"):
        r = so[by_name[name]]
        assert int(r["status"]) == U and int(r["terms"]) == 0 and int(r["onset_sum"]) == 0 and int(r["r0"]) == 0
        assert not got[2][by_name[name]].any()
    assert int(so["terms"][by_name["noise_H512_1ch"]]) == 1 and int(so["status"][by_name["noise_H512_1ch"]]) == 0
    r = so[by_name["silence"]]
    assert int(r["lag"]) == 0 and int(r["lag_peak"]) == 0 and int(r["status"]) == 0 and int(r["r0"]) == 0
    assert so[by_name["nyquist_hops"]].tobytes() == so[by_name["nyquist_hops_stereo"]].tobytes()   # mono = dual mono
    assert np.array_equal(got[2][by_name["nyquist_hops"]], got[2][by_name["nyquist_hops_stereo"]])


def test_other_lag_ranges(gpu_lib, corpus):
    some = [s for s in corpus if s[0].startswith(("click_", "noise_H640", "noise_H512", "silence", "dc_3"))]
    for lo, hi in ((1, 510), (1, 1), (510, 510), (100, 101), (44, 300)):
        assert_equal(run(gpu_lib, pairs(some), lo=lo, hi=hi), some, lo, hi, what=f"lags [{lo}, {hi}]")


def test_every_pcm_offset_that_is_a_multiple_of_8(gpu_lib, corpus):
    by_name = {name: (name, pcm, ch) for name, pcm, ch in corpus}
    names = ["noise_H19_1ch", "noise_H19_2ch", "noise_H513_1ch", "noise_H513_2ch", "noise_H3_1ch", "noise_H4_2ch",
             "noise_H640_1ch", "noise_H640_2ch"]
    for shift in range(8):
        named = [by_name[n] for n in names[shift:] + names[:shift]]
        offsets, off = [], 0
        for k, (_, pcm, _) in enumerate(named):       # song k sits at 8 k mod 64
            off = (off + 63) // 64 * 64 + 8 * k
            offsets.append(off)
            off += pcm.size
        assert sorted(o % 64 for o in offsets) == list(range(0, 64, 8))
        arena, items = place(pairs(named), offsets=offsets)
        c = Call(gpu_lib, arena, items)
        assert c.rc == 0
        assert_equal(c.read(), named, what=f"offsets shifted by {shift}")


@pytest.mark.parametrize("k", [0, 1], ids=["mono", "stereo"])
def test_long_song_alone_and_in_a_mixed_batch(gpu_lib, corpus, long_songs, k):
    """40 000 hops: the hop pass splits the song over many workgroups and the lag kernel over 39 chunks; inside a batch
    the split is another one (more songs share the grid), and the bytes are the same"""
    long = long_songs[k]
    alone = run(gpu_lib, pairs([long]))
    assert_equal(alone, [long], what="alone")
    assert int(alone[0]["hops"][0]) == rr.LONG_HOPS and int(alone[0]["lag"][0]) > 0
    pool = [s for s in corpus if s[0].startswith(("noise_H1500", "noise_H3_", "click_86", "noise_H511", "late"))]
    batch = pool[:3] + [long] + pool[3:]
    got = run(gpu_lib, pairs(batch))
    at = sum(rr.hops_of(p.size, c) for _, p, c in batch[:3])
    assert got[0][3].tobytes() == alone[0][0].tobytes()
    assert got[1][at:at + rr.LONG_HOPS].tobytes() == alone[1].tobytes()
    assert got[2][3].tobytes() == alone[2][0].tobytes()
    assert_equal(got, batch, what="batch")
    # permuting the batch permutes the records, the curves and the rows
    perm = [4, 0, 6, 3, 1, 5, 2] + list(range(7, len(batch)))
    got2 = run(gpu_lib, pairs([batch[j] for j in perm]))
    at2 = 0
    for i, j in enumerate(perm):
        h = rr.hops_of(batch[j][1].size, batch[j][2])
        atj = sum(rr.hops_of(p.size, c) for _, p, c in batch[:j])
        assert got2[0][i].tobytes() == got[0][j].tobytes() and got2[2][i].tobytes() == got[2][j].tobytes()
        assert got2[1][at2:at2 + h].tobytes() == got[1][atj:atj + h].tobytes()
        at2 += h


def test_optional_outputs_do_not_change_the_records(gpu_lib, corpus, long_songs):
    named = corpus[::3] + [long_songs[1]]
    full = run(gpu_lib, pairs(named))
    for onsets, acf in ((False, False), (True, False), (False, True)):
        so, oo, ao = run(gpu_lib, pairs(named), onsets=onsets, acf=acf)
        assert so.tobytes() == full[0].tobytes()
        assert (oo is None) == (not onsets) and (ao is None) == (not acf)
        assert oo is None or oo.tobytes() == full[1].tobytes()
        assert ao is None or ao.tobytes() == full[2].tobytes()
    # n_onsets is ignored without an onset output
    arena, items = place(pairs(named))
    c = Call(gpu_lib, arena, items, onsets=False, n_onsets=-5)
    assert c.rc == 0 and c.read()[0].tobytes() == full[0].tobytes()
    # outputs that start from zeros end the same: every byte is written
    zero = run(gpu_lib, pairs(named), fill=0)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(zero, full))


def test_context_form_and_two_contexts_on_two_streams(gpu_lib, corpus, long_songs):
    import torch
    half_a, half_b = corpus[0::2] + [long_songs[0]], corpus[1::2]
    want_a, want_b = run(gpu_lib, pairs(half_a)), run(gpu_lib, pairs(half_b))
    arena_a, items_a = place(pairs(half_a))
    arena_b, items_b = place(pairs(half_b))
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    with bliss_amd.Context(0) as ca, bliss_amd.Context(0) as cb:
        calls = []
        for _ in range(3):
            calls.append((Call(gpu_lib, arena_a, items_a, ctx=ca, stream=sa, defer=True), want_a))
            calls.append((Call(gpu_lib, arena_b, items_b, ctx=cb, stream=sb, defer=True), want_b))
            calls.append((Call(gpu_lib, arena_b, items_b, ctx=ca, stream=sa, acf=False, defer=True), want_b))
        torch.cuda.synchronize()    # the sentinels are in place; from here on nothing waits until every call is enqueued
        for c, _ in calls:
            c.rc = c.enqueue()
        assert all(c.rc == 0 for c, _ in calls)
        for c, want in calls:
            got = c.read()
            for g, w in zip(got, want):
                assert g is None or g.tobytes() == w.tobytes()
    assert_equal(want_a, half_a, what="half a")


def test_launch_groups_of_five_songs(gpu_lib, corpus, monkeypatch):
    """A context reads BL_AMD_GROUP_SONGS when it is created: with 5 the corpus' 38 songs run as eight launch groups that share
    the scratch one after the other, with the caller's rows and with rows of the library's own"""
    want = run(gpu_lib, pairs(corpus))
    monkeypatch.setenv("BL_AMD_GROUP_SONGS", "5")
    arena, items = place(pairs(corpus))
    with bliss_amd.Context(0) as ctx:
        for acf in (True, False):
            c = Call(gpu_lib, arena, items, ctx=ctx, acf=acf)
            assert c.rc == 0
            for g, w in zip(c.read(), want):
                assert g is None or g.tobytes() == w.tobytes()


def test_host_form_and_python_wrappers(gpu_lib, corpus):
    named = corpus
    want = run(gpu_lib, pairs(named), lo=30, hi=400)
    n = len(named)
    ptrs = (C.c_void_p * n)(*[p.ctypes.data for _, p, _ in named])
    ns = (C.c_int32 * n)(*[p.size for _, p, _ in named])
    chs = (C.c_int32 * n)(*[c for _, _, c in named])
    hs, ho, ha = (_lib.SongRhythm * n)(), (C.c_uint32 * want[1].size)(), (C.c_uint64 * (512 * n))()
    for buf in (hs, ho, ha):
        C.memset(buf, SENTINEL, C.sizeof(buf))
    assert gpu_lib.bl_amd_rhythm_batch_host(ptrs, ns, chs, n, 30, 400, hs, ho, ha) == 0
    assert bytes(hs) == want[0].tobytes() and bytes(ho) == want[1].tobytes() and bytes(ha) == want[2].tobytes()
    C.memset(hs, SENTINEL, C.sizeof(hs))
    assert gpu_lib.bl_amd_rhythm_batch_host(ptrs, ns, chs, n, 30, 400, hs, None, None) == 0
    assert bytes(hs) == want[0].tobytes()
    assert gpu_lib.bl_amd_rhythm_batch_host(ptrs, ns, chs, n, 30, 511, hs, None, None) == U
    # Python: the host form, and the free function on a corpus
    ps, po, pa = rh.rhythm_batch_host([p for _, p, _ in named], [c for _, _, c in named], 30, 400, acf=True)
    assert ps.tobytes() == want[0].tobytes() and po.tobytes() == want[1].tobytes() and pa.tobytes() == want[2].tobytes()
    ps, po, pa = rh.rhythm_batch_host([p for _, p, _ in named], [c for _, _, c in named], 30, 400, onsets=False)
    assert ps.tobytes() == want[0].tobytes() and po is None and pa is None
    dc = bliss_amd.DeviceCorpus([p.size for _, p, _ in named], [c for _, _, c in named], 1)
    dc.pcm.fill_(rr.ARENA_FILL)
    for i, (_, p, _) in enumerate(named):
        dc.upload(i, p)
    rec_t, ons_t, acf_t = rh.rhythm_device(dc, 30, 400, acf=True)
    assert rec_t.is_cuda and ons_t.numel() == want[1].size and tuple(acf_t.shape) == (n, 512)
    cs, co, ca = rh.fetch_rhythm(dc)
    assert cs.tobytes() == want[0].tobytes() and co.tobytes() == want[1].tobytes() and ca.tobytes() == want[2].tobytes()
    with bliss_amd.Context(0) as ctx:
        rh.rhythm_device(dc, 30, 400, onsets=False, ctx=ctx)
        cs, co, ca = rh.fetch_rhythm(dc)
    assert cs.tobytes() == want[0].tobytes() and co is None and ca is None
    # beats per minute and strength from the exact integers
    bpm, strength = rh.rhythm_bpm(cs)
    for i, (name, pcm, ch) in enumerate(named):
        rec = reference(name, pcm, ch, 30, 400)[0]
        w = rr.bpm(rec)
        assert (np.isnan(bpm[i]) and np.isnan(w)) or abs(bpm[i] - w) <= 1e-12 * w
        assert abs(strength[i] - rr.strength(rec)) <= 1e-12 * rr.strength(rec)
    i43 = [name for name, _, _ in named].index("click_43")
    assert abs(bpm[i43] - 60 * 22050 / (128 * 43)) < 2.5 and 0.8 < strength[i43] < 1.1


def test_rejections_write_nothing(gpu_lib):
    rng = np.random.default_rng(7400)
    songs = [(rng.integers(-3000, 3000, 600 * 128 * 2).astype(np.int16), 2), (rng.integers(-3000, 3000, 700).astype(np.int16), 1)]
    arena, items = place(songs)
    assert Call(gpu_lib, arena, items).rc == 0
    bad = [
        dict(items=[(0, items[0][1], 3), items[1]]), dict(items=[(0, items[0][1], 0), items[1]]),    # channels
        dict(items=[items[0], (items[1][0], 127, 1)]), dict(items=[items[0], (items[1][0], 255, 2)]),  # H = 0
        dict(n_onsets=604), dict(n_onsets=606), dict(n_onsets=0),                                    # sum of H is 605
        dict(lo=31, hi=30), dict(lo=0, hi=30), dict(lo=1, hi=511), dict(lo=511, hi=511), dict(lo=-1, hi=-1),
        dict(items=[items[0], (items[1][0] + 4, 700, 1)]), dict(items=[items[0], (items[1][0] + 1, 700, 1)]),
        dict(items=[]),
    ]
    for kw in bad:
        kw = dict(kw)
        its = kw.pop("items", items)
        c = Call(gpu_lib, arena, its, **kw)
        assert c.rc == U, kw
        assert c.untouched(), kw
    import torch
    desc = (_lib.SongDesc * 2)()
    for i, (at, ns, ch) in enumerate(items):
        desc[i].pcm_offset, desc[i].n_samples, desc[i].channels = at, ns, ch
    so = torch.full((2 * 72,), SENTINEL, dtype=torch.uint8, device="cuda")
    oo = torch.full((605 * 4,), SENTINEL, dtype=torch.uint8, device="cuda")
    ao = torch.full((2 * 4096,), SENTINEL, dtype=torch.uint8, device="cuda")
    p, s, o, a = arena.data_ptr(), so.data_ptr(), oo.data_ptr(), ao.data_ptr()
    fn = gpu_lib.bl_amd_rhythm_batch_device
    assert fn(None, desc, 2, LO, HI, s, o, 605, a, None) == U
    assert fn(p, None, 2, LO, HI, s, o, 605, a, None) == U
    assert fn(p, desc, 2, LO, HI, None, o, 605, a, None) == U
    assert fn(p + 8, desc, 2, LO, HI, s, o, 605, a, None) == U           # d_pcm not 16-byte aligned
    assert fn(p, desc, 2, LO, HI, s + 4, o, 605, a, None) == U
    assert fn(p, desc, 2, LO, HI, s, o + 2, 605, a, None) == U
    assert fn(p, desc, 2, LO, HI, s, o, 605, a + 4, None) == U
    assert gpu_lib.bl_amd_ctx_rhythm_batch_device(None, p, desc, 2, LO, HI, s, o, 605, a, None) == U
    torch.cuda.synchronize()
    for t in (so, oo, ao):
        assert bytes(t.cpu().numpy()) == bytes([SENTINEL]) * t.numel()


def _from_onsets(lib, curves, lo, hi, acf=True):
    n = len(curves)
    flat = np.ascontiguousarray(np.concatenate(curves), dtype=np.uint32)
    hops = (C.c_int32 * n)(*[c.size for c in curves])
    out, rows = (_lib.SongRhythm * n)(), (C.c_uint64 * (512 * n))()
    C.memset(out, SENTINEL, C.sizeof(out))
    C.memset(rows, SENTINEL, C.sizeof(rows))
    rc = lib.bl_amd_rhythm_from_onsets(flat.ctypes.data_as(C.POINTER(C.c_uint32)), hops, n, lo, hi, out,
                                       rows if acf else None)
    return rc, np.frombuffer(bytes(out), dtype=RHYTHM_DTYPE), np.frombuffer(bytes(rows), dtype=np.uint64).reshape(n, 512)


def _assert_curves(so, ao, curves, lo, hi):
    refs = []
    for i, o in enumerate(curves):
        rec, R = rr.record_from_onsets(o, lo, hi)
        for f in rr.FIELDS:
            assert int(so[f][i]) == rec[f], f"curve {i}: {f} {int(so[f][i])}, want {rec[f]}"
        if ao is not None:
            assert [int(x) for x in ao[i]] == R, f"curve {i}"
        refs.append((rec, R))
    return refs


def test_from_onsets_sums_beyond_2_to_the_53(gpu_lib):
    o = rr.big_curve()
    rc, so, ao = _from_onsets(gpu_lib, [o], 1, 510)
    assert rc == 0
    (rec, R), = _assert_curves(so, ao, [o], 1, 510)
    assert min(R) > 2 ** 53 and rec["terms"] == 140000 - 511 and rec["onset_max"] < 2 ** 18
    py = rh.rhythm_from_onsets([o], 1, 510)
    assert py.tobytes() == so.tobytes()


def test_from_onsets_takes_every_branch_of_the_pick(gpu_lib):
    H = 1400
    accents = np.zeros(H, np.int64)
    accents[0::100] = 1000
    accents[50::100] = 900                      # R[100] > R[50], within 1/16: the local-maximum rule picks 50
    slope = np.arange(H, 0, -1, dtype=np.int64) * 150   # R falls with the lag: the maximum sits at lag_min on a slope
    flat = np.full(H, 77, np.int64)             # every lag ties: the smallest wins
    impulse = np.zeros(H, np.int64)
    impulse[0] = 2 ** 18 - 1                    # r0 > 0 and nothing else: r_peak = 0
    zeros = np.zeros(H, np.int64)
    short = np.arange(100, dtype=np.int64)      # H < 512
    edge = np.zeros(600, np.int64)
    edge[[0, 88]] = 5                           # T = 89: only R[0] and R[88] are non-zero
    curves = [accents, slope, flat, impulse, zeros, short, edge, rr.big_curve()[:5000].astype(np.int64)]
    rc, so, ao = _from_onsets(gpu_lib, curves, 10, 200)
    assert rc == 0
    refs = _assert_curves(so, ao, curves, 10, 200)
    (r_acc, _), (r_slope, R_slope), (r_flat, _), (r_imp, _), (r_zero, _), (r_short, _), (r_edge, _) = refs[:7]
    assert (r_acc["lag"], r_acc["lag_peak"]) == (50, 100) and r_acc["r_lag"] < r_acc["r_peak"]
    assert r_slope["lag"] == r_slope["lag_peak"] == 10 and R_slope[9] > R_slope[10] > R_slope[11]   # the fallback
    assert r_flat["lag"] == r_flat["lag_peak"] == 10 and r_flat["r_prev"] == r_flat["r_lag"] == r_flat["r_peak"]
    assert (r_imp["lag"], r_imp["lag_peak"], r_imp["r_peak"], r_imp["r_prev"]) == (0, 0, 0, 0) and r_imp["r0"] == (2 ** 18 - 1) ** 2
    assert r_zero["lag"] == 0 and r_zero["r0"] == 0 and r_zero["status"] == 0
    assert r_short["status"] == U and r_short["hops"] == 100 and r_short["onset_sum"] == 0
    assert (r_edge["lag"], r_edge["r_lag"], r_edge["r0"]) == (88, 25, 50)
    # the same without the rows; another range moves the pick only
    rc, so2, _ = _from_onsets(gpu_lib, curves, 10, 200, acf=False)
    assert rc == 0 and so2.tobytes() == so.tobytes()
    rc, so3, ao3 = _from_onsets(gpu_lib, curves, 60, 510)
    assert rc == 0 and ao3.tobytes() == ao.tobytes()
    _assert_curves(so3, ao3, curves, 60, 510)
    # the Python wrapper
    py, rows = rh.rhythm_from_onsets(curves, 10, 200, acf=True)
    assert py.tobytes() == so.tobytes() and rows.tobytes() == ao.tobytes()
    # refusals: a value of 2^18, hops < 1, a bad range
    bad = accents.copy()
    bad[700] = 2 ** 18
    assert _from_onsets(gpu_lib, [flat, bad], 10, 200)[0] == U
    assert _from_onsets(gpu_lib, [flat], 10, 511)[0] == U
    out = (_lib.SongRhythm * 1)()
    flat32 = flat.astype(np.uint32)
    assert gpu_lib.bl_amd_rhythm_from_onsets(flat32.ctypes.data_as(C.POINTER(C.c_uint32)), (C.c_int32 * 1)(0), 1, 10, 200,
                                             out, None) == U


def test_the_analysis_is_untouched(gpu_lib, corpus):
    songs = [s for s in corpus if s[0].startswith("click_")]
    dc = bliss_amd.DeviceCorpus([p.size for _, p, _ in songs], [c for _, _, c in songs], [7, 8, 9, 11])
    for i, (_, p, _) in enumerate(songs):
        dc.upload(i, p)
    total = sum(2 * (p.size // 512) for _, p, _ in songs)

    def energies():
        en = np.zeros(total, dtype=np.float32)
        assert gpu_lib.bl_amd_last_energies(en.ctypes.data_as(C.POINTER(C.c_float)), total) == total
        return en
    dc.analyze()
    res = dc.fetch().tobytes()
    en, st = energies(), bliss_amd.last_freq_stats()
    run(gpu_lib, pairs(corpus))
    run(gpu_lib, pairs(songs), onsets=False, acf=False)
    en2, st2 = energies(), bliss_amd.last_freq_stats()
    assert en2.tobytes() == en.tobytes() and st2["n_songs"] == st["n_songs"] == len(songs) and st2["parts"] == st["parts"]
    for name in ("spectrum", "sum", "sumsq", "hist"):
        assert st2[name].tobytes() == st[name].tobytes(), name
    dc.analyze()
    assert dc.fetch().tobytes() == res
