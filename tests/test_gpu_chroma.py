"""Chroma and key on the GPU (bl_amd_chroma_batch_device, bl_amd_ctx_chroma_batch_device, bl_amd_chroma_batch_host,
bliss_amd.chroma): every frame's twelve sums and every field of bl_amd_song_chroma are exact integers and are compared
with == against tests/chroma_reference.py.  There is no tolerance anywhere.

Every arena is filled with 32767 before the songs are placed and the outputs with 0xA5 before the call, so a read outside
a song's frames and a byte the kernels do not write both show.  The corpus is tests/chroma_reference.py's, whose
deliberate mistakes tests/test_chroma_reference_host.py shows to change a named song of it.  The reference of each song
is computed once per session and shared."""
import ctypes as C

import numpy as np
import pytest

import bliss_amd
import bliss_amd.chroma as ch
from bliss_amd import _lib
from bliss_amd.records import CHROMA_DTYPE, FRAME_CHROMA_DTYPE
from tests import chroma_reference as cr

pytestmark = pytest.mark.gpu

U = _lib.BL_UNEXPECTED
SENTINEL = 0xA5
SCALARS = ("score", "score_next", "frames", "key", "status", "reserved")
_REF = {}


def reference(name, pcm, chn):
    if name not in _REF:
        _REF[name] = cr.song(pcm, chn)
    return _REF[name]


# ---- running the library -----------------------------------------------------------------------------------------

def place(songs, offsets=None):
    """(torch int16 arena filled with 32767, list of (pcm_offset, n_samples, channels)): the songs at multiples of 8
    samples one behind the other, or at `offsets`"""
    import torch
    items, off = [], 0
    for i, (pcm, chn) in enumerate(songs):
        at = offsets[i] if offsets is not None else off
        items.append((at, pcm.size, chn))
        off = at + ((pcm.size + 7) & ~7)
    end = max(at + n for at, n, _ in items)
    host = np.full(end + 64, cr.ARENA_FILL, dtype=np.int16)
    for (at, n, _), (pcm, _) in zip(items, songs):
        host[at:at + n] = pcm
    return torch.from_numpy(host).cuda(), items


class Call:
    """one call whose outputs were filled with `fill`; read() waits for the device"""

    def __init__(self, lib, arena, items, frames=True, ctx=None, n_records=None, fill=SENTINEL, stream=None, defer=False):
        import torch
        n = len(items)
        desc = (_lib.SongDesc * max(n, 1))()
        for i, (at, ns, chn) in enumerate(items):
            desc[i].pcm_offset, desc[i].n_samples, desc[i].channels, desc[i].duration = at, ns, chn, 0
        self.n = n
        self.total = sum(cr.frames_of(ns, chn) if chn in (1, 2) and ns >= 0 else 0 for _, ns, chn in items)
        self.so = torch.full((max(n, 1) * 128,), fill, dtype=torch.uint8, device="cuda")
        self.fo = torch.full((max(self.total, 1) * 96,), fill, dtype=torch.uint8, device="cuda") if frames else None
        args = (C.c_void_p(arena.data_ptr()), desc, n, C.c_void_p(self.so.data_ptr()),
                C.c_void_p(self.fo.data_ptr()) if frames else None, self.total if n_records is None else n_records,
                C.c_void_p(stream.cuda_stream) if stream is not None else None)
        self.enqueue = ((lambda: lib.bl_amd_chroma_batch_device(*args)) if ctx is None
                        else (lambda: lib.bl_amd_ctx_chroma_batch_device(ctx.handle, *args)))
        self.rc = None if defer else self.enqueue()

    def read(self):
        import torch
        torch.cuda.synchronize()
        so = np.frombuffer(self.so.cpu().numpy().tobytes(), dtype=CHROMA_DTYPE)[:self.n]
        fo = None if self.fo is None else np.frombuffer(self.fo.cpu().numpy().tobytes(),
                                                        dtype=FRAME_CHROMA_DTYPE)[:self.total]
        return so, fo

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return all(t is None or bytes(t.cpu().numpy()) == bytes([SENTINEL]) * t.numel() for t in (self.so, self.fo))


def run(lib, songs, **kw):
    arena, items = place(songs)
    c = Call(lib, arena, items, **kw)
    assert c.rc == 0
    return c.read()


def assert_equal(got, named, what=""):
    """got: (records, frames or None); named: [(name, pcm, channels)] in the call's order"""
    so, fo = got
    at = 0
    for i, (name, pcm, chn) in enumerate(named):
        rec, X = reference(name, pcm, chn)
        where = f"{what} song {i} {name} ({chn} ch, T {X.shape[0]})"
        got_chroma = [int(v) for v in so["chroma"][i]]
        assert got_chroma == rec["chroma"], f"{where}: chroma {got_chroma}, want {rec['chroma']}"
        for f in SCALARS:
            assert int(so[f][i]) == rec[f], f"{where}: {f} {int(so[f][i])}, want {rec[f]}"
        if fo is not None:
            g = fo["x"][at:at + X.shape[0]].astype(np.int64)
            if not np.array_equal(g, X):
                t, k = (int(v[0]) for v in np.nonzero(g != X))
                raise AssertionError(f"{where}: X[{t}][{k}] {int(g[t, k])}, want {int(X[t, k])}; "
                                     f"{int((g != X).sum())} of {X.size} values differ")
        at += X.shape[0]
    if fo is not None:
        assert at == fo.size


@pytest.fixture(scope="module")
def corpus():
    return [(name, pcm, chn) for name, (pcm, chn) in cr.corpus().items()]


def pairs(named):
    return [(pcm, chn) for _, pcm, chn in named]


def pick(corpus, *prefixes):
    return [s for s in corpus if s[0].startswith(prefixes)]


# ---- tests -------------------------------------------------------------------------------------------------------

def test_corpus_in_one_mixed_batch(gpu_lib, corpus):
    got = run(gpu_lib, pairs(corpus))
    assert_equal(got, corpus, what="corpus")
    so = got[0]
    by_name = {name: i for i, (name, _, _) in enumerate(corpus)}
    assert {int(t) for t in so["frames"]} >= set(cr.SHAPES_T) | {0, 70, 71}
    for name in ("short_Fr1_1ch", "short_Fr1_2ch", "short_Fr4095_1ch", "short_Fr4095_2ch"):
        r = so[by_name[name]]
        assert int(r["status"]) == U and int(r["key"]) == -1 and int(r["frames"]) == 0 and not r["chroma"].any()
    r = so[by_name["silence"]]
    assert int(r["status"]) == 0 and int(r["key"]) == -1 and int(r["frames"]) == 3 and int(r["score"]) == 0
    for p in cr.TONES:                                  # a tone's class carries most of the energy
        r = so[by_name[f"tone_{p}"]]
        assert int(np.argmax(r["chroma"])) == (p + 9) % 12
    assert int(so["key"][by_name["c_major"]]) == 0 and int(so["key"][by_name["a_minor"]]) == 21
    r = so[by_name["tie"]]
    assert int(r["score"]) == int(r["score_next"]) > 0 and int(r["key"]) == reference("tie", *cr.corpus()["tie"])[0]["key"]
    for mono, dual in (("tone_13", "tone_13_dual"), ("noise_T3_1ch", "noise_T3_dual")):   # mono = dual mono
        assert so[by_name[mono]].tobytes() == so[by_name[dual]].tobytes()


def test_every_pcm_offset_that_is_a_multiple_of_8(gpu_lib, corpus):
    by_name = {name: (name, pcm, chn) for name, pcm, chn in corpus}
    names = ["noise_T1_1ch", "noise_T2_2ch", "noise_T3_1ch", "noise_T1_2ch", "short_Fr4095_2ch", "noise_T17_1ch",
             "noise_T2_1ch", "noise_T16_2ch"]
    for shift in (0, 3):
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


def test_a_song_alone_in_a_batch_of_50_and_in_another_order(gpu_lib, corpus):
    for name in ("noise_T70_1ch", "noise_T71_2ch", "noise_T17_2ch"):
        song = next(s for s in corpus if s[0] == name)
        alone = run(gpu_lib, pairs([song]))
        assert_equal(alone, [song], what="alone")
        pool = [s for s in corpus if s[0] != name]
        batch = (pool + pool)[:49]
        batch.insert(20, song)
        assert len(batch) == 50
        got = run(gpu_lib, pairs(batch))
        T = alone[1].size
        at = sum(cr.frames_of(p.size, c) for _, p, c in batch[:20])
        assert got[0][20].tobytes() == alone[0][0].tobytes()
        assert got[1][at:at + T].tobytes() == alone[1].tobytes()
        rev = batch[::-1]
        got2 = run(gpu_lib, pairs(rev))
        at2 = sum(cr.frames_of(p.size, c) for _, p, c in rev[:29])
        assert got2[0][::-1].tobytes() == got[0].tobytes()
        assert got2[1][at2:at2 + T].tobytes() == alone[1].tobytes()
    assert_equal(got, batch, what="batch of 50")


def test_frames_are_optional_and_every_byte_is_written(gpu_lib, corpus):
    full = run(gpu_lib, pairs(corpus))
    so, fo = run(gpu_lib, pairs(corpus), frames=False)
    assert fo is None and so.tobytes() == full[0].tobytes()
    arena, items = place(pairs(corpus))
    c = Call(gpu_lib, arena, items, frames=False, n_records=-5)    # n_frame_records is ignored without the output
    assert c.rc == 0 and c.read()[0].tobytes() == full[0].tobytes()
    zero = run(gpu_lib, pairs(corpus), fill=0)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(zero, full))


def test_context_form_on_side_streams(gpu_lib, corpus):
    import torch
    half_a, half_b = corpus[0::2], corpus[1::2]
    want_a, want_b = run(gpu_lib, pairs(half_a)), run(gpu_lib, pairs(half_b))
    arena_a, items_a = place(pairs(half_a))
    arena_b, items_b = place(pairs(half_b))
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    with bliss_amd.Context(0) as ca, bliss_amd.Context(0) as cb:
        calls = []
        for _ in range(2):
            calls.append((Call(gpu_lib, arena_a, items_a, ctx=ca, stream=sa, defer=True), want_a))
            calls.append((Call(gpu_lib, arena_b, items_b, ctx=cb, stream=sb, defer=True), want_b))
            calls.append((Call(gpu_lib, arena_b, items_b, ctx=ca, stream=sa, frames=False, defer=True), want_b))
        torch.cuda.synchronize()    # the sentinels are in place; from here on nothing waits until every call is enqueued
        for c, _ in calls:
            c.rc = c.enqueue()
        assert all(c.rc == 0 for c, _ in calls)
        for c, want in calls:
            for g, w in zip(c.read(), want):
                assert g is None or g.tobytes() == w.tobytes()
    assert_equal(want_a, half_a, what="half a")
    assert_equal(want_b, half_b, what="half b")


def test_launch_groups_of_five_songs(gpu_lib, corpus, monkeypatch):
    """A context reads BL_AMD_GROUP_SONGS when it is created: with 5 the corpus runs as launch groups that follow each
    other on the stream"""
    want = run(gpu_lib, pairs(corpus))
    monkeypatch.setenv("BL_AMD_GROUP_SONGS", "5")
    arena, items = place(pairs(corpus))
    with bliss_amd.Context(0) as ctx:
        for frames in (True, False):
            c = Call(gpu_lib, arena, items, ctx=ctx, frames=frames)
            assert c.rc == 0
            for g, w in zip(c.read(), want):
                assert g is None or g.tobytes() == w.tobytes()


def test_host_form_and_python_wrappers(gpu_lib, corpus):
    named = corpus
    want = run(gpu_lib, pairs(named))
    n = len(named)
    ptrs = (C.c_void_p * n)(*[p.ctypes.data for _, p, _ in named])
    ns = (C.c_int32 * n)(*[p.size for _, p, _ in named])
    chs = (C.c_int32 * n)(*[c for _, _, c in named])
    hs, hf = (_lib.SongChroma * n)(), (_lib.FrameChroma * want[1].size)()
    for buf in (hs, hf):
        C.memset(buf, SENTINEL, C.sizeof(buf))
    assert gpu_lib.bl_amd_chroma_batch_host(ptrs, ns, chs, n, hs, hf) == 0
    assert bytes(hs) == want[0].tobytes() and bytes(hf) == want[1].tobytes()
    C.memset(hs, SENTINEL, C.sizeof(hs))
    assert gpu_lib.bl_amd_chroma_batch_host(ptrs, ns, chs, n, hs, None) == 0
    assert bytes(hs) == want[0].tobytes()
    assert gpu_lib.bl_amd_chroma_batch_host(ptrs, ns, chs, 0, hs, None) == U
    # Python: the host form, and the free function on a corpus
    ps, pf = ch.chroma_batch_host([p for _, p, _ in named], [c for _, _, c in named], frames=True)
    assert ps.tobytes() == want[0].tobytes() and pf.tobytes() == want[1].tobytes()
    ps, pf = ch.chroma_batch_host([p for _, p, _ in named], [c for _, _, c in named])
    assert ps.tobytes() == want[0].tobytes() and pf is None
    dc = bliss_amd.DeviceCorpus([p.size for _, p, _ in named], [c for _, _, c in named], 1)
    dc.pcm.fill_(cr.ARENA_FILL)
    for i, (_, p, _) in enumerate(named):
        dc.upload(i, p)
    rec_t, fr_t = ch.chroma_device(dc, frames=True)
    assert rec_t.is_cuda and fr_t.numel() == want[1].size * 96
    cs, cf = ch.fetch_chroma(dc)
    assert cs.tobytes() == want[0].tobytes() and cf.tobytes() == want[1].tobytes()
    with bliss_amd.Context(0) as ctx:
        ch.chroma_device(dc, ctx=ctx)
        cs, cf = ch.fetch_chroma(dc)
    assert cs.tobytes() == want[0].tobytes() and cf is None
    names = ch.key_names(cs)
    assert names == [cr.key_name(int(k)) for k in cs["key"]]
    by_name = {name: i for i, (name, _, _) in enumerate(named)}
    assert names[by_name["c_major"]] == "C" and names[by_name["a_minor"]] == "Am" and names[by_name["silence"]] == ""


def test_host_form_in_waves(gpu_lib, corpus, tmp_path):
    """BL_AMD_HOST_WAVE_BYTES is read when the default context is created, so the waves need a process of their own:
    64 KiB per wave cuts these songs into several waves, whose frame records must still follow each other"""
    import os
    import subprocess
    import sys
    names = [s[0] for s in pick(corpus, "noise_T1_", "noise_T3_", "short_", "tone_", "noise_T15_")]
    named = [s for s in corpus if s[0] in names]
    want = run(gpu_lib, pairs(named))
    code = ("import sys, numpy as np, bliss_amd.chroma as ch\n"
            "from tests import chroma_reference as cr\n"
            "c = cr.corpus(); names = sys.argv[2].split(',')\n"
            "s, f = ch.chroma_batch_host([c[n][0] for n in names], [c[n][1] for n in names], frames=True)\n"
            "np.savez(sys.argv[1], s=np.frombuffer(s.tobytes(), np.uint8), f=np.frombuffer(f.tobytes(), np.uint8))\n")
    out = str(tmp_path / "waves.npz")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code, out, ",".join(names)], cwd=root, text=True, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300,
                       env=dict(os.environ, BL_AMD_HOST_WAVE_BYTES=str(64 * 1024), PYTHONPATH=root))
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    assert got["s"].tobytes() == want[0].tobytes() and got["f"].tobytes() == want[1].tobytes()


def test_rejections_write_nothing(gpu_lib, corpus):
    songs = pairs(pick(corpus, "noise_T2_2ch", "noise_T3_1ch"))
    arena, items = place(songs)
    assert Call(gpu_lib, arena, items).rc == 0
    total = sum(cr.frames_of(ns, chn) for _, ns, chn in items)
    bad = [
        dict(items=[(0, items[0][1], 3), items[1]]), dict(items=[(0, items[0][1], 0), items[1]]),    # channels
        dict(items=[items[0], (items[1][0], 0, 1)]), dict(items=[items[0], (items[1][0], 1, 2)]),    # Fr = 0
        dict(items=[items[0], (items[1][0], -4, 1)]),
        dict(n_records=total - 1), dict(n_records=total + 1), dict(n_records=0),
        dict(items=[items[0], (items[1][0] + 4, items[1][1] - 8, 1)]),                               # misaligned offsets
        dict(items=[items[0], (items[1][0] + 1, items[1][1] - 8, 1)]),
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
    for i, (at, ns, chn) in enumerate(items):
        desc[i].pcm_offset, desc[i].n_samples, desc[i].channels = at, ns, chn
    so = torch.full((2 * 128,), SENTINEL, dtype=torch.uint8, device="cuda")
    fo = torch.full((total * 96,), SENTINEL, dtype=torch.uint8, device="cuda")
    p, s, f = arena.data_ptr(), so.data_ptr(), fo.data_ptr()
    fn = gpu_lib.bl_amd_chroma_batch_device
    assert fn(None, desc, 2, s, f, total, None) == U
    assert fn(p, None, 2, s, f, total, None) == U
    assert fn(p, desc, 2, None, f, total, None) == U
    assert fn(p + 8, desc, 2, s, f, total, None) == U           # d_pcm not 16-byte aligned
    assert fn(p, desc, 2, s + 4, f, total, None) == U
    assert fn(p, desc, 2, s, f + 4, total, None) == U
    assert fn(p, desc, 0, s, f, total, None) == U
    assert gpu_lib.bl_amd_ctx_chroma_batch_device(None, p, desc, 2, s, f, total, None) == U
    torch.cuda.synchronize()
    for t in (so, fo):
        assert bytes(t.cpu().numpy()) == bytes([SENTINEL]) * t.numel()


def test_profile_names(gpu_lib, corpus):
    gpu_lib.bl_amd_profile(1)
    gpu_lib.bl_amd_profile_reset()
    run(gpu_lib, pairs(corpus[:6]))
    n = C.c_int(0)
    for name in (b"chroma_pitch", b"chroma_key"):
        ms = gpu_lib.bl_amd_profile_ms(name, C.byref(n))
        assert ms >= 0.0 and n.value == 1, name
    gpu_lib.bl_amd_profile(0)


def test_the_analysis_is_untouched(gpu_lib, corpus):
    songs = pick(corpus, "noise_T15", "noise_T16_1ch", "tone_0")
    dc = bliss_amd.DeviceCorpus([p.size for _, p, _ in songs], [c for _, _, c in songs], [7, 8, 9, 11][:len(songs)])
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
    run(gpu_lib, pairs(songs), frames=False)
    en2, st2 = energies(), bliss_amd.last_freq_stats()
    assert en2.tobytes() == en.tobytes() and st2["n_songs"] == st["n_songs"] == len(songs) and st2["parts"] == st["parts"]
    for name in ("spectrum", "sum", "sumsq", "hist"):
        assert st2[name].tobytes() == st[name].tobytes(), name
    dc.analyze()
    assert dc.fetch().tobytes() == res
