"""K-weighted gated loudness on the GPU (bl_amd_loud_batch_device, its context and host forms, bl_amd_loud_from_hops,
bliss_amd.loudness): the hop energies Z and every field of bl_amd_song_loud are compared with == against
tests/loud_reference.py.  There is no tolerance anywhere except the standards' own on the EBU sequences.

The outputs are filled with 0xA5 before the call, so a byte the kernels do not write shows, and the arena between the
songs holds noise, so a sample read from outside a song would show in its result.  The shapes are the smallest at which
the kernels take another path: hop counts around the chunk of 16 and the block of 4, hops of 1 (a chunk shorter than a
row of the staging), odd hops, warm-ups of 0, less than a row, a row and more than a whole chunk.  The reference of a
(batch, parameters) is computed once per session and shared."""
import ctypes as C
import math

import numpy as np
import pytest

import bliss_amd
import bliss_amd.loudness as ld
from bliss_amd import _lib
from bliss_amd.records import LOUD_DTYPE
from tests import loud_reference as lr

pytestmark = pytest.mark.gpu

EBU_3341, ORDER, sine = lr.EBU_3341, lr.ORDER, lr.sine
U = _lib.BL_UNEXPECTED
SENTINEL = 0xA5
HS = (0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49)
_REF = {}


def params_of(p):
    q = lr.plain(p)
    return ld.params(q.s1_b, q.s1_a, q.s2_a, q.hop, q.warm, q.abs_gate)


def reference(songs, p):
    key = (tuple((x.tobytes(), ch) for x, ch in songs), repr(lr.plain(p)))
    if key not in _REF:
        _REF[key] = lr.loud([x for x, _ in songs], [ch for _, ch in songs], p)
    return _REF[key]


# ---- running the library -----------------------------------------------------------------------------------------

class Call:
    """one device call on `songs` = [(pcm, channels)] laid out with gaps of noise; the outputs were filled with 0xA5.
    `stream`: a torch stream instead of the default one; `defer`: the call is made by go() (tests/test_gpu_side_ws.py)"""

    def __init__(self, lib, songs, p, hops=True, ctx=None, gap=8, n=None, n_hops=None, shift=(0, 0, 0), out=True,
                 channels=None, stream=None, defer=False):
        import torch
        self.p = params_of(p)
        hop = int(self.p.hop)
        self.n = len(songs) if n is None else n
        self.H = [x.size // ch // hop for x, ch in songs]
        self.total = sum(self.H)
        rng = np.random.default_rng(99)
        size = sum(((x.size + 7) & ~7) + gap for x, _ in songs) + gap + 64
        arena = rng.integers(-32768, 32768, size).astype(np.int16)
        desc = (_lib.SongDesc * len(songs))()
        at = gap
        for i, (x, ch) in enumerate(songs):
            arena[at:at + x.size] = x
            desc[i] = _lib.SongDesc(at, x.size, ch if channels is None else channels[i], 0)
            at += ((x.size + 7) & ~7) + gap
        self.arena = torch.from_numpy(arena).cuda()

        def fill(nbytes):
            return torch.full((nbytes + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.so = fill(len(songs) * 88)
        self.zo = fill(self.total * 16) if hops else None
        args = (C.c_void_p(self.arena.data_ptr() + shift[0]), desc, self.n, C.byref(self.p),
                C.c_void_p(self.so.data_ptr() + shift[1]) if out else None,
                C.c_void_p(self.zo.data_ptr() + shift[2]) if hops else None,
                self.total if n_hops is None else n_hops)
        self._call = ((lib.bl_amd_loud_batch_device, args) if ctx is None
                      else (lib.bl_amd_ctx_loud_batch_device, (ctx.handle,) + args))
        self.rc = None if defer else self.go(stream)

    def go(self, stream=None):
        fn, args = self._call
        self.rc = fn(*args, None if stream is None else C.c_void_p(stream.cuda_stream))
        return self.rc

    def _host(self, t, nbytes):
        raw = t.cpu().numpy()
        assert (raw[nbytes:] == SENTINEL).all(), "written past the end"
        return raw[:nbytes].tobytes()

    def read(self):
        import torch
        torch.cuda.synchronize()
        rec = np.frombuffer(self._host(self.so, self.n * 88), dtype=LOUD_DTYPE)
        z = None if self.zo is None else np.frombuffer(self._host(self.zo, self.total * 16),
                                                       dtype=np.uint64).reshape(-1, 2)
        return rec, z

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return all(t is None or bool((t == SENTINEL).all()) for t in (self.so, self.zo))


def run(lib, songs, p, **kw):
    c = Call(lib, songs, p, **kw)
    assert c.rc == 0
    return c.read()


def assert_equal(got, songs, p, what=""):
    rec, z = got
    want_rec, want_z = reference(songs, p)
    at = 0
    for i, (x, ch) in enumerate(songs):
        H = want_z[i].shape[0]
        where = f"{what} song {i} (H {H}, {ch} channels, hop {p.hop}, warm {p.warm})"
        if z is not None:
            g = z[at:at + H]
            if not np.array_equal(g, want_z[i]):
                h = int(np.flatnonzero((g != want_z[i]).any(axis=1))[0])
                raise AssertionError(f"{where}: Z of hop {h} {g[h].tolist()}, want {want_z[i][h].tolist()}; "
                                     f"{int((g != want_z[i]).any(axis=1).sum())} hops differ")
        g = lr.rec_ints(rec, i)
        for f in lr.FIELDS:
            assert g[f] == want_rec[i][f], f"{where}: {f} {g[f]}, want {want_rec[i][f]}"
        at += H
    assert z is None or at == z.shape[0]


# ---- material -----------------------------------------------------------------------------------------------------

def noise(frames, ch, seed, amp=32768):
    x = np.random.default_rng(seed).integers(-amp, amp, frames * ch).astype(np.int16)
    x[x.size // 2:] //= 8   # the second half 18 dB down: under the relative gate, a mono one at the absolute gate (GATE)
    if x.size >= 4:
        x[0], x[-1], x[x.size // 2] = -32768, 32767, -32768
    return x


def batch(hop, seed=0):
    """every hop count of HS, mono and stereo alternating, each with a partial hop behind its last whole one, and the
    alternating full-scale song"""
    songs = []
    for k, H in enumerate(HS):
        ch = 1 + (k + seed) % 2
        frames = H * hop + hop // 2
        if frames == 0:   # no whole hop at a hop of 1: half a stereo frame
            songs.append((np.array([12345], dtype=np.int16), 2))
            continue
        songs.append((noise(frames, ch, 10 * seed + k), ch))
    full = np.tile(np.array([32767, 32767, -32768, -32768], dtype=np.int16), (17 * hop + 1) // 2 + 1)[:2 * (17 * hop)]
    songs.append((full, 2))
    songs.append((np.tile(np.array([32767, -32768], dtype=np.int16), 9 * hop)[:18 * hop], 1))
    return songs


KW = lr.kweight(22050)
GATE = 10_000_000   # per frame of a block: between the quiet halves of the mono and the stereo noise


@pytest.mark.parametrize("warm", [0, 5, 64, 4096])
@pytest.mark.parametrize("hop", [1, 7, 32, 100, 441])
def test_every_shape_matches_the_reference(lib, hop, warm):
    """the gate sits at the quiet halves of the mono songs, so both gates remove blocks (the thresholds themselves are
    pinned through from_hops below)"""
    p = lr.plain(KW, hop=hop, warm=warm, abs_gate=hop * 4 * GATE)
    songs = batch(hop, seed=hop % 2)
    assert_equal(run(lib, songs, p), songs, p)


def test_summation_order_shows_on_the_device(lib):
    """the input on which another order of the five terms changes a floored energy (test_loud_reference_host.py)"""
    songs = [(np.full(8, 4, dtype=np.int16), 1), (np.full(16, 4, dtype=np.int16), 2)]
    assert_equal(run(lib, songs, ORDER), songs, ORDER)
    want = lr.loud([songs[0][0]], [1], ORDER, ("sum_order",))[1][0]
    assert not np.array_equal(run(lib, songs, ORDER)[1][:8], want)


def test_state_decays_to_zero_under_silence(lib):
    """a fast-decaying coefficient set, a burst, then silence: inside one chunk the state runs down through the smallest
    f64 values to 0.  This is the issue's case; it cannot tell honoured denormals from flushed ones (a denormal y has
    y * y = 0 either way), which is what the next test is for."""
    p = lr.plain(KW, s1_b=[1.0, 0.25, 0.125], s1_a=[-0.013, 0.00004], s2_a=[-0.01, 0.00002], hop=32, warm=5, abs_gate=10)
    burst = np.zeros(2 * 40 * 32, dtype=np.int16)
    burst[:40] = noise(20, 2, 3)
    mono = np.zeros(50 * 32, dtype=np.int16)
    mono[700:720] = noise(20, 1, 4)
    songs = [(burst, 2), (mono, 1)]
    assert_equal(run(lib, songs, p), songs, p)


def test_denormals_are_honoured(lib):
    """A coefficient set that brings a denormal state back into the normal range: b0 = 2^-1040 makes v0 = 2^-1030 of a
    sample of 1024, a denormal product, and A1 = -2^519 multiplies it up twice, y1 = 2^-511 and y2 = 2^8, so the one hop
    of three frames has Z = 2^16 (2^14 for the other channel's 512).  A device that flushed f64 denormals, as inputs or
    as results, would give 0."""
    p = lr.plain(KW, s1_b=[2.0 ** -1040, 0.0, 0.0], s1_a=[0.0, 0.0], s2_a=[-(2.0 ** 519), 0.0], hop=3, warm=0, abs_gate=0)
    songs = [(np.array([1024, 0, 0], dtype=np.int16), 1), (np.array([1024, 512, 0, 0, 0, 0], dtype=np.int16), 2)]
    want = reference(songs, p)[1]
    assert want[0].tolist() == [[1 << 16, 0]] and want[1].tolist() == [[1 << 16, 1 << 14]]
    assert 0.0 < 2.0 ** -1040 * 1024.0 < 2.3e-308
    assert_equal(run(lib, songs, p), songs, p)


def test_batch_size_order_and_optional_output_leave_the_bytes_alone(lib):
    hop = 7
    p = lr.plain(KW, hop=hop, warm=64, abs_gate=hop * 4 * GATE)
    base = batch(hop)
    many = [base[i % len(base)] for i in range(67)]
    rec67, z67 = run(lib, many, p)
    assert_equal((rec67, z67), many, p, "67 songs")
    rec_no, _ = run(lib, many, p, hops=False)
    assert rec_no.tobytes() == rec67.tobytes(), "the records depend on the optional output"
    starts = np.concatenate([[0], np.cumsum([x.size // ch // hop for x, ch in many])])
    perm = np.random.default_rng(4).permutation(67)
    recp, zp = run(lib, [many[i] for i in perm], p)
    at = 0
    for k, i in enumerate(perm):
        H = int(starts[i + 1] - starts[i])
        assert recp[k].tobytes() == rec67[i].tobytes(), f"song {i} differs at position {k}"
        assert zp[at:at + H].tobytes() == z67[starts[i]:starts[i + 1]].tobytes(), f"Z of song {i} differs"
        at += H
    for count in (1, 2):
        for first in (8, 9, 15):   # H = 17 stereo, H = 31 mono, the full-scale song
            sub = many[first:first + count]
            rec, z = run(lib, sub, p)
            assert rec.tobytes() == rec67[first:first + count].tobytes()
            assert z.tobytes() == z67[starts[first]:starts[first + count]].tobytes()
            assert run(lib, sub, p, hops=False)[0].tobytes() == rec.tobytes()


def test_context_form_and_gaps(lib):
    hop = 32
    p = lr.plain(KW, hop=hop, warm=5, abs_gate=hop * 4 * GATE)
    songs = batch(hop)
    with bliss_amd.Context(0) as ctx:
        assert_equal(run(lib, songs, p, ctx=ctx, gap=24), songs, p, "context")
        assert_equal(run(lib, songs, p, ctx=ctx, gap=0, hops=False), songs, p, "context, no gaps")


def test_the_workspace_goes_with_its_context(lib):
    """three contexts one after the other, each created, called and destroyed: the loudness workspace of a context is
    freed with it, and a new context (at the same address or not) starts from none"""
    hop = 7
    p = lr.plain(KW, hop=hop, warm=64, abs_gate=hop * 4 * GATE)
    songs = batch(hop)
    for k in range(3):
        with bliss_amd.Context(0) as ctx:
            assert_equal(run(lib, songs, p, ctx=ctx, hops=bool(k & 1)), songs, p, f"context {k}")
    assert_equal(run(lib, songs, p), songs, p, "default context afterwards")


def test_rejected_calls_write_nothing(lib):
    hop = 7
    p = lr.plain(KW, hop=hop, warm=5, abs_gate=1000)
    songs = batch(hop)[:4]
    bad = [dict(n=0), dict(n_hops=1), dict(shift=(2, 0, 0)), dict(shift=(0, 4, 0)), dict(shift=(0, 0, 4)),
           dict(out=False), dict(channels=[1, 2, 3, 1]), dict(channels=[0, 2, 1, 1])]
    for kw in bad:
        c = Call(lib, songs, p, **kw)
        assert c.rc == U and c.untouched(), kw
    for field, value in (("hop", 0), ("hop", 4801), ("warm", -1), ("warm", 8193), ("abs_gate", 1 << 56)):
        c = Call(lib, songs, p)
        q = params_of(p)
        setattr(q, field, value)
        out = C.c_void_p(c.so.data_ptr())
        desc = (_lib.SongDesc * 1)(_lib.SongDesc(8, songs[3][0].size, songs[3][1], 0))
        import torch
        torch.cuda.synchronize()
        c.so.fill_(SENTINEL)
        c.zo.fill_(SENTINEL)
        assert lib.bl_amd_loud_batch_device(C.c_void_p(c.arena.data_ptr()), desc, 1, C.byref(q), out, None, 0,
                                            None) == U
        assert c.untouched(), (field, value)
    q = params_of(p)
    q.s1_b[1] = math.inf
    c = Call(lib, songs, p)
    import torch
    torch.cuda.synchronize()
    c.so.fill_(SENTINEL)
    c.zo.fill_(SENTINEL)
    desc = (_lib.SongDesc * 1)(_lib.SongDesc(8, 64, 1, 0))
    assert lib.bl_amd_loud_batch_device(C.c_void_p(c.arena.data_ptr()), desc, 1, C.byref(q),
                                        C.c_void_p(c.so.data_ptr()), None, 0, None) == U
    assert lib.bl_amd_loud_batch_device(C.c_void_p(c.arena.data_ptr()), desc, 1, None,
                                        C.c_void_p(c.so.data_ptr()), None, 0, None) == U
    assert c.untouched()
    assert_equal(run(lib, songs, p), songs, p, "after the rejections")


# ---- the gates, through from_hops ----------------------------------------------------------------------------------------

def levels(*runs):
    return np.concatenate([np.full(n, v, dtype=np.int64) for n, v in runs])


def ramp(m):
    """30 + 10 (m - 1) hops whose m short-term starts all differ and all pass the gates"""
    return np.repeat(np.arange(1000, 1000 + m + 2), 10)[:30 + 10 * (m - 1)]


GATE_CASES = {
    "no hops": (levels((0, 0)), 1000),
    "three hops": (levels((3, 5000)), 1000),
    "all under the gate": (levels((64, 250)), 1001),
    "all exactly on the absolute gate": (levels((64, 250)), 1000),
    "one above the absolute gate": (levels((32, 250), (1, 251), (31, 250)), 1000),
    "on the relative threshold": (np.array([100, 0, 0, 0, 1900]), 0),
    "just over the relative threshold": (np.array([101, 0, 0, 0, 1899]), 0),
    "relative gate removes the quiet half": (levels((12, 1), (4, 40), (12, 400)), 100),
    "short-term on its absolute gate": (levels((60, 250)), 1000),          # 2 ST == 15 gates
    "short-term over its absolute gate": (levels((59, 250), (1, 251)), 1000),
    "short-term on its relative threshold": (levels((10, 1), (20, 0), (10, 199)), 0),   # ST0 100 N == S = 2000
    "short-term over its relative threshold": (levels((10, 1), (20, 0), (10, 198)), 0),
    "M = 0": (levels((29, 1 << 40)), 0),
    "M = 1": (ramp(1), 0),
    "M = 2": (ramp(2), 0),
    "M = 101": (ramp(101), 0),
    "two channels": (np.random.default_rng(6).integers(0, 1 << 46, (333, 2)), 1 << 47),
    "carry into the high limb": (np.full((40000, 2), (1 << 46) - 1, dtype=np.int64), 0),
    "near 2^45": (np.random.default_rng(7).integers((1 << 45) - 1000, 1 << 45, (70000, 2)), 1 << 40),
}


def test_gates_on_designed_hop_energies():
    names = list(GATE_CASES)
    by_gate = {}
    for n in names:
        by_gate.setdefault(GATE_CASES[n][1], []).append(n)
    for gate, group in by_gate.items():
        p = params_of(lr.plain(KW, abs_gate=gate))
        got = ld.from_hops([GATE_CASES[n][0] for n in group], p)
        for i, n in enumerate(group):
            want = lr.gates(GATE_CASES[n][0], gate)
            assert lr.rec_ints(got, i) == want, (n, lr.rec_ints(got, i), want)
    want = lr.gates(GATE_CASES["carry into the high limb"][0], 0)
    assert want["abs_sum"] >= 1 << 64 and want["gated_sum"] >= 1 << 64
    assert [lr.gates(GATE_CASES[f"M = {m}"][0], 0)["st_gated"] for m in (0, 1, 2, 101)] == [0, 1, 2, 101]
    # alone and in a batch: the same record
    alone = ld.from_hops([GATE_CASES["M = 101"][0]], params_of(lr.plain(KW, abs_gate=0)))
    assert lr.rec_ints(alone, 0) == lr.gates(GATE_CASES["M = 101"][0], 0)


def test_from_hops_continues_the_device_call(lib):
    """stages 4 to 6 on the Z a device call returned give that call's records"""
    hop = 7
    p = lr.plain(KW, hop=hop, warm=64, abs_gate=hop * 4 * GATE)
    songs = batch(hop)
    rec, z = run(lib, songs, p)
    H = [x.size // ch // hop for x, ch in songs]
    cuts = np.cumsum(H)[:-1]
    again = ld.from_hops([a.astype(np.int64) for a in np.split(z, cuts)], params_of(p))
    assert again.tobytes() == rec.tobytes()


# ---- the wrappers and the EBU sequences, end to end from PCM ------------------------------------------------------------

def test_host_and_corpus_wrappers_agree_with_the_reference():
    hop = 100
    p = lr.plain(KW, hop=hop, warm=64, abs_gate=hop * 4 * GATE)
    songs = [s for s in batch(hop) if s[0].size]
    rec, z = ld.loud_host([x for x, _ in songs], [ch for _, ch in songs], params_of(p), hops=True)
    assert_equal((rec, z), songs, p, "host form")
    assert ld.loud_host([x for x, _ in songs], [ch for _, ch in songs], params_of(p))[0].tobytes() == rec.tobytes()
    import torch
    corpus = bliss_amd.DeviceCorpus([x.size for x, _ in songs], [ch for _, ch in songs], 1)
    for i, (x, _) in enumerate(songs):
        corpus.upload(i, x)
    raw, zd = ld.loud_device(corpus, params_of(p), hops=True)
    torch.cuda.synchronize()
    assert ld.loud_to_numpy(raw.cpu().numpy()).tobytes() == rec.tobytes()
    assert zd.cpu().numpy().view(np.uint64).tobytes() == z.tobytes()


def test_tech_3341_case_1_at_48k():
    p = ld.kweight(48000)
    rec, _ = ld.loud_host([sine(48000, EBU_3341[1][0])], 2, p)
    got = ld.lufs(rec, p.hop)[0][0]
    print("case 1 at 48 kHz", got)
    assert abs(got - (-23.0)) <= 0.1
    assert ld.gain_db(rec, p.hop, -23.0)[0] == pytest.approx(-23.0 - got, abs=1e-12)


def test_tech_3341_cases_3_to_5_at_22050():
    p = ld.kweight(22050)
    rec, _ = ld.loud_host([sine(22050, EBU_3341[c][0]) for c in (3, 4, 5)], 2, p)
    got = ld.lufs(rec, p.hop)[0]
    print("cases 3 to 5 at 22 050 Hz", got)
    for c, g in zip((3, 4, 5), got):
        assert abs(g - EBU_3341[c][1]) <= 0.1, (c, g)
