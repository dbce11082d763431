"""True peak on the GPU (bl_amd_tpeak_batch_device, its context and host forms, bliss_amd.truepeak): every byte of
bl_amd_song_tpeak and every block of the profile is compared with == against tests/tpeak_reference.py.  There is no
tolerance anywhere.

The outputs are filled with 0xA5 before the call, so a byte the kernels do not write shows, and the arena between the
songs holds +-32767, so a sample taken from outside a song shows in its result (a profile with a block of one frame
lets a test see every frame).  The lengths are the smallest at which the kernel takes another path: around the 5 + 6
frames of the interpolator's reach and around the lane's run L and the workgroup's W frames (bl_amd_tpeak_shape).  A
pcm_offset is a multiple of 8 samples, so a song always starts on 16 bytes; the offsets here are odd multiples of 8, and
of 24 and 40, so that songs start off the 32-, 64- and 128-byte lines the lanes' rows are cut at.  The reference of a
(song, ceiling, block) is computed once per session and shared."""
import ctypes as C

import numpy as np
import pytest

import bliss_amd
import bliss_amd.truepeak as tp
from bliss_amd import _lib
from bliss_amd.records import TPEAK_DTYPE
from tests import tpeak_reference as tr

pytestmark = pytest.mark.gpu

U = _lib.BL_UNEXPECTED
SENTINEL = 0xA5
_REF, _SHAPE = {}, []


def LW():
    if not _SHAPE:
        _SHAPE.extend(tp.shape())
    return tuple(_SHAPE)


def reference(x, ch, ceiling, block):
    key = (x.tobytes(), ch, ceiling, block)
    if key not in _REF:
        _REF[key] = tr.song(x, ch, ceiling, block, lane=LW()[0])
    return _REF[key]


# ---- running the library -----------------------------------------------------------------------------------------------------

class Call:
    """one device call on `songs` = [(pcm, channels)] laid out with gaps of +-32767; the outputs were filled with 0xA5.
    `stream`: a torch stream instead of the default one; `defer`: the call is made by go() (tests/test_gpu_side_ws.py)"""

    def __init__(self, lib, songs, ceiling=32767, block=1, blocks=True, ctx=None, gaps=(8, 24, 40), n=None,
                 n_blocks=None, shift=(0, 0, 0), out=True, channels=None, stream=None, defer=False):
        import torch
        self.n = len(songs) if n is None else n
        size_of = min(max(block, 1), 65536)   # a rejected block still gets a profile of a plausible size
        self.nb = [(x.size // ch + size_of - 1) // size_of for x, ch in songs]
        self.total = sum(self.nb)
        size = sum(((x.size + 7) & ~7) + max(gaps) for x, _ in songs) + max(gaps) + 64
        arena = np.where(np.arange(size) % 3 == 0, -32767, 32767).astype(np.int16)
        desc = (_lib.SongDesc * len(songs))()
        at = gaps[0]
        for i, (x, ch) in enumerate(songs):
            arena[at:at + x.size] = x
            desc[i] = _lib.SongDesc(at, x.size, ch if channels is None else channels[i], 0)
            at += ((x.size + 7) & ~7) + gaps[(i + 1) % len(gaps)]
        self.arena = torch.from_numpy(arena).cuda()

        def fill(nbytes):
            return torch.full((nbytes + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.so = fill(len(songs) * 56)
        self.bo = fill(self.total * 8) if blocks else None
        args = (C.c_void_p(self.arena.data_ptr() + shift[0]), desc, self.n, ceiling, block,
                C.c_void_p(self.so.data_ptr() + shift[1]) if out else None,
                C.c_void_p(self.bo.data_ptr() + shift[2]) if blocks else None,
                self.total if n_blocks is None else n_blocks)
        self._call = ((lib.bl_amd_tpeak_batch_device, args) if ctx is None
                      else (lib.bl_amd_ctx_tpeak_batch_device, (ctx.handle,) + args))
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
        rec = np.frombuffer(self._host(self.so, self.n * 56), dtype=TPEAK_DTYPE)
        b = None if self.bo is None else np.frombuffer(self._host(self.bo, self.total * 8),
                                                       dtype=np.uint32).reshape(-1, 2)
        return rec, b

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return all(t is None or bool((t == SENTINEL).all()) for t in (self.so, self.bo))


def run(lib, songs, **kw):
    c = Call(lib, songs, **kw)
    assert c.rc == 0
    return c.read()


def assert_equal(got, songs, ceiling=32767, block=1, what=""):
    rec, blocks = got
    at = 0
    for i, (x, ch) in enumerate(songs):
        want, want_blocks = reference(x, ch, ceiling, block)
        where = f"{what} song {i} (F {x.size // ch}, {ch} channels, ceiling {ceiling}, block {block})"
        for f in TPEAK_DTYPE.names:
            assert np.array_equal(rec[f][i], want[f][0]), f"{where}: {f} {rec[f][i].tolist()}, want {want[f][0].tolist()}"
        assert rec[i].tobytes() == want.tobytes(), where
        assert all(int(rec["tpeak"][i, c]) >= int(rec["peak"][i, c]) << 14 for c in (0, 1)), where
        if blocks is not None:
            g = blocks[at:at + want_blocks.shape[0]]
            if not np.array_equal(g, want_blocks):
                b = int(np.flatnonzero((g != want_blocks).any(axis=1))[0])
                raise AssertionError(f"{where}: block {b} {g[b].tolist()}, want {want_blocks[b].tolist()}; "
                                     f"{int((g != want_blocks).any(axis=1).sum())} blocks differ")
            at += want_blocks.shape[0]
    assert blocks is None or at == blocks.shape[0]


# ---- material ---------------------------------------------------------------------------------------------------------------

def noise(frames, ch, seed):
    x = np.random.default_rng(seed).integers(-32768, 32768, frames * ch).astype(np.int16)
    if x.size >= 3:
        x[0], x[-1], x[x.size // 2] = -32768, 32767, -32768
    return x


def edge_songs():
    """mono and stereo at every edge length, a stereo song without a frame and two with an odd n_samples"""
    L, W = LW()
    lengths = (1, 2, 5, 6, 7, 11, 12, 13, L - 1, L, L + 1, 2 * L + 1, W - 1, W, W + 1, 2 * W + 5, 3 * W - 6)
    songs = [(np.array([12345], dtype=np.int16), 2)]
    for k, F in enumerate(lengths):
        songs.append((noise(F, 1, 2 * k), 1))
        songs.append((noise(F, 2, 2 * k + 1), 2))
    songs.append((noise(75, 1, 90), 2))            # 37 frames and a sample
    songs.append((noise(2 * L + 1, 1, 91), 2))     # L frames and a sample: the sample sits where a halo is loaded
    return songs


def small_songs():
    L, _ = LW()
    return [s for s in edge_songs() if s[0].size // s[1] <= 2 * L + 1]


def impulse_songs():
    """one impulse of -32768 at each of the first 13 and last 13 frames of a song of W + 13 frames: every tap at both
    ends of a song and across the seam between two workgroups; mono and stereo alternate, the stereo ones carry the
    impulse in one channel and a second one, mirrored, in the other"""
    _, W = LW()
    F = W + 13
    songs = []
    for k, t in enumerate(list(range(13)) + list(range(F - 13, F))):
        if k % 2:
            x = np.zeros(F, dtype=np.int16)
            x[t] = -32768
            songs.append((x, 1))
        else:
            x = np.zeros(2 * F, dtype=np.int16)
            x[2 * t + (k // 2) % 2] = -32768
            x[2 * (F - 1 - t) + 1 - (k // 2) % 2] = -32768
            songs.append((x, 2))
    return songs


def designed_songs():
    L, W = LW()
    worst = np.zeros(2 * (L + 30), dtype=np.int16)
    for j in range(-5, 7):
        worst[2 * (L + 3 + j)] = 32767 if tr.TABLE[2][j + 5] > 0 else -32767    # reaches 30544 * 32767, in phase 2
    worst[1::2] = -32768
    twin = np.zeros(3 * L, dtype=np.int16)
    twin[5], twin[2 * L + 3] = 12345, -12345                                    # equal maxima in phase 0, two lanes
    twin2 = np.zeros(2 * (W + 40), dtype=np.int16)
    for t0 in (L - 1, W + 7):                                                   # equal maxima in phase 2, two groups
        twin2[2 * t0], twin2[2 * (t0 + 1)] = 20000, 20000
        twin2[2 * t0 + 1], twin2[2 * (t0 + 1) + 1] = -20000, -20000
    return [(worst, 2), (np.full(W + 3, -32768, dtype=np.int16), 1), (np.full(2 * (L + 7), -32768, dtype=np.int16), 2),
            (twin, 1), (twin2, 2)]


# ---- tests ----------------------------------------------------------------------------------------------------------------------

def blocks_param():
    return ["1", "7", "L", "W", "W+1", "65536"]


def block_of(name):
    L, W = LW()
    return {"1": 1, "7": 7, "L": L, "W": W, "W+1": W + 1, "65536": 65536}[name]


@pytest.mark.parametrize("block_name", blocks_param())
def test_every_edge_length_matches_the_reference(lib, block_name):
    block = block_of(block_name)
    ceiling = {"1": 32767, "7": 0, "L": 65535, "W": 20000, "W+1": 9000, "65536": 32767}[block_name]
    songs = edge_songs()
    assert_equal(run(lib, songs, ceiling=ceiling, block=block), songs, ceiling, block)


def test_impulses_see_every_tap_at_the_ends_and_at_a_seam(lib):
    songs = impulse_songs()
    assert_equal(run(lib, songs, ceiling=100, block=1), songs, 100, 1)
    # the impulse response is the table: the blocks around an impulse are the columns' largest magnitudes
    _, W = LW()
    x, ch = songs[1]
    t = int(np.flatnonzero(x)[0])
    want = reference(x, ch, 100, 1)[1][:, 0]
    col = np.abs(tr.TABLE).max(axis=0) * 32768
    assert [int(want[t + j]) if 0 <= t + j < W + 13 else None for j in range(-6, 6)] == \
        [int(col[5 - j]) if 0 <= t + j else None for j in range(-6, 6)]


def test_range_and_first_of_equal_maxima(lib):
    L, W = LW()
    songs = designed_songs()
    rec, blocks = run(lib, songs, ceiling=12345, block=1)
    assert_equal((rec, blocks), songs, 12345, 1)
    assert rec["tpeak"][0, 0] == 30544 * 32767 and rec["at"][0, 0] == 4 * (L + 3) + 2     # a maximum in phase 2
    assert rec["peak"][1, 0] == 32768 and rec["tpeak"][1, 0] >= 16400 * 32768
    assert rec["at"][3, 0] == 4 * 5 and rec["tpeak"][3, 0] == 12345 << 14                 # a maximum in phase 0
    assert rec["overs"][3, 0] == 0                                                        # two points equal the ceiling
    assert rec["at"][4].tolist() == [4 * (L - 1) + 2] * 2                                 # the first of two groups


@pytest.mark.parametrize("ceiling", [0, 12345, 65535])
def test_ceilings(lib, ceiling):
    songs = small_songs() + designed_songs()
    rec, _ = run(lib, songs, ceiling=ceiling, block=7)
    assert_equal((rec, _), songs, ceiling, 7)
    if ceiling == 65535:
        assert not rec["overs"].any()


def test_alone_reordered_and_in_a_batch_of_300(lib):
    base = small_songs() + designed_songs()[:1] + impulse_songs()[:2]
    many = [base[i % len(base)] for i in range(300)]
    rec, blocks = run(lib, many, ceiling=9000, block=7)
    assert_equal((rec, blocks), many, 9000, 7, "300 songs")
    rec_no, _ = run(lib, many, ceiling=9000, block=7, blocks=False)
    assert rec_no.tobytes() == rec.tobytes(), "the records depend on the optional output"
    starts = np.concatenate([[0], np.cumsum([(x.size // ch + 6) // 7 for x, ch in many])])
    perm = np.random.default_rng(4).permutation(300)
    recp, blocksp = run(lib, [many[i] for i in perm], ceiling=9000, block=7, gaps=(24, 8))
    at = 0
    for k, i in enumerate(perm):
        nb = int(starts[i + 1] - starts[i])
        assert recp[k].tobytes() == rec[i].tobytes(), f"song {i} differs at position {k}"
        assert blocksp[at:at + nb].tobytes() == blocks[starts[i]:starts[i + 1]].tobytes(), f"blocks of song {i} differ"
        at += nb
    for i in (0, 1, 2, len(base) - 1, len(base) - 3):
        one, one_blocks = run(lib, [many[i]], ceiling=9000, block=7)
        assert one.tobytes() == rec[i:i + 1].tobytes()
        assert one_blocks.tobytes() == blocks[starts[i]:starts[i + 1]].tobytes()


def test_positions_beyond_2_31(lib):
    """a mono song of a little over 2^29 frames (1 GiB, made on the device) that is silent but for two equal impulses:
    both lie at oversampled positions above 2^31, and the first must win.  Between the impulses zeros stand, so the
    reference is computed on the 64 frames around each and moved to its place."""
    import torch
    _, W = LW()
    F = (1 << 29) + 5 * W + 3
    t_a, t_b, block, ceiling = (1 << 29) + 7, F - 3, 65536, 100
    nb = (F + block - 1) // block
    arena = torch.zeros(F + 16, dtype=torch.int16, device="cuda")
    arena[8 + t_a] = -32768
    arena[8 + t_b] = -32768
    so = torch.full((56 + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    bo = torch.full((8 * nb + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    desc = (_lib.SongDesc * 1)(_lib.SongDesc(8, F, 1, 0))
    assert lib.bl_amd_tpeak_batch_device(C.c_void_p(arena.data_ptr()), desc, 1, ceiling, block, C.c_void_p(so.data_ptr()),
                                         C.c_void_p(bo.data_ptr()), nb, None) == 0
    torch.cuda.synchronize()
    raw, raw_blocks = so.cpu().numpy(), bo.cpu().numpy()
    assert (raw[56:] == SENTINEL).all() and (raw_blocks[8 * nb:] == SENTINEL).all(), "written past the end"
    rec = np.frombuffer(raw[:56].tobytes(), dtype=TPEAK_DTYPE)
    blocks = np.frombuffer(raw_blocks[:8 * nb].tobytes(), dtype=np.uint32).reshape(-1, 2)
    mid, tail = np.zeros(64, dtype=np.int16), np.zeros(64, dtype=np.int16)
    mid[32], tail[64 - 3] = -32768, -32768
    (ref_a, frames_a), (ref_b, frames_b) = tr.song(mid, 1, ceiling, 1), tr.song(tail, 1, ceiling, 1)
    assert ref_a["at"][0, 0] == 4 * 32 and 4 * t_a > 1 << 31
    assert rec["at"][0].tolist() == [4 * t_a, -1]
    assert rec["tpeak"][0].tolist() == [1 << 29, 0] and rec["peak"][0].tolist() == [32768, 0]
    assert rec["overs"][0].tolist() == [int(ref_a["overs"][0, 0] + ref_b["overs"][0, 0]), 0]
    assert rec["frames"][0] == F and rec["status"][0] == 0
    want = np.zeros((nb, 2), dtype=np.uint32)
    for start, per_frame in ((t_a - 32, frames_a), (F - 64, frames_b)):
        np.maximum.at(want[:, 0], (start + np.arange(64)) // block, per_frame[:, 0])
    assert np.array_equal(blocks, want)


def test_context_form_and_the_workspace_going_with_its_context(lib):
    songs = small_songs()
    for k in range(3):
        with bliss_amd.Context(0) as ctx:
            assert_equal(run(lib, songs, ceiling=100, block=3, ctx=ctx, blocks=bool(k & 1), gaps=(0, 8)), songs, 100, 3,
                         f"context {k}")
            assert_equal(run(lib, songs[:5], ceiling=100, block=3, ctx=ctx), songs[:5], 100, 3, f"context {k} again")
    assert_equal(run(lib, songs, ceiling=100, block=3), songs, 100, 3, "default context afterwards")


def test_rejected_calls_write_nothing(lib):
    songs = small_songs()[1:5]
    bad = [dict(n=0), dict(n_blocks=1), dict(shift=(2, 0, 0)), dict(shift=(8, 0, 0)), dict(shift=(0, 4, 0)),
           dict(shift=(0, 0, 2)), dict(out=False), dict(channels=[1, 2, 3, 1]), dict(channels=[0, 2, 1, 1]),
           dict(ceiling=-1), dict(ceiling=65536), dict(block=0), dict(block=65537), dict(gaps=(4, 8)),
           dict(ceiling=-1, blocks=False), dict(block=0, blocks=False)]
    for kw in bad:
        c = Call(lib, songs, **kw)
        assert c.rc == U and c.untouched(), kw
    assert_equal(run(lib, songs), songs, what="after the rejections")


def test_host_and_corpus_wrappers_agree_with_the_reference():
    L, W = LW()
    songs = [s for s in edge_songs() if s[0].size >= 2] + designed_songs()
    pcm, chans = [x for x, _ in songs], [ch for _, ch in songs]
    rec, blocks = tp.tpeak_host(pcm, chans, ceiling=9000, block=L)
    assert_equal((rec, blocks), songs, 9000, L, "host form")
    rec_no, none = tp.tpeak_host(pcm, chans, ceiling=9000)
    assert none is None and rec_no.tobytes() == rec.tobytes()
    import torch
    corpus = bliss_amd.DeviceCorpus([x.size for x in pcm], chans, 1)
    for i, x in enumerate(pcm):
        corpus.upload(i, x)
    raw, prof = tp.tpeak_device(corpus, ceiling=9000, block=L)
    raw_no, prof_no = tp.tpeak_device(corpus, ceiling=9000)
    torch.cuda.synchronize()
    assert tp.tpeak_to_numpy(raw.cpu().numpy()).tobytes() == rec.tobytes()
    assert prof_no is None and tp.tpeak_to_numpy(raw_no.cpu().numpy()).tobytes() == rec.tobytes()
    assert prof.cpu().numpy().view(np.uint32).tobytes() == blocks.tobytes()
    per, song = tp.dbtp(rec)
    assert per[0, 0] == pytest.approx(tr.dbtp(int(rec["tpeak"][0, 0])), abs=1e-12) and song[0] == per[0].max()


def test_profile_counts_the_launches(lib):
    songs = small_songs()[:6]
    lib.bl_amd_profile(1)
    try:
        n = C.c_int(0)
        lib.bl_amd_tpeak_profile_ms(b"tpeak_scan", C.byref(n))
        lib.bl_amd_tpeak_profile_ms(b"tpeak_finish", C.byref(n))
        for _ in range(2):
            assert_equal(run(lib, songs, ceiling=100, block=3), songs, 100, 3)
        assert lib.bl_amd_tpeak_profile_ms(b"tpeak_scan", C.byref(n)) > 0.0 and n.value == 2
        assert lib.bl_amd_tpeak_profile_ms(b"tpeak_finish", C.byref(n)) > 0.0 and n.value == 2
        assert lib.bl_amd_tpeak_profile_ms(b"tpeak_scan", C.byref(n)) == 0.0 and n.value == 0
    finally:
        lib.bl_amd_profile(0)
