"""Tempo over time on the GPU (bl_amd_tgram_device, its context and host forms, bliss_amd.tempogram): every byte of
bl_amd_song_tgram, of bl_amd_tgram_frame and of the lag products is compared with == against tests/tgram_reference.py,
which forms every frame's row directly from the curve.  There is no tolerance anywhere.

The outputs are filled with 0xA5 before the call and carry 16 guard bytes, so a byte the kernels do not write, or one
they write too far, shows; 600 hops of 2^18 - 1 follow the last curve and the curves stand one behind the other, so a
factor read from behind a song shows.  The shapes are the smallest at which the kernels can go wrong: frame counts
around the run length and block counts around the staged tile (bl_amd_tgram_shape), every ring length that matters
(m = 1, 2, 15, 16), the strides at both ends of the range and one that does not divide the tile, and the named input
of every mistake the reference can make."""
import ctypes as C

import numpy as np
import pytest

import bliss_amd
import bliss_amd.rhythm as rh
import bliss_amd.tempogram as tg
from bliss_amd import _lib
from bliss_amd.records import TGRAM_DTYPE, TGRAM_FRAME_DTYPE
from tests import rhythm_reference as rr
from tests import tgram_reference as tr

pytestmark = pytest.mark.gpu

UNEXPECTED = _lib.BL_UNEXPECTED
SENTINEL, GUARD, BEHIND = 0xA5, 16, (1 << 18) - 1


def filled(nbytes):
    import torch
    return torch.full((nbytes + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")


def fetch(t, nbytes):
    import torch
    torch.cuda.synchronize()
    raw = t.cpu().numpy()
    assert (raw[nbytes:] == SENTINEL).all(), "written past the end"
    return raw[:nbytes].tobytes()


def make(p):
    return tg.params(p["stride"], p["blocks"], p["lag_min"], p["lag_max"], p["tol"], bool(p["octaves"]))


class Call:
    """one device call over curves (a list of integer arrays); every output was filled with 0xA5"""

    def __init__(self, lib, curves, p, gram=True, ctx=None, bad=None):
        import torch
        self.curves, self.p, self.params = [np.asarray(o, dtype=np.int64) for o in curves], p, make(p)
        self.n = len(curves)
        self.counts = [tr.frames_count(o.size, p) for o in self.curves]
        self.nf = sum(self.counts)
        flat = np.concatenate(self.curves + [np.full(600, BEHIND, np.int64)]).astype(np.int32)
        self.onsets = torch.from_numpy(flat).cuda()
        self.rows = self.nf if gram else 0          # without the rows, only their guard
        self.songs, self.frames, self.gram = filled(56 * self.n), filled(40 * self.nf), filled(4096 * self.rows)
        ptr = lambda t: C.c_void_p(t.data_ptr())
        arg = dict(o=ptr(self.onsets), h=(C.c_int32 * max(self.n, 1))(*[o.size for o in self.curves]), n=self.n,
                   p=C.byref(self.params), songs=ptr(self.songs), frames=ptr(self.frames), nf=self.nf,
                   gram=ptr(self.gram) if gram else None)
        for k, v in (bad or {}).items():
            arg[k] = v(self) if callable(v) else v
        args = tuple(arg[k] for k in ("o", "h", "n", "p", "songs", "frames", "nf", "gram"))
        if ctx is None:
            self.rc = lib.bl_amd_tgram_device(*args, None)
        else:
            self.rc = lib.bl_amd_ctx_tgram_device(ctx.handle, *args, None)
        self.with_gram = gram

    def read(self):
        assert self.rc == 0
        songs = np.frombuffer(fetch(self.songs, 56 * self.n), dtype=TGRAM_DTYPE)
        frames = np.frombuffer(fetch(self.frames, 40 * self.nf), dtype=TGRAM_FRAME_DTYPE)
        gram = np.frombuffer(fetch(self.gram, 4096 * self.rows), dtype=np.uint64).reshape(self.rows, 512)
        return songs, frames, gram

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return all(bool((t == SENTINEL).all()) for t in (self.songs, self.frames, self.gram))


def assert_tgram(call, want=None, what=""):
    songs, frames, gram = call.read()
    wsongs, wframes, wgram = want if want is not None else tr.batch(call.curves, call.p)
    assert frames.size == wframes.size, what
    if call.with_gram:
        diff = np.nonzero((gram != wgram).any(axis=1))[0]
        assert diff.size == 0, (f"{what}: the rows of {diff.size} frames differ, the first is frame {diff[0]}, at lags "
                                f"{np.nonzero(gram[diff[0]] != wgram[diff[0]])[0][:8]}")
    for k in TGRAM_FRAME_DTYPE.names:
        diff = np.nonzero(frames[k] != wframes[k])[0]
        assert diff.size == 0, f"{what}: {k} of {diff.size} frames differs, the first is frame {diff[0]}: " \
                               f"{frames[diff[0]]}, want {wframes[diff[0]]}"
    assert frames.tobytes() == wframes.tobytes(), what
    for i in range(call.n):
        for k in TGRAM_DTYPE.names:
            assert int(songs[k][i]) == int(wsongs[k][i]), (f"{what}: song {i} of {call.curves[i].size} hops: {k} "
                                                           f"{int(songs[k][i])}, want {int(wsongs[k][i])}")
    assert songs.tobytes() == wsongs.tobytes(), what
    return songs, frames, gram


def P(stride, blocks, **kw):
    return tr.params(stride=stride, blocks=blocks, **kw)


def test_the_first_frame_appears_at_527_hops(gpu_lib):
    p = P(16, 1)
    call = Call(gpu_lib, [tr.noise(526, 1), tr.noise(527, 2), tr.noise(1, 3), tr.noise(511, 4), tr.noise(512, 5)], p)
    songs, _, _ = assert_tgram(call)
    assert call.counts == [0, 1, 0, 0, 0] and songs["status"].tolist() == [UNEXPECTED, 0, UNEXPECTED, UNEXPECTED,
                                                                          UNEXPECTED]


@pytest.mark.parametrize("stride,blocks", [(16, 1), (16, 2), (16, 15), (16, 16), (48, 1), (48, 2), (48, 16), (1024, 1),
                                           (1024, 2)])
def test_exact_multiples_and_one_hop_short(gpu_lib, stride, blocks):
    """T - W an exact multiple of S (3 frames), one hop short of it (2 frames) and S - 1 hops past it (3 frames)"""
    p = P(stride, blocks)
    h = tr.hops_for(3, p)
    call = Call(gpu_lib, [tr.noise(h, 40), tr.noise(h - 1, 41), tr.noise(h + stride - 1, 42)], p)
    assert call.counts == [3, 2, 3]
    assert_tgram(call, what=f"S {stride} m {blocks}")


def shape_cases():
    """(S, m, F): frame counts one below, at and one above the run length and its double, and block counts
    F + m - 1 one below, at and one above the blocks of a staged tile and their double"""
    tile, run = tg.shape()
    out = set()
    for s, m in ((16, 1), (16, 2), (16, 16), (48, 2), (48, 15)):
        for edge in (run, 2 * run):
            out |= {(s, m, f) for f in (edge - 1, edge, edge + 1)}
        per_tile = max(1, tile // s)
        for edge in (per_tile, 2 * per_tile):
            out |= {(s, m, b - (m - 1)) for b in (edge - 1, edge, edge + 1) if b - (m - 1) >= 1}
    return sorted(out)


def test_lengths_around_every_value_of_shape(gpu_lib):
    assert tg.shape() == (1024, 64)
    by_params = {}
    for s, m, f in shape_cases():
        by_params.setdefault((s, m), []).append(f)
    for (s, m), fs in sorted(by_params.items()):
        p = P(s, m)
        curves = [tr.noise(tr.hops_for(f, p, extra=(7 * f) % s), 100 + f) for f in fs]
        call = Call(gpu_lib, curves, p)
        assert call.counts == fs
        assert_tgram(call, what=f"S {s} m {m} F {fs}")


def test_fewer_blocks_than_the_ring_and_silence(gpu_lib):
    p = P(16, 16)
    z = lambda n: np.zeros(n, dtype=np.int64)
    call = Call(gpu_lib, [tr.noise(511 + 16 * 5, 50), z(tr.hops_for(5, p)), tr.noise(tr.hops_for(1, p) - 1, 51),
                          z(600), tr.noise(tr.hops_for(2, p), 52), z(1)], p)
    songs, frames, _ = assert_tgram(call)
    assert call.counts == [0, 5, 0, 0, 2, 0]
    assert (songs["n_tempo"][1], songs["frame_first"][1], songs["status"][1]) == (0, -1, 0) and not frames[:5]["lag"].any()


def test_the_bound(gpu_lib):
    """2^18 - 1 throughout at S = 1024, m = 16: r0 = 16 384 (2^18 - 1)^2, just below 2^50; two frames, so a row is
    retired at the bound as well"""
    p = P(1024, 16, lag_min=1, lag_max=510)
    call = Call(gpu_lib, [np.full(tr.hops_for(2, p), BEHIND, np.int64)], p)
    _, frames, gram = assert_tgram(call)
    assert int(frames["r0"][1]) == 16384 * BEHIND * BEHIND and (gram == np.uint64(16384 * BEHIND * BEHIND)).all()


def test_the_worked_tempo_change(gpu_lib):
    call = Call(gpu_lib, [tr.worked_curve()], tr.WORKED)
    songs, frames, _ = assert_tgram(call)
    assert frames["lag"].tolist() == [40] * 30 + [50] * 25
    assert (songs["lag_first"][0], songs["lag_last"][0], songs["lag_median"][0], songs["n_near"][0],
            songs["n_jumps"][0]) == (40, 50, 40, 30, 1)
    assert tg.steadiness(songs)[0] == 30 / 55


@pytest.mark.parametrize("switch", sorted(tr.named()))
def test_the_named_input_of_every_mistake(gpu_lib, switch):
    o, p, _ = tr.named()[switch]
    assert_tgram(Call(gpu_lib, [o], p), what=switch)


@pytest.fixture(scope="module")
def mixed():
    """short songs between exact copies of a long one, and the reference of the whole call, computed once"""
    p = tr.SMALL
    long = tr.gapped_curve()
    curves = [long, tr.noise(3, 60), long, tr.noise(tr.hops_for(1, p) - 1, 61), tr.noise(tr.hops_for(1, p), 62), long,
              tr.octave_curve(), np.zeros(700, dtype=np.int64), tr.noise(tr.hops_for(70, p, extra=5), 63)]
    return p, curves, tr.batch(curves, p)


def _slices(counts):
    at = np.concatenate([[0], np.cumsum(counts)])
    return [slice(int(at[i]), int(at[i + 1])) for i in range(len(counts))]


def test_short_songs_between_copies_of_a_long_one(gpu_lib, mixed):
    p, curves, want = mixed
    call = Call(gpu_lib, curves, p)
    songs, frames, gram = assert_tgram(call, want)
    sl = _slices(call.counts)
    for i in (2, 5):
        assert songs[i].tobytes() == songs[0].tobytes() and frames[sl[i]].tobytes() == frames[sl[0]].tobytes()
        assert gram[sl[i]].tobytes() == gram[sl[0]].tobytes()


def test_a_mixed_call_equals_each_song_alone_in_any_order_on_any_context(gpu_lib, mixed):
    p, curves, want = mixed
    sl = _slices([tr.frames_count(o.size, p) for o in curves])
    for i, o in enumerate(curves):
        assert_tgram(Call(gpu_lib, [o], p), (want[0][i:i + 1], want[1][sl[i]], want[2][sl[i]]), what=f"song {i} alone")
    order = [4, 8, 0, 7, 1, 6, 3, 5, 2]
    permuted = (want[0][order], np.concatenate([want[1][sl[i]] for i in order]),
                np.concatenate([want[2][sl[i]] for i in order]))
    assert_tgram(Call(gpu_lib, [curves[i] for i in order], p), permuted, what="permuted")
    with bliss_amd.Context(0) as ctx:
        assert_tgram(Call(gpu_lib, [curves[i] for i in order], p, ctx=ctx), permuted, what="second context")
        assert_tgram(Call(gpu_lib, curves, p, ctx=ctx), want, what="second context, again")
    assert_tgram(Call(gpu_lib, curves, p), want, what="default context, after the other")


def _tiled(p, distinct, picks, gram=True):
    """the call that takes distinct[k] for k in picks, and its reference from one reference per distinct curve"""
    ref = [tr.batch([o], p) for o in distinct]
    return [distinct[k] for k in picks], (np.concatenate([ref[k][0] for k in picks]),
                                          np.concatenate([ref[k][1] for k in picks]),
                                          np.concatenate([ref[k][2] for k in picks]) if gram else None)


def test_the_launch_shape_does_not_show(gpu_lib):
    """a call of few songs cuts a song of 70 or 130 frames into runs of 64; one of 2 100 songs (more than eight per
    compute unit) takes every song in one run: the same bytes"""
    p = P(16, 2)
    distinct = [tr.noise(tr.hops_for(70, p, extra=3), 90), tr.noise(tr.hops_for(130, p), 91), tr.noise(530, 92)]
    few, want_few = _tiled(p, distinct, [0, 1, 2])
    assert_tgram(Call(gpu_lib, few, p), want_few, what="few songs")
    many, want_many = _tiled(p, distinct, [k % 3 for k in range(2100)], gram=False)
    assert_tgram(Call(gpu_lib, many, p, gram=False), want_many, what="many songs")


def test_more_songs_than_one_launch_takes(gpu_lib):
    """33 000 songs: the block kernel is launched twice, and the songs of the second launch land where they belong"""
    p = P(16, 1)
    distinct = [tr.noise(527, 93), tr.noise(tr.hops_for(3, p), 94), tr.noise(100, 95)]
    picks = [0] * 33000
    picks[5], picks[32767], picks[32768], picks[32770], picks[32999] = 1, 1, 2, 1, 1
    songs, want = _tiled(p, distinct, picks, gram=False)
    assert_tgram(Call(gpu_lib, songs, p, gram=False), want, what="33 000 songs")


def test_records_do_not_depend_on_the_optional_output(gpu_lib, mixed):
    p, curves, want = mixed
    assert_tgram(Call(gpu_lib, curves, p, gram=False), want)


def test_the_host_form_and_the_python_device_form(gpu_lib, mixed):
    import torch
    p, curves, want = mixed
    songs, frames, gram = tg.tgram_host(curves, make(p), gram=True)
    assert songs.tobytes() == want[0].tobytes() and frames.tobytes() == want[1].tobytes()
    assert gram.tobytes() == want[2].tobytes()
    songs, frames, gram = tg.tgram_host(curves[:2], make(p))
    assert gram is None and songs.tobytes() == want[0][:2].tobytes()
    songs, frames, gram = tg.tgram_host([curves[1], curves[3]], make(p), gram=True)       # no frame at all
    assert frames.size == 0 and gram.shape == (0, 512) and songs["status"].tolist() == [UNEXPECTED, UNEXPECTED]
    flat = torch.from_numpy(np.concatenate(curves).astype(np.int32)).cuda()
    out = tg.tgram_device(flat, [o.size for o in curves], make(p), gram=True)
    torch.cuda.synchronize()
    s, f = tg.tgram_to_numpy(out["songs"].cpu().numpy().tobytes(), out["frames"].cpu().numpy().tobytes())
    assert s.tobytes() == want[0].tobytes() and f.tobytes() == want[1].tobytes()
    assert out["gram"].cpu().numpy().view(np.uint64).tobytes() == want[2].tobytes()
    assert out["counts"] == [int(c) for c in want[0]["frames"]]
    assert np.array_equal(tg.bpm(f), [tr.bpm(x) for x in f], equal_nan=True)


@pytest.mark.parametrize("stride,blocks", [(16, 5), (48, 7), (1024, 1), (128, 16)])
def test_a_single_frame_over_all_terms_is_the_tempo_call(gpu_lib, stride, blocks):
    """W = T: the frame's row, lags and neighbours are those of bl_amd_rhythm_from_onsets on the same curve"""
    p = P(stride, blocks, lag_min=20, lag_max=450)
    curves = [tr.noise(tr.hops_for(1, p), 70 + blocks), tr.clicks(43, tr.hops_for(1, p)) + tr.noise(tr.hops_for(1, p), 71, 50)]
    songs, frames, gram = Call(gpu_lib, curves, p).read()
    rec, acf = rh.rhythm_from_onsets(curves, 20, 450, acf=True)
    assert songs["frames"].tolist() == [1, 1] and gram.tobytes() == acf.tobytes()
    for k in ("r0", "r_prev", "r_lag", "r_next", "lag", "lag_peak"):
        assert frames[k].tolist() == rec[k].tolist(), k
    assert np.array_equal(tg.bpm(frames), rh.rhythm_bpm(rec)[0], equal_nan=True)


def test_rejected_calls_write_nothing(gpu_lib):
    p = tr.TINY
    curves = [tr.noise(tr.hops_for(2, p), 80), tr.noise(tr.hops_for(3, p), 81)]
    hops = lambda *v: (C.c_int32 * len(v))(*v)

    def bad_params(**kw):
        q = make(p)
        for k, v in kw.items():
            if k == "reserved":
                q.reserved[v] = 1
            else:
                setattr(q, k, v)
        return q
    keep = [bad_params(**kw) for kw in (dict(stride=24), dict(stride=0), dict(stride=2048), dict(blocks=0), dict(blocks=17),
                                        dict(lag_min=0), dict(lag_max=511), dict(lag_min=300), dict(tol=1001),
                                        dict(tol=-1), dict(octaves=2), dict(reserved=0), dict(reserved=1))]
    cases = [dict(o=None), dict(h=None), dict(p=None), dict(songs=None), dict(frames=None), dict(n=0), dict(n=-1),
             dict(nf=4), dict(nf=6), dict(nf=-1), dict(h=hops(curves[0].size, 0)), dict(h=hops(1 << 24, curves[1].size)),
             dict(o=lambda c: C.c_void_p(c.onsets.data_ptr() + 2)), dict(songs=lambda c: C.c_void_p(c.songs.data_ptr() + 2)),
             dict(frames=lambda c: C.c_void_p(c.frames.data_ptr() + 4)),
             dict(gram=lambda c: C.c_void_p(c.gram.data_ptr() + 4))] + [dict(p=C.byref(q)) for q in keep]
    for bad in cases:
        call = Call(gpu_lib, curves, p, bad=bad)
        assert call.rc == UNEXPECTED and call.untouched(), list(bad)
    with bliss_amd.Context(0) as ctx:
        call = Call(gpu_lib, curves, p, ctx=ctx, bad=dict(nf=4))
        assert call.rc == UNEXPECTED and call.untouched()
    over = [curves[0].copy(), curves[1]]
    over[0][5] = 1 << 18
    with pytest.raises(ValueError):
        tg.tgram_host(over, make(p))
    assert_tgram(Call(gpu_lib, curves, p), what="after the rejected calls")


def test_from_pcm_on_a_click_track(gpu_lib):
    period, hops, ch = rr.CLICKS[0]
    pcm = rr.click_track(period, hops, ch, seed=period)
    p = P(32, 8, lag_min=rr.LAG_MIN, lag_max=rr.LAG_MAX)
    songs, frames, gram, hop_counts = tg.from_pcm([pcm], ch, make(p), gram=True)
    want = tr.batch([rr.onsets(pcm, ch)], p)
    assert hop_counts == [hops] and songs.tobytes() == want[0].tobytes() and frames.tobytes() == want[1].tobytes()
    assert gram.tobytes() == want[2].tobytes()
    assert songs["n_tempo"][0] == songs["frames"][0] and songs["lag_median"][0] == period and songs["n_jumps"][0] == 0
