"""The beat grid's reference (tests/beat_reference.py) and the host arithmetic of bl_amd_beats_* without a device.

The reference is what tests/test_gpu_beats.py compares the kernel with, so it is itself pinned here: every deliberate
mistake it can make changes a named curve of its corpus, the block-wise evaluation the kernel uses equals the hop-by-hop
definition, the bound on the log error that the header's bit counts rest on holds for every period, and on the click
tracks of the tempo corpus the grid is exactly the clicks.

Two switches, hi_short and tail_wide, cannot change anything on their own, on any curve: the docstring of
tests/beat_reference.py proves it (d = L is free, so d = 2 L never wins and hop H - L - 1 is never the end).  They are
pinned together with the tie rule beside them, against that tie rule alone.
"""
import ctypes as C
import math

import numpy as np
import pytest

import bliss_amd.rhythm as rh
from bliss_amd import _lib
from tests import beat_reference as br
from tests import rhythm_reference as rr


@pytest.fixture(scope="module")
def corpus():
    return br.corpus()


@pytest.fixture(scope="module")
def plain(corpus):
    return {name: br.track(*song) for name, song in corpus.items()}


def test_ilog2_restatement():
    for e in range(0, 40):
        assert br.ilog2_q12(1 << e) == 4096 * e
    assert br.ilog2_q12(3) == int(4096 * math.log2(3))          # 6491: truncation only ever lowers it
    for x in (5, 7, 86, 255, 510, 1020, 12345, (1 << 33) + 5):
        assert 0 <= 4096 * math.log2(x) - br.ilog2_q12(x) < 1.01


def test_log_error_is_at_most_one_octave():
    worst = max(br.log_error(L, d) for L in range(br.L_MIN, br.L_MAX + 1) for d in range((L + 1) >> 1, 2 * L + 1))
    assert worst == 4096


def test_bounds_of_the_bounds_curves(plain):
    r = plain["bounds_L510"]
    assert r["rec"]["pen_scale"] == 4096 * br.OMAX < 1 << 30
    assert int(br.penalties(510, r["rec"]["pen_scale"], 255, 1020).max()) < 1 << 26
    assert (1 << 32) < plain["bounds_long_L2"]["rec"]["score"] < 1 << 42


@pytest.mark.parametrize("switch", br.SWITCHES)
def test_every_switch_changes_its_named_curve(corpus, plain, switch):
    name = br.WITNESS[switch]
    if switch in br.PAIRED:
        other = br.PAIRED[switch]
        assert br.same(plain[name], br.track(*corpus[name], **{switch: True})), "provably the definition"
        base = br.track(*corpus[name], **{other: True})
        assert not br.same(base, br.track(*corpus[name], **{other: True, switch: True}))
    else:
        assert not br.same(plain[name], br.track(*corpus[name], **{switch: True}))


def test_blocks_of_lo_equal_the_hop_by_hop_loop(corpus, plain):
    for name, song in corpus.items():
        assert br.same(plain[name], br.track_blocks(*song)), name
    rng = np.random.default_rng(8200)
    for L in (2, 3, 4, 5, 31, 33, 64, 255, 510):
        for H in br.lengths_for(L)[:8]:
            o = rng.integers(0, 1 << 18, H)
            assert br.same(br.track(o, L, 16), br.track_blocks(o, L, 16)), (L, H)


def test_records_of_special_songs(plain):
    z = plain["zeros"]
    assert z["rec"] == dict(score=0, pen_scale=0, hops=90, period=9, n_beats=0, first=-1, last=-1, status=0)
    assert not z["flags"].any() and not z["links"].any() and not z["scores"].any()
    for L in br.BAD_PERIODS:
        r = br.track(np.arange(50), L, 16)
        assert r["rec"] == dict(score=0, pen_scale=0, hops=50, period=L, n_beats=0, first=0, last=0, status=-2)
        assert not r["flags"].any() and not r["links"].any() and not r["scores"].any()
    s = plain["spike_last"]
    assert br.beat_hops(s["flags"]) == [99] and s["rec"]["n_beats"] == 1 and s["rec"]["first"] == s["rec"]["last"] == 99


@pytest.mark.parametrize("period,hops,channels", rr.CLICKS)
def test_click_tracks_give_exactly_the_clicks(period, hops, channels):
    """the corpus tracks of the tempo tests (their seed is the period), and the same tracks from seed 7"""
    for seed in (period, 7):
        o = rr.onsets(rr.click_track(period, hops, channels, seed=seed), channels)
        lag = rr.record_from_onsets(o, rr.LAG_MIN, rr.LAG_MAX)[0]["lag"]
        assert lag == period
        want = list(range(period // 2, hops, period))
        assert len(want) == {43: 26, 86: 16, 130: 13, 200: 10}[period]
        for tight in (16, 128, 1024):
            got = br.track_blocks(o, lag, tight)
            assert br.beat_hops(got["flags"]) == want, (seed, tight)
            assert got["rec"]["n_beats"] == len(want) and got["rec"]["first"] == want[0]
            assert got["rec"]["last"] == want[-1]
            assert br.grid_bpm(got["rec"]) == 60.0 * 22050 / (128.0 * period)


def test_jittered_clicks_are_followed_at_every_tight_from_16_to_256():
    for seed in range(4):
        o = br.jitter_clicks(86, 1400, seed)
        clicks = [int(h) for h in np.flatnonzero(o >= 40000)]
        for tight in (16, 32, 64, 128, 256):
            assert br.beat_hops(br.track_blocks(o, 86, tight)["flags"]) == clicks, (seed, tight)


def test_beats_list_against_python(lib):
    rng = np.random.default_rng(8300)
    i32, f64, u8 = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    for hops, rate in ((1, 22050), (300, 22050), (1000, 44100), (257, 8000)):
        flags = (rng.integers(0, 5, hops) == 0).astype(np.uint8)
        flags[rng.integers(0, hops)] = 7          # any non-zero byte is a set flag
        want = [int(h) for h in np.flatnonzero(flags)]
        fp = flags.ctypes.data_as(u8)
        for cap in (0, 1, len(want) // 2, len(want), len(want) + 5):
            hop, sec = np.full(cap + 1, -9, np.int32), np.full(cap + 1, -9.0)
            assert lib.bl_amd_beats_list(fp, hops, rate, hop.ctypes.data_as(i32), sec.ctypes.data_as(f64), cap) == len(want)
            k = min(cap, len(want))
            assert list(hop[:k]) == want[:k] and (hop[k:] == -9).all()
            assert list(sec[:k]) == [128.0 * h / rate for h in want[:k]] and (sec[k:] == -9.0).all()
            assert lib.bl_amd_beats_list(fp, hops, rate, None, sec.ctypes.data_as(f64), cap) == len(want)
            assert lib.bl_amd_beats_list(fp, hops, rate, hop.ctypes.data_as(i32), None, cap) == len(want)
            assert lib.bl_amd_beats_list(fp, hops, rate, None, None, cap) == len(want)
        h2, s2 = rh.beat_list(flags, rate)
        assert list(h2) == want and list(s2) == [128.0 * h / rate for h in want]
    one = np.ones(4, np.uint8).ctypes.data_as(u8)
    assert lib.bl_amd_beats_list(one, 0, 22050, None, None, 0) == 0
    for bad in ((None, 4, 22050, 0), (one, -1, 22050, 0), (one, 4, 0, 0), (one, 4, 22050, -1)):
        assert lib.bl_amd_beats_list(bad[0], bad[1], bad[2], None, None, bad[3]) == -1


def test_beats_bpm_against_python(lib):
    rec = np.zeros(5, rh.BEATS_DTYPE)
    rec["n_beats"] = [26, 2, 1, 0, 16]
    rec["first"] = [21, 0, 7, -1, 43]
    rec["last"] = [1096, 1, 7, -1, 1333]
    got = rh.beats_bpm(rec, 22050)
    for i in range(5):
        want = br.grid_bpm({k: int(rec[k][i]) for k in ("n_beats", "first", "last")})
        assert (math.isnan(want) and math.isnan(got[i])) or got[i] == want, i
    assert got[0] == 60.0 * 22050 / (128.0 * 43) and math.isnan(got[2]) and math.isnan(got[3])
    one = _lib.SongBeats(n_beats=3, first=10, last=30)
    assert lib.bl_amd_beats_bpm(C.byref(one), 48000) == 60.0 * 48000 * 2 / (128.0 * 20)
    assert math.isnan(lib.bl_amd_beats_bpm(C.byref(one), 0)) and math.isnan(lib.bl_amd_beats_bpm(None, 22050))
    assert rh.BEATS_DTYPE.itemsize == C.sizeof(_lib.SongBeats) == 40
    assert rh.BEATS_DTYPE.names == br.FIELDS


def test_python_checks():
    with pytest.raises(ValueError):
        rh.beats_host([], [])
    with pytest.raises(ValueError):
        rh.beats_host([np.array([1 << 18])], [4])
    with pytest.raises(ValueError):
        rh.beats_host([np.arange(4)], [4, 5])
    with pytest.raises(ValueError):
        rh.beats_host([np.arange(4)], [4], tight=4097)
    with pytest.raises(ValueError):
        rh.beat_list(np.zeros((2, 2), np.uint8))
    with pytest.raises(ValueError):
        rh.beats_bpm(np.zeros(2, rh.RHYTHM_DTYPE))


def test_host_form_fails_loudly_without_a_device(lib):
    import torch
    if torch.cuda.is_available():
        return
    o = np.arange(100, dtype=np.uint32)
    hops, per = (C.c_int32 * 1)(100), (C.c_int32 * 1)(10)
    rec, flags = (_lib.SongBeats * 1)(), np.full(100, 0xA5, np.uint8)
    assert lib.bl_amd_beats_host(o.ctypes.data_as(C.POINTER(C.c_uint32)), hops, 1, per, 16, rec,
                                 flags.ctypes.data_as(C.POINTER(C.c_uint8)), None, None) == _lib.BL_UNEXPECTED
    assert (flags == 0xA5).all()
    assert lib.bl_amd_beats_device(None, hops, 1, None, 4, 16, None, None, None, None, None) == _lib.BL_UNEXPECTED
    with pytest.raises(RuntimeError):
        rh.beats_host([o], [10])
