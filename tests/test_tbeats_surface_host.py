"""The beats that follow the tempo over time (bliss_amd.tempogram: beats_*; bl_amd_tbeats_*) without a device: the
records and the parameters have the header's layout, the host arithmetic (params_from_tgram, edge_bpm, shape) gives
values worked out in Python floats and its refusals, and a rejected argument list is refused before any device call."""
import ctypes as C
import math

import numpy as np
import pytest

import bliss_amd
import bliss_amd.tempogram as tg
from bliss_amd import _lib
from bliss_amd.records import TBEATS_DTYPE
from tests import tbeats_reference as tb
from tests import tgram_reference as tr

UNEXPECTED = _lib.BL_UNEXPECTED


def raw_params(**kw):
    """a bl_amd_tbeats_params with seg 64, origin 96, tight 128 and the given fields, unchecked"""
    p = tg.beats_params(seg=64, origin=96)
    for k, v in kw.items():
        if k == "reserved":
            p.reserved[v] = 1
        else:
            setattr(p, k, v)
    return p


BAD = [dict(seg=15), dict(seg=0), dict(seg=16385), dict(seg=-64), dict(origin=-1), dict(origin=1 << 24), dict(tight=-1),
       dict(tight=4097), dict(fold=2), dict(fold=-1), dict(reserved=0), dict(reserved=1), dict(reserved=2),
       dict(reserved=3)]


def test_the_records_are_the_headers():
    assert not hasattr(bliss_amd, "beats_from_pcm")
    assert C.sizeof(_lib.TbeatsParams) == 32 and C.sizeof(_lib.SongTbeats) == 64 == TBEATS_DTYPE.itemsize
    assert TBEATS_DTYPE == tb.SONG_DTYPE and TBEATS_DTYPE.names == tb.FIELDS
    assert [TBEATS_DTYPE.fields[n][1] for n in TBEATS_DTYPE.names] == [0, 8] + list(range(16, 64, 4))
    P = _lib.TbeatsParams
    assert [f[0] for f in P._fields_] == ["seg", "origin", "tight", "fold", "reserved"]
    assert P.reserved.offset == 16 and P.reserved.size == 16
    # what beats_device() reads in place
    assert _lib.TgramFrame.lag.offset == 32 and C.sizeof(_lib.TgramFrame) == 40
    assert _lib.SongTgram.lag_median.offset == 40 and C.sizeof(_lib.SongTgram) == 56


def test_params_from_tgram(lib):
    for tp, tight, fold in ((tr.WORKED, 128, 0), (tr.SMALL, 0, 1), (tr.TINY, 4096, 1), (tr.params(1024, 16), 16, 0),
                            (tr.params(16, 1), 16, 0), (tr.params(48, 15), 7, 1), (tr.params(48, 4), 7, 1)):
        bp = tg.beats_params(tg.params(tp["stride"], tp["blocks"], tp["lag_min"], tp["lag_max"], tp["tol"],
                                       bool(tp["octaves"])), tight, bool(fold))
        want = tb.from_tgram(tp, tight, fold)
        assert (bp.seg, bp.origin, bp.tight, bp.fold, list(bp.reserved)) == (want["seg"], want["origin"], tight, fold,
                                                                             [0] * 4)
    bp = tg.beats_params()
    assert (bp.seg, bp.origin, bp.tight, bp.fold) == (128, 960, 128, 0)
    bp = tg.beats_params(seg=16384, origin=(1 << 24) - 1, tight=0, fold=True)
    assert (bp.seg, bp.origin, bp.tight, bp.fold) == (16384, (1 << 24) - 1, 0, 1)
    out, good = _lib.TbeatsParams(), tg.params()
    out.seg = 77
    bad = tg.params()
    bad.stride = 24
    for args in ((None, 128, 0, C.byref(out)), (C.byref(good), 128, 0, None), (C.byref(bad), 128, 0, C.byref(out)),
                 (C.byref(good), -1, 0, C.byref(out)), (C.byref(good), 4097, 0, C.byref(out)),
                 (C.byref(good), 128, 2, C.byref(out)), (C.byref(good), 128, -1, C.byref(out))):
        assert lib.bl_amd_tbeats_params_from_tgram(*args) == -1
    assert out.seg == 77
    for kw in (dict(tight=-1), dict(tight=4097), dict(seg=15, origin=0), dict(seg=16385), dict(seg=64, origin=-1),
               dict(seg=64, origin=1 << 24), dict(p=dict(stride=16))):
        with pytest.raises(ValueError):
            tg.beats_params(**kw)


def test_edge_bpm(lib):
    flags = np.zeros(400, np.uint8)
    beats = [3, 43, 84, 126, 170, 215, 262, 310, 399]
    flags[beats] = 1
    for n in (2, 3, 8, 9, 10, 1000):
        k = min(n, len(beats))
        assert tg.edge_bpm(flags, n) == 60.0 * 22050 * (k - 1) / (128.0 * (beats[k - 1] - beats[0]))
        assert tg.edge_bpm(flags, n, at_end=True) == 60.0 * 22050 * (k - 1) / (128.0 * (beats[-1] - beats[-k]))
        assert tg.edge_bpm(flags, n) == tb.edge_bpm(flags, 22050, n, False)
        assert tg.edge_bpm(flags, n, True, rate=44100) == tb.edge_bpm(flags, 44100, n, True)
    assert tg.edge_bpm(flags[:44], 8) == 60.0 * 22050 / (128.0 * 40)
    for nan in (tg.edge_bpm(flags, 1), tg.edge_bpm(flags, 0), tg.edge_bpm(flags[:43], 8), tg.edge_bpm(flags[:3], 8),
                tg.edge_bpm(np.zeros(0, np.uint8), 8), tg.edge_bpm(flags[:43], 8, at_end=True)):
        assert math.isnan(nan)
    ptr = C.c_void_p(flags.ctypes.data)
    assert math.isnan(lib.bl_amd_tbeats_edge_bpm(None, 400, 22050, 8, 0))
    assert math.isnan(lib.bl_amd_tbeats_edge_bpm(ptr, 400, 0, 8, 0))
    assert math.isnan(lib.bl_amd_tbeats_edge_bpm(ptr, -1, 22050, 8, 0))
    assert math.isnan(lib.bl_amd_tbeats_edge_bpm(ptr, 400, 22050, -2, 1))
    # bl_amd_beats_list works on the same flags
    hops = (C.c_int32 * 16)()
    assert lib.bl_amd_beats_list(flags.ctypes.data_as(C.POINTER(C.c_uint8)), 400, 22050, hops, None, 16) == 9
    assert list(hops[:9]) == beats


def test_shape_and_profile_ms_know_their_names(lib):
    assert tg.beats_shape() == (2048, 256) and tb.TILE == 256
    lib.bl_amd_tbeats_shape(None, None)
    n = C.c_int(-1)
    assert lib.bl_amd_tbeats_profile_ms(b"tgram_blocks", C.byref(n)) == -1.0 and n.value == 0
    assert lib.bl_amd_tbeats_profile_ms(None, None) == -1.0
    for name in (b"tbeats_track", b"tbeats"):
        assert lib.bl_amd_tbeats_profile_ms(name, C.byref(n)) == 0.0 and n.value == 0


def test_arguments_are_refused_before_any_device_call(lib):
    """every list below is rejected by the argument checks, which come before the context is asked for: the answers
    are the same with and without a device, and the outputs keep their fill"""
    good = raw_params()
    curve = np.full(300 + 200, 5, dtype=np.uint32)
    lags = np.array([40, 40, 0, 90, 90], np.int32)
    anchors = np.array([40, 90], np.int32)
    for bad in (dict(onsets_list=[]), dict(onsets_list=[np.full(600, 1 << 18)] * 2), dict(lags_list=[[40]]),
                dict(anchors=[40]), dict(bp=dict(seg=64)), dict(onsets_list=[np.zeros(0, np.uint32)] * 2)):
        kw = dict(onsets_list=[curve[:300], curve[300:]], lags_list=[lags[:3], lags[3:]], anchors=None, bp=good)
        kw.update(bad)
        with pytest.raises(ValueError):
            tg.beats_host(**kw)

    hops, frames = (C.c_int32 * 2)(300, 200), (C.c_int32 * 2)(3, 2)
    i32 = lambda *v: (C.c_int32 * len(v))(*v)
    songs, flags, links, scores, track = (np.full(n, 0xA5, dtype=np.uint8) for n in (128, 500, 1000, 4000, 20))
    outs = (songs, flags, links, scores, track)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    host = lambda **kw: lib.bl_amd_tbeats_host(*[kw.get(k, v) for k, v in (
        ("o", ptr(curve)), ("h", hops), ("f", frames), ("n", 2), ("lag", ptr(lags)), ("anchor", ptr(anchors)),
        ("p", C.byref(good)), ("songs", ptr(songs)), ("flags", ptr(flags)), ("links", ptr(links)),
        ("scores", ptr(scores)), ("track", ptr(track)))])
    over = curve.copy()
    over[499] = 1 << 18
    bad_params = [raw_params(**kw) for kw in BAD]
    for kw in [dict(o=None), dict(h=None), dict(f=None), dict(p=None), dict(songs=None), dict(flags=None), dict(lag=None),
               dict(n=0), dict(n=-1), dict(h=i32(300, 0)), dict(h=i32(1 << 24, 200)), dict(f=i32(3, -1)),
               dict(f=i32((1 << 20) + 1, 2)), dict(o=ptr(over))] + [dict(p=C.byref(b)) for b in bad_params]:
        assert host(**kw) == UNEXPECTED, list(kw)
    assert all((a == 0xA5).all() for a in outs)
    # the device forms check pointers they never follow: aligned and misaligned dummies
    for fn, lead in ((lib.bl_amd_tbeats_device, ()), (lib.bl_amd_ctx_tbeats_device, (None,))):
        dev = lambda **kw: fn(*lead, *[kw.get(k, v) for k, v in (
            ("o", C.c_void_p(4096)), ("h", hops), ("f", frames), ("n", 2), ("lag", C.c_void_p(8192)), ("ls", 40),
            ("anchor", C.c_void_p(12288)), ("as", 56), ("p", C.byref(good)), ("songs", C.c_void_p(16384)),
            ("flags", C.c_void_p(20481)), ("links", C.c_void_p(24576)), ("scores", C.c_void_p(28672)),
            ("track", C.c_void_p(32768)), ("stream", None))])
        for kw in [dict(o=None), dict(h=None), dict(f=None), dict(p=None), dict(songs=None), dict(flags=None),
                   dict(lag=None), dict(o=C.c_void_p(4096 + 2)), dict(lag=C.c_void_p(8192 + 2)),
                   dict(anchor=C.c_void_p(12288 + 1)), dict(songs=C.c_void_p(16384 + 4)), dict(links=C.c_void_p(24576 + 1)),
                   dict(scores=C.c_void_p(28672 + 4)), dict(track=C.c_void_p(32768 + 2)), dict(ls=0), dict(ls=2),
                   dict(ls=6), dict(ls=-4), dict(**{"as": 0}), dict(**{"as": 58}), dict(**{"as": -56}), dict(n=0),
                   dict(n=-3), dict(h=i32(300, -1)), dict(h=i32(1 << 24, 200)), dict(f=i32(-1, 2)),
                   dict(f=i32(3, (1 << 20) + 1))] + [dict(p=C.byref(b)) for b in bad_params]:
            assert dev(**kw) == UNEXPECTED, list(kw)
