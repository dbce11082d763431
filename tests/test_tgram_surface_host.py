"""bliss_amd.tempogram without a device: the module imports, the records and the parameters have the header's layout,
the host arithmetic of bl_amd_tgram_* (frames, bpm, seconds, steadiness, shape) gives values worked out by hand and its
refusals, and a rejected argument list is refused before any device call."""
import ctypes as C
import math

import numpy as np
import pytest

import bliss_amd
import bliss_amd.tempogram as tg
from bliss_amd import _lib
from bliss_amd.records import TGRAM_DTYPE, TGRAM_FRAME_DTYPE
from tests import rhythm_reference as rr
from tests import tgram_reference as tr


def make(p):
    return tg.params(p["stride"], p["blocks"], p["lag_min"], p["lag_max"], p["tol"], bool(p["octaves"]))


def raw_params(**kw):
    """a bl_amd_tgram_params with the defaults and the given fields, unchecked"""
    p = tg.params()
    for k, v in kw.items():
        if k == "reserved":
            p.reserved[v] = 1
        else:
            setattr(p, k, v)
    return p


BAD = [dict(stride=0), dict(stride=8), dict(stride=24), dict(stride=1040), dict(stride=-16), dict(blocks=0),
       dict(blocks=17), dict(blocks=-1), dict(lag_min=0), dict(lag_max=511), dict(lag_min=201), dict(lag_min=-1),
       dict(tol=-1), dict(tol=1001), dict(octaves=2), dict(octaves=-1), dict(reserved=0), dict(reserved=1)]


def test_module_is_explicit_and_the_records_are_the_headers():
    assert not hasattr(bliss_amd, "tgram_device") and "tempogram" not in getattr(bliss_amd, "__all__", [])
    assert C.sizeof(_lib.TgramParams) == 32 and C.sizeof(_lib.TgramFrame) == 40 and C.sizeof(_lib.SongTgram) == 56
    assert C.sizeof(_lib.TgramParams) % 16 == 0
    assert TGRAM_FRAME_DTYPE == tr.FRAME_DTYPE and TGRAM_DTYPE == tr.SONG_DTYPE
    assert TGRAM_DTYPE.names == tr.SONG_FIELDS and [TGRAM_DTYPE.fields[n][1] for n in TGRAM_DTYPE.names] == \
        list(range(0, 56, 4))
    assert [TGRAM_FRAME_DTYPE.fields[n][1] for n in TGRAM_FRAME_DTYPE.names] == [0, 8, 16, 24, 32, 36]
    P = _lib.TgramParams
    assert [f[0] for f in P._fields_] == ["stride", "blocks", "lag_min", "lag_max", "tol", "octaves", "reserved"]
    assert P.reserved.offset == 24 and P.reserved.size == 8


def test_params_defaults_and_ranges():
    p = tg.params()
    assert (p.stride, p.blocks, p.lag_min, p.lag_max, p.tol, p.octaves, list(p.reserved)) == (128, 16, 20, 200, 60, 1,
                                                                                              [0, 0])
    q = tg.params(1024, 1, 1, 510, 1000, False)
    assert (q.stride, q.blocks, q.lag_min, q.lag_max, q.tol, q.octaves) == (1024, 1, 1, 510, 1000, 0)
    for kw in (dict(stride=8), dict(stride=24), dict(stride=1040), dict(stride=16.0), dict(blocks=0), dict(blocks=17),
               dict(lag_min=0), dict(lag_max=511), dict(lag_min=30, lag_max=29), dict(tol=-1), dict(tol=1001)):
        with pytest.raises(ValueError):
            tg.params(**kw)
    with pytest.raises(ValueError):
        tg.frames_count(1000, dict(stride=16))


def test_frames_by_hand_and_refusals(lib):
    p = tg.params(16, 1)
    assert [tg.frames_count(h, p) for h in (1, 511, 526, 527, 542, 543)] == [0, 0, 0, 1, 1, 2]
    q = tg.params(1024, 16)
    assert tg.frames_count(511 + 16384 - 1, q) == 0 and tg.frames_count(511 + 16384, q) == 1
    assert tg.frames_count((1 << 24) - 1, p) == ((1 << 24) - 1 - 511 - 16) // 16 + 1
    for ref in (tr.TINY, tr.SMALL, tr.WORKED, tr.params(48, 15)):
        for h in (1, 600, 1551, 4511, 20000):
            assert tg.frames_count(h, make(ref)) == tr.frames_count(h, ref)
    assert lib.bl_amd_tgram_frames(0, C.byref(p)) == -1 and lib.bl_amd_tgram_frames(1 << 24, C.byref(p)) == -1
    assert lib.bl_amd_tgram_frames(-5, C.byref(p)) == -1 and lib.bl_amd_tgram_frames(1000, None) == -1
    for kw in BAD:
        assert lib.bl_amd_tgram_frames(4511, C.byref(raw_params(**kw))) == -1, kw
    with pytest.raises(ValueError):
        tg.frames_count(0, p)
    with pytest.raises(ValueError):
        tg.frames_count(1 << 24, p)


def test_bpm_seconds_and_steadiness(lib):
    fr = np.zeros(3, dtype=TGRAM_FRAME_DTYPE)
    fr[0] = (1000, 700, 900, 800, 43, 86)
    fr[1] = (1000, 0, 0, 0, 0, 0)
    fr[2] = (5, 9, 9, 9, 100, 100)          # flat top: no vertex
    got = tg.bpm(fr)
    assert got[0] == tr.bpm(fr[0]) == rr.bpm(dict(lag=43, r_prev=700, r_lag=900, r_next=800))
    assert math.isnan(got[1]) and got[2] == 60.0 * 22050 / (128 * 100)
    assert tg.bpm(fr, rate=44100)[0] == tr.bpm(fr[0], 44100)
    assert math.isnan(lib.bl_amd_tgram_bpm(None, 22050))
    assert math.isnan(lib.bl_amd_tgram_bpm(fr.ctypes.data_as(C.POINTER(_lib.TgramFrame)), 0))
    p = tg.params(64, 8)
    assert tg.seconds(0, p) == 128 * 256 / 22050 and tg.seconds(54, p) == 128 * (54 * 64 + 256) / 22050
    assert tg.seconds(3, p, rate=44100) == tr.seconds(3, tr.WORKED, 44100)
    assert math.isnan(lib.bl_amd_tgram_seconds(-1, C.byref(p), 22050))
    assert math.isnan(lib.bl_amd_tgram_seconds(0, C.byref(p), 0)) and math.isnan(lib.bl_amd_tgram_seconds(0, None, 22050))
    assert math.isnan(lib.bl_amd_tgram_seconds(0, C.byref(raw_params(stride=24)), 22050))
    st = np.zeros(2, dtype=TGRAM_DTYPE)
    st["n_tempo"], st["n_near"] = (55, 0), (30, 0)
    assert tg.steadiness(st).tolist() == [30 / 55, 0.0] and math.isnan(lib.bl_amd_tgram_steadiness(None))
    with pytest.raises(ValueError):
        tg.steadiness(fr)
    with pytest.raises(ValueError):
        tg.bpm(st)


def test_shape_and_profile_ms_know_their_names(lib):
    tile, run = tg.shape()
    assert tile == 1024 and run == 64
    lib.bl_amd_tgram_shape(None, None)
    n = C.c_int(-1)
    assert lib.bl_amd_tgram_profile_ms(b"nothing", C.byref(n)) == -1.0 and n.value == 0
    assert lib.bl_amd_tgram_profile_ms(None, None) == -1.0
    for name in (b"tgram_blocks", b"tgram_songs"):
        assert lib.bl_amd_tgram_profile_ms(name, C.byref(n)) == 0.0 and n.value == 0


def test_arguments_are_refused_before_any_device_call(lib):
    """every list below is rejected by the argument checks, which come before the context is asked for: the answers
    are the same with and without a device, and the outputs keep their fill"""
    good = tg.params(16, 1)
    curve = np.full(527 + 543, 5, dtype=np.uint32)          # two songs: 1 and 2 frames
    for bad in ([], [np.zeros(0, np.uint32)], [np.full(600, 1 << 18)], [np.full(600, -1)], [np.zeros((2, 300), np.int64)],
                [np.zeros(600)]):
        with pytest.raises(ValueError):
            tg.tgram_host(bad, good)
    with pytest.raises(ValueError):
        tg.tgram_host([curve], dict(stride=16))

    hops = (C.c_int32 * 2)(527, 543)
    songs, frames, gram = (np.full(n, 0xA5, dtype=np.uint8) for n in (112, 120, 3 * 4096))
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    host = lambda **kw: lib.bl_amd_tgram_host(*[kw.get(k, v) for k, v in (
        ("o", ptr(curve)), ("h", hops), ("n", 2), ("p", C.byref(good)), ("songs", ptr(songs)), ("frames", ptr(frames)),
        ("gram", ptr(gram)))])
    over = curve.copy()
    over[1069] = 1 << 18
    bad_params = [raw_params(**kw) for kw in BAD]
    for kw in [dict(o=None), dict(h=None), dict(p=None), dict(songs=None), dict(frames=None), dict(n=0), dict(n=-1),
               dict(h=(C.c_int32 * 2)(527, 0)), dict(h=(C.c_int32 * 2)(1 << 24, 543)), dict(o=ptr(over))] + \
              [dict(p=C.byref(b)) for b in bad_params]:
        assert host(**kw) == _lib.BL_UNEXPECTED, list(kw)
    assert (songs == 0xA5).all() and (frames == 0xA5).all() and (gram == 0xA5).all()
    # the device forms check pointers they never follow: aligned and misaligned dummies
    for fn, lead in ((lib.bl_amd_tgram_device, ()), (lib.bl_amd_ctx_tgram_device, (None,))):
        dev = lambda **kw: fn(*lead, *[kw.get(k, v) for k, v in (
            ("o", C.c_void_p(4096)), ("h", hops), ("n", 2), ("p", C.byref(good)), ("songs", C.c_void_p(8192)),
            ("frames", C.c_void_p(12288)), ("nf", 3), ("gram", C.c_void_p(16384)), ("stream", None))])
        for kw in [dict(o=None), dict(h=None), dict(p=None), dict(songs=None), dict(frames=None),
                   dict(o=C.c_void_p(4096 + 2)), dict(songs=C.c_void_p(8192 + 2)), dict(frames=C.c_void_p(12288 + 4)),
                   dict(gram=C.c_void_p(16384 + 4)), dict(n=0), dict(n=-3), dict(nf=2), dict(nf=4), dict(nf=-1),
                   dict(h=(C.c_int32 * 2)(527, -1)), dict(h=(C.c_int32 * 2)(1 << 24, 543))] + \
                  [dict(p=C.byref(b)) for b in bad_params]:
            assert dev(**kw) == _lib.BL_UNEXPECTED, list(kw)
