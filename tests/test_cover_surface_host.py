"""bliss_amd.cover without a device: the module imports, the host arithmetic of bl_amd_cover_* (score, tempo_ratio,
seconds, shape) gives values worked out by hand and its documented NaNs, the records have the header's layout, and a
rejected argument list is refused before any device call."""
import ctypes as C
import math

import numpy as np
import pytest

import bliss_amd
import bliss_amd.cover as cover
from bliss_amd import _lib
from bliss_amd.records import COVER_MATCH_DTYPE


def test_module_is_explicit_and_the_records_are_the_headers():
    assert not hasattr(bliss_amd, "match_device") and "cover" not in getattr(bliss_amd, "__all__", [])
    assert C.sizeof(_lib.CoverMatch) == 40 and C.sizeof(_lib.CoverParams) == 16
    assert COVER_MATCH_DTYPE.itemsize == 40 and COVER_MATCH_DTYPE.names == (
        "score", "a_start", "a_end", "b_start", "b_end", "transpose", "units_a", "units_b", "status", "reserved")
    assert [COVER_MATCH_DTYPE.fields[n][1] for n in COVER_MATCH_DTYPE.names] == list(range(0, 40, 4))
    assert [f[0] for f in _lib.CoverParams._fields_] == ["thr", "gap", "transpose", "reserved"]
    assert (cover.UNITS_MAX, cover.NO_MATCH, cover.TOO_LONG, cover.BAD_INDEX, cover.HOP) == (8192, 1, 2, 4, 2048)
    assert cover.pairs_from_knn(np.array([[1, 2], [0, -1]])).tolist() == [[0, 1], [0, 2], [1, 0], [1, -1]]


def test_params_defaults_and_ranges():
    p = cover.params()
    assert isinstance(p, _lib.CoverParams) and (p.thr, p.gap, p.transpose, p.reserved) == (12000, 4000, -1, 0)
    p = cover.params(thr=1, gap=1 << 20, transpose=11)
    assert (p.thr, p.gap, p.transpose) == (1, 1 << 20, 11) and cover.params(thr=16128, gap=0).gap == 0
    for kw in (dict(thr=0), dict(thr=16129), dict(gap=-1), dict(gap=(1 << 20) + 1), dict(transpose=-2),
               dict(transpose=12), dict(thr=2.5)):
        with pytest.raises(ValueError):
            cover.params(**kw)


def test_score(lib):
    rec = np.zeros(6, dtype=COVER_MATCH_DTYPE)
    rec["score"] = [4129 * 100, 4129 * 50, 7, 7, 7, 7]
    rec["units_a"], rec["units_b"] = [100, 100, 0, 10, 10, 10], [300, 40, 10, 10, 10, 10]
    rec["status"] = [0, 0, 0, cover.NO_MATCH, cover.TOO_LONG, cover.BAD_INDEX]
    s = cover.score(rec, 12000)
    assert s[0] == 1.0 and s[1] == 50 / 40 and all(math.isnan(v) for v in s[2:])
    assert cover.score(rec[:1], 16128)[0] == 4129.0 and cover.score(rec[:1], 129)[0] == 4129 / 16000
    assert math.isnan(lib.bl_amd_cover_score(None, 12000))
    one = _lib.CoverMatch(score=5, units_a=1, units_b=1)
    assert lib.bl_amd_cover_score(C.byref(one), 16124) == 1.0
    assert math.isnan(lib.bl_amd_cover_score(C.byref(one), 16129))      # a zero denominator
    assert math.isnan(lib.bl_amd_cover_score(C.byref(one), 20000))
    with pytest.raises(ValueError):
        cover.score(np.zeros(0, dtype=COVER_MATCH_DTYPE))
    with pytest.raises(ValueError):
        cover.score(np.zeros(3, dtype=np.int32))


def test_tempo_ratio(lib):
    rec = np.zeros(4, dtype=COVER_MATCH_DTYPE)
    rec["a_start"], rec["a_end"], rec["b_start"], rec["b_end"] = [0, 10, 5, 0], [99, 109, 5, 9], [20, 0, 7, 0], [144, 88, 7, 9]
    rec["status"] = [0, 0, 0, cover.NO_MATCH]
    t = cover.tempo_ratio(rec)
    assert t[0] == 1.25 and t[1] == 0.89 and t[2] == 1.0 and math.isnan(t[3])
    assert math.isnan(lib.bl_amd_cover_tempo_ratio(None))


def test_seconds(lib):
    assert cover.seconds(0) == 0.0 and cover.seconds(97) == 97 * 2048 / 22050
    assert cover.seconds(10, pool=4, rate=44100) == 10 * 4 * 2048 / 44100
    assert math.isnan(lib.bl_amd_cover_seconds(-1, 1, 22050)) and math.isnan(lib.bl_amd_cover_seconds(1, 0, 22050))
    assert math.isnan(lib.bl_amd_cover_seconds(1, 17, 22050)) and math.isnan(lib.bl_amd_cover_seconds(1, 1, 0))
    for bad in (dict(unit=-1), dict(unit=1, pool=0), dict(unit=1, pool=17), dict(unit=1, rate=0)):
        with pytest.raises(ValueError):
            cover.seconds(**bad)


def test_shape_reports_one_column_per_lane(lib):
    assert cover.shape() == (64, 64)
    lib.bl_amd_cover_shape(None, None)


def test_profile_ms_knows_its_two_kernels(lib):
    n = C.c_int(-1)
    assert lib.bl_amd_cover_profile_ms(b"nothing", C.byref(n)) == -1.0 and n.value == 0
    assert lib.bl_amd_cover_profile_ms(None, None) == -1.0
    for name in (b"cover_profile", b"cover_align"):
        assert lib.bl_amd_cover_profile_ms(name, C.byref(n)) == 0.0 and n.value == 0


def test_arguments_are_refused_before_any_device_call(lib):
    """every list below is rejected by the argument checks, which come before the context is asked for: the answers
    are the same with and without a device, and the outputs keep their fill"""
    units = np.zeros((8, 16), dtype=np.uint8)
    with pytest.raises(ValueError):
        cover.match_host(units, [4, 4], [(0, 1)], dict(thr=12000))
    with pytest.raises(ValueError):
        cover.match_host(units, [4, 5], [(0, 1)])
    with pytest.raises(ValueError):
        cover.match_host(units, [], [(0, 1)])
    with pytest.raises(ValueError):
        cover.match_host(units, [4, 4], np.zeros((0, 2), np.int32))
    with pytest.raises(ValueError):
        cover.match_host(units, [4, 4], [0, 1, 2])
    with pytest.raises(ValueError):
        cover.match_host(units, [4, 1 << 20], [(0, 1)])
    with pytest.raises(ValueError):
        cover.units_host(np.zeros((4, 12), np.uint64), [5])
    with pytest.raises(ValueError):
        cover.units_host(np.zeros((4, 11), np.uint64), [4])
    with pytest.raises(ValueError):
        cover.units_host(np.zeros((4, 12), np.uint64), [4], pool=17)
    with pytest.raises(ValueError):
        cover.units_host(np.zeros((0, 12), np.uint64), [])

    cnt, pairs = (C.c_int32 * 2)(4, 4), np.array([[0, 1]], dtype=np.int32)
    out = np.full(40, 0xA5, dtype=np.uint8)
    good = _lib.CoverParams(12000, 4000, -1, 0)
    u, pp, o = C.c_void_p(units.ctypes.data), C.c_void_p(pairs.ctypes.data), C.c_void_p(out.ctypes.data)
    host = lambda **kw: lib.bl_amd_cover_match_host(*[kw.get(k, v) for k, v in (
        ("a", u), ("ca", cnt), ("na", 2), ("b", u), ("cb", cnt), ("nb", 2), ("pairs", pp), ("n", 1),
        ("p", C.byref(good)), ("out", o))])
    bad_params = [_lib.CoverParams(*v) for v in ((0, 4000, -1, 0), (16129, 4000, -1, 0), (12000, -1, -1, 0),
                                                 (12000, (1 << 20) + 1, -1, 0), (12000, 4000, -2, 0),
                                                 (12000, 4000, 12, 0), (12000, 4000, -1, 1), (12000, 4000, -1, -1))]
    for kw in [dict(a=None), dict(ca=None), dict(b=None), dict(cb=None), dict(pairs=None), dict(p=None), dict(out=None),
               dict(na=0), dict(nb=-1), dict(n=0), dict(ca=(C.c_int32 * 2)(4, -1)), dict(cb=(C.c_int32 * 2)(1 << 20, 4))] + \
              [dict(p=C.byref(b)) for b in bad_params]:
        assert host(**kw) == _lib.BL_UNEXPECTED, list(kw)
    assert (out == 0xA5).all()
    # the device forms check pointers they never follow: aligned and misaligned dummies
    dev = lambda **kw: lib.bl_amd_cover_match_device(*[kw.get(k, v) for k, v in (
        ("a", C.c_void_p(4096)), ("ca", cnt), ("na", 2), ("b", C.c_void_p(4096)), ("cb", cnt), ("nb", 2),
        ("pairs", C.c_void_p(8192)), ("n", 1), ("p", C.byref(good)), ("out", C.c_void_p(12288)), ("stream", None))])
    for kw in (dict(a=C.c_void_p(4096 + 8)), dict(b=C.c_void_p(4096 + 4)), dict(pairs=C.c_void_p(8192 + 4)),
               dict(out=C.c_void_p(12288 + 2)), dict(a=None), dict(out=None), dict(n=0), dict(p=C.byref(bad_params[0]))):
        assert dev(**kw) == _lib.BL_UNEXPECTED, list(kw)
    frames_cnt = (C.c_int32 * 2)(6, 5)
    udev = lambda **kw: lib.bl_amd_cover_units_device(*[kw.get(k, v) for k, v in (
        ("frames", C.c_void_p(4096)), ("counts", frames_cnt), ("n", 2), ("pool", 2), ("out", C.c_void_p(8192)),
        ("n_units", 5), ("stream", None))])
    for kw in (dict(frames=None), dict(frames=C.c_void_p(4100)), dict(counts=None), dict(n=0), dict(pool=0), dict(pool=17),
               dict(out=None), dict(out=C.c_void_p(8200)), dict(n_units=4), dict(n_units=6),
               dict(counts=(C.c_int32 * 2)(6, -1)), dict(counts=(C.c_int32 * 2)(1 << 20, 5))):
        assert udev(**kw) == _lib.BL_UNEXPECTED, list(kw)
    assert lib.bl_amd_cover_units_host(None, frames_cnt, 2, 2, o) == _lib.BL_UNEXPECTED
    assert lib.bl_amd_cover_units_host(u, frames_cnt, 2, 0, o) == _lib.BL_UNEXPECTED and (out == 0xA5).all()
