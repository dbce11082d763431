"""bliss_amd.chords without a device: the module imports, the records and the parameters have the header's layout, the
host arithmetic of bl_amd_chords_* (costs, name, segments, shape) gives values worked out by hand and its refusals, and a
rejected argument list is refused before any device call."""
import ctypes as C

import numpy as np
import pytest

import bliss_amd
import bliss_amd.chords as chords
from bliss_amd import _lib
from bliss_amd.records import CHORDS_DTYPE
from tests import chords_reference as cr


def test_module_is_explicit_and_the_records_are_the_headers():
    assert not hasattr(bliss_amd, "chords_device") and "chords" not in getattr(bliss_amd, "__all__", [])
    assert C.sizeof(_lib.SongChords) == 32 and C.sizeof(_lib.ChordsParams) == 1264
    assert CHORDS_DTYPE.itemsize == 32 and CHORDS_DTYPE.names == (
        "units", "status", "score", "changes", "top", "top_units", "none_units", "reserved")
    assert [CHORDS_DTYPE.fields[n][1] for n in CHORDS_DTYPE.names] == list(range(0, 32, 4))
    assert CHORDS_DTYPE == cr.CHORDS_DTYPE
    P = _lib.ChordsParams
    assert [f[0] for f in P._fields_] == ["none", "reserved", "cost", "pad"]
    assert (P.none.offset, P.reserved.offset, P.cost.offset, P.pad.offset) == (0, 4, 8, 1258)
    assert (P.cost.size, P.pad.size) == (1250, 6)
    assert (chords.LABELS, chords.NONE, chords.EMPTY, chords.COST_MAX, chords.EMISSION_MAX) == (25, 24, 1, 1024, 381)


def test_costs_by_hand_and_refusals(lib):
    c = chords.costs(60, 15)
    assert c.shape == (25, 25) and c.dtype == np.uint16
    assert c[0, 21] == 60 - 2 * 15            # C (C E G) to Am (A C E): two classes shared
    assert c[0, 5] == 60 - 15                 # C to F (F A C): one
    assert c[0, 6] == 60                      # C to F# (F# A# C#): none
    assert c[0, 12] == 30 and c[21, 0] == 30 and c[0, 24] == 60 and c[24, 13] == 60 and (np.diag(c) == 0).all()
    assert (c == c.T).all() and np.array_equal(c, cr.costs(60, 15))
    assert np.array_equal(chords.costs(1024, 512), cr.costs(1024, 512)) and not chords.costs(0, 0).any()
    out = (C.c_uint16 * 625)(*([0xA5A5] * 625))
    for change, related in ((60, 31), (1025, 0), (-1, 0), (60, -1), (0, 1), (1 << 30, 1 << 30)):
        assert lib.bl_amd_chords_costs(change, related, out) == _lib.BL_UNEXPECTED, (change, related)
    assert all(v == 0xA5A5 for v in out) and lib.bl_amd_chords_costs(60, 15, None) == _lib.BL_UNEXPECTED
    for kw in (dict(change=60, related=31), dict(change=1025), dict(change=-1), dict(related=-1), dict(change=2.0)):
        with pytest.raises(ValueError):
            chords.costs(**kw)


def test_params_defaults_and_ranges():
    p = chords.params()
    assert isinstance(p, _lib.ChordsParams) and (p.none, p.reserved, list(p.pad)) == (150, 0, [0, 0, 0])
    assert np.array_equal(np.array(p.cost).reshape(25, 25), cr.costs(60, 15))
    table = cr.asymmetric_cost(3)
    p = chords.params(none=0, cost=table)
    assert p.none == 0 and np.array_equal(np.array(p.cost).reshape(25, 25), table)
    assert chords.params(none=381).none == 381
    bad = table.copy()
    bad[3, 4] = 1025
    for kw in (dict(none=-1), dict(none=382), dict(none=1.5), dict(cost=bad), dict(cost=-table), dict(cost=table[:24]),
               dict(cost=table.astype(np.float64)), dict(change=10, related=6)):
        with pytest.raises(ValueError):
            chords.params(**kw)


def test_name(lib):
    assert [chords.name(k) for k in range(25)] == [cr.name(k) for k in range(25)]
    assert (chords.name(0), chords.name(11), chords.name(12), chords.name(21), chords.name(24)) == ("C", "B", "Cm", "Am", "N")
    assert chords.name(25) == "" and chords.name(-1) == "" and lib.bl_amd_chords_name(1 << 30) == b""


def test_segments_with_a_cap_smaller_than_the_run_count(lib):
    lab = np.array([0, 0, 7, 7, 7, 24, 0, 0, 5], dtype=np.uint8)
    starts, ch = chords.segments(lab)
    assert starts.tolist() == [0, 2, 5, 6, 8] and ch.tolist() == [0, 7, 24, 0, 5]
    assert (starts.tolist(), ch.tolist()) == cr.segments(lab)
    s, c = np.full(4, -7, dtype=np.int32), np.full(4, 0xA5, dtype=np.uint8)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    assert lib.bl_amd_chords_segments(ptr(lab), 9, ptr(s), ptr(c), 2) == 5        # all runs counted, two written
    assert s.tolist() == [0, 2, -7, -7] and c.tolist() == [0, 7, 0xA5, 0xA5]
    assert lib.bl_amd_chords_segments(ptr(lab), 9, None, None, 0) == 5
    assert lib.bl_amd_chords_segments(ptr(lab), 1, None, ptr(c), 4) == 1 and c[0] == 0
    assert lib.bl_amd_chords_segments(None, 0, None, None, 0) == 0
    assert lib.bl_amd_chords_segments(None, 3, None, None, 0) == -1
    assert lib.bl_amd_chords_segments(ptr(lab), -1, None, None, 0) == -1
    assert lib.bl_amd_chords_segments(ptr(lab), 9, None, None, -1) == -1
    e = chords.segments([])
    assert e[0].size == 0 and e[1].size == 0


def test_shape_and_profile_ms_know_their_names(lib):
    step, trace, spw = chords.shape()
    assert step == 4 and trace == 256 and spw in (1, 2)
    lib.bl_amd_chords_shape(None, None, None)
    n = C.c_int(-1)
    assert lib.bl_amd_chords_profile_ms(b"nothing", C.byref(n)) == -1.0 and n.value == 0
    assert lib.bl_amd_chords_profile_ms(None, None) == -1.0
    for name in (b"chords_forward", b"chords_trace"):
        assert lib.bl_amd_chords_profile_ms(name, C.byref(n)) == 0.0 and n.value == 0


def _bad_params():
    out = []
    for kw in (dict(none=-1), dict(none=382), dict(reserved=1), dict(reserved=-1), dict(pad=0), dict(pad=2),
               dict(cost=(0, 1025)), dict(cost=(624, 0xFFFF)), dict(cost=(313, 2000))):
        p = chords.params()
        if "pad" in kw:
            p.pad[kw["pad"]] = 1
        elif "cost" in kw:
            p.cost[kw["cost"][0]] = kw["cost"][1]
        else:
            setattr(p, *list(kw.items())[0])
        out.append(p)
    return out


def test_arguments_are_refused_before_any_device_call(lib):
    """every list below is rejected by the argument checks, which come before the context is asked for: the answers
    are the same with and without a device, and the outputs keep their fill"""
    units = np.zeros((8, 16), dtype=np.uint8)
    with pytest.raises(ValueError):
        chords.chords_host(units, [4, 4], dict(none=150))
    with pytest.raises(ValueError):
        chords.chords_host(units, [4, 5])
    with pytest.raises(ValueError):
        chords.chords_host(units, [])
    with pytest.raises(ValueError):
        chords.chords_host(units, [4, 1 << 20])
    with pytest.raises(ValueError):
        chords.chords_host(units, [4, -1])
    with pytest.raises(ValueError):
        chords.chords_host(units, [4, 2.0])

    cnt = (C.c_int32 * 2)(4, 4)
    rec, lab, hist = (np.full(n, 0xA5, dtype=np.uint8) for n in (64, 8, 200))
    good = chords.params()
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    host = lambda **kw: lib.bl_amd_chords_host(*[kw.get(k, v) for k, v in (
        ("u", ptr(units)), ("c", cnt), ("n", 2), ("p", C.byref(good)), ("rec", ptr(rec)), ("lab", ptr(lab)),
        ("hist", ptr(hist)))])
    bad_params = _bad_params()
    for kw in [dict(u=None), dict(c=None), dict(p=None), dict(rec=None), dict(n=0), dict(n=-1),
               dict(c=(C.c_int32 * 2)(4, -1)), dict(c=(C.c_int32 * 2)(1 << 20, 4))] + \
              [dict(p=C.byref(b)) for b in bad_params]:
        assert host(**kw) == _lib.BL_UNEXPECTED, list(kw)
    assert (rec == 0xA5).all() and (lab == 0xA5).all() and (hist == 0xA5).all()
    # the device forms check pointers they never follow: aligned and misaligned dummies
    for fn, lead in ((lib.bl_amd_chords_device, ()), (lib.bl_amd_ctx_chords_device, (None,))):
        dev = lambda **kw: fn(*lead, *[kw.get(k, v) for k, v in (
            ("u", C.c_void_p(4096)), ("c", cnt), ("n", 2), ("total", 8), ("p", C.byref(good)), ("rec", C.c_void_p(8192)),
            ("lab", C.c_void_p(12289)), ("hist", C.c_void_p(16384)), ("stream", None))])
        for kw in [dict(u=None), dict(c=None), dict(p=None), dict(rec=None), dict(u=C.c_void_p(4096 + 8)),
                   dict(rec=C.c_void_p(8192 + 2)), dict(hist=C.c_void_p(16384 + 2)), dict(n=0), dict(n=-3),
                   dict(total=7), dict(total=9), dict(total=-1), dict(c=(C.c_int32 * 2)(9, -1)),
                   dict(c=(C.c_int32 * 2)(1 << 20, 4), total=(1 << 20) + 4)] + [dict(p=C.byref(b)) for b in bad_params]:
            assert dev(**kw) == _lib.BL_UNEXPECTED, list(kw)
