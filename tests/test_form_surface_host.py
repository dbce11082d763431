"""bliss_amd.form without a device: the module imports, and the host arithmetic of bl_amd_form_* (units_count, seconds,
score, shape), sections() and the argument checks are compared with values worked out by hand."""
import math

import numpy as np
import pytest

import bliss_amd
import bliss_amd.form as form
from bliss_amd import _lib
from bliss_amd.records import FORM_DTYPE


def test_module_is_explicit_and_the_record_is_the_headers():
    assert not hasattr(bliss_amd, "form_device") and "form" not in getattr(bliss_amd, "__all__", [])
    assert FORM_DTYPE.itemsize == 48 and FORM_DTYPE.names == (
        "units", "status", "thumb_start", "thumb_lag", "thumb_score", "thumb_self", "boundaries", "nov_max_unit",
        "nov_max", "reserved")
    assert [FORM_DTYPE.fields[n][1] for n in FORM_DTYPE.names] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 40]
    assert (form.UNITS_MAX, form.NO_THUMB, form.TOO_LONG, form.HOP) == (8192, 1, 2, 2048)


def test_units_count(lib):
    assert [form.units_count(t, p) for t, p in ((0, 1), (5, 1), (5, 2), (15, 16), (16, 16), (1937, 4))] == \
        [0, 5, 2, 0, 1, 484]
    assert form.units_count(7) == 7
    assert lib.bl_amd_form_units(-1, 1) == -1 and lib.bl_amd_form_units(5, 0) == -1 and lib.bl_amd_form_units(5, 17) == -1
    for bad in ((-1, 1), (5, 0), (5, 17)):
        with pytest.raises(ValueError):
            form.units_count(*bad)


def test_seconds(lib):
    assert form.seconds(0) == 0.0 and form.seconds(97) == 97 * 2048 / 22050
    assert form.seconds(10, pool=4, rate=44100) == 10 * 4 * 2048 / 44100
    assert math.isnan(lib.bl_amd_form_seconds(-1, 1, 22050)) and math.isnan(lib.bl_amd_form_seconds(1, 0, 22050))
    assert math.isnan(lib.bl_amd_form_seconds(1, 17, 22050)) and math.isnan(lib.bl_amd_form_seconds(1, 1, 0))


def test_score(lib):
    rec = np.zeros(4, dtype=FORM_DTYPE)
    rec["thumb_score"], rec["thumb_self"] = [3, 700000, 5, 5], [4, 700000, 0, 10]
    rec["status"] = [0, form.TOO_LONG * 0, 0, form.NO_THUMB]
    s = form.score(rec)
    assert s[0] == 0.75 and s[1] == 1.0 and math.isnan(s[2]) and math.isnan(s[3])
    assert math.isnan(lib.bl_amd_form_score(None))
    with pytest.raises(ValueError):
        form.score(np.zeros(0, dtype=FORM_DTYPE))


def test_shape_reports_positive_lengths(lib):
    chunk, block = form.shape()
    assert chunk >= 64 and block >= 64
    lib.bl_amd_form_shape(None, None)


def test_sections():
    flags = np.zeros(12, dtype=np.uint8)
    assert form.sections(flags, 12) == [(0, 12)] and form.sections(flags, 0) == []
    flags[[3, 4, 9]] = 1
    assert form.sections(flags, 12) == [(0, 3), (3, 4), (4, 9), (9, 12)]
    assert form.sections(flags, 9) == [(0, 3), (3, 4), (4, 9)]
    flags[0], flags[11] = 1, 3                                  # a boundary at 0 opens nothing; only bit 0 counts
    assert form.sections(flags, 12) == [(0, 3), (3, 4), (4, 9), (9, 11), (11, 12)]
    flags[11] = 2
    assert form.sections(flags, 12)[-1] == (9, 12)
    with pytest.raises(ValueError):
        form.sections(flags, 13)


def test_params_are_checked_before_the_library_sees_them():
    p = form.params(pool=4, seg=40, nov=11)
    assert (p.pool, p.seg, p.min_lag, p.nov, p.peak_num, p.peak_den, p.reserved) == (4, 40, 40, 11, 1, 4, 0)
    assert isinstance(p, _lib.FormParams) and form.params(min_lag=7).min_lag == 7
    for kw in (dict(pool=0), dict(pool=17), dict(seg=1), dict(seg=1025), dict(min_lag=0), dict(min_lag=8193),
               dict(nov=0), dict(nov=65), dict(peak_den=0), dict(peak_den=257), dict(peak_num=-1), dict(peak_num=5),
               dict(seg=2.5)):
        with pytest.raises(ValueError):
            form.params(**kw)
    with pytest.raises(ValueError):
        form.form_host(np.zeros((4, 12), np.uint64), [4], dict(pool=1))
    with pytest.raises(ValueError):
        form.form_host(np.zeros((4, 12), np.uint64), [5], p)
    with pytest.raises(ValueError):
        form.form_host(np.zeros((4, 11), np.uint64), [4], p)
    with pytest.raises(ValueError):
        form.form_host(np.zeros((0, 12), np.uint64), [], p)
