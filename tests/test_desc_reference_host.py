"""tests/desc_reference.py against itself (no device): the two forms of d^2 agree, every switch that makes a kernel's
mistake on purpose changes a named case of the ones tests/test_gpu_desc.py runs, and the host side of
bliss_amd.descriptor: features() on hand-made records and the argument checks."""
import numpy as np
import pytest

import bliss_amd.descriptor as D
from bliss_amd import _lib
from bliss_amd.records import (CHROMA_DTYPE, LEVELS_DTYPE, RESULT_DTYPE, RHYTHM_DTYPE, TIMBRE_SONG_DTYPE, levels_db,
                               timbre_hz)
from bliss_amd.rhythm import rhythm_bpm
from tests import desc_reference as R

M = R.SCALE_MAX


def _unit_range(**lo0):
    lo, hi = np.zeros(32, np.float32), np.ones(32, np.float32)
    lo[0] = lo0.get("lo0", 0.0)
    return lo, hi


def test_the_two_forms_of_d2_agree():
    rng = np.random.default_rng(11)
    a = rng.integers(-M, M + 1, size=(70, 32)).astype(np.int16)
    b = rng.integers(-M, M + 1, size=(45, 32)).astype(np.int16)
    ext = (rng.integers(0, 2, size=(40, 32)) * 2 - 1).astype(np.int16) * np.int16(M)   # every |q| = 32512
    ext[0], ext[1] = M, -M
    for p, q in ((a, b), (ext, ext), (a, ext)):
        direct = R.d2_direct(p, q)
        assert np.array_equal(direct, R.d2_planes(p, q))
        brute = ((p[:, None, :].astype(np.int64) - q[None, :, :].astype(np.int64)) ** 2).sum(axis=2)
        assert np.array_equal(direct, brute)
    assert R.d2_direct(ext[:1], ext[1:2])[0, 0] == 32 * 65024 ** 2 < 2 ** 37


def test_digit_split_is_two_signed_bytes():
    q = np.arange(-M, M + 1, dtype=np.int16)
    h, l = R.split(q)
    assert np.array_equal(256 * h + l, q.astype(np.int64))
    assert h.min() == -127 and h.max() == 127 and l.min() == -128 and l.max() == 127
    assert np.array_equal(l, q.astype(np.int8).astype(np.int64))   # l is the low byte of q as a signed byte


def test_range_definition():
    x = np.array([[1.0, np.nan, -0.0, np.inf], [-2.0, np.nan, 0.0, -np.inf], [np.nan, np.nan, -0.0, 5.0]], np.float32)
    lo, hi, cnt = R.desc_range(x)
    assert list(cnt[:5]) == [2, 0, 3, 1, 0]
    assert list(lo[:4]) == [-2.0, 0.0, 0.0, 5.0] and list(hi[:4]) == [1.0, 0.0, 0.0, 5.0]
    assert not np.signbit(lo).any() or lo[0] < 0
    assert not np.signbit(hi).any() and not np.signbit(lo[1:]).any()


def test_quantiser_switches_change_named_cases():
    # a fused scale: t = 15/64 + 2^-55, u rounds to -17/32 (a tie, to even), times 112 is the tie -59.5 -> -60; the
    # fused form sees -59.5 + 1.75 * 2^-48, which rounds to the next double towards zero -> -59
    lo, hi = _unit_range(lo0=-2.0 ** -55)
    x = np.array([[0.234375]], np.float32)
    assert R.quantize(x, lo, hi, [112])[0, 0] == -60 and R.quantize(x, lo, hi, [112], bugs={"fused"})[0, 0] == -59
    # ties: u = 0.5, 1.5 / 3, -0.5 with scale 1 and 3
    lo, hi = _unit_range()
    x = np.array([[0.75], [0.25]], np.float32)
    assert list(R.quantize(x, lo, hi, [1])[:, 0]) == [0, 0]
    assert list(R.quantize(x, lo, hi, [1], bugs={"half_away"})[:, 0]) == [1, -1]
    assert list(R.quantize(x, lo, hi, [3])[:, 0]) == [2, -2]    # 1.5 -> 2 either way: only some ties tell
    # outside the fitted range
    x = np.array([[2.0], [-1.0]], np.float32)
    assert list(R.quantize(x, lo, hi)[:, 0]) == [M, -M]
    assert list(R.quantize(x, lo, hi, bugs={"no_clamp"})[:, 0]) != [M, -M]
    # every other case is 0
    x = np.array([[np.nan, 0.5], [np.inf, 0.5], [0.5, 0.5]], np.float32)
    lo2, hi2 = _unit_range()
    hi2[1] = 0.0   # hi <= lo
    assert not R.quantize(x, lo2, hi2)[:2].any() and list(R.quantize(x, lo2, hi2)[2, :3]) == [0, 0, 0]


def test_pair_switches_change_named_cases():
    a, b = R.one_hot_sets()
    base = R.d2_planes(a, b)
    assert np.array_equal(base, R.d2_direct(a, b))
    # where the dimensions meet: a[i] against b[j] with (7 j + 3) % 32 == i; (0, 27) is one, its mirror (27, 0) is not
    meet = [(i, j) for i in range(32) for j in range(32) if (7 * j + 3) % 32 == i]
    assert len(meet) == 32 and (0, 27) in meet and (27, 0) not in meet
    i, j = 3, 0   # dimension 3: a[3] = 774 (h 3, l 6), b[0] = 11 (h 0, l 11)
    assert base[i, j] == (774 - 11) ** 2
    assert R.d2_planes(a, b, {"hl_only"})[i, j] == base[i, j]        # LH = 6 * 0: silent here, hence distinct digits:
    assert R.d2_planes(a, b, {"hl_only"})[0, 27] != base[0, 27]      # a[0] = 3 (h 0, l 3), b[27] = 7004 (h 27): LH = 81
    for bug in ("unsigned_low", "cross_k", "swap_rc"):
        assert R.d2_planes(a, b, {bug})[i, j] != base[i, j], bug
    # the self form is symmetric and its dot products vanish: only the norms and the row / column mapping show there
    assert np.array_equal(R.d2_planes(a, a, {"cross_k"}) != R.d2_planes(a, a), np.eye(32, dtype=bool))
    # d^2 near 2^37
    ext = np.full((2, 32), M, np.int16)
    ext[1] = -M
    assert R.d2_planes(ext, ext, {"trunc32"})[0, 1] != R.d2_planes(ext, ext)[0, 1] == 32 * 65024 ** 2


def test_selection_switches_change_named_cases():
    rng = np.random.default_rng(5)
    proto = rng.integers(-M, M + 1, size=(3, 32)).astype(np.int16)
    lib = proto[rng.integers(0, 3, size=40)]     # most distances tie: the index decides
    idx, d2 = R.knn(lib, 5)
    for r in range(40):
        same = [j for j in range(40) if j != r and np.array_equal(lib[j], lib[r])]
        assert list(idx[r]) == same[:5] and not d2[r].any() and r not in idx[r]
    assert not np.array_equal(R.knn(lib, 5, bugs={"tie_larger"})[0], idx)
    kept = R.knn(lib, 5, bugs={"keep_self"})[0]
    assert all(r in kept[r] for r in range(4)) and kept[0, 0] == 0 != idx[0, 0]
    # the cross form excludes nothing, and slots beyond the candidates are empty
    ci, cd = R.knn(lib, 5, queries=lib[:4])
    assert all(r in ci[r] for r in range(4))
    i2, e2 = R.knn(lib[:3], 4)
    assert (i2[:, 2:] == -1).all() and (e2[:, 2:] == np.uint64(R.EMPTY)).all() and (i2[:, :2] >= 0).all()
    # ranges are rows of the full call
    assert np.array_equal(R.knn(lib, 5, row_begin=7, n_rows=9)[0], idx[7:16])


def _records(n):
    res = np.zeros(n, RESULT_DTYPE)
    res["tempo"], res["amplitude"] = np.arange(n) - 1.5, 2.0
    res["frequency"], res["attack"] = -np.arange(n), 0.25
    lv = np.zeros(n, LEVELS_DTYPE)
    lv["frames"] = 1000
    lv["peak"] = [[1000 * (i + 1), 500] for i in range(n)]
    lv["sum_sq"] = [[10 ** 9 * (i + 1), 10 ** 7] for i in range(n)]
    lv["zero_cross"] = [[10 * i, 3] for i in range(n)]
    tb = np.zeros(n, TIMBRE_SONG_DTYPE)
    tb["used"] = 4
    tb["centroid_sum"], tb["centroid_sumsq"] = 4 * 40 * 65536, 4 * (40 * 65536) ** 2
    tb["rolloff_sum"], tb["rolloff_sumsq"] = [4 * (60 + i) for i in range(n)], [4 * (60 + i) ** 2 for i in range(n)]
    rh = np.zeros(n, RHYTHM_DTYPE)
    rh["lag"], rh["r0"], rh["r_lag"], rh["r_prev"], rh["r_next"] = 40, 1000, 500, 400, 400
    ch = np.zeros(n, CHROMA_DTYPE)
    ch["chroma"][1:] = np.arange(1, 13, dtype=np.uint64)
    return res, lv, tb, rh, ch


def test_features_on_hand_made_records():
    n = 3
    res, lv, tb, rh, ch = _records(n)
    x, names = D.features(res)
    assert names == ["tempo", "amplitude", "frequency", "attack"] and x.shape == (n, 4) and x.dtype == np.float32
    assert np.array_equal(x[:, 0], res["tempo"])
    x, names = D.features(res, levels=lv, timbre=tb, rhythm=rh, chroma=ch)
    assert x.shape == (n, 25) and len(names) == 25 and len(set(names)) == 25
    assert names[4:7] == ["rms_db", "peak_db", "zcr"] and names[11:13] == ["bpm", "strength"] and names[13] == "chroma_0"
    db, hz = levels_db(lv), timbre_hz(tb)
    bpm, strength = rhythm_bpm(rh)
    assert np.array_equal(x[:, 4], db["rms_db"].max(axis=1).astype(np.float32))
    assert np.array_equal(x[:, 5], db["peak_db"][:, 0].astype(np.float32))
    assert np.array_equal(x[:, 6], db["zcr"].max(axis=1).astype(np.float32)) and x[0, 6] == np.float32(3 / 999)
    for k, name in enumerate(("centroid_hz", "centroid_std_hz", "rolloff_hz", "rolloff_std_hz")):
        assert np.array_equal(x[:, 7 + k], hz[name].astype(np.float32), equal_nan=True)
    assert np.array_equal(x[:, 11], bpm.astype(np.float32), equal_nan=True)
    assert np.array_equal(x[:, 12], strength.astype(np.float32), equal_nan=True)
    assert not x[0, 13:].any()                                   # a zero chroma sum: twelve zeros, no NaN
    assert np.array_equal(x[1, 13:], (np.arange(1, 13) / 78.0).astype(np.float32))
    assert D.features(res, chroma=ch)[1] == names[:4] + names[13:]   # groups not passed are left out
    with pytest.raises(ValueError):
        D.features(res, levels=lv[:2])
    with pytest.raises(ValueError):
        D.features(res, chroma=lv)
    with pytest.raises(ValueError):
        D.features(np.zeros(3))


def test_argument_checks_of_the_python_module():
    x = np.zeros((4, 5), np.float32)
    desc = np.zeros((4, 32), np.int16)
    for bad in (np.zeros((4, 33), np.float32), np.zeros((0, 5), np.float32), np.zeros(5, np.float32)):
        with pytest.raises(ValueError):
            D.fit(bad)
    for scale in (M + 1, -1, [1, 2, 3], [1.5] * 5, True):
        with pytest.raises(ValueError):
            D.fit(x, scale=scale)
    with pytest.raises(ValueError):
        D.quantize(x, np.zeros(2, D.RANGE_DTYPE))
    with pytest.raises(ValueError):
        D.quantize(x, np.zeros(384, np.uint8))
    for k in (0, 129, 1.0, True):
        with pytest.raises(ValueError):
            D.knn(desc, k)
    for bad in (desc.astype(np.int32), np.zeros((4, 31), np.int16), np.zeros((0, 32), np.int16)):
        with pytest.raises(ValueError):
            D.knn(bad, 1)
        with pytest.raises(ValueError):
            D.knn(desc, 1, queries=bad)
    assert D.DESC_DTYPE.itemsize == 64 and D.RANGE_DTYPE.itemsize == 384
    assert (D.DIMS, D.SCALE_MAX) == (R.DIMS, R.SCALE_MAX) == (_lib.BL_AMD_DESC_DIMS, _lib.BL_AMD_DESC_SCALE_MAX)
    d = D.distance(np.array([0, M * M, 4 * M * M, R.EMPTY], dtype=np.uint64))
    assert d.dtype == np.float64 and list(d) == [0.0, 1.0, 2.0, np.inf]


def test_the_calls_fail_loudly_without_a_device():
    import torch
    if torch.cuda.is_available():
        return
    with pytest.raises(RuntimeError):
        D.fit(np.zeros((4, 5), np.float32))
    with pytest.raises(RuntimeError):
        D.knn(np.zeros((4, 32), np.int16), 1)
    assert _lib.load().bl_amd_desc_knn_scratch_bytes(100000, 1, 10) == 0
