"""Chains under rules (bl_amd_mix_*, bliss_amd.mix / mix_device) without a device: the constant matches
include/bliss_amd.h, the family is the three declared names, the Python wrappers check their arguments before they
reach the library, and the C entry points have no CPU path and leave their outputs alone when they refuse."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bliss_amd
from bliss_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIST, COS = _lib.BL_AMD_KNN_DISTANCE, _lib.BL_AMD_KNN_COSINE


def test_constant_and_symbols_match_the_header():
    text = open(os.path.join(ROOT, "include", "bliss_amd.h")).read()
    found = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (BL_AMD_MIX_\w+) (\d+)", text)}
    assert found == {"BL_AMD_MIX_MAX_GAP": _lib.BL_AMD_MIX_MAX_GAP}
    assert _lib.BL_AMD_MIX_MAX_GAP == 16
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(bl_amd_(?:ctx_)?mix_\w+)\s*\(", code))
    assert declared == {"bl_amd_mix_device", "bl_amd_ctx_mix_device", "bl_amd_mix_host"}
    assert declared <= set(_lib.SYMBOLS)
    lib = bliss_amd.load()
    for name in declared:
        assert hasattr(lib, name)
    assert "mix" in bliss_amd.__all__ and "mix_device" in bliss_amd.__all__


def _vecs(fn, n=10):
    v = np.zeros((n, 4), dtype=np.float32)
    if fn == "mix_device":
        torch = pytest.importorskip("torch")
        return torch.zeros((n, 4), dtype=torch.float32), torch   # the checks come before anything touches a device
    return v, None


def _as(torch, a):
    return torch.from_numpy(np.asarray(a)) if torch is not None else np.asarray(a)


@pytest.mark.parametrize("fn", ["mix", "mix_device"])
@pytest.mark.parametrize("gap", [-1, 17, 100, 2.0, 1.5, True, False, None, "3"])
def test_wrappers_reject_a_bad_gap(fn, gap):
    v, torch = _vecs(fn)
    tags = _as(torch, np.arange(10, dtype=np.int32))
    with pytest.raises(ValueError):
        getattr(bliss_amd, fn)(v, 0, 5, tags=tags, gap=gap)


@pytest.mark.parametrize("fn", ["mix", "mix_device"])
def test_wrappers_reject_bad_tags_and_masks(fn):
    v, torch = _vecs(fn)
    call = getattr(bliss_amd, fn)
    good_tags = np.arange(10, dtype=np.int32)
    for tags in (np.arange(9, dtype=np.int32), np.arange(11, dtype=np.int32), np.zeros((10, 1), dtype=np.int32),
                 np.zeros(10, dtype=np.float32), np.zeros(10, dtype=np.float64), np.zeros(10, dtype=bool)):
        with pytest.raises(ValueError):
            call(v, 0, 5, tags=_as(torch, tags), gap=2)
    with pytest.raises(ValueError):   # a gap without tags
        call(v, 0, 5, gap=1)
    with pytest.raises(ValueError):
        call(v, 0, 5, tags=None, gap=16)
    for exclude in (np.zeros(9, dtype=bool), np.zeros(11, dtype=np.uint8), np.zeros((2, 5), dtype=bool),
                    np.zeros(10, dtype=np.float32), np.zeros(10, dtype=np.int32)):
        with pytest.raises(ValueError):
            call(v, 0, 5, tags=_as(torch, good_tags), gap=1, exclude=_as(torch, exclude))
        with pytest.raises(ValueError):
            call(v, 0, 5, exclude=_as(torch, exclude))


@pytest.mark.parametrize("fn", ["mix", "mix_device"])
def test_wrappers_want_exactly_one_kind_of_seed(fn):
    v, torch = _vecs(fn)
    call = getattr(bliss_amd, fn)
    q = _as(torch, np.zeros((2, 4), dtype=np.float32))
    with pytest.raises(ValueError):   # both
        call(v, [0, 1], 5, seed_vecs=q)
    with pytest.raises(ValueError):   # neither
        call(v, None, 5)
    for bad in (np.zeros((2, 3), dtype=np.float32), np.zeros(4, dtype=np.float32), np.zeros((0, 4), dtype=np.float32),
                np.zeros((2, 4), dtype=np.float64), np.zeros((2, 4), dtype=np.int32), np.zeros((1, 2, 4), dtype=np.float32)):
        with pytest.raises(ValueError):
            call(v, None, 5, seed_vecs=_as(torch, bad))


@pytest.mark.parametrize("fn", ["mix", "mix_device"])
@pytest.mark.parametrize("seeds, length, metric, shape", [
    (0, 0, "distance", (10, 4)), (0, -3, "cosine", (10, 4)), (0, 2.0, "distance", (10, 4)), (0, True, "distance", (10, 4)),
    (0, 5, "euclidean", (10, 4)), (0, 5, None, (10, 4)), (0, 5, "distance", (10, 3)), (0, 5, "cosine", (40,)),
    (0, 5, "distance", (0, 4)), (1.0, 5, "distance", (10, 4)), ([True, False], 5, "cosine", (10, 4)),
    ([], 5, "distance", (10, 4)), ([[0, 1], [2, 3]], 5, "distance", (10, 4)), (2 ** 40, 5, "distance", (10, 4)),
])
def test_wrappers_keep_the_chain_checks(fn, seeds, length, metric, shape):
    v = np.zeros(shape, dtype=np.float32)
    if fn == "mix_device":
        torch = pytest.importorskip("torch")
        v = torch.zeros(shape, dtype=torch.float32)
    with pytest.raises(ValueError):
        getattr(bliss_amd, fn)(v, seeds, length, metric=metric)


@pytest.mark.parametrize("seeds", [-1, 10, [0, 10], [3, -2, 4]])
def test_mix_rejects_seeds_out_of_range(seeds):
    with pytest.raises(ValueError):
        bliss_amd.mix(np.zeros((10, 4), dtype=np.float32), seeds, 3)


def test_well_formed_calls_pass_the_python_checks():
    """The Python checks let every well-formed call through to bl_amd_mix_host: none raises ValueError.  What the
    library then answers is not this test's subject (without a device it refuses, which the wrapper reports as a
    RuntimeError that names the entry point; the results on a device are tests/test_gpu_mix.py's)."""
    v = np.random.default_rng(0).standard_normal((50, 4)).astype(np.float32)
    tags = np.arange(50) // 5
    ex = np.zeros(50, dtype=bool)
    ex[3] = True
    calls = [dict(seeds=7), dict(seeds=[0, 49], tags=tags, gap=16), dict(seeds=[1], exclude=ex),
             dict(seeds=[1], exclude=ex.astype(np.uint8), tags=tags.astype(np.int64), gap=1),
             dict(seeds=None, seed_vecs=v[:3]), dict(seeds=None, seed_vecs=[[1, 2, 3, 4]], tags=tags, gap=0)]
    for kw in calls:
        kw = dict(kw)
        seeds = kw.pop("seeds")
        for metric in ("distance", "cosine"):
            try:
                bliss_amd.mix(v, seeds, 20, metric=metric, **kw)
            except RuntimeError as e:
                assert "bl_amd_mix_host" in str(e)


def _buffers(n=16, nc=3, length=5):
    v = (_lib.ForceVector * n)()
    seeds = (C.c_int32 * nc)(0, 5, 15)
    q = (_lib.ForceVector * nc)()
    tags = (C.c_int32 * n)(*range(n))
    ex = (C.c_uint8 * n)()
    order = (C.c_int32 * (nc * length))(*([7] * (nc * length)))
    value = (C.c_float * (nc * length))(*([3.5] * (nc * length)))
    return v, seeds, q, tags, ex, order, value


def test_mix_fails_loudly_without_a_device():
    """No CPU fallback: every C entry point returns BL_UNEXPECTED when there is no HIP device, outputs untouched."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    lib = bliss_amd.load()
    n, nc, length = 16, 3, 5
    v, seeds, q, tags, ex, order, value = _buffers(n, nc, length)
    A = C.addressof
    for metric in (DIST, COS):
        for s, sv in ((seeds, None), (None, q)):
            assert lib.bl_amd_mix_host(v, n, s, sv, nc, length, metric, tags, 2, ex, order, value) == _lib.BL_UNEXPECTED
            assert lib.bl_amd_mix_host(v, n, s, sv, nc, length, metric, None, 0, None, order, None) == _lib.BL_UNEXPECTED
            ds, dq = (A(s) if s else None), (A(sv) if sv else None)
            assert lib.bl_amd_mix_device(A(v), n, ds, dq, nc, length, metric, A(tags), 2, A(ex), A(order), A(value),
                                         None) == _lib.BL_UNEXPECTED
            assert lib.bl_amd_ctx_mix_device(None, A(v), n, ds, dq, nc, length, metric, A(tags), 2, A(ex), A(order),
                                             A(value), None) == _lib.BL_UNEXPECTED
    assert list(order) == [7] * (nc * length) and list(value) == [3.5] * (nc * length)


def test_c_entry_points_refuse_bad_arguments_with_or_without_a_device():
    """Arguments and index seeds are checked before any device work: BL_UNEXPECTED and nothing written."""
    lib = bliss_amd.load()
    n, nc, length = 16, 3, 5
    v, good, q, tags, ex, order, value = _buffers(n, nc, length)
    for bad in ((0, 16, 1), (-1, 2, 3), (0, 1, 2 ** 31 - 1)):
        seeds = (C.c_int32 * nc)(*bad)
        assert lib.bl_amd_mix_host(v, n, seeds, None, nc, length, DIST, tags, 1, ex, order, value) == _lib.BL_UNEXPECTED
    host_bad = [
        (None, n, good, None, nc, length, DIST, tags, 1, ex, order, value),
        (v, 0, good, None, nc, length, DIST, tags, 1, ex, order, value),
        (v, -4, good, None, nc, length, DIST, tags, 1, ex, order, value),
        (v, n, None, None, nc, length, DIST, tags, 1, ex, order, value),      # neither kind of seed
        (v, n, good, q, nc, length, DIST, tags, 1, ex, order, value),         # both
        (v, n, good, None, 0, length, DIST, tags, 1, ex, order, value),
        (v, n, good, None, -1, length, DIST, tags, 1, ex, order, value),
        (v, n, good, None, nc, 0, DIST, tags, 1, ex, order, value),
        (v, n, good, None, nc, -7, DIST, tags, 1, ex, order, value),
        (v, n, good, None, nc, length, 2, tags, 1, ex, order, value),
        (v, n, good, None, nc, length, -1, tags, 1, ex, order, value),
        (v, n, good, None, nc, length, DIST, tags, -1, ex, order, value),
        (v, n, good, None, nc, length, DIST, tags, 17, ex, order, value),
        (v, n, good, None, nc, length, DIST, None, 1, ex, order, value),      # a gap without tags
        (v, n, None, q, nc, length, COS, None, 16, None, order, value),
        (v, n, good, None, nc, length, DIST, tags, 1, ex, None, value),
    ]
    for args in host_bad:
        assert lib.bl_amd_mix_host(*args) == _lib.BL_UNEXPECTED, args
    A = C.addressof
    V, S, Q, T, X, O, F = A(v), A(good), A(q), A(tags), A(ex), A(order), A(value)
    dev_bad = [
        (None, n, S, None, nc, length, DIST, T, 1, X, O, F), (V, 0, S, None, nc, length, DIST, T, 1, X, O, F),
        (V, n, None, None, nc, length, DIST, T, 1, X, O, F), (V, n, S, Q, nc, length, DIST, T, 1, X, O, F),
        (V, n, S, None, 0, length, DIST, T, 1, X, O, F), (V, n, S, None, nc, 0, COS, T, 1, X, O, F),
        (V, n, S, None, nc, length, 7, T, 1, X, O, F), (V, n, S, None, nc, length, DIST, T, -1, X, O, F),
        (V, n, S, None, nc, length, DIST, T, 17, X, O, F), (V, n, S, None, nc, length, DIST, None, 3, X, O, F),
        (V, n, None, Q, nc, length, DIST, None, 1, None, O, F), (V, n, S, None, nc, length, DIST, T, 1, X, None, F),
        (V, n, S, None, nc, length, DIST, T, 1, X, O, None),
    ]
    for args in dev_bad:
        assert lib.bl_amd_mix_device(*args, None) == _lib.BL_UNEXPECTED, args
        assert lib.bl_amd_ctx_mix_device(None, *args, None) == _lib.BL_UNEXPECTED, args
    assert list(order) == [7] * (nc * length) and list(value) == [3.5] * (nc * length)
