"""Song-to-song chains (bl_amd_chain_*, bliss_amd.chain / chain_device) without a device: the constants match
include/bliss_amd.h, the Python wrappers check their arguments before they reach the library, and the C entry points
have no CPU path and leave their outputs alone when they refuse."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bliss_amd
from bliss_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_and_symbols_match_the_header():
    text = open(os.path.join(ROOT, "include", "bliss_amd.h")).read()
    found = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (BL_AMD_CHAIN_\w+) (\d+)", text)}
    assert found == {"BL_AMD_CHAIN_AUTO": _lib.BL_AMD_CHAIN_AUTO, "BL_AMD_CHAIN_PER_CHAIN": _lib.BL_AMD_CHAIN_PER_CHAIN,
                     "BL_AMD_CHAIN_SPLIT": _lib.BL_AMD_CHAIN_SPLIT}
    assert (_lib.BL_AMD_CHAIN_AUTO, _lib.BL_AMD_CHAIN_PER_CHAIN, _lib.BL_AMD_CHAIN_SPLIT) == (0, 1, 2)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(bl_amd_(?:ctx_)?chain_\w+)\s*\(", code))
    assert declared == {"bl_amd_chain_device", "bl_amd_ctx_chain_device", "bl_amd_chain_host", "bl_amd_chain_shape",
                        "bl_amd_chain_force_shape"}
    assert declared <= set(_lib.SYMBOLS)
    lib = bliss_amd.load()
    for name in declared:
        assert hasattr(lib, name)
    assert "chain" in bliss_amd.__all__ and "chain_device" in bliss_amd.__all__


@pytest.mark.parametrize("fn", ["chain", "chain_device"])
@pytest.mark.parametrize("seeds, length, metric, shape", [
    (0, 0, "distance", (10, 4)), (0, -3, "cosine", (10, 4)), (0, 2.0, "distance", (10, 4)), (0, True, "distance", (10, 4)),
    (0, None, "distance", (10, 4)),
    (0, 5, "euclidean", (10, 4)), (0, 5, None, (10, 4)),
    (0, 5, "distance", (10, 3)), (0, 5, "cosine", (40,)), (0, 5, "distance", (0, 4)), (0, 5, "distance", (2, 5, 4)),
    (1.0, 5, "distance", (10, 4)), ([0, 1.5], 5, "distance", (10, 4)), ([True, False], 5, "cosine", (10, 4)),
    ("3", 5, "distance", (10, 4)), ([], 5, "distance", (10, 4)), ([[0, 1], [2, 3]], 5, "distance", (10, 4)),
    (2 ** 40, 5, "distance", (10, 4)),
])
def test_wrappers_reject_bad_arguments(fn, seeds, length, metric, shape):
    v = np.zeros(shape, dtype=np.float32)
    if fn == "chain_device":
        torch = pytest.importorskip("torch")
        v = torch.zeros(shape, dtype=torch.float32)   # the checks come before anything touches a device
    with pytest.raises(ValueError):
        getattr(bliss_amd, fn)(v, seeds, length, metric=metric)


@pytest.mark.parametrize("seeds", [-1, 10, [0, 10], [3, -2, 4], np.array([0, 99], dtype=np.int64)])
def test_chain_rejects_seeds_out_of_range(seeds):
    with pytest.raises(ValueError):
        bliss_amd.chain(np.zeros((10, 4), dtype=np.float32), seeds, 3)


def test_chain_device_rejects_tensors_it_cannot_use():
    torch = pytest.importorskip("torch")
    v = torch.zeros((10, 4), dtype=torch.float32)
    with pytest.raises(ValueError):   # a host tensor of vectors
        bliss_amd.chain_device(v, [0], 3)
    with pytest.raises(ValueError):   # float64 vectors
        bliss_amd.chain_device(v.double(), [0], 3)
    with pytest.raises(ValueError):   # seeds as a tensor of the wrong type (vectors are rejected first or seeds: either)
        bliss_amd.chain_device(v, torch.zeros(2, dtype=torch.int64), 3)


def test_wrappers_accept_scalar_and_sequence_seeds():
    """Well-formed calls pass the Python checks (and then fail in the library only for want of a device)."""
    import torch
    v = np.random.default_rng(0).standard_normal((50, 4)).astype(np.float32)
    for seeds, rows in ((7, 1), (np.int64(7), 1), ([7], 1), ([0, 49, 7], 3), (np.arange(50, dtype=np.int16), 50)):
        for metric in ("distance", "cosine"):
            if torch.cuda.is_available():
                order, value = bliss_amd.chain(v, seeds, 60, metric=metric)
                assert order.shape == value.shape == (rows, 60)
                assert order.dtype == np.int32 and value.dtype == np.float32
            else:
                with pytest.raises(RuntimeError):
                    bliss_amd.chain(v, seeds, 60, metric=metric)


def test_chain_fails_loudly_without_a_device():
    """No CPU fallback: every C entry point returns BL_UNEXPECTED when there is no HIP device, outputs untouched."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    lib = bliss_amd.load()
    n, nc, length = 16, 3, 5
    v = (_lib.ForceVector * n)()
    seeds = (C.c_int32 * nc)(0, 5, 15)
    order = (C.c_int32 * (nc * length))(*([7] * (nc * length)))
    value = (C.c_float * (nc * length))(*([3.5] * (nc * length)))
    for metric in (_lib.BL_AMD_KNN_DISTANCE, _lib.BL_AMD_KNN_COSINE):
        assert lib.bl_amd_chain_host(v, n, seeds, nc, length, metric, order, value) == _lib.BL_UNEXPECTED
        assert lib.bl_amd_chain_host(v, n, seeds, nc, length, metric, order, None) == _lib.BL_UNEXPECTED
        assert lib.bl_amd_chain_device(C.addressof(v), n, C.addressof(seeds), nc, length, metric, C.addressof(order),
                                       C.addressof(value), None) == _lib.BL_UNEXPECTED
        assert lib.bl_amd_ctx_chain_device(None, C.addressof(v), n, C.addressof(seeds), nc, length, metric,
                                           C.addressof(order), C.addressof(value), None) == _lib.BL_UNEXPECTED
    assert lib.bl_amd_chain_shape(1000, 1) == _lib.BL_UNEXPECTED
    assert list(order) == [7] * (nc * length) and list(value) == [3.5] * (nc * length)


def test_chain_host_refuses_bad_arguments_and_seeds_with_or_without_a_device():
    """Arguments and seeds are checked before any device work: BL_UNEXPECTED and nothing written."""
    lib = bliss_amd.load()
    n, nc, length = 16, 3, 5
    DIST = _lib.BL_AMD_KNN_DISTANCE
    v = (_lib.ForceVector * n)()
    good = (C.c_int32 * nc)(0, 5, 15)
    order = (C.c_int32 * (nc * length))(*([7] * (nc * length)))
    value = (C.c_float * (nc * length))(*([3.5] * (nc * length)))
    for bad in ((0, 16, 1), (-1, 2, 3), (0, 1, 2 ** 31 - 1)):
        seeds = (C.c_int32 * nc)(*bad)
        assert lib.bl_amd_chain_host(v, n, seeds, nc, length, DIST, order, value) == _lib.BL_UNEXPECTED
    for args in [(None, n, good, nc, length, DIST, order, value), (v, 0, good, nc, length, DIST, order, value),
                 (v, -4, good, nc, length, DIST, order, value), (v, n, None, nc, length, DIST, order, value),
                 (v, n, good, 0, length, DIST, order, value), (v, n, good, -1, length, DIST, order, value),
                 (v, n, good, nc, 0, DIST, order, value), (v, n, good, nc, -7, DIST, order, value),
                 (v, n, good, nc, length, 2, order, value), (v, n, good, nc, length, -1, order, value),
                 (v, n, good, nc, length, DIST, None, value)]:
        assert lib.bl_amd_chain_host(*args) == _lib.BL_UNEXPECTED, args
    assert list(order) == [7] * (nc * length) and list(value) == [3.5] * (nc * length)
    # the shape hook refuses what is no shape, and what is no corpus, before it looks for a device
    assert lib.bl_amd_chain_force_shape(3) == _lib.BL_UNEXPECTED
    assert lib.bl_amd_chain_force_shape(-1) == _lib.BL_UNEXPECTED
    assert lib.bl_amd_chain_shape(0, 1) == _lib.BL_UNEXPECTED and lib.bl_amd_chain_shape(10, 0) == _lib.BL_UNEXPECTED
    assert lib.bl_amd_chain_force_shape(_lib.BL_AMD_CHAIN_AUTO) == _lib.BL_AMD_CHAIN_AUTO
