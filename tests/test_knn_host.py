"""k nearest songs (bl_amd_knn_*, bliss_amd.knn / knn_device) without a device: the Python wrappers check their
arguments before they reach the library, the constants match include/bliss_amd.h, and the C entry points have no
CPU path."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bliss_amd
from bliss_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "bliss_amd.h")).read()
    found = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (BL_AMD_KNN_\w+) (\d+)", text)}
    assert found == {"BL_AMD_KNN_DISTANCE": _lib.BL_AMD_KNN_DISTANCE, "BL_AMD_KNN_COSINE": _lib.BL_AMD_KNN_COSINE,
                     "BL_AMD_KNN_MAX_K": _lib.BL_AMD_KNN_MAX_K}
    assert (_lib.BL_AMD_KNN_DISTANCE, _lib.BL_AMD_KNN_COSINE, _lib.BL_AMD_KNN_MAX_K) == (0, 1, 128)


@pytest.mark.parametrize("fn", ["knn", "knn_device"])
@pytest.mark.parametrize("k, metric, shape", [
    (0, "distance", (10, 4)), (129, "distance", (10, 4)), (-1, "cosine", (10, 4)), (2.0, "distance", (10, 4)),
    (True, "distance", (10, 4)),
    (5, "euclidean", (10, 4)), (5, None, (10, 4)),
    (5, "distance", (10, 3)), (5, "cosine", (40,)), (5, "distance", (0, 4)), (5, "distance", (2, 5, 4)),
])
def test_wrappers_reject_bad_arguments(fn, k, metric, shape):
    v = np.zeros(shape, dtype=np.float32)
    if fn == "knn_device":
        torch = pytest.importorskip("torch")
        v = torch.zeros(shape, dtype=torch.float32)   # the checks come before anything touches a device
    with pytest.raises(ValueError):
        getattr(bliss_amd, fn)(v, k, metric=metric)


def test_wrappers_accept_the_limits_of_k():
    """k = 1 and k = 128 pass the Python checks (and then fail in the library only for want of a device)."""
    import torch
    v = np.random.default_rng(0).standard_normal((200, 4)).astype(np.float32)
    for k in (1, _lib.BL_AMD_KNN_MAX_K):
        for metric in ("distance", "cosine"):
            if torch.cuda.is_available():
                idx, val = bliss_amd.knn(v, k, metric=metric)
                assert idx.shape == val.shape == (200, k)
            else:
                with pytest.raises(RuntimeError):
                    bliss_amd.knn(v, k, metric=metric)


def test_knn_fails_loudly_without_a_device():
    """No CPU fallback: both C entry points return BL_UNEXPECTED when there is no HIP device."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    lib = bliss_amd.load()
    n, k = 16, 4
    v = (_lib.ForceVector * n)()
    idx = (C.c_int32 * (n * k))(*([7] * (n * k)))
    val = (C.c_float * (n * k))()
    for metric in (_lib.BL_AMD_KNN_DISTANCE, _lib.BL_AMD_KNN_COSINE):
        assert lib.bl_amd_knn_host(v, n, k, metric, idx, val) == _lib.BL_UNEXPECTED
        assert lib.bl_amd_knn_host(v, n, k, metric, idx, None) == _lib.BL_UNEXPECTED
        assert lib.bl_amd_knn_device(C.addressof(v), n, 0, n, k, metric, C.addressof(idx), C.addressof(val),
                                     None) == _lib.BL_UNEXPECTED
    assert list(idx) == [7] * (n * k)
