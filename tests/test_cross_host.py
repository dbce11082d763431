"""Queries from vectors outside the library (bl_amd_cross_knn_*, bl_amd_cross_radius_*, bl_amd_playlist_vec_*,
bliss_amd.knn_cross / radius_cross / playlist_vec) without a device: the Python wrappers check their arguments before
they reach the library, the header, the bindings and the package agree on the names, and the C entry points have no
CPU path."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bliss_amd
from bliss_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = {
    "bl_amd_cross_knn_device", "bl_amd_cross_knn_host",
    "bl_amd_cross_radius_count_device", "bl_amd_ctx_cross_radius_count_device",
    "bl_amd_cross_radius_fill_device", "bl_amd_ctx_cross_radius_fill_device", "bl_amd_cross_radius_host",
    "bl_amd_playlist_vec_device", "bl_amd_playlist_vec_host",
}


def test_header_bindings_and_package_agree():
    text = open(os.path.join(ROOT, "include", "bliss_amd.h")).read()
    declared = set(re.findall(r"\bint (bl_amd_(?:(?:ctx_)?cross_|playlist_vec_)\w+)\(", text))
    assert declared == NEW_SYMBOLS
    lib = bliss_amd.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS, name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == _lib.SYMBOLS[name][1]
    # the seed of a playlist travels by value, as bl_distance takes its vectors
    assert _lib.SYMBOLS["bl_amd_playlist_vec_device"][1][2] is _lib.ForceVector
    assert _lib.SYMBOLS["bl_amd_playlist_vec_host"][1][2] is _lib.ForceVector
    for name in ("knn_cross", "knn_cross_device", "radius_cross", "radius_cross_device", "playlist_vec"):
        assert callable(getattr(bliss_amd, name)) and name in bliss_amd.__all__
    # the one semantic difference from the self forms is stated where the contract is
    assert "No candidate is ever excluded" in text and "pads from n - 1" in text


def _pair(fn, q_shape, v_shape):
    """zeros of the two shapes as the wrapper `fn` takes them: numpy arrays, or CPU tensors for the device forms
    (the checks come before anything touches a device)"""
    if fn.endswith("_device"):
        torch = pytest.importorskip("torch")
        return torch.zeros(q_shape, dtype=torch.float32), torch.zeros(v_shape, dtype=torch.float32)
    return np.zeros(q_shape, dtype=np.float32), np.zeros(v_shape, dtype=np.float32)


@pytest.mark.parametrize("fn", ["knn_cross", "knn_cross_device"])
@pytest.mark.parametrize("k, metric, q_shape, v_shape", [
    (0, "distance", (3, 4), (10, 4)), (129, "distance", (3, 4), (10, 4)), (-1, "cosine", (3, 4), (10, 4)),
    (True, "distance", (3, 4), (10, 4)), (2.0, "distance", (3, 4), (10, 4)),
    (5, "euclidean", (3, 4), (10, 4)), (5, None, (3, 4), (10, 4)),
    (5, "distance", (3, 3), (10, 4)), (5, "distance", (3, 4), (10, 3)),
    (5, "distance", (0, 4), (10, 4)), (5, "cosine", (3, 4), (0, 4)),
    (5, "distance", (4,), (10, 4)), (5, "distance", (3, 4), (2, 5, 4)),
])
def test_knn_wrappers_reject_bad_arguments(fn, k, metric, q_shape, v_shape):
    q, v = _pair(fn, q_shape, v_shape)
    with pytest.raises(ValueError):
        getattr(bliss_amd, fn)(q, v, k, metric=metric)


@pytest.mark.parametrize("fn", ["radius_cross", "radius_cross_device"])
@pytest.mark.parametrize("r, metric, q_shape, v_shape", [
    (float("nan"), "distance", (3, 4), (10, 4)), (np.float32("nan"), "cosine", (3, 4), (10, 4)),
    (True, "distance", (3, 4), (10, 4)), ("1", "distance", (3, 4), (10, 4)), (None, "cosine", (3, 4), (10, 4)),
    (1.0, "euclidean", (3, 4), (10, 4)),
    (1.0, "distance", (3, 3), (10, 4)), (1.0, "distance", (0, 4), (10, 4)), (1.0, "cosine", (3, 4), (0, 4)),
    (1.0, "distance", (3, 4), (10, 3)),
])
def test_radius_wrappers_reject_bad_arguments(fn, r, metric, q_shape, v_shape):
    q, v = _pair(fn, q_shape, v_shape)
    with pytest.raises(ValueError):
        getattr(bliss_amd, fn)(q, v, r, metric=metric)


def test_wrappers_reject_mismatched_dtypes_and_devices():
    torch = pytest.importorskip("torch")
    q32, v32 = np.zeros((3, 4), np.float32), np.zeros((10, 4), np.float32)
    for q, v in ((q32.astype(np.float64), v32), (q32, v32.astype(np.float64)), (q32.astype(np.float16), v32)):
        with pytest.raises(ValueError):
            bliss_amd.knn_cross(q, v, 2)
        with pytest.raises(ValueError):
            bliss_amd.radius_cross(q, v, 1.0)
    tq, tv = torch.zeros((3, 4)), torch.zeros((10, 4))
    elsewhere = torch.zeros((10, 4), device="meta")           # another device than the CPU tensor's, no GPU needed
    cases = [(tq.double(), tv), (tq, tv.double()), (tq.half(), tv.half()),     # dtypes
             (tq, elsewhere), (torch.zeros((3, 4), device="meta"), tv),          # devices
             (tq, tv),                                                           # the same device, but not a GPU
             (torch.zeros((3, 8))[:, ::2], tv), (tq, torch.zeros((4, 10)).t()),  # not contiguous
             (q32, v32)]                                                         # not tensors
    for q, v in cases:
        with pytest.raises(ValueError):
            bliss_amd.knn_cross_device(q, v, 2)
        with pytest.raises(ValueError):
            bliss_amd.radius_cross_device(q, v, 1.0)


@pytest.mark.parametrize("vecs, seed", [
    (np.zeros((10, 3), np.float32), np.zeros(4, np.float32)), (np.zeros((0, 4), np.float32), np.zeros(4, np.float32)),
    (np.zeros((10, 4), np.float32), np.zeros(3, np.float32)), (np.zeros((10, 4), np.float32), np.zeros((2, 4), np.float32)),
    (np.zeros((10, 4), np.float32), 3),
])
def test_playlist_vec_rejects_bad_arguments(vecs, seed):
    with pytest.raises(ValueError):
        bliss_amd.playlist_vec(vecs, seed)


def test_wrappers_accept_the_limits():
    """k = 1 and k = 128, infinite and negative radii, one query against one song pass the Python checks (and then
    fail in the library only for want of a device)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present: tests/test_gpu_cross.py runs these calls")
    q, v = np.ones((1, 4), np.float32), np.ones((1, 4), np.float32)
    for metric in ("distance", "cosine"):
        for k in (1, _lib.BL_AMD_KNN_MAX_K):
            with pytest.raises(RuntimeError):
                bliss_amd.knn_cross(q, v, k, metric=metric)
        for r in (0, -1.0, float("inf"), float("-inf"), np.float32(2.5)):
            with pytest.raises(RuntimeError):
                bliss_amd.radius_cross(q, v, r, metric=metric)
    with pytest.raises(RuntimeError):
        bliss_amd.playlist_vec(v, [1, 2, 3, 4])


def test_cross_queries_fail_loudly_without_a_device():
    """No CPU fallback: every new C entry point returns BL_UNEXPECTED when there is no HIP device, and writes nothing."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    lib = bliss_amd.load()
    n, m, k = 16, 3, 4
    v, q = (_lib.ForceVector * n)(), (_lib.ForceVector * m)()
    idx = (C.c_int32 * (m * n))(*([7] * (m * n)))
    val = (C.c_float * (m * n))(*([3.5] * (m * n)))
    off = (C.c_int64 * (m + 1))(*([9] * (m + 1)))
    V, Q, I, F, O = C.addressof(v), C.addressof(q), C.addressof(idx), C.addressof(val), C.addressof(off)
    p_index, p_value = C.POINTER(C.c_int32)(), C.POINTER(C.c_float)()
    seed = _lib.ForceVector(1, 2, 3, 4)
    ctx = C.c_void_p()
    assert lib.bl_amd_ctx_create(0, C.byref(ctx)) == _lib.BL_UNEXPECTED and not ctx.value
    U = _lib.BL_UNEXPECTED
    for metric in (_lib.BL_AMD_KNN_DISTANCE, _lib.BL_AMD_KNN_COSINE):
        assert lib.bl_amd_cross_knn_device(Q, m, V, n, k, metric, I, F, None) == U
        assert lib.bl_amd_cross_knn_host(q, m, v, n, k, metric, idx, val) == U
        assert lib.bl_amd_cross_knn_host(q, m, v, n, k, metric, idx, None) == U
        assert lib.bl_amd_cross_radius_count_device(Q, m, V, n, metric, 1.0, O, None) == U
        assert lib.bl_amd_ctx_cross_radius_count_device(None, Q, m, V, n, metric, 1.0, O, None) == U
        assert lib.bl_amd_cross_radius_fill_device(Q, m, V, n, metric, 1.0, O, I, F, None) == U
        assert lib.bl_amd_ctx_cross_radius_fill_device(None, Q, m, V, n, metric, 1.0, O, I, F, None) == U
        assert lib.bl_amd_cross_radius_host(q, m, v, n, metric, 1.0, off, C.byref(p_index), C.byref(p_value)) == U
    assert lib.bl_amd_playlist_vec_device(V, n, seed, I, F, None) == U
    assert lib.bl_amd_playlist_vec_host(v, n, seed, idx, val) == U
    assert list(idx) == [7] * (m * n) and list(val) == [3.5] * (m * n) and list(off) == [9] * (m + 1)
    assert not p_index and not p_value
