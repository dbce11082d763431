"""Radius queries and duplicate groups (bl_amd_radius_*, bl_amd_groups_*, bliss_amd.radius / radius_device /
duplicate_groups / duplicate_groups_device) without a device: the header, the symbol table and the exports agree, the
Python wrappers check their arguments before they reach the library, the C entry points have no CPU path and leave
their outputs alone when they refuse, and the bound the distance filter runs on is exact."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bliss_amd
from bliss_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX = np.finfo(np.float32).max
INF = np.float32(np.inf)


def test_constants_and_symbols_match_the_header():
    text = open(os.path.join(ROOT, "include", "bliss_amd.h")).read()
    # the metric constants are kNN's; the feature adds none of its own
    found = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (BL_AMD_RADIUS_\w+) (\d+)", text)}
    assert found == {k: getattr(_lib, k) for k in dir(_lib) if k.startswith("BL_AMD_RADIUS_")} == {}
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(bl_amd_(?:ctx_)?(?:radius|groups)_\w+)\s*\(", code))
    assert declared == {"bl_amd_radius_bound", "bl_amd_radius_count_device", "bl_amd_ctx_radius_count_device",
                        "bl_amd_radius_fill_device", "bl_amd_ctx_radius_fill_device", "bl_amd_radius_host",
                        "bl_amd_groups_device", "bl_amd_ctx_groups_device", "bl_amd_groups_host"}
    assert declared <= set(_lib.SYMBOLS)
    lib = bliss_amd.load()
    for name in declared:
        assert hasattr(lib, name)
    for name in ("radius", "radius_device", "duplicate_groups", "duplicate_groups_device"):
        assert name in bliss_amd.__all__ and callable(getattr(bliss_amd, name))


@pytest.mark.parametrize("fn", ["radius", "radius_device", "duplicate_groups", "duplicate_groups_device"])
@pytest.mark.parametrize("r, metric, shape", [
    (float("nan"), "distance", (10, 4)), (np.float32("nan"), "cosine", (10, 4)),
    ("1.0", "distance", (10, 4)), (None, "distance", (10, 4)), ([1.0], "distance", (10, 4)), (True, "cosine", (10, 4)),
    (1 + 2j, "distance", (10, 4)),
    (1.0, "euclidean", (10, 4)), (1.0, None, (10, 4)), (1.0, 0, (10, 4)),
    (1.0, "distance", (10, 3)), (1.0, "cosine", (40,)), (1.0, "distance", (0, 4)), (1.0, "distance", (2, 5, 4)),
])
def test_wrappers_reject_bad_arguments(fn, r, metric, shape):
    v = np.zeros(shape, dtype=np.float32)
    if fn.endswith("_device"):
        torch = pytest.importorskip("torch")
        v = torch.zeros(shape, dtype=torch.float32)   # the checks come before anything touches a device
    with pytest.raises(ValueError):
        getattr(bliss_amd, fn)(v, r, metric=metric)


def test_device_wrappers_reject_tensors_and_rows_they_cannot_use():
    torch = pytest.importorskip("torch")
    v = torch.zeros((10, 4), dtype=torch.float32)
    for fn in (bliss_amd.radius_device, bliss_amd.duplicate_groups_device):
        with pytest.raises(ValueError):   # a host tensor
            fn(v, 1.0)
        with pytest.raises(ValueError):   # float64 vectors
            fn(v.double(), 1.0)
        with pytest.raises(ValueError):   # not contiguous
            fn(torch.zeros((4, 10), dtype=torch.float32).t(), 1.0)


def test_wrappers_accept_every_legal_radius():
    """Well-formed calls pass the Python checks (and then fail in the library only for want of a device)."""
    import torch
    v = np.random.default_rng(0).standard_normal((50, 4)).astype(np.float32)
    for r in (0, -0.0, -3, 1, 2.5, np.float32(1e-20), np.float64(1e300), float("inf"), float("-inf"), np.int64(7)):
        for metric in ("distance", "cosine"):
            if torch.cuda.is_available():
                off, idx, val = bliss_amd.radius(v, r, metric=metric)
                assert off.dtype == np.int64 and off.shape == (51,) and off[0] == 0
                assert idx.dtype == np.int32 and val.dtype == np.float32 and idx.shape == val.shape == (off[-1],)
                g = bliss_amd.duplicate_groups(v, r, metric=metric)
                assert g.dtype == np.int32 and g.shape == (50,)
            else:
                with pytest.raises(RuntimeError):
                    bliss_amd.radius(v, r, metric=metric)
                with pytest.raises(RuntimeError):
                    bliss_amd.duplicate_groups(v, r, metric=metric)


def _outputs(n):
    off = (C.c_int64 * (n + 1))(*([7] * (n + 1)))
    idx = (C.c_int32 * (4 * n))(*([7] * (4 * n)))
    val = (C.c_float * (4 * n))(*([3.5] * (4 * n)))
    grp = (C.c_int32 * n)(*([7] * n))
    return off, idx, val, grp


def _untouched(off, idx, val, grp):
    return (all(x == 7 for x in off) and all(x == 7 for x in idx) and all(x == 3.5 for x in val)
            and all(x == 7 for x in grp))


def test_radius_and_groups_fail_loudly_without_a_device():
    """No CPU fallback: every C entry point returns BL_UNEXPECTED when there is no HIP device, outputs untouched."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    lib = bliss_amd.load()
    n = 16
    v = (_lib.ForceVector * n)()
    off, idx, val, grp = _outputs(n)
    V, O, I, F, G = (C.addressof(x) for x in (v, off, idx, val, grp))
    p_idx, p_val = C.POINTER(C.c_int32)(), C.POINTER(C.c_float)()
    for metric in (_lib.BL_AMD_KNN_DISTANCE, _lib.BL_AMD_KNN_COSINE):
        assert lib.bl_amd_radius_count_device(V, n, 0, n, metric, 1.0, O, None) == _lib.BL_UNEXPECTED
        assert lib.bl_amd_ctx_radius_count_device(None, V, n, 0, n, metric, 1.0, O, None) == _lib.BL_UNEXPECTED
        assert lib.bl_amd_radius_fill_device(V, n, 0, n, metric, 1.0, O, I, F, None) == _lib.BL_UNEXPECTED
        assert lib.bl_amd_radius_fill_device(V, n, 0, n, metric, 1.0, O, I, None, None) == _lib.BL_UNEXPECTED
        assert lib.bl_amd_ctx_radius_fill_device(None, V, n, 0, n, metric, 1.0, O, I, F, None) == _lib.BL_UNEXPECTED
        assert lib.bl_amd_radius_host(v, n, metric, 1.0, off, C.byref(p_idx), C.byref(p_val)) == _lib.BL_UNEXPECTED
        assert lib.bl_amd_radius_host(v, n, metric, 1.0, off, C.byref(p_idx), None) == _lib.BL_UNEXPECTED
        assert lib.bl_amd_groups_device(V, n, metric, 1.0, G, None) == _lib.BL_UNEXPECTED
        assert lib.bl_amd_ctx_groups_device(None, V, n, metric, 1.0, G, None) == _lib.BL_UNEXPECTED
        assert lib.bl_amd_groups_host(v, n, metric, 1.0, grp) == _lib.BL_UNEXPECTED
    assert _untouched(off, idx, val, grp) and not p_idx and not p_val


def test_entry_points_refuse_bad_arguments_with_or_without_a_device():
    """Arguments are checked before any device work: BL_UNEXPECTED and nothing written, a NaN radius included."""
    lib = bliss_amd.load()
    n = 16
    DIST, nan = _lib.BL_AMD_KNN_DISTANCE, float("nan")
    v = (_lib.ForceVector * n)()
    off, idx, val, grp = _outputs(n)
    V, O, I, F, G = (C.addressof(x) for x in (v, off, idx, val, grp))
    p_idx, p_val = C.POINTER(C.c_int32)(), C.POINTER(C.c_float)()
    rows = [(V, n, 0, n, DIST, nan), (None, n, 0, n, DIST, 1.0), (V, 0, 0, 1, DIST, 1.0), (V, -4, 0, 1, DIST, 1.0),
            (V, n, -1, 2, DIST, 1.0), (V, n, n, 1, DIST, 1.0), (V, n, 0, 0, DIST, 1.0), (V, n, 0, -5, DIST, 1.0),
            (V, n, 10, 7, DIST, 1.0), (V, n, 1, n, DIST, 1.0), (V, n, 0, n, 2, 1.0), (V, n, 0, n, -1, 1.0)]
    for a in rows:
        assert lib.bl_amd_radius_count_device(*a, O, None) == _lib.BL_UNEXPECTED, a
        assert lib.bl_amd_radius_fill_device(*a, O, I, F, None) == _lib.BL_UNEXPECTED, a
    assert lib.bl_amd_radius_count_device(V, n, 0, n, DIST, 1.0, None, None) == _lib.BL_UNEXPECTED
    assert lib.bl_amd_radius_fill_device(V, n, 0, n, DIST, 1.0, None, I, F, None) == _lib.BL_UNEXPECTED
    assert lib.bl_amd_radius_fill_device(V, n, 0, n, DIST, 1.0, O, None, F, None) == _lib.BL_UNEXPECTED
    for a in [(v, n, DIST, nan), (None, n, DIST, 1.0), (v, 0, DIST, 1.0), (v, -2, DIST, 1.0), (v, n, 2, 1.0),
              (v, n, -1, 1.0)]:
        assert lib.bl_amd_radius_host(*a, off, C.byref(p_idx), C.byref(p_val)) == _lib.BL_UNEXPECTED, a
        assert lib.bl_amd_groups_host(*a, grp) == _lib.BL_UNEXPECTED, a
        d = (V if a[0] is not None else None,) + a[1:]
        assert lib.bl_amd_groups_device(*d, G, None) == _lib.BL_UNEXPECTED, a
    assert lib.bl_amd_radius_host(v, n, DIST, 1.0, None, C.byref(p_idx), C.byref(p_val)) == _lib.BL_UNEXPECTED
    assert lib.bl_amd_radius_host(v, n, DIST, 1.0, off, None, C.byref(p_val)) == _lib.BL_UNEXPECTED
    assert lib.bl_amd_groups_host(v, n, DIST, 1.0, None) == _lib.BL_UNEXPECTED
    assert lib.bl_amd_groups_device(V, n, DIST, 1.0, None, None) == _lib.BL_UNEXPECTED
    assert _untouched(off, idx, val, grp) and not p_idx and not p_val


# ---- the bound of the distance filter -----------------------------------------------------------------------------

def root32(s):
    """the correctly rounded f32 root, as bl_amd_selftest_sqrt defines it"""
    with np.errstate(invalid="ignore"):
        return np.sqrt(s.astype(np.float64)).astype(np.float32)


def s_max(r):
    """The procedure of the contract, restated for an array of non-NaN f32 radii: start at fl(r * r), clamped to
    FLT_MAX, step down while the rounded root is above r, then up while the next one's is not."""
    r_in = np.asarray(r, dtype=np.float32)
    r = np.where(r_in < 0, np.float32(0), r_in).astype(np.float32)   # a negative radius: decided below, nothing to step
    with np.errstate(over="ignore", under="ignore"):
        s = (r * r).astype(np.float32)
    s = np.where(s <= FLT_MAX, s, FLT_MAX).astype(np.float32)
    while True:
        down = (s > 0) & (root32(s) > r)
        if not down.any():
            break
        s = np.where(down, np.nextafter(s, np.float32(0)), s).astype(np.float32)
    while True:
        with np.errstate(over="ignore"):
            nxt = np.nextafter(s, INF)
        up = (s < FLT_MAX) & (root32(nxt) <= r)
        if not up.any():
            break
        s = np.where(up, nxt, s).astype(np.float32)
    s = np.where(r_in < 0, -INF, s)
    return np.where(r_in == INF, INF, s).astype(np.float32)


def lib_bound(r):
    fn = bliss_amd.load().bl_amd_radius_bound
    return np.array([fn(float(x)) for x in np.asarray(r, dtype=np.float32)], dtype=np.float32)


def test_bound_is_the_largest_sum_whose_rounded_root_is_within_the_radius():
    """10^6 radii drawn from all finite positive bit patterns: the bound's root is within (never too large), the next
    f32's is not (maximal) — with the root's monotonicity that is the brute-force definition — and the library's
    function returns the same bits."""
    rng = np.random.default_rng(2024)
    r = rng.integers(1, 0x7F800000, 1_000_000, dtype=np.int64).astype(np.uint32).view(np.float32)
    b = s_max(r)
    assert np.all(root32(b) <= r)
    top = b == FLT_MAX
    assert np.all(root32(np.nextafter(b[~top], INF)) > r[~top])
    assert np.all(r[top] >= root32(np.float32(FLT_MAX)))
    assert np.array_equal(lib_bound(r).view(np.uint32), b.view(np.uint32))
    # the bound is not fl(r * r): it differs from it for a large share of the radii, by one ulp at most
    with np.errstate(over="ignore", under="ignore"):
        naive = (r * r).astype(np.float32)
    mid = (r > 1e-15) & (r < 1e15)
    diff = b[mid].view(np.int32).astype(np.int64) - naive[mid].view(np.int32).astype(np.int64)
    assert np.abs(diff).max() == 1 and 0.3 < np.mean(diff != 0) < 0.7


def test_bound_against_an_exhaustive_window_search():
    """the definition itself on 4 000 radii: among the 33 f32 around fl(r * r), the largest whose rounded root is
    <= r (the window always holds both a passing and a failing value)"""
    rng = np.random.default_rng(7)
    r = np.concatenate([rng.uniform(1e-3, 1e3, 2000), np.exp(rng.uniform(-40, 40, 2000))]).astype(np.float32)
    centre = (r * r).astype(np.float32).view(np.int32)
    cand = (centre[:, None] + np.arange(-16, 17, dtype=np.int32)[None, :]).view(np.float32)
    ok = root32(cand) <= r[:, None]
    assert ok[:, 0].all() and not ok[:, -1].any()
    want = cand[np.arange(len(r)), ok.sum(axis=1) - 1]
    assert np.array_equal(s_max(r).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(lib_bound(r).view(np.uint32), want.view(np.uint32))


def test_bound_at_the_edges():
    tiny = np.float32(1e-45)                            # the smallest subnormal
    big = root32(np.float32(FLT_MAX))                   # the largest finite root there is
    cases = [
        (np.float32(0), np.float32(0)), (np.float32(-0.0), np.float32(0)),          # only a zero sum is within
        (np.float32(-1.5), -INF), (-INF, -INF), (np.float32(-1e-45), -INF),         # nothing is within
        (tiny, np.float32(0)),                                                      # sqrt(1e-45) is 3.7e-23
        (np.float32(1e-20), None), (np.float32(1e-23), None),                       # r * r underflows
        (np.float32(FLT_MAX), np.float32(FLT_MAX)), (np.float32(1e30), np.float32(FLT_MAX)),   # r * r overflows
        (big, np.float32(FLT_MAX)), (np.nextafter(big, np.float32(0)), None),
        (INF, INF),                                                                 # an overflowed sum is within
        (np.float32(3), np.float32(9)), (np.nextafter(np.float32(3), INF), None),
    ]
    for r, want in cases:
        got = lib_bound([r])[0]
        assert got.view(np.uint32) == s_max([r])[0].view(np.uint32), (r, got)
        if want is not None:
            assert got.view(np.uint32) == want.view(np.uint32), (r, got, want)
        if r >= 0 and np.isfinite(r):
            assert root32(got) <= r and (got == FLT_MAX or root32(np.nextafter(got, INF)) > r)
    assert lib_bound([np.float32(0)])[0].view(np.uint32) == 0    # +0, which equals the -0 a sum can never be
    # 3 + 1 ulp: both 9 + 2^-19 and 9 + 2^-20 have that root (the rounding-tie pair of the kNN tests), 9 has not
    b = lib_bound([np.nextafter(np.float32(3), INF)])[0]
    assert b >= np.float32(9) + np.float32(2.0 ** -19) and lib_bound([np.float32(3)])[0] == np.float32(9)
    assert np.isnan(bliss_amd.load().bl_amd_radius_bound(float("nan")))
