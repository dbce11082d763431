"""k nearest songs on the device (bl_amd_knn_*, bliss_amd.knn / knn_device) against the oracle's matrices and the
f32 numpy restatement of bl_distance: indices in the contract's exact order (value, then smaller index; the query
itself never listed) and values by their bits."""
import ctypes as C

import numpy as np
import pytest

import bliss_amd
from bliss_amd import _lib

pytestmark = pytest.mark.gpu

KS = (1, 10, 32, 33, 64, 65, 128)


def dist_rows(v, rows):
    """bl_distance of songs `rows` to every song: f32 sums left to right, the correctly rounded root"""
    d = v[rows][:, None, :] - v[None, :, :]
    s = d[..., 0] * d[..., 0]
    for c in (1, 2, 3):
        s = (s + d[..., c] * d[..., c]).astype(np.float32)
    with np.errstate(invalid="ignore"):
        return np.sqrt(s).astype(np.float32)


def expected(mat, rows, k, metric):
    """stable argsort of each matrix row (of -row for the cosine), the query removed, cut to k, padded"""
    n = mat.shape[1]
    order = np.argsort(-mat if metric == "cosine" else mat, axis=1, kind="stable")
    rows = np.asarray(rows)
    keep = order != rows[:, None]
    order = order[keep].reshape(len(rows), n - 1)[:, :k]
    vals = np.take_along_axis(mat, order, axis=1)
    if order.shape[1] < k:
        pad = k - order.shape[1]
        order = np.concatenate([order, np.full((len(rows), pad), -1)], axis=1)
        vals = np.concatenate([vals, np.full((len(rows), pad), np.nan, np.float32)], axis=1)
    return order.astype(np.int32), vals.astype(np.float32)


def assert_same(idx, val, want_idx, want_val, nan_bits=True):
    assert np.array_equal(idx, want_idx), np.argwhere(idx != want_idx)[:5]
    if nan_bits:
        real = want_idx >= 0
        assert np.array_equal(val.view(np.int32)[real], want_val.view(np.int32)[real])
    else:
        assert np.array_equal(np.isnan(val), np.isnan(want_val))
        ok = ~np.isnan(want_val)
        assert np.array_equal(val.view(np.int32)[ok], want_val.view(np.int32)[ok])
    assert np.all(np.isnan(val[want_idx < 0]))


def ord_key(val, idx):
    """the contract's ascending order as one unsigned 64-bit key (see bl_metric.h bl_ord); pass -value for the
    cosine"""
    u = val.view(np.uint32).copy()
    u[val == 0] = 0
    u = np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint64)
    u[np.isnan(val)] = 0xFFFFFFFF
    return (u << np.uint64(32)) | idx.astype(np.uint32).astype(np.uint64)


def mixed_set():
    """the vectors of test_cosine_matrix_bit_exact_including_degenerate_vectors: ordinary force vectors, tiny and
    huge norms, a zero vector, duplicates, sign flips, orthogonal and collinear vectors"""
    rng = np.random.default_rng(11)
    v = (rng.standard_normal((3000, 4)) * 10).astype(np.float32)
    v[100:200] *= np.float32(1e-18)
    v[200:300] *= np.float32(1e17)
    v[300] = 0
    v[301] = v[5]; v[302] = -v[5]; v[303] = v[5] * np.float32(3)
    v[304] = [1, 0, 0, 0]; v[305] = [0, 1, 0, 0]; v[306] = [0, 0, -2, 0]
    v[310:330, 1:] = 0
    return v


@pytest.mark.parametrize("metric", ["distance", "cosine"])
def test_knn_matches_the_oracle_on_mixed_scales(gpu_lib, oracle, metric):
    v = mixed_set()
    mat = oracle.distance_matrix(v) if metric == "distance" else oracle.cosine_matrix(v)
    rows = np.arange(len(v))
    for k in KS:
        idx, val = bliss_amd.knn(v, k, metric=metric)
        want_idx, want_val = expected(mat, rows, k, metric)
        assert_same(idx, val, want_idx, want_val)
    if metric == "cosine":
        assert np.isnan(val[300]).all()             # the zero vector: every cosine 0 / 0


def test_rounding_ties_go_to_the_smaller_index(gpu_lib):
    """9 + 2^-19 and 9 + 2^-20 have the same correctly rounded root, 3 + 1 ulp: the larger sum, at the smaller
    index, comes first.  Ordering by the squared sum would swap them."""
    e = np.float32(2.0 ** -10)
    v = np.array([[0, 0, 0, 0], [3, e, e, 0], [3, e, 0, 0], [5, 0, 0, 0], [3, 0, 0, 0]], dtype=np.float32)
    s = dist_rows(v, [0])[0]
    assert s[1] == s[2] == np.nextafter(np.float32(3), np.float32(4))
    for k, want in ((2, [4, 1]), (4, [4, 1, 2, 3]), (8, [4, 1, 2, 3, -1, -1, -1, -1])):
        idx, val = bliss_amd.knn(v, k)
        assert list(idx[0]) == want
        assert val[0, 1].view(np.int32) == s[1].view(np.int32)
    assert val[0, 2].view(np.int32) == s[2].view(np.int32)
    # the same pair far from the query's neighbourhood of zero: many songs, the tie pair at high indices too
    rng = np.random.default_rng(3)
    w = (rng.standard_normal((2000, 4)) * 50 + 100).astype(np.float32)
    w[0] = 0
    w[1500] = [3, e, e, 0]
    w[1700] = [3, e, 0, 0]
    idx, val = bliss_amd.knn(w, 5)
    assert list(idx[0][:2]) == [1500, 1700]


@pytest.mark.parametrize("k", [32, 128])
def test_rounding_tie_at_the_kth_slot_after_many_flushes(gpu_lib, k):
    """The same tie where the squared-sum filter decides: k - 1 songs closer than 3 spread over the corpus, then the
    pair (3 + 1 ulp both, the larger sum at the smaller index) at the k-th slot, then more songs at exactly that
    distance and a corpus of farther ones, so that the list is full, the queue has been flushed many times and the
    threshold is the pair's distance when the rest arrive.  Slot k - 1 is the pair's smaller index; with k + 1 the
    other follows.  The single query takes the column-split path, the all-rows call the other."""
    import torch
    n = 20000
    e = np.float32(2.0 ** -10)
    rng = np.random.default_rng(12)
    dirs = rng.standard_normal((n, 4)).astype(np.float32)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    v = (dirs * rng.uniform(4, 100, (n, 1))).astype(np.float32)   # farther than the pair
    v[0] = 0                                                        # the query
    closer = np.sort(rng.choice(np.arange(1, 9000), k - 1, replace=False))
    v[closer] = (dirs[closer] * rng.uniform(0.5, 2.9, (k - 1, 1))).astype(np.float32)
    v[9100] = [3, e, e, 0]     # sum 9 + 2^-19
    v[9300] = [3, e, 0, 0]     # sum 9 + 2^-20, the same rounded root
    v[[9500, 12000, 19999]] = [[3, e, 0, 0], [3, e, e, 0], [3, 0, e, e]]   # later songs at that distance
    d = dist_rows(v, [0])[0]
    t = np.nextafter(np.float32(3), np.float32(4))
    assert d[9100] == d[9300] == d[9500] == d[12000] == d[19999] == t and np.sum(d < t) == k - 1 + 1  # + the query
    want_i, want_v = expected(d[None, :], [0], min(k + 1, 128), "distance")
    assert want_i[0, k - 1] == 9100 and (k == 128 or want_i[0, k] == 9300)
    dv = torch.from_numpy(v).cuda()
    for kk in sorted({k, min(k + 1, 128)}):
        one_i, one_v = bliss_amd.knn_device(dv, kk, row_begin=0, n_rows=1)
        all_i, all_v = bliss_amd.knn(v, kk)
        assert_same(one_i.cpu().numpy(), one_v.cpu().numpy(), want_i[:, :kk], want_v[:, :kk])
        assert_same(all_i[:1], all_v[:1], want_i[:, :kk], want_v[:, :kk])


def test_duplicates_signed_zeros_infinities_and_nans(gpu_lib):
    rng = np.random.default_rng(4)
    v = (rng.standard_normal((64, 4)) * 3).astype(np.float32)
    v[10] = v[3]; v[20] = v[3]; v[30] = v[7]
    idx, val = bliss_amd.knn(v, 8)
    assert list(idx[3][:2]) == [10, 20] and val[3, 0] == 0 and val[3, 1] == 0   # the query's duplicates, by index
    assert idx[10][0] == 3 and idx[10][1] == 20
    assert_same(idx, val, *expected(dist_rows(v, np.arange(64)), np.arange(64), 8, "distance"))

    # +0 and -0 cosines tie (index decides); the bits returned are the real ones
    c = np.array([[1, 0, 0, 0], [-0.0, -1, -1, -1], [0, 1, 1, 1], [-1, 0, 0, 0], [1, 1, 0, 0]], dtype=np.float32)
    idx, val = bliss_amd.knn(c, 4, metric="cosine")
    assert list(idx[0]) == [4, 1, 2, 3]
    assert val[0, 1].view(np.uint32) == 0x80000000 and val[0, 2].view(np.uint32) == 0

    # infinite distances after every number, NaN distances after those
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    w = np.array([[0, 0, 0, 0], [nan, 0, 0, 0], [inf, 0, 0, 0], [1, 2, 3, 4], [0, 0, 0, -inf], [nan, 1, 1, 1],
                  [2, 0, 0, 0]], dtype=np.float32)
    idx, val = bliss_amd.knn(w, 6)
    assert list(idx[0]) == [6, 3, 2, 4, 1, 5]
    assert np.isinf(val[0, 2:4]).all() and np.isnan(val[0, 4:]).all()
    assert_same(idx, val, *expected(dist_rows(w, np.arange(7)), np.arange(7), 6, "distance"), nan_bits=False)


@pytest.mark.parametrize("metric", ["distance", "cosine"])
def test_short_lists_are_padded(gpu_lib, metric):
    for n in (1, 5):
        v = np.random.default_rng(n).standard_normal((n, 4)).astype(np.float32)
        idx, val = bliss_amd.knn(v, 8, metric=metric)
        assert idx.shape == (n, 8)
        assert np.all(idx[:, n - 1:] == -1) and np.isnan(val[:, n - 1:]).all()
        for r in range(n):
            assert sorted(idx[r, :n - 1]) == [j for j in range(n) if j != r]


@pytest.mark.parametrize("n", [10000, 20000])
@pytest.mark.parametrize("metric", ["distance", "cosine"])
def test_row_ranges_equal_the_full_call(gpu_lib, n, metric):
    """three uneven shards (different column splits inside) concatenated = the full call, byte for byte"""
    import torch
    v = (np.random.default_rng(5).standard_normal((n, 4)) * 8).astype(np.float32)
    d = torch.from_numpy(v).cuda()
    for k in (32, 100):
        full_i, full_v = bliss_amd.knn_device(d, k, metric=metric)
        again_i, again_v = bliss_amd.knn_device(d, k, metric=metric)
        parts = [bliss_amd.knn_device(d, k, metric=metric, row_begin=a, n_rows=b - a)
                 for a, b in ((0, 3001), (3001, 3007), (3007, n))]
        torch.cuda.synchronize()
        assert torch.equal(torch.cat([p[0] for p in parts]), full_i) and torch.equal(again_i, full_i)
        cat_v = torch.cat([p[1] for p in parts])
        assert torch.equal(cat_v.view(torch.int32), full_v.view(torch.int32))
        assert torch.equal(again_v.view(torch.int32), full_v.view(torch.int32))
    rows = np.arange(0, n, 997)
    mat = dist_rows(v, rows) if metric == "distance" else None
    if mat is not None:
        assert_same(full_i.cpu().numpy()[rows], full_v.cpu().numpy()[rows], *expected(mat, rows, 100, metric))


def check_rows_sorted(idx, val, metric, row_begin=0):
    key = ord_key(-val if metric == "cosine" else val, idx)
    assert np.all(key[:, 1:] > key[:, :-1])        # strictly: the contract's order, indices distinct
    assert not np.any(idx == (np.arange(len(idx)) + row_begin)[:, None])


@pytest.mark.parametrize("metric", ["distance", "cosine"])
def test_full_size_65536(gpu_lib, metric):
    import torch
    n, k = 65536, 32
    rng = np.random.default_rng(6)
    v = (rng.standard_normal((n, 4)) * 8).astype(np.float32)
    d = torch.from_numpy(v).cuda()
    idx, val = bliss_amd.knn_device(d, k, metric=metric)
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    check_rows_sorted(idx, val, metric)
    rows = np.sort(rng.choice(n, 256, replace=False))
    if metric == "distance":
        mat = np.concatenate([dist_rows(v, rows[i:i + 16]) for i in range(0, 256, 16)])
    else:
        out = torch.empty((1, n), dtype=torch.float32, device="cuda")
        mat = np.empty((256, n), dtype=np.float32)
        for i, r in enumerate(rows):
            assert gpu_lib.bl_amd_cosine_matrix_device(d.data_ptr(), n, int(r), 1, out.data_ptr(), None) == 0
            torch.cuda.synchronize()
            mat[i] = out.cpu().numpy()[0]
    assert_same(idx[rows], val[rows], *expected(mat, rows, k, metric))


def test_a_million_songs_one_and_64_queries(gpu_lib):
    """the column-split path: 1 and 64 queries over N = 1 048 576"""
    import torch
    n, k = 1 << 20, 32
    v = (np.random.default_rng(7).standard_normal((n, 4)) * 8).astype(np.float32)
    d = torch.from_numpy(v).cuda()
    for begin, cnt in ((123457, 1), (500000, 64)):
        idx, val = bliss_amd.knn_device(d, k, row_begin=begin, n_rows=cnt)
        idx, val = idx.cpu().numpy(), val.cpu().numpy()
        check_rows_sorted(idx, val, "distance", begin)
        rows = np.arange(begin, begin + cnt)
        for i, r in enumerate(rows):
            want_i, want_v = expected(dist_rows(v, [r]), [r], k, "distance")
            assert_same(idx[i:i + 1], val[i:i + 1], want_i, want_v)


@pytest.mark.parametrize("metric", ["distance", "cosine"])
def test_knn_device_on_a_side_stream_equals_knn(gpu_lib, metric):
    import torch
    v = (np.random.default_rng(8).standard_normal((5000, 4)) * 8).astype(np.float32)
    want_i, want_v = bliss_amd.knn(v, 40, metric=metric)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d = torch.from_numpy(v).cuda()
        idx, val = bliss_amd.knn_device(d, 40, metric=metric, stream=s)
    s.synchronize()
    assert np.array_equal(idx.cpu().numpy(), want_i)
    assert np.array_equal(val.cpu().numpy().view(np.int32), want_v.view(np.int32))


def test_argument_errors_leave_the_outputs_untouched(gpu_lib):
    import torch
    n, k = 100, 8
    d = torch.randn((n, 4), dtype=torch.float32, device="cuda")
    oi = torch.full((n, 2 * k), 7, dtype=torch.int32, device="cuda")
    ov = torch.full((n, 2 * k), 3.5, dtype=torch.float32, device="cuda")
    V, I, F = d.data_ptr(), oi.data_ptr(), ov.data_ptr()
    DIST, COS = _lib.BL_AMD_KNN_DISTANCE, _lib.BL_AMD_KNN_COSINE
    bad = [
        (V, n, 0, n, 0, DIST, I, F), (V, n, 0, n, 129, DIST, I, F), (V, n, 0, n, -3, COS, I, F),
        (V, n, 0, n, k, 2, I, F), (V, n, 0, n, k, -1, I, F),
        (V, n, -1, 2, k, DIST, I, F), (V, n, n, 1, k, DIST, I, F), (V, n, 0, 0, k, DIST, I, F),
        (V, n, 0, -5, k, DIST, I, F), (V, n, 90, 11, k, COS, I, F), (V, n, 1, n, k, DIST, I, F),
        (V, 0, 0, 1, k, DIST, I, F), (V, -4, 0, 1, k, DIST, I, F),
        (None, n, 0, n, k, DIST, I, F), (V, n, 0, n, k, DIST, None, F), (V, n, 0, n, k, COS, I, None),
    ]
    for args in bad:
        assert gpu_lib.bl_amd_knn_device(*args, None) == _lib.BL_UNEXPECTED, args
    torch.cuda.synchronize()
    assert torch.all(oi == 7) and torch.all(ov == 3.5)
    hv = np.random.default_rng(9).standard_normal((n, 4)).astype(np.float32)
    hp = hv.ctypes.data_as(C.POINTER(_lib.ForceVector))
    hi = np.full(n * 2 * k, 7, dtype=np.int32)
    hf = np.full(n * 2 * k, 3.5, dtype=np.float32)
    ip, fp = hi.ctypes.data_as(C.POINTER(C.c_int32)), hf.ctypes.data_as(C.POINTER(C.c_float))
    for args in [(hp, n, 0, DIST, ip, fp), (hp, n, 129, COS, ip, fp), (hp, n, k, 5, ip, fp), (hp, 0, k, DIST, ip, fp),
                 (None, n, k, DIST, ip, fp), (hp, n, k, DIST, None, fp)]:
        assert gpu_lib.bl_amd_knn_host(*args) == _lib.BL_UNEXPECTED, args
    assert np.all(hi == 7) and np.all(hf == 3.5)
    # h_value may be NULL
    assert gpu_lib.bl_amd_knn_host(hp, n, k, DIST, ip, None) == _lib.BL_OK
    assert np.array_equal(hi[:n * k].reshape(n, k), bliss_amd.knn(hv, k)[0])
