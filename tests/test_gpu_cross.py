"""Queries from vectors outside the library on the device (bl_amd_cross_knn_*, bl_amd_cross_radius_*,
bl_amd_playlist_vec_*) against the cross matrix X[q][j] = metric(queries[q], vecs[j]): rows n.. and columns :n of the
oracle's matrix of the concatenation vecs || queries, the f32 numpy restatement of bl_distance for larger sets, and for
the cosine of a larger set the rows bl_amd_cosine_matrix_device writes for that concatenation, which is how the
contract defines X.  Everything is exact: indices as integers, values by their bits, NaN as NaN.  No candidate is
ever excluded: that is the difference from tests/test_gpu_knn.py and tests/test_gpu_radius.py."""
import ctypes as C

import numpy as np
import pytest

import bliss_amd
from bliss_amd import _lib

pytestmark = pytest.mark.gpu

METRICS = ("distance", "cosine")


def dist_cross(q, v):
    """bl_distance of every query to every song, the query the first operand: f32 sums left to right, the correctly
    rounded root (the restatement tests/test_gpu_knn.py calls dist_rows, with the queries an array of their own)"""
    with np.errstate(invalid="ignore", over="ignore"):
        d = q[:, None, :] - v[None, :, :]
        s = d[..., 0] * d[..., 0]
        for c in (1, 2, 3):
            s = (s + d[..., c] * d[..., c]).astype(np.float32)
        return np.sqrt(s).astype(np.float32)


def mixed_set():
    """the vectors of tests/test_gpu_knn.py: ordinary force vectors, tiny and huge norms, a zero vector, duplicates,
    sign flips, orthogonal and collinear vectors"""
    rng = np.random.default_rng(11)
    v = (rng.standard_normal((3000, 4)) * 10).astype(np.float32)
    v[100:200] *= np.float32(1e-18)
    v[200:300] *= np.float32(1e17)
    v[300] = 0
    v[301] = v[5]; v[302] = -v[5]; v[303] = v[5] * np.float32(3)
    v[304] = [1, 0, 0, 0]; v[305] = [0, 1, 0, 0]; v[306] = [0, 0, -2, 0]
    v[310:330, 1:] = 0
    return v


def oracle_cross(oracle, q, v, metric):
    cat = np.concatenate([v, q])
    mat = oracle.distance_matrix(cat) if metric == "distance" else oracle.cosine_matrix(cat)
    return np.ascontiguousarray(mat[len(v):, :len(v)])


def device_cosine_cross(gpu_lib, q, v):
    """X for the cosine as the contract defines it: rows n.. of bl_amd_cosine_matrix_device over vecs || queries"""
    import torch
    n, m = len(v), len(q)
    cat = torch.from_numpy(np.concatenate([v, q])).cuda()
    out = torch.empty((m, n + m), dtype=torch.float32, device="cuda")
    assert gpu_lib.bl_amd_cosine_matrix_device(cat.data_ptr(), n + m, n, m, out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    return np.ascontiguousarray(out.cpu().numpy()[:, :n])


def expected_knn(X, k, metric):
    """stable argsort of each row of X (of -row for the cosine), nothing removed, cut to k, padded from n"""
    m, n = X.shape
    order = np.argsort(-X if metric == "cosine" else X, axis=1, kind="stable")[:, :k]
    vals = np.take_along_axis(X, order, axis=1)
    if n < k:
        order = np.concatenate([order, np.full((m, k - n), -1)], axis=1)
        vals = np.concatenate([vals, np.full((m, k - n), np.nan, np.float32)], axis=1)
    return order.astype(np.int32), vals.astype(np.float32)


def assert_same(idx, val, want_idx, want_val):
    assert idx.shape == want_idx.shape and val.shape == want_val.shape
    assert np.array_equal(idx, want_idx), np.argwhere(idx != want_idx)[:5]
    assert np.array_equal(np.isnan(val), np.isnan(want_val))
    ok = ~np.isnan(want_val)
    assert np.array_equal(val.view(np.int32)[ok], want_val.view(np.int32)[ok])


def knn_dev(dq, dv, k, metric="distance", stream=None):
    import torch
    idx, val = bliss_amd.knn_cross_device(dq, dv, k, metric=metric, stream=stream)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), val.cpu().numpy()


# ---------------------------------------------------------------------------- kNN

QUERY_COUNTS = (1, 3, 4, 5, 16, 17)     # the edges of KNN_QPW x KNN_WAVES
KS = (1, 64, 65, 128)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 3000])
def test_knn_shapes_against_the_oracle(gpu_lib, oracle, n, metric):
    import torch
    rng = np.random.default_rng(100 + n)
    v = (rng.standard_normal((n, 4)) * 8).astype(np.float32)
    q = (rng.standard_normal((max(QUERY_COUNTS), 4)) * 8).astype(np.float32)
    q[2] = v[n // 2]                                    # one query is a song of the library
    X = oracle_cross(oracle, q, v, metric)              # once: query q's row does not depend on the other queries
    dv, dq = torch.from_numpy(v).cuda(), torch.from_numpy(q).cuda()
    for m in QUERY_COUNTS:
        for k in KS:
            idx, val = knn_dev(dq[:m], dv, k, metric)
            assert_same(idx, val, *expected_knn(X[:m], k, metric))
    if n < 128:
        assert np.all(idx[:, n:] == -1) and np.all(idx[:, :n] >= 0)      # padded from slot n, not n - 1


@pytest.mark.parametrize("metric", METRICS)
def test_more_queries_than_songs(gpu_lib, oracle, metric):
    rng = np.random.default_rng(21)
    v = (rng.standard_normal((7, 4)) * 5).astype(np.float32)
    q = (rng.standard_normal((300, 4)) * 5).astype(np.float32)
    q[::50] = v[3]
    X = oracle_cross(oracle, q, v, metric)
    for k in (7, 8, 16, 128):
        idx, val = bliss_amd.knn_cross(q, v, k, metric=metric)
        assert_same(idx, val, *expected_knn(X, k, metric))
        assert np.all(idx[:, 7:] == -1) and np.isnan(val[:, 7:]).all()
        assert np.all(np.sort(idx[:, :7], axis=1) == np.arange(7))


@pytest.mark.parametrize("metric", METRICS)
def test_knn_matches_the_oracle_on_mixed_scales(gpu_lib, oracle, metric):
    import torch
    v = mixed_set()
    rng = np.random.default_rng(22)
    # tiny, huge, the zero vector, collinear, sign-flipped, axis and low-rank rows of the library, then new vectors
    drawn = v[[100, 150, 200, 250, 300, 303, 302, 304, 306, 315, 5]]
    fresh = (rng.standard_normal((6, 4)) * 10).astype(np.float32)
    fresh[1] *= np.float32(1e-18); fresh[2] *= np.float32(1e17)
    q = np.concatenate([drawn, fresh])
    X = oracle_cross(oracle, q, v, metric)
    dv, dq = torch.from_numpy(v).cuda(), torch.from_numpy(q).cuda()
    for k in KS:
        idx, val = knn_dev(dq, dv, k, metric)
        assert_same(idx, val, *expected_knn(X, k, metric))
    if metric == "cosine":
        assert np.isnan(val[4]).all() and list(idx[4]) == list(range(128))   # the zero query: every cosine 0 / 0
    else:
        assert idx[4, 0] == 300 and val[4, 0] == 0                           # ... and at distance 0 from song 300


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("m", [1, 5])
def test_column_split_path(gpu_lib, m, metric):
    """n = 8 229: twice KNN_SPLIT_MIN_COLS and more, no multiple of 64, few queries: the columns are split and merged"""
    import torch
    n = 8229
    rng = np.random.default_rng(23)
    v = (rng.standard_normal((n, 4)) * 8).astype(np.float32)
    v[4200] = v[17]; v[8228] = v[17]                    # duplicates on both sides of the split, one in the last column
    q = (rng.standard_normal((m, 4)) * 8).astype(np.float32)
    q[0] = v[17]
    X = dist_cross(q, v) if metric == "distance" else device_cosine_cross(gpu_lib, q, v)
    dv, dq = torch.from_numpy(v).cuda(), torch.from_numpy(q).cuda()
    for k in (1, 32, 64, 65, 128):
        idx, val = knn_dev(dq, dv, k, metric)
        assert_same(idx, val, *expected_knn(X, k, metric))
    assert list(idx[0, :3]) == [17, 4200, 8228]


@pytest.mark.parametrize("k", [32, 128])
def test_rounding_tie_at_the_kth_slot_after_many_flushes(gpu_lib, k):
    """The tie of tests/test_gpu_knn.py with the query outside the library: k - 1 songs closer than 3 spread over the
    corpus, then a pair at 3 + 1 ulp (the larger squared sum at the smaller index) at the k-th slot, more songs at that
    distance and a corpus of farther ones.  Slot k - 1 is the pair's smaller index; with k + 1 the other follows.
    One query over 20 000 songs takes the column-split path; 16 384 copies of it are 4 096 query waves, 16 for each of
    256 compute units, which is where blk_split_plan stops splitting."""
    import torch
    n = 20000
    e = np.float32(2.0 ** -10)
    rng = np.random.default_rng(12)
    dirs = rng.standard_normal((n, 4)).astype(np.float32)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    v = (dirs * rng.uniform(4, 100, (n, 1))).astype(np.float32)   # farther than the pair
    closer = np.sort(rng.choice(np.arange(0, 9000), k - 1, replace=False))
    v[closer] = (dirs[closer] * rng.uniform(0.5, 2.9, (k - 1, 1))).astype(np.float32)
    v[9100] = [3, e, e, 0]     # sum 9 + 2^-19
    v[9300] = [3, e, 0, 0]     # sum 9 + 2^-20, the same rounded root
    v[[9500, 12000, 19999]] = [[3, e, 0, 0], [3, e, e, 0], [3, 0, e, e]]   # later songs at that distance
    q = np.zeros((1, 4), dtype=np.float32)                         # the query: no song of the library
    X = dist_cross(q, v)
    t = np.nextafter(np.float32(3), np.float32(4))
    d = X[0]
    assert d[9100] == d[9300] == d[9500] == d[12000] == d[19999] == t and np.sum(d < t) == k - 1
    kmax = min(k + 1, 128)
    want_i, want_v = expected_knn(X, kmax, "distance")
    assert want_i[0, k - 1] == 9100 and (k == 128 or want_i[0, k] == 9300)
    dv = torch.from_numpy(v).cuda()
    one = torch.from_numpy(q).cuda()
    many = one.repeat(16384, 1)
    for kk in sorted({k, kmax}):
        assert_same(*knn_dev(one, dv, kk), want_i[:, :kk], want_v[:, :kk])
        mi, mv = knn_dev(many, dv, kk)
        assert_same(mi[[0, 8191, 16383]], mv[[0, 8191, 16383]], np.repeat(want_i[:, :kk], 3, 0),
                    np.repeat(want_v[:, :kk], 3, 0))
        assert np.all(mi == mi[0]) and np.all(mv.view(np.int32) == mv.view(np.int32)[0])


def test_a_query_that_is_in_the_library_lists_itself(gpu_lib):
    rng = np.random.default_rng(4)
    v = (rng.standard_normal((64, 4)) * 3).astype(np.float32)
    v[10] = v[3]; v[20] = v[3]
    q = v[[3, 7]].copy()
    for metric in METRICS:
        idx, val = bliss_amd.knn_cross(q, v, 8, metric=metric)
        assert list(idx[0][:3]) == [3, 10, 20] and idx[1][0] == 7
    idx, val = bliss_amd.knn_cross(q, v, 8)
    assert np.all(val[0, :3] == 0) and val[1, 0] == 0 and val[0, 3] > 0
    assert_same(idx, val, *expected_knn(dist_cross(q, v), 8, "distance"))


@pytest.mark.parametrize("metric", METRICS)
def test_cross_minus_the_query_is_the_self_form(gpu_lib, metric):
    """the library's own rows as queries (the library tensor itself): the k + 1 nearest with the row itself taken out,
    cut to k, are the self form's k nearest, byte for byte.  Row 40 has a NaN component, so its own value is NaN too
    and it comes 41st among its equals; rows 7, 41 and 200 are one vector, so a row need not be its own first."""
    import torch
    n = 300
    v = (np.random.default_rng(24).standard_normal((n, 4)) * 6).astype(np.float32)
    v[41] = v[7]; v[200] = v[7]
    v[40, 2] = np.nan
    dv = torch.from_numpy(v).cuda()
    rows = np.arange(n)
    for k in (1, 31, 64, 127):
        ci, cv = knn_dev(dv, dv, k + 1, metric)
        si, sv = bliss_amd.knn_device(dv, k, metric=metric)
        si, sv = si.cpu().numpy(), sv.cpu().numpy()
        assert np.all(np.sum(ci == rows[:, None], axis=1) <= 1)
        got_i = np.stack([ci[r][ci[r] != r][:k] for r in rows])
        got_v = np.stack([cv[r].view(np.int32)[ci[r] != r][:k] for r in rows])
        assert np.array_equal(got_i, si) and np.array_equal(got_v, sv.view(np.int32))
    assert np.isnan(cv[40]).all()


@pytest.mark.parametrize("metric", METRICS)
def test_queries_are_independent_and_need_16_byte_alignment_only(gpu_lib, metric):
    import torch
    rng = np.random.default_rng(25)
    v = (rng.standard_normal((5000, 4)) * 8).astype(np.float32)
    m = 11
    dv = torch.from_numpy(v).cuda()
    base = torch.from_numpy((rng.standard_normal((m + 2, 4)) * 8).astype(np.float32)).cuda()
    dq = base[2:]                                         # 32 bytes into an allocation
    for k in (5, 100):
        full_i, full_v = knn_dev(dq, dv, k, metric)
        parts = []
        for a, b in ((0, 3), (3, 4), (4, m)):
            part = dq[a:b]
            assert part.data_ptr() % 16 == 0 and part.data_ptr() % 64 != 0 and part.is_contiguous()
            parts.append(knn_dev(part, dv, k, metric))
        assert np.array_equal(np.concatenate([p[0] for p in parts]), full_i)
        assert np.array_equal(np.concatenate([p[1] for p in parts]).view(np.int32), full_v.view(np.int32))
    # queries that are a view into the library tensor itself
    view_i, view_v = knn_dev(dv[100:117], dv, 20, metric)
    copy_i, copy_v = knn_dev(dv[100:117].clone(), dv, 20, metric)
    assert np.array_equal(view_i, copy_i) and np.array_equal(view_v.view(np.int32), copy_v.view(np.int32))
    if metric == "distance":
        assert np.array_equal(view_i[:, 0], np.arange(100, 117)) and np.all(view_v[:, 0] == 0)
        assert_same(view_i, view_v, *expected_knn(dist_cross(v[100:117], v), 20, metric))


@pytest.mark.parametrize("metric", METRICS)
def test_knn_cross_device_on_a_side_stream_equals_the_default_stream(gpu_lib, metric):
    import torch
    rng = np.random.default_rng(8)
    v = (rng.standard_normal((5000, 4)) * 8).astype(np.float32)
    q = (rng.standard_normal((37, 4)) * 8).astype(np.float32)
    want_i, want_v = knn_dev(torch.from_numpy(q).cuda(), torch.from_numpy(v).cuda(), 40, metric)
    host_i, host_v = bliss_amd.knn_cross(q, v, 40, metric=metric)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dv, dq = torch.from_numpy(v).cuda(), torch.from_numpy(q).cuda()
        idx, val = bliss_amd.knn_cross_device(dq, dv, 40, metric=metric, stream=s)
    s.synchronize()
    for i, f in ((idx.cpu().numpy(), val.cpu().numpy()), (host_i, host_v)):
        assert np.array_equal(i, want_i) and np.array_equal(f.view(np.int32), want_v.view(np.int32))


def test_signed_zeros_infinities_and_nans(gpu_lib):
    # +0 and -0 cosines tie (index decides); the bits returned are the real ones
    q = np.array([[1, 0, 0, 0]], dtype=np.float32)
    c = np.array([[-0.0, -1, -1, -1], [0, 1, 1, 1], [-1, 0, 0, 0], [1, 1, 0, 0]], dtype=np.float32)
    idx, val = bliss_amd.knn_cross(q, c, 4, metric="cosine")
    assert list(idx[0]) == [3, 0, 1, 2]
    assert val[0, 1].view(np.uint32) == 0x80000000 and val[0, 2].view(np.uint32) == 0

    # infinite distances after every number, NaN distances after those
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    z = np.zeros((1, 4), dtype=np.float32)
    w = np.array([[nan, 0, 0, 0], [inf, 0, 0, 0], [1, 2, 3, 4], [0, 0, 0, -inf], [nan, 1, 1, 1], [2, 0, 0, 0]],
                 dtype=np.float32)
    idx, val = bliss_amd.knn_cross(z, w, 8)
    assert list(idx[0]) == [5, 2, 1, 3, 0, 4, -1, -1]
    assert np.isinf(val[0, 2:4]).all() and np.isnan(val[0, 4:]).all()
    assert_same(idx, val, *expected_knn(dist_cross(z, w), 8, "distance"))

    # a zero-vector query under the cosine: every value NaN, so the songs come by index
    idx, val = bliss_amd.knn_cross(z, w, 3, metric="cosine")
    assert list(idx[0]) == [0, 1, 2] and np.isnan(val).all()
    # a NaN query: the same for the distance
    idx, val = bliss_amd.knn_cross(np.array([[nan, 1, 2, 3]], dtype=np.float32), w, 6)
    assert list(idx[0]) == [0, 1, 2, 3, 4, 5] and np.isnan(val).all()


# ---------------------------------------------------------------------------- radius

def expected_radius(X, r, metric):
    within = (X >= np.float32(r)) if metric == "cosine" else (X <= np.float32(r))    # a NaN entry is never within
    counts = within.sum(axis=1)
    offsets = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)]).astype(np.int64)
    rows, cols = np.nonzero(within)                                                   # row-major: ascending songs
    return offsets, cols.astype(np.int32), X[rows, cols]


def assert_same_csr(got, want):
    assert got[0].dtype == np.int64 and np.array_equal(got[0], want[0])
    assert got[1].dtype == np.int32 and np.array_equal(got[1], want[1])
    if got[2] is not None:
        assert got[2].shape == want[2].shape
        assert np.array_equal(got[2].view(np.int32), want[2].view(np.int32))          # a listed entry is never NaN


def radius_dev(dq, dv, r, metric, values=True):
    out = bliss_amd.radius_cross_device(dq, dv, r, metric=metric, values=values)
    return tuple(None if t is None else t.cpu().numpy() for t in out)


RADIUS_QUERY_COUNTS = (1, 7, 8, 9, 32, 33)     # the edges of RAD_QPW x RAD_WAVES


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", [1, 65, 2053])
def test_radius_shapes_and_radii_against_the_oracle(gpu_lib, oracle, n, metric):
    """n = 2 053 is twice RAD_SPLIT_MIN_COLS and more, no multiple of 64: with these few queries the columns are split"""
    import torch
    rng = np.random.default_rng(200 + n)
    v = (rng.standard_normal((n, 4)) * 4).astype(np.float32)
    q = (rng.standard_normal((max(RADIUS_QUERY_COUNTS), 4)) * 4).astype(np.float32)
    q[0] = v[n // 3]                                   # in the library: radius 0 finds it
    q[8] = v[n - 1]                                    # ... and one in the last column
    if n > 1:
        v[n // 2] = 0                                  # a zero song: its cosines are NaN, never within
        q[5] = 0                                       # a zero query: an empty cosine row, whatever the radius
    X = oracle_cross(oracle, q, v, metric)
    dv, dq = torch.from_numpy(v).cuda(), torch.from_numpy(q).cuda()
    finite = X[np.isfinite(X)]
    mid = float(np.median(finite))
    for m in RADIUS_QUERY_COUNTS:
        for r in (mid, 0.0, -1.0, float("inf"), float("-inf")):
            want = expected_radius(X[:m], r, metric)
            got = radius_dev(dq[:m], dv, r, metric)
            assert_same_csr(got, want)
            if m in (1, 33):
                assert_same_csr(radius_dev(dq[:m], dv, r, metric, values=False), want)     # d_value = NULL
                assert_same_csr(bliss_amd.radius_cross(q[:m], v, r, metric=metric), want)  # the host form
    if metric == "distance":
        off, idx, val = radius_dev(dq, dv, 0.0, metric)
        assert idx[off[0]:off[1]].tolist() == [n // 3] and val[off[0]] == 0    # the self form would not list it
        assert n - 1 in idx[off[8]:off[9]]
        assert radius_dev(dq, dv, -1.0, metric)[0].tolist() == [0] * (len(q) + 1)
    elif n > 1:
        off = radius_dev(dq, dv, float("-inf"), metric)[0]
        assert off[6] == off[5]                                                 # the zero query lists nothing
        assert off[1] - off[0] == n - 1                                         # every song but the zero one


def test_an_empty_total_is_a_valid_result(gpu_lib):
    import torch
    rng = np.random.default_rng(31)
    v = (rng.standard_normal((100, 4)) + 50).astype(np.float32)
    q = rng.standard_normal((5, 4)).astype(np.float32)
    for metric, r in (("distance", 1.0), ("distance", -0.5), ("cosine", float("inf"))):
        for got in (bliss_amd.radius_cross(q, v, r, metric=metric),
                    radius_dev(torch.from_numpy(q).cuda(), torch.from_numpy(v).cuda(), r, metric)):
            assert got[0].tolist() == [0] * 6 and got[0].dtype == np.int64
            assert got[1].shape == (0,) and got[2].shape == (0,)
    # the C host form hands out free()-able blocks for it
    p_index, p_value = C.POINTER(C.c_int32)(), C.POINTER(C.c_float)()
    off = np.full(6, 9, dtype=np.int64)
    fv = C.POINTER(_lib.ForceVector)
    assert gpu_lib.bl_amd_cross_radius_host(q.ctypes.data_as(fv), 5, v.ctypes.data_as(fv), 100, _lib.BL_AMD_KNN_DISTANCE,
                                            1.0, off.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(p_index),
                                            C.byref(p_value)) == _lib.BL_OK
    assert off.tolist() == [0] * 6 and p_index and p_value
    libc = C.CDLL(None)
    libc.free(C.cast(p_index, C.c_void_p))
    libc.free(C.cast(p_value, C.c_void_p))


def test_radius_through_an_explicit_context_and_a_dense_result(gpu_lib):
    """bl_amd_ctx_cross_radius_*: the same lists through a context of the caller's; +inf lists every song of every
    row, so the offsets are the multiples of n"""
    import torch
    rng = np.random.default_rng(32)
    n, m = 3001, 40
    v = (rng.standard_normal((n, 4)) * 4).astype(np.float32)
    q = (rng.standard_normal((m, 4)) * 4).astype(np.float32)
    dv, dq = torch.from_numpy(v).cuda(), torch.from_numpy(q).cuda()
    want = radius_dev(dq, dv, float("inf"), "distance")
    assert want[0].tolist() == [n * i for i in range(m + 1)] and np.array_equal(want[1], np.tile(np.arange(n), m))
    assert np.array_equal(want[2].view(np.int32), dist_cross(q, v).reshape(-1).view(np.int32))
    ctx = C.c_void_p()
    assert gpu_lib.bl_amd_ctx_create(0, C.byref(ctx)) == _lib.BL_OK
    try:
        off = torch.empty(m + 1, dtype=torch.int64, device="cuda")
        idx = torch.empty(n * m, dtype=torch.int32, device="cuda")
        val = torch.empty(n * m, dtype=torch.float32, device="cuda")
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        args = (ctx, dq.data_ptr(), m, dv.data_ptr(), n, _lib.BL_AMD_KNN_DISTANCE, float("inf"), off.data_ptr())
        assert gpu_lib.bl_amd_ctx_cross_radius_count_device(*args, s) == _lib.BL_OK
        assert gpu_lib.bl_amd_ctx_cross_radius_fill_device(*args, idx.data_ptr(), val.data_ptr(), s) == _lib.BL_OK
        torch.cuda.synchronize()
        assert_same_csr((off.cpu().numpy(), idx.cpu().numpy(), val.cpu().numpy()), want)
    finally:
        gpu_lib.bl_amd_ctx_destroy(ctx)


# ---------------------------------------------------------------------------- playlist

def test_playlist_vec_of_a_song_equals_playlist(gpu_lib):
    rng = np.random.default_rng(41)
    v = (rng.standard_normal((1500, 4)) * 8).astype(np.float32)
    v[700] = v[3]; v[1499] = v[3]
    for s in (0, 3, 1499):
        want_o, want_d = bliss_amd.playlist(v, s)
        got_o, got_d = bliss_amd.playlist_vec(v, v[s])
        assert np.array_equal(got_o, want_o) and np.array_equal(got_d.view(np.int32), want_d.view(np.int32))
    assert list(bliss_amd.playlist_vec(v, v[3])[0][:3]) == [3, 700, 1499]


def test_playlist_vec_of_a_seed_outside_the_library(gpu_lib):
    e = np.float32(2.0 ** -10)
    rng = np.random.default_rng(42)
    v = (rng.standard_normal((777, 4)) * 8 + 20).astype(np.float32)
    v[600] = [3, e, e, 0]; v[20] = [3, e, 0, 0]          # the same rounded root from two sums: an exact tie
    v[5] = v[300]; v[776] = v[300]                       # exact duplicates
    seed = np.zeros(4, dtype=np.float32)
    d = dist_cross(seed[None, :], v)[0]
    assert d[600] == d[20]
    order, dist = bliss_amd.playlist_vec(v, seed)
    assert np.array_equal(dist.view(np.int32), d.view(np.int32))
    assert np.array_equal(order, np.argsort(d, kind="stable").astype(np.int32))
    assert list(order[:2]) == [20, 600]
    one_o, one_d = bliss_amd.playlist_vec(v[:1], [1.5, -2, 0, 7])     # a list as the seed, a library of one
    assert list(one_o) == [0] and one_d.view(np.int32)[0] == dist_cross(np.float32([[1.5, -2, 0, 7]]), v[:1]).view(np.int32)[0, 0]


# ---------------------------------------------------------------------------- argument errors

def test_argument_errors_leave_the_outputs_untouched(gpu_lib):
    import torch
    n, m, k = 100, 6, 8
    d = torch.randn((n, 4), dtype=torch.float32, device="cuda")
    dq = torch.randn((m, 4), dtype=torch.float32, device="cuda")
    oi = torch.full((m, n), 7, dtype=torch.int32, device="cuda")
    ov = torch.full((m, n), 3.5, dtype=torch.float32, device="cuda")
    oo = torch.full((m + 1,), 9, dtype=torch.int64, device="cuda")
    order = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    dist = torch.full((n,), 3.5, dtype=torch.float32, device="cuda")
    V, Q, I, F, O = d.data_ptr(), dq.data_ptr(), oi.data_ptr(), ov.data_ptr(), oo.data_ptr()
    DIST, COS = _lib.BL_AMD_KNN_DISTANCE, _lib.BL_AMD_KNN_COSINE
    nan = float("nan")
    U = _lib.BL_UNEXPECTED
    for args in [(None, m, V, n, k, DIST, I, F), (Q, m, None, n, k, DIST, I, F), (Q, m, V, n, k, DIST, None, F),
                 (Q, m, V, n, k, COS, I, None), (Q, 0, V, n, k, DIST, I, F), (Q, -2, V, n, k, DIST, I, F),
                 (Q, m, V, 0, k, DIST, I, F), (Q, m, V, -1, k, COS, I, F), (Q, m, V, n, 0, DIST, I, F),
                 (Q, m, V, n, 129, DIST, I, F), (Q, m, V, n, -3, COS, I, F), (Q, m, V, n, k, 2, I, F),
                 (Q, m, V, n, k, -1, I, F)]:
        assert gpu_lib.bl_amd_cross_knn_device(*args, None) == U, args
    ctx = C.c_void_p()
    assert gpu_lib.bl_amd_ctx_create(0, C.byref(ctx)) == _lib.BL_OK
    try:
        for args in [(None, m, V, n, DIST, 1.0, O), (Q, m, None, n, DIST, 1.0, O), (Q, m, V, n, DIST, 1.0, None),
                     (Q, 0, V, n, DIST, 1.0, O), (Q, -1, V, n, COS, 0.5, O), (Q, m, V, 0, DIST, 1.0, O),
                     (Q, m, V, -7, DIST, 1.0, O), (Q, m, V, n, 2, 1.0, O), (Q, m, V, n, -1, 1.0, O),
                     (Q, m, V, n, DIST, nan, O), (Q, m, V, n, COS, nan, O)]:
            assert gpu_lib.bl_amd_cross_radius_count_device(*args, None) == U, args
            assert gpu_lib.bl_amd_ctx_cross_radius_count_device(ctx, *args, None) == U, args
            assert gpu_lib.bl_amd_cross_radius_fill_device(*args, I, F, None) == U, args
            assert gpu_lib.bl_amd_ctx_cross_radius_fill_device(ctx, *args, I, F, None) == U, args
        good = (Q, m, V, n, DIST, 1.0, O)
        assert gpu_lib.bl_amd_ctx_cross_radius_count_device(None, *good, None) == U
        assert gpu_lib.bl_amd_cross_radius_fill_device(*good, None, F, None) == U
        assert gpu_lib.bl_amd_ctx_cross_radius_fill_device(ctx, *good, None, F, None) == U
        assert gpu_lib.bl_amd_ctx_cross_radius_fill_device(None, *good, I, F, None) == U
    finally:
        gpu_lib.bl_amd_ctx_destroy(ctx)
    seed = _lib.ForceVector(1, 2, 3, 4)
    for args in [(None, n, seed, order.data_ptr(), dist.data_ptr()), (V, 0, seed, order.data_ptr(), dist.data_ptr()),
                 (V, -3, seed, order.data_ptr(), dist.data_ptr()), (V, n, seed, None, dist.data_ptr()),
                 (V, n, seed, order.data_ptr(), None)]:
        assert gpu_lib.bl_amd_playlist_vec_device(*args, None) == U, args
    torch.cuda.synchronize()
    assert torch.all(oi == 7) and torch.all(ov == 3.5) and torch.all(oo == 9)
    assert torch.all(order == 7) and torch.all(dist == 3.5)

    hv = np.random.default_rng(9).standard_normal((n, 4)).astype(np.float32)
    hq = np.random.default_rng(10).standard_normal((m, 4)).astype(np.float32)
    fv = C.POINTER(_lib.ForceVector)
    hp, qp = hv.ctypes.data_as(fv), hq.ctypes.data_as(fv)
    hi = np.full(m * n, 7, dtype=np.int32)
    hf = np.full(m * n, 3.5, dtype=np.float32)
    ho = np.full(m + 1, 9, dtype=np.int64)
    ip, fp = hi.ctypes.data_as(C.POINTER(C.c_int32)), hf.ctypes.data_as(C.POINTER(C.c_float))
    op = ho.ctypes.data_as(C.POINTER(C.c_int64))
    for args in [(qp, m, hp, n, 0, DIST, ip, fp), (qp, m, hp, n, 129, COS, ip, fp), (qp, m, hp, n, k, 5, ip, fp),
                 (qp, m, hp, 0, k, DIST, ip, fp), (qp, 0, hp, n, k, DIST, ip, fp), (None, m, hp, n, k, DIST, ip, fp),
                 (qp, m, None, n, k, DIST, ip, fp), (qp, m, hp, n, k, DIST, None, fp)]:
        assert gpu_lib.bl_amd_cross_knn_host(*args) == U, args
    p_index, p_value = C.POINTER(C.c_int32)(), C.POINTER(C.c_float)()
    pi, pv = C.byref(p_index), C.byref(p_value)
    for args in [(None, m, hp, n, DIST, 1.0, op, pi, pv), (qp, m, None, n, DIST, 1.0, op, pi, pv),
                 (qp, 0, hp, n, DIST, 1.0, op, pi, pv), (qp, m, hp, 0, DIST, 1.0, op, pi, pv),
                 (qp, m, hp, n, 3, 1.0, op, pi, pv), (qp, m, hp, n, COS, nan, op, pi, pv),
                 (qp, m, hp, n, DIST, 1.0, None, pi, pv), (qp, m, hp, n, DIST, 1.0, op, None, pv)]:
        assert gpu_lib.bl_amd_cross_radius_host(*args) == U, args
    for args in [(None, n, seed, ip, fp), (hp, 0, seed, ip, fp), (hp, n, seed, None, fp)]:
        assert gpu_lib.bl_amd_playlist_vec_host(*args) == U, args
    assert np.all(hi == 7) and np.all(hf == 3.5) and np.all(ho == 9) and not p_index and not p_value
    # h_value / h_dist may be NULL
    assert gpu_lib.bl_amd_cross_knn_host(qp, m, hp, n, k, DIST, ip, None) == _lib.BL_OK
    assert np.array_equal(hi[:m * k].reshape(m, k), bliss_amd.knn_cross(hq, hv, k)[0]) and np.all(hf == 3.5)
    assert gpu_lib.bl_amd_playlist_vec_host(hp, n, seed, ip, None) == _lib.BL_OK
    assert np.array_equal(hi[:n], bliss_amd.playlist_vec(hv, [1, 2, 3, 4])[0]) and np.all(hf == 3.5)
    assert gpu_lib.bl_amd_cross_radius_host(qp, m, hp, n, DIST, 2.0, op, pi, None) == _lib.BL_OK
    want = bliss_amd.radius_cross(hq, hv, 2.0)
    assert np.array_equal(ho, want[0])
    assert np.array_equal(np.ctypeslib.as_array(p_index, shape=(max(int(ho[m]), 1),))[:int(ho[m])], want[1])
    C.CDLL(None).free(C.cast(p_index, C.c_void_p))
