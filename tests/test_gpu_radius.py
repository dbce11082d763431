"""Radius queries and duplicate groups on the device (bl_amd_radius_*, bl_amd_groups_*, bliss_amd.radius /
radius_device / duplicate_groups / duplicate_groups_device) against numpy on the oracle's matrices and the f32
restatement of bl_distance: offsets, indices in ascending song order and values by their bits; group labels against a
numpy union-find over the expected lists.  The library's own matrix calls are never the expectation."""
import ctypes as C
import threading

import numpy as np
import pytest

import bliss_amd
from bliss_amd import _lib

pytestmark = pytest.mark.gpu

INF = np.float32(np.inf)


def sq_rows(v, rows):
    """the f32 sum whose root bl_distance returns, songs `rows` to every song: left to right"""
    d = v[rows][:, None, :] - v[None, :, :]
    s = d[..., 0] * d[..., 0]
    for c in (1, 2, 3):
        s = (s + d[..., c] * d[..., c]).astype(np.float32)
    return s


def dist_rows(v, rows):
    """bl_distance of songs `rows` to every song: f32 sums left to right, the correctly rounded root"""
    d = v[rows][:, None, :] - v[None, :, :]
    s = d[..., 0] * d[..., 0]
    for c in (1, 2, 3):
        s = (s + d[..., c] * d[..., c]).astype(np.float32)
    with np.errstate(invalid="ignore"):
        return np.sqrt(s).astype(np.float32)


def mixed_set():
    """the vectors of the kNN test: ordinary force vectors, tiny and huge norms, a zero vector, duplicates, sign
    flips, orthogonal and collinear vectors"""
    rng = np.random.default_rng(11)
    v = (rng.standard_normal((3000, 4)) * 10).astype(np.float32)
    v[100:200] *= np.float32(1e-18)
    v[200:300] *= np.float32(1e17)
    v[300] = 0
    v[301] = v[5]; v[302] = -v[5]; v[303] = v[5] * np.float32(3)
    v[304] = [1, 0, 0, 0]; v[305] = [0, 1, 0, 0]; v[306] = [0, 0, -2, 0]
    v[310:330, 1:] = 0
    return v


def within(mat, rows, r, metric):
    """the contract on matrix rows: a plain f32 compare on the entry (NaN never passes), the query itself removed"""
    r = np.float32(r)
    with np.errstate(invalid="ignore"):
        w = mat >= r if metric == "cosine" else mat <= r
    w[np.arange(len(rows)), np.asarray(rows)] = False
    return w


def expected(mat, rows, r, metric):
    w = within(mat, rows, r, metric)
    off = np.concatenate([[0], np.cumsum(w.sum(axis=1, dtype=np.int64))]).astype(np.int64)
    ri, ci = np.nonzero(w)                       # row-major: ascending song index inside a row
    return off, ci.astype(np.int32), mat[ri, ci].astype(np.float32)


def assert_same(got, want):
    off, idx, val = (np.asarray(x.cpu()) if hasattr(x, "cpu") else x for x in got)
    assert off.dtype == np.int64 and idx.dtype == np.int32 and val.dtype == np.float32
    assert np.array_equal(off, want[0]), np.argwhere(off != want[0])[:5]
    assert np.array_equal(idx, want[1])
    assert np.array_equal(val.view(np.int32), want[2].view(np.int32))


DIST_RADII = [0.0, -0.0, -2.5, 1e-20, 1.0, 30.0, 1e18, np.inf]
COS_RADII = [-1.0, 0.0, 0.5, 1.0, 1.0000001, -np.inf]


@pytest.mark.parametrize("metric, radii", [("distance", DIST_RADII), ("cosine", COS_RADII)])
def test_radius_matches_the_oracle_on_mixed_scales(gpu_lib, oracle, metric, radii):
    v = mixed_set()
    n = len(v)
    mat = oracle.distance_matrix(v) if metric == "distance" else oracle.cosine_matrix(v)
    rows = np.arange(n)
    totals = []
    for r in radii:
        got = bliss_amd.radius(v, r, metric=metric)
        assert_same(got, expected(mat, rows, r, metric))
        off, idx, val = got
        assert not np.any(idx == np.repeat(rows, np.diff(off)))      # row i never lists i
        assert not np.isnan(val).any()                               # a NaN entry is never within
        totals.append(int(off[-1]))
    if metric == "distance":
        assert totals[0] == totals[1] > 0 and totals[2] == 0 and totals[-1] == n * (n - 1)
        assert totals[0] <= totals[3] < totals[4] < totals[5] <= totals[6] < totals[7]
    else:
        assert np.isnan(mat[300]).all()                              # the zero vector: every cosine 0 / 0
        got = bliss_amd.radius(v, -np.inf, metric=metric)
        assert got[0][301] == got[0][300] and totals[-1] == (n - 1) * (n - 2)   # it lists nothing, nothing lists it
        assert totals[0] > totals[1] > totals[2] > totals[3] > 0 and totals[4] <= totals[3]


def one_row(d, i, r, metric):
    off, idx, val = bliss_amd.radius_device(d, r, metric=metric, row_begin=int(i), n_rows=1)
    return idx.cpu().numpy()


@pytest.mark.parametrize("metric", ["distance", "cosine"])
def test_the_boundary_is_exact(gpu_lib, oracle, metric):
    """radius = the pair's own matrix entry lists the pair, one ulp tighter does not.  For the distance a quarter of
    the pairs have a squared sum above fl(r * r): a filter on that product would drop them."""
    import torch
    rng = np.random.default_rng(11)
    v = (rng.standard_normal((3000, 4)) * 10).astype(np.float32)
    n = len(v)
    mat = oracle.distance_matrix(v) if metric == "distance" else oracle.cosine_matrix(v)
    d = torch.from_numpy(v).cuda()
    ii = rng.integers(0, n, 240)
    jj = rng.integers(0, n, 240)
    keep = ii != jj
    ii, jj = ii[keep], jj[keep]
    assert len(ii) >= 200
    if metric == "distance":
        s = np.array([sq_rows(v, [i])[0, j] for i, j in zip(ii, jj)], dtype=np.float32)
        r = mat[ii, jj]
        above = s > (r * r).astype(np.float32)
        print("pairs with a sum above fl(r * r):", above.mean())
        assert above.mean() >= 0.10
    for i, j in zip(ii, jj):
        r = mat[i, j]
        tighter = np.nextafter(r, INF if metric == "cosine" else -INF)
        assert j in one_row(d, i, r, metric), (i, j, r)
        assert j not in one_row(d, i, tighter, metric), (i, j, tighter)
        row = mat[i:i + 1]
        assert np.array_equal(one_row(d, i, r, metric), expected(row, [i], r, metric)[1])
        assert np.array_equal(one_row(d, i, tighter, metric), expected(row, [i], tighter, metric)[1])


def test_rounding_ties_are_both_within_or_both_outside(gpu_lib):
    """9 + 2^-19 and 9 + 2^-20 have the same correctly rounded root, 3 + 1 ulp: at that radius both songs are listed,
    at radius 3 neither is"""
    e = np.float32(2.0 ** -10)
    v = np.array([[0, 0, 0, 0], [3, e, e, 0], [3, e, 0, 0], [5, 0, 0, 0], [3, 0, 0, 0]], dtype=np.float32)
    t = np.nextafter(np.float32(3), np.float32(4))
    dm = dist_rows(v, [0])[0]
    assert dm[1] == dm[2] == t and dm[4] == 3
    off, idx, val = bliss_amd.radius(v, t)
    assert list(idx[off[0]:off[1]]) == [1, 2, 4]
    assert list(val[off[0]:off[1]].view(np.int32)) == [t.view(np.int32)] * 2 + [np.float32(3).view(np.int32)]
    off, idx, val = bliss_amd.radius(v, np.float32(3))
    assert list(idx[off[0]:off[1]]) == [4]
    assert_same((off, idx, val), expected(dist_rows(v, np.arange(5)), np.arange(5), 3, "distance"))


@pytest.mark.parametrize("metric", ["distance", "cosine"])
def test_row_ranges_equal_the_full_call(gpu_lib, metric):
    """row ranges down to a single row (which takes the column split at this n) = slices of the all-rows call, byte
    for byte, offsets rebased to 0"""
    import torch
    n = 20000
    v = (np.random.default_rng(5).standard_normal((n, 4)) * 8).astype(np.float32)
    d = torch.from_numpy(v).cuda()
    r = 2.0 if metric == "distance" else 0.995
    off, idx, val = bliss_amd.radius_device(d, r, metric=metric)
    again = bliss_amd.radius_device(d, r, metric=metric)
    assert all(torch.equal(a, b) for a, b in zip((off, idx, val.view(torch.int32)),
                                                 (again[0], again[1], again[2].view(torch.int32))))
    assert off[-1] > n
    for a, b in ((0, 3001), (3001, 3007), (3007, n), (12345, 12346), (n - 1, n), (0, 1), (64, 200), (19000, 19999)):
        po, pi, pv = bliss_amd.radius_device(d, r, metric=metric, row_begin=a, n_rows=b - a)
        assert po[0] == 0 and torch.equal(po, off[a:b + 1] - off[a])
        lo, hi = int(off[a]), int(off[b])
        assert torch.equal(pi, idx[lo:hi]) and torch.equal(pv.view(torch.int32), val[lo:hi].view(torch.int32))
    rows = np.arange(0, n, 997)
    if metric == "distance":
        want = expected(dist_rows(v, rows), rows, r, metric)
        o = off.cpu().numpy()
        sel = np.concatenate([np.arange(o[i], o[i + 1]) for i in rows])
        assert np.array_equal(np.diff(o)[rows], np.diff(want[0]))
        assert np.array_equal(idx.cpu().numpy()[sel], want[1])
        assert np.array_equal(val.cpu().numpy()[sel].view(np.int32), want[2].view(np.int32))


@pytest.mark.parametrize("metric", ["distance", "cosine"])
def test_fill_variants_null_values_side_stream_and_two_contexts(gpu_lib, metric):
    import torch
    n = 6000
    v = (np.random.default_rng(8).standard_normal((n, 4)) * 8).astype(np.float32)
    r = 2.5 if metric == "distance" else 0.99
    m = _lib.BL_AMD_KNN_DISTANCE if metric == "distance" else _lib.BL_AMD_KNN_COSINE
    want = bliss_amd.radius(v, r, metric=metric)
    assert want[0][-1] > 0
    # values=False: d_value = NULL
    d = torch.from_numpy(v).cuda()
    off, idx, val = bliss_amd.radius_device(d, r, metric=metric, values=False)
    assert val is None
    assert np.array_equal(off.cpu().numpy(), want[0]) and np.array_equal(idx.cpu().numpy(), want[1])
    # a non-default stream
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d2 = torch.from_numpy(v).cuda()
        got = bliss_amd.radius_device(d2, r, metric=metric, stream=s)
    s.synchronize()
    assert_same(got, want)
    # the ctx forms on two contexts, driven from two threads at once; one of them a row range through the column split
    torch.cuda.synchronize()
    results, errors = {}, []

    def run(name, a, b):
        try:
            with bliss_amd.Context(0) as ctx:
                st = torch.cuda.Stream()
                o = torch.empty(b - a + 1, dtype=torch.int64, device="cuda")
                for _ in range(3):
                    assert gpu_lib.bl_amd_ctx_radius_count_device(ctx.handle, d.data_ptr(), n, a, b - a, m, r, o.data_ptr(),
                                                                  C.c_void_p(st.cuda_stream)) == 0
                    st.synchronize()
                    total = int(o[-1].item())
                    i = torch.empty(max(total, 1), dtype=torch.int32, device="cuda")
                    f = torch.empty(max(total, 1), dtype=torch.float32, device="cuda")
                    assert gpu_lib.bl_amd_ctx_radius_fill_device(ctx.handle, d.data_ptr(), n, a, b - a, m, r, o.data_ptr(),
                                                                 i.data_ptr(), f.data_ptr(),
                                                                 C.c_void_p(st.cuda_stream)) == 0
                    g = torch.empty(n, dtype=torch.int32, device="cuda")
                    assert gpu_lib.bl_amd_ctx_groups_device(ctx.handle, d.data_ptr(), n, m, r, g.data_ptr(),
                                                            C.c_void_p(st.cuda_stream)) == 0
                    st.synchronize()
                results[name] = (o.cpu().numpy(), i[:total].cpu().numpy(), f[:total].cpu().numpy(), g.cpu().numpy())
        except BaseException as e:   # noqa: BLE001 - reported below, in the test's thread
            errors.append(e)

    threads = [threading.Thread(target=run, args=("all", 0, n)), threading.Thread(target=run, args=("few", 1000, 1040))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert_same(results["all"][:3], want)
    lo, hi = want[0][1000], want[0][1040]
    assert_same(results["few"][:3], (want[0][1000:1041] - lo, want[1][lo:hi], want[2][lo:hi]))
    groups = bliss_amd.duplicate_groups(v, r, metric=metric)
    assert np.array_equal(results["all"][3], groups) and np.array_equal(results["few"][3], groups)


@pytest.mark.parametrize("metric", ["distance", "cosine"])
def test_one_split_with_and_without_values(gpu_lib, oracle, metric):
    """n = 1 027 is below twice RAD_SPLIT_MIN_COLS and no multiple of 64, so every call runs as one split, which the
    larger shapes of this file never do: all rows and a row range, with values and with d_value = NULL"""
    import torch
    n = 1027
    v = (np.random.default_rng(9).standard_normal((n, 4)) * 8).astype(np.float32)
    v[n - 1] = v[3]                                     # a duplicate in the last column
    mat = oracle.distance_matrix(v) if metric == "distance" else oracle.cosine_matrix(v)
    r = 6.0 if metric == "distance" else 0.9
    d = torch.from_numpy(v).cuda()
    for a, b in ((0, n), (500, 541), (n - 1, n)):
        rows = np.arange(a, b)
        want = expected(mat[a:b], rows, r, metric)
        assert want[0][-1] > 0
        assert_same(bliss_amd.radius_device(d, r, metric=metric, row_begin=a, n_rows=b - a), want)
        off, idx, val = bliss_amd.radius_device(d, r, metric=metric, row_begin=a, n_rows=b - a, values=False)
        assert val is None
        assert np.array_equal(off.cpu().numpy(), want[0]) and np.array_equal(idx.cpu().numpy(), want[1])


@pytest.mark.parametrize("metric", ["distance", "cosine"])
def test_an_empty_total(gpu_lib, metric):
    """a radius below every entry: offsets all 0, fill writes nothing (and is given zero-length lists' worth of room)"""
    import torch
    n = 5000
    v = (np.random.default_rng(9).standard_normal((n, 4)) * 8 + 1).astype(np.float32)
    r = 1e-6 if metric == "distance" else 1.5
    for got in (bliss_amd.radius(v, r, metric=metric), bliss_amd.radius_device(torch.from_numpy(v).cuda(), r, metric),
                bliss_amd.radius_device(torch.from_numpy(v).cuda(), r, metric, row_begin=7, n_rows=1)):
        off, idx, val = (np.asarray(x.cpu()) if hasattr(x, "cpu") else x for x in got)
        assert not off.any() and idx.shape == val.shape == (0,)
    # the C call itself with canaries behind the (empty) lists
    d = torch.from_numpy(v).cuda()
    m = _lib.BL_AMD_KNN_DISTANCE if metric == "distance" else _lib.BL_AMD_KNN_COSINE
    off = torch.full((n + 1,), 7, dtype=torch.int64, device="cuda")
    idx = torch.full((64,), 7, dtype=torch.int32, device="cuda")
    val = torch.full((64,), 3.5, dtype=torch.float32, device="cuda")
    assert gpu_lib.bl_amd_radius_count_device(d.data_ptr(), n, 0, n, m, r, off.data_ptr(), None) == 0
    assert gpu_lib.bl_amd_radius_fill_device(d.data_ptr(), n, 0, n, m, r, off.data_ptr(), idx.data_ptr(),
                                             val.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert not off.any() and torch.all(idx == 7) and torch.all(val == 3.5)


def test_a_dense_row_and_int64_offsets(gpu_lib):
    """radius = +inf at n = 20 000: every row lists the n - 1 others, 4e8 entries in all (more than 2^31 / 8).  Counts
    in full; indices and values on a sample of 40 rows (the one stated sampling of this file)."""
    import torch
    n = 20000
    v = (np.random.default_rng(10).standard_normal((n, 4)) * 8).astype(np.float32)
    d = torch.from_numpy(v).cuda()
    off, idx, val = bliss_amd.radius_device(d, np.inf)
    assert n * (n - 1) > 2 ** 31 // 8
    assert torch.equal(off.cpu(), torch.arange(n + 1, dtype=torch.int64) * (n - 1))
    assert idx.numel() == val.numel() == n * (n - 1)
    rows = np.sort(np.random.default_rng(1).choice(n, 40, replace=False))
    rows[0], rows[-1] = 0, n - 1
    mat = dist_rows(v, rows)
    for k, i in enumerate(rows):
        lo = int(i) * (n - 1)
        others = np.delete(np.arange(n, dtype=np.int32), i)
        assert np.array_equal(idx[lo:lo + n - 1].cpu().numpy(), others)
        assert np.array_equal(val[lo:lo + n - 1].cpu().numpy().view(np.int32), mat[k, others].view(np.int32))


def test_a_million_songs_one_and_64_queries(gpu_lib):
    """the column-split path at N = 1 048 576, compared in full for every query row"""
    import torch
    n = 1 << 20
    v = (np.random.default_rng(7).standard_normal((n, 4)) * 8).astype(np.float32)
    d = torch.from_numpy(v).cuda()
    for begin, cnt in ((123457, 1), (500000, 64)):
        rows = np.arange(begin, begin + cnt)
        mat = np.concatenate([dist_rows(v, rows[i:i + 8]) for i in range(0, cnt, 8)])
        nearest = np.where(np.arange(n)[None, :] == rows[:, None], INF, mat).min(axis=1)
        r = np.float32(nearest.max() * 1.5)        # every list holds its nearest song at least
        want = expected(mat, rows, r, "distance")
        sizes = np.diff(want[0])
        print("list sizes at n = 2^20:", sizes.min(), sizes.max())
        assert sizes.min() >= 1 and sizes.max() <= 100000
        assert_same(bliss_amd.radius_device(d, r, row_begin=begin, n_rows=cnt), want)


# ---- duplicate groups ---------------------------------------------------------------------------------------------

def components(n, src, dst):
    """smallest index of each connected component: min-label propagation with pointer jumping, edges both ways"""
    label = np.arange(n, dtype=np.int64)
    a, b = np.concatenate([src, dst]), np.concatenate([dst, src])
    while True:
        new = label.copy()
        np.minimum.at(new, a, label[b])
        new = new[new]
        if np.array_equal(new, label):
            return label.astype(np.int32)
        label = new


def expected_groups(v, r, metric, oracle=None, chunk=500):
    n = len(v)
    src, dst = [], []
    full = None if metric == "distance" else oracle.cosine_matrix(v)
    for a in range(0, n, chunk):
        rows = np.arange(a, min(n, a + chunk))
        mat = dist_rows(v, rows) if full is None else full[rows]
        ri, ci = np.nonzero(within(mat, rows, r, metric))
        src.append(rows[ri])
        dst.append(ci)
    src, dst = np.concatenate(src), np.concatenate(dst)
    return components(n, src, dst), len(src)


def check_labels(g):
    assert g.dtype == np.int32
    assert np.all(g <= np.arange(len(g))) and np.array_equal(g[g], g)


def planted(n=20000, exact=200, near=100, seed=21):
    rng = np.random.default_rng(seed)
    v = (rng.standard_normal((n, 4)) * 10).astype(np.float32)
    pick = rng.choice(n, 2 * (exact + near), replace=False)
    src, dst = pick[:exact + near], pick[exact + near:]
    v[dst[:exact]] = v[src[:exact]]
    v[dst[exact:]] = v[src[exact:]] + np.float32(1e-3)
    return v


def test_groups_find_planted_duplicates_and_chains(gpu_lib):
    v = planted()
    n = len(v)
    sizes = {}
    for r in (0.0, 0.01, 3.0):
        want, edges = expected_groups(v, r, "distance")
        off, idx, val = bliss_amd.radius(v, r)
        assert off[-1] == edges
        g = bliss_amd.duplicate_groups(v, r)
        check_labels(g)
        assert np.array_equal(g, want)
        sizes[r] = (edges, np.bincount(g, minlength=n).max())
    print("within-radius entries and largest group:", sizes)
    assert sizes[0.0] == (400, 2) and sizes[0.01] == (600, 2)
    assert sizes[3.0][0] > 50000 and sizes[3.0][1] > 2        # no longer pairs: chains
    # the same with the song order reversed and mapped back, up to the min-index relabelling
    g = bliss_amd.duplicate_groups(v, 3.0)
    back = bliss_amd.duplicate_groups(v[::-1].copy(), 3.0)[::-1]          # labels in reversed numbering, song order
    back = (n - 1 - back).astype(np.int64)                                # a member of each group, original numbering
    relabel = np.full(n, n, dtype=np.int64)
    np.minimum.at(relabel, back, np.arange(n))                            # smallest song of each such group
    assert np.array_equal(relabel[back].astype(np.int32), g)


@pytest.mark.parametrize("descending", [False, True])
def test_groups_follow_a_chain_of_1000(gpu_lib, descending):
    """0-1-2-...-999 with only consecutive songs within the radius: one group of the deepest kind, beside far songs"""
    import torch
    n = 3000
    v = np.zeros((n, 4), dtype=np.float32)
    v[:1000, 0] = np.arange(1000, dtype=np.float32)
    v[1000:, 1] = 1000 + 10 * np.arange(n - 1000, dtype=np.float32)
    if descending:
        v[:1000] = v[:1000][::-1].copy()
    off, idx, val = bliss_amd.radius(v, 1.0)
    assert off[-1] == 2 * 999
    g = bliss_amd.duplicate_groups(v, 1.0)
    check_labels(g)
    assert np.all(g[:1000] == 0) and np.array_equal(g[1000:], np.arange(1000, n))
    assert np.array_equal(bliss_amd.duplicate_groups_device(torch.from_numpy(v).cuda(), 1.0).cpu().numpy(), g)
    assert np.array_equal(g, expected_groups(v, 1.0, "distance")[0])


def test_groups_at_the_extremes(gpu_lib):
    n = 20000
    v = (np.random.default_rng(13).standard_normal((n, 4)) * 8).astype(np.float32)
    g = bliss_amd.duplicate_groups(v, np.inf)            # the dense case: one group, label 0
    assert g.dtype == np.int32 and not g.any()
    for r in (1e-6, -1.0, -np.inf):                      # below everything: identity
        assert np.array_equal(bliss_amd.duplicate_groups(v, r), np.arange(n))
    assert np.array_equal(bliss_amd.duplicate_groups(v, 1.5, metric="cosine"), np.arange(n))
    assert np.array_equal(bliss_amd.duplicate_groups(v[:1], np.inf), [0])


def test_groups_under_the_cosine_with_a_zero_vector(gpu_lib, oracle):
    """NaN edges join nothing: the zero vector stays alone whatever the radius"""
    v = mixed_set()
    n = len(v)
    for r in (0.999, 0.9, -np.inf):
        want, edges = expected_groups(v, r, "cosine", oracle)
        g = bliss_amd.duplicate_groups(v, r, metric="cosine")
        check_labels(g)
        assert np.array_equal(g, want)
        assert g[300] == 300 and np.sum(g == 300) == 1
    assert np.sum(g == 0) == n - 1                       # -inf: everything else is one group


def test_argument_errors_leave_the_outputs_untouched(gpu_lib):
    import torch
    n = 100
    d = torch.randn((n, 4), dtype=torch.float32, device="cuda")
    off = torch.full((n + 1,), 7, dtype=torch.int64, device="cuda")
    oi = torch.full((n * n,), 7, dtype=torch.int32, device="cuda")
    ov = torch.full((n * n,), 3.5, dtype=torch.float32, device="cuda")
    og = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    V, O, I, F, G = d.data_ptr(), off.data_ptr(), oi.data_ptr(), ov.data_ptr(), og.data_ptr()
    DIST, COS, nan = _lib.BL_AMD_KNN_DISTANCE, _lib.BL_AMD_KNN_COSINE, float("nan")
    bad = [(V, n, 0, n, DIST, nan), (V, n, 0, n, COS, nan), (V, n, 0, n, 2, 1.0), (V, n, 0, n, -1, 1.0),
           (V, n, -1, 2, DIST, 1.0), (V, n, n, 1, DIST, 1.0), (V, n, 0, 0, DIST, 1.0), (V, n, 0, -5, DIST, 1.0),
           (V, n, 90, 11, COS, 1.0), (V, n, 1, n, DIST, 1.0), (V, 0, 0, 1, DIST, 1.0), (V, -4, 0, 1, DIST, 1.0),
           (None, n, 0, n, DIST, 1.0)]
    for a in bad:
        assert gpu_lib.bl_amd_radius_count_device(*a, O, None) == _lib.BL_UNEXPECTED, a
        assert gpu_lib.bl_amd_radius_fill_device(*a, O, I, F, None) == _lib.BL_UNEXPECTED, a
    assert gpu_lib.bl_amd_radius_count_device(V, n, 0, n, DIST, 1.0, None, None) == _lib.BL_UNEXPECTED
    assert gpu_lib.bl_amd_radius_fill_device(V, n, 0, n, DIST, 1.0, None, I, F, None) == _lib.BL_UNEXPECTED
    assert gpu_lib.bl_amd_radius_fill_device(V, n, 0, n, DIST, 1.0, O, None, F, None) == _lib.BL_UNEXPECTED
    for a in [(V, n, DIST, nan), (V, n, 2, 1.0), (V, 0, DIST, 1.0), (None, n, DIST, 1.0)]:
        assert gpu_lib.bl_amd_groups_device(*a, G, None) == _lib.BL_UNEXPECTED, a
    assert gpu_lib.bl_amd_groups_device(V, n, DIST, 1.0, None, None) == _lib.BL_UNEXPECTED
    torch.cuda.synchronize()
    assert torch.all(off == 7) and torch.all(oi == 7) and torch.all(ov == 3.5) and torch.all(og == 7)
    # the host form: h_value may be NULL, and what it returns is free()-able
    hv = np.random.default_rng(9).standard_normal((n, 4)).astype(np.float32)
    hoff = np.empty(n + 1, dtype=np.int64)
    p_idx = C.POINTER(C.c_int32)()
    assert gpu_lib.bl_amd_radius_host(hv.ctypes.data_as(C.POINTER(_lib.ForceVector)), n, DIST, 1.0,
                                      hoff.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(p_idx), None) == _lib.BL_OK
    want = bliss_amd.radius(hv, 1.0)
    assert np.array_equal(hoff, want[0]) and hoff[-1] > 0
    assert np.array_equal(np.ctypeslib.as_array(p_idx, shape=(int(hoff[-1]),)), want[1])
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    libc.free(p_idx)
