"""Song-to-song chains on the device (bl_amd_chain_*, bliss_amd.chain / chain_device) against a plain numpy greedy
over the oracle's matrices or the f32 restatement of bl_distance: per step the row of the current song, the played
songs masked out, the minimum of the contract's order key.  Indices equal, values equal by their bits; no tolerance.

Launch shapes (bl_amd_chain_shape): PER_CHAIN = one workgroup per chain, SPLIT = columns split over workgroups with
one launch per step.  Tests that depend on the shape say which one they exercise and assert it."""
import ctypes as C

import numpy as np
import pytest

import bliss_amd
from bliss_amd import _lib

pytestmark = pytest.mark.gpu

PER_CHAIN, SPLIT = _lib.BL_AMD_CHAIN_PER_CHAIN, _lib.BL_AMD_CHAIN_SPLIT


def dist_rows(v, rows):
    """bl_distance of songs `rows` to every song: f32 sums left to right, the correctly rounded root
    (the helper of tests/test_gpu_knn.py)"""
    with np.errstate(invalid="ignore"):
        d = v[rows][:, None, :] - v[None, :, :]
        s = d[..., 0] * d[..., 0]
        for c in (1, 2, 3):
            s = (s + d[..., c] * d[..., c]).astype(np.float32)
        return np.sqrt(s).astype(np.float32)


def ord_key(val, idx):
    """the contract's ascending order as one unsigned 64-bit key (tests/test_gpu_knn.py); pass -value for the cosine"""
    u = val.view(np.uint32).copy()
    u[val == 0] = 0
    u = np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint64)
    u[np.isnan(val)] = 0xFFFFFFFF
    return (u << np.uint64(32)) | idx.astype(np.uint32).astype(np.uint64)


def mixed_set():
    """the vectors of the kNN test: ordinary force vectors, tiny and huge norms, a zero vector, duplicates, sign flips,
    orthogonal and collinear vectors"""
    rng = np.random.default_rng(11)
    v = (rng.standard_normal((3000, 4)) * 10).astype(np.float32)
    v[100:200] *= np.float32(1e-18)
    v[200:300] *= np.float32(1e17)
    v[300] = 0
    v[301] = v[5]; v[302] = -v[5]; v[303] = v[5] * np.float32(3)
    v[304] = [1, 0, 0, 0]; v[305] = [0, 1, 0, 0]; v[306] = [0, 0, -2, 0]
    v[310:330, 1:] = 0
    return v


def greedy(row_of, n, seed, length, metric="distance"):
    """the expected chain: row_of(i) = row i of the matrix as float32"""
    order = np.full(length, -1, dtype=np.int32)
    value = np.full(length, np.nan, dtype=np.float32)
    if not 0 <= seed < n:
        return order, value
    idx = np.arange(n)
    played = np.zeros(n, dtype=bool)
    cur = int(seed)
    order[0] = cur
    value[0] = row_of(cur)[cur]
    played[cur] = True
    for t in range(1, min(length, n)):
        row = np.ascontiguousarray(row_of(cur), dtype=np.float32)
        key = ord_key(-row if metric == "cosine" else row, idx)
        key[played] = np.uint64(0xFFFFFFFFFFFFFFFF)
        cur = int(np.argmin(key))
        assert not played[cur]
        order[t] = cur
        value[t] = row[cur]
        played[cur] = True
    return order, value


def assert_chain(order, value, want_order, want_value):
    """indices equal; values equal by bits where the expected value is a number, NaN where it is NaN"""
    assert order.dtype == np.int32 and value.dtype == np.float32
    assert np.array_equal(order, want_order), np.argwhere(order != want_order)[:5]
    assert np.array_equal(np.isnan(value), np.isnan(want_value))
    ok = ~np.isnan(want_value)
    assert np.array_equal(value.view(np.int32)[ok], want_value.view(np.int32)[ok])


class forced:
    """pin the launch shape for the block (process-wide switch of the library), then give it back"""

    def __init__(self, lib, shape):
        self.lib, self.shape = lib, shape

    def __enter__(self):
        self.prev = self.lib.bl_amd_chain_force_shape(self.shape)
        assert self.prev >= 0

    def __exit__(self, *exc):
        self.lib.bl_amd_chain_force_shape(self.prev)


def cpu(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("shape", [PER_CHAIN, SPLIT])
@pytest.mark.parametrize("metric", ["distance", "cosine"])
def test_full_length_chains_match_the_oracle_on_mixed_scales(gpu_lib, oracle, metric, shape):
    """length = n = 3000 on the kNN test's vectors, seeds: ordinary, tiny, huge, the zero vector, a duplicate pair;
    each launch shape forced in turn (3000 songs would always take PER_CHAIN)"""
    v = mixed_set()
    n = len(v)
    mat = oracle.distance_matrix(v) if metric == "distance" else oracle.cosine_matrix(v)
    seeds = [0, 150, 250, 300, 5, 301, 2999]
    with forced(gpu_lib, shape):
        assert gpu_lib.bl_amd_chain_shape(n, len(seeds)) == shape
        order, value = bliss_amd.chain(v, seeds, n, metric=metric)
    for c, s in enumerate(seeds):
        want_o, want_v = greedy(lambda i: mat[i], n, s, n, metric)
        assert_chain(order[c], value[c], want_o, want_v)
        assert sorted(order[c]) == list(range(n))


@pytest.mark.parametrize("shape", [PER_CHAIN, SPLIT])
def test_rounding_tie_and_duplicates_of_the_seed(gpu_lib, shape):
    """9 + 2^-19 and 9 + 2^-20 have the same correctly rounded root (test_rounding_ties_go_to_the_smaller_index of the
    kNN test).  The chain starts at the zero vector, plays its exact duplicates in index order with value +0, and
    then stands 3 + 1 ulp away from both songs of the pair: the larger sum, at the smaller index, is played first.
    Picking by the squared sum would swap them."""
    e = np.float32(2.0 ** -10)
    v = np.array([[0, 0, 0, 0], [3, e, e, 0], [3, e, 0, 0], [50, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [-0.0, 0, 0, 0]],
                 dtype=np.float32)
    s = dist_rows(v, [0])[0]
    assert s[1] == s[2] == np.nextafter(np.float32(3), np.float32(4))
    with forced(gpu_lib, shape):
        order, value = bliss_amd.chain(v, 0, 4 + 1)
    assert list(order[0]) == [0, 4, 5, 6, 1]
    assert list(value[0, :4].view(np.int32)) == [0, 0, 0, 0]       # +0, not -0
    assert value[0, 4].view(np.int32) == s[1].view(np.int32)
    want_o, want_v = greedy(lambda i: dist_rows(v, [i])[0], len(v), 0, len(v))
    with forced(gpu_lib, shape):
        order, value = bliss_amd.chain(v, 0, len(v))
    assert_chain(order[0], value[0], want_o, want_v)
    # the tie pair among many songs, at high indices: from song 0 the pair is nearest, smaller index first
    rng = np.random.default_rng(3)
    w = (rng.standard_normal((2000, 4)) * 50 + 100).astype(np.float32)
    w[0] = 0
    w[1500] = [3, e, e, 0]
    w[1700] = [3, e, 0, 0]
    with forced(gpu_lib, shape):
        order, value = bliss_amd.chain(w, 0, 2)
    assert list(order[0]) == [0, 1500]
    assert value[0, 1].view(np.int32) == s[1].view(np.int32)


@pytest.mark.parametrize("shape", [PER_CHAIN, SPLIT])
@pytest.mark.parametrize("metric", ["distance", "cosine"])
def test_nan_and_inf_songs_come_last_in_index_order(gpu_lib, metric, shape):
    """Songs with a NaN component have a NaN value against every song: they are taken last, by index, once only
    they remain, so the chain still has min(length, n) entries.  Songs with an infinite component are an infinite
    distance from every finite song: after every finite song, before the NaN ones.  Expected chain: the greedy over
    dist_rows (distance) or over the library's own cosine matrix, whose entries the contract names (cosine)."""
    rng = np.random.default_rng(21)
    n = 700
    v = (rng.standard_normal((n, 4)) * 5).astype(np.float32)
    nans, infs = [3, 310, 650], [77, 311]
    v[3, 1] = np.nan; v[310] = np.nan; v[650, 2] = np.nan
    v[77, 0] = np.inf; v[311, 3] = -np.inf
    seeds = [10, 77, 310]
    mat = bliss_amd.cosine_matrix(v) if metric == "cosine" else None
    row_of = (lambda i: mat[i]) if metric == "cosine" else (lambda i: dist_rows(v, [i])[0])
    with forced(gpu_lib, shape):
        order, value = bliss_amd.chain(v, seeds, n + 5, metric=metric)
    for c, seed in enumerate(seeds):
        o, x = order[c], value[c]
        assert list(o[n:]) == [-1] * 5 and np.all(np.isnan(x[n:]))
        assert sorted(o[:n]) == list(range(n))                       # min(length, n) real entries, each song once
        assert_chain(o, x, *greedy(row_of, n, seed, n + 5, metric))
    # from the finite seed: ..., the songs with an infinity, the songs with a NaN; each group by index
    # (distance only: a cosine against a song with an infinity is itself NaN, so the two groups are one)
    if metric == "distance":
        assert list(order[0][n - 3:n]) == nans and np.all(np.isnan(value[0][n - 3:n]))
        assert list(order[0][n - 5:n - 3]) == infs
        assert np.isinf(value[0][n - 5]) and not np.any(np.isnan(value[0][:n - 5]))
    # from a NaN seed every value is NaN until a finite song is the current one: first step goes to index 0
    assert list(order[2][:2]) == [310, 0] and np.all(np.isnan(value[2][:2]))


@pytest.mark.parametrize("shape", [PER_CHAIN, SPLIT])
@pytest.mark.parametrize("metric", ["distance", "cosine"])
def test_tiny_corpora_padding_and_length_one(gpu_lib, oracle, metric, shape):
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 65, 300):
        v = (rng.standard_normal((n, 4)) * 3).astype(np.float32)
        mat = oracle.distance_matrix(v) if metric == "distance" else oracle.cosine_matrix(v)
        for length in (1, 2, n, n + 1, 2 * n + 70):
            seeds = sorted({0, n - 1, n // 2})
            with forced(gpu_lib, shape):
                order, value = bliss_amd.chain(v, seeds, length, metric=metric)
            assert order.shape == (len(seeds), length)
            for c, s in enumerate(seeds):
                want_o, want_v = greedy(lambda i: mat[i], n, s, length, metric)
                assert_chain(order[c], value[c], want_o, want_v)
                assert order[c, 0] == s and list(order[c, n:]) == [-1] * max(0, length - n)
                assert np.all(np.isnan(value[c, n:]))


@pytest.mark.parametrize("shape", [PER_CHAIN, SPLIT])
def test_out_of_range_seed_in_a_device_batch(gpu_lib, shape):
    import torch
    n, length = 900, 40
    v = (np.random.default_rng(6).standard_normal((n, 4)) * 4).astype(np.float32)
    d = torch.from_numpy(v).cuda()
    seeds = np.array([5, -1, n, 7, 2 ** 31 - 1, -2 ** 31, 899], dtype=np.int32)
    with forced(gpu_lib, shape):
        order, value = bliss_amd.chain_device(d, torch.from_numpy(seeds).cuda(), length)
        torch.cuda.synchronize()
    order, value = cpu(order), cpu(value)
    for c, s in enumerate(seeds):
        want_o, want_v = greedy(lambda i: dist_rows(v, [i])[0], n, int(s), length)
        assert_chain(order[c], value[c], want_o, want_v)
        if not 0 <= s < n:
            assert list(order[c]) == [-1] * length and np.all(np.isnan(value[c]))


@pytest.mark.parametrize("metric", ["distance", "cosine"])
@pytest.mark.parametrize("n", [4096, 1 << 20])
def test_a_chain_does_not_depend_on_the_batch_or_the_shape(gpu_lib, n, metric):
    """One seed alone, in a batch of 2 and in a batch of 1 024: byte-identical.  n = 4 096: all three take PER_CHAIN
    (fewer songs than the split's minimum).  n = 2^20: alone and in the pair SPLIT, in the 1 024 PER_CHAIN (asserted).  Then both
    shapes forced on the single chain."""
    import torch
    length = 48
    rng = np.random.default_rng(31)
    v = (rng.standard_normal((n, 4)) * 8).astype(np.float32)
    d = torch.from_numpy(v).cuda()
    seed = n // 3
    others = rng.integers(0, n, size=1023).astype(np.int32)
    want_shape = {1: PER_CHAIN if n == 4096 else SPLIT, 2: PER_CHAIN if n == 4096 else SPLIT, 1024: PER_CHAIN}
    got = {}
    for batch in (1, 2, 1024):
        assert gpu_lib.bl_amd_chain_shape(n, batch) == want_shape[batch]
        seeds = np.concatenate([others[:batch // 2], [seed], others[batch // 2:batch - 1]]).astype(np.int32)
        assert len(seeds) == batch
        o, x = bliss_amd.chain_device(d, torch.from_numpy(seeds).cuda(), length, metric=metric)
        got[batch] = (cpu(o)[batch // 2], cpu(x)[batch // 2])
    for shape in (PER_CHAIN, SPLIT):
        with forced(gpu_lib, shape):
            assert gpu_lib.bl_amd_chain_shape(n, 1) == shape
            o, x = bliss_amd.chain_device(d, [seed], length, metric=metric)
            got[("forced", shape)] = (cpu(o)[0], cpu(x)[0])
    ref_o, ref_x = got[1]
    assert ref_o[0] == seed and len(set(ref_o)) == length
    for key, (o, x) in got.items():
        assert o.tobytes() == ref_o.tobytes(), key
        assert x.tobytes() == ref_x.tobytes(), key


def test_a_million_songs_three_chains(gpu_lib):
    """n = 2^20, 3 chains of 64 against dist_rows; the call takes SPLIT (asserted), then PER_CHAIN forced: the LDS
    bitmap at its largest (128 KiB of played bits, one workgroup per CU)"""
    import torch
    n, length = 1 << 20, 64
    v = (np.random.default_rng(7).standard_normal((n, 4)) * 8).astype(np.float32)
    d = torch.from_numpy(v).cuda()
    seeds = [123457, 0, n - 1]
    want = [greedy(lambda i: dist_rows(v, [i])[0], n, s, length) for s in seeds]
    assert gpu_lib.bl_amd_chain_shape(n, 3) == SPLIT
    for shape in (_lib.BL_AMD_CHAIN_AUTO, PER_CHAIN):
        with forced(gpu_lib, shape):
            order, value = bliss_amd.chain_device(d, seeds, length)
        order, value = cpu(order), cpu(value)
        for c in range(3):
            assert_chain(order[c], value[c], *want[c])


@pytest.mark.parametrize("metric", ["distance", "cosine"])
def test_played_bits_in_the_workspace_beyond_what_lds_holds(gpu_lib, metric):
    """PER_CHAIN forced at n = 1.5 million: the played bits of a chain no longer fit LDS and live in the context's
    workspace; same bytes as SPLIT, and the distance chain equals dist_rows"""
    import torch
    n, length = 1_500_000, 12
    v = (np.random.default_rng(17).standard_normal((n, 4)) * 8).astype(np.float32)
    d = torch.from_numpy(v).cuda()
    seeds = [n - 1, 64]
    out = {}
    for shape in (PER_CHAIN, SPLIT):
        with forced(gpu_lib, shape):
            o, x = bliss_amd.chain_device(d, seeds, length, metric=metric)
            out[shape] = (cpu(o), cpu(x))
    assert out[PER_CHAIN][0].tobytes() == out[SPLIT][0].tobytes()
    assert out[PER_CHAIN][1].tobytes() == out[SPLIT][1].tobytes()
    if metric == "distance":
        for c, s in enumerate(seeds):
            assert_chain(out[PER_CHAIN][0][c], out[PER_CHAIN][1][c], *greedy(lambda i: dist_rows(v, [i])[0], n, s, length))


@pytest.mark.parametrize("n", [5000, 40000])
@pytest.mark.parametrize("metric", ["distance", "cosine"])
def test_side_stream_second_context_and_back_to_back_calls(gpu_lib, n, metric):
    """chain_device on a non-default stream equals chain(); two calls enqueued back to back on one stream with
    different seeds (the workspace, arrival counters and played bits are re-initialised by each call; n = 40 000
    takes SPLIT, n = 5 000 PER_CHAIN); the same through a second context of the same device."""
    import torch
    length = 70
    assert gpu_lib.bl_amd_chain_shape(n, 2) == (SPLIT if n == 40000 else PER_CHAIN)
    v = (np.random.default_rng(8).standard_normal((n, 4)) * 8).astype(np.float32)
    seeds_a, seeds_b = [17, n - 2], [n // 2, 17]
    want_a = bliss_amd.chain(v, seeds_a, length, metric=metric)
    want_b = bliss_amd.chain(v, seeds_b, length, metric=metric)
    assert want_a[0][0].tobytes() == want_b[0][1].tobytes()     # seed 17 in both
    if metric == "distance":
        assert_chain(want_a[0][0], want_a[1][0], *greedy(lambda i: dist_rows(v, [i])[0], n, 17, length))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d = torch.from_numpy(v).cuda()
        oa, xa = bliss_amd.chain_device(d, seeds_a, length, metric=metric, stream=s)
        ob, xb = bliss_amd.chain_device(d, seeds_b, length, metric=metric, stream=s)
    s.synchronize()
    for (o, x), (wo, wx) in (((oa, xa), want_a), ((ob, xb), want_b)):
        assert np.array_equal(cpu(o), wo)
        assert np.array_equal(cpu(x).view(np.int32), wx.view(np.int32))
    ctx = C.c_void_p()
    assert gpu_lib.bl_amd_ctx_create(0, C.byref(ctx)) == 0
    try:
        m = _lib.BL_AMD_KNN_COSINE if metric == "cosine" else _lib.BL_AMD_KNN_DISTANCE
        outs = []
        with torch.cuda.stream(s):
            for seeds in (seeds_a, seeds_b):
                ds = torch.tensor(seeds, dtype=torch.int32, device="cuda")
                o = torch.full((2, length), 7, dtype=torch.int32, device="cuda")
                x = torch.full((2, length), 3.5, dtype=torch.float32, device="cuda")
                assert gpu_lib.bl_amd_ctx_chain_device(ctx, d.data_ptr(), n, ds.data_ptr(), 2, length, m, o.data_ptr(),
                                                       x.data_ptr(), C.c_void_p(s.cuda_stream)) == 0
                outs.append((ds, o, x))
        s.synchronize()
        for (_, o, x), (wo, wx) in zip(outs, (want_a, want_b)):
            assert np.array_equal(cpu(o), wo)
            assert np.array_equal(cpu(x).view(np.int32), wx.view(np.int32))
    finally:
        gpu_lib.bl_amd_ctx_destroy(ctx)


@pytest.mark.parametrize("shape", [PER_CHAIN, SPLIT])
def test_rows_are_permutation_prefixes_with_the_matrix_entries(gpu_lib, shape):
    """needs no reference: no song twice in a row, and value[c][t] is bl_amd_distance_matrix_device's entry for the
    pair (order[c][t-1], order[c][t]) by its bits"""
    import torch
    n, length = 20000, 150
    v = (np.random.default_rng(9).standard_normal((n, 4)) * 8).astype(np.float32)
    v[500:520] = v[499]       # a run of duplicates
    d = torch.from_numpy(v).cuda()
    seeds = [499, 0, 19999, 7777]
    with forced(gpu_lib, shape):
        order, value = bliss_amd.chain_device(d, seeds, length)
    order, value = cpu(order), cpu(value)
    row = torch.empty((1, n), dtype=torch.float32, device="cuda")
    for c, s in enumerate(seeds):
        assert order[c, 0] == s and len(set(order[c])) == length and order[c].min() >= 0 and order[c].max() < n
        prev = s
        for t in range(length):
            assert gpu_lib.bl_amd_distance_matrix_device(d.data_ptr(), n, int(prev), 1, row.data_ptr(), None) == 0
            torch.cuda.synchronize()
            r = cpu(row)[0]
            assert value[c, t].view(np.int32) == r[order[c, t]].view(np.int32), (c, t)
            if t > 0:   # nothing unplayed is nearer
                key = ord_key(r, np.arange(n))
                key[order[c, :t]] = np.uint64(0xFFFFFFFFFFFFFFFF)
                assert int(np.argmin(key)) == order[c, t]
            prev = order[c, t]
    assert list(order[0, :21]) == list(range(499, 520)) and not value[0, :21].any()


def test_argument_errors_leave_the_outputs_untouched(gpu_lib):
    import torch
    n, nc, length = 100, 3, 8
    d = torch.randn((n, 4), dtype=torch.float32, device="cuda")
    ds = torch.tensor([0, 5, 99], dtype=torch.int32, device="cuda")
    oi = torch.full((nc, 2 * length), 7, dtype=torch.int32, device="cuda")
    ov = torch.full((nc, 2 * length), 3.5, dtype=torch.float32, device="cuda")
    V, S, I, F = d.data_ptr(), ds.data_ptr(), oi.data_ptr(), ov.data_ptr()
    DIST, COS = _lib.BL_AMD_KNN_DISTANCE, _lib.BL_AMD_KNN_COSINE
    bad = [
        (None, n, S, nc, length, DIST, I, F), (V, n, None, nc, length, DIST, I, F), (V, n, S, nc, length, DIST, None, F),
        (V, n, S, nc, length, COS, I, None), (V, 0, S, nc, length, DIST, I, F), (V, -4, S, nc, length, DIST, I, F),
        (V, n, S, 0, length, DIST, I, F), (V, n, S, -1, length, COS, I, F), (V, n, S, nc, 0, DIST, I, F),
        (V, n, S, nc, -2, DIST, I, F), (V, n, S, nc, length, 2, I, F), (V, n, S, nc, length, -1, I, F),
    ]
    for args in bad:
        assert gpu_lib.bl_amd_chain_device(*args, None) == _lib.BL_UNEXPECTED, args
    assert gpu_lib.bl_amd_ctx_chain_device(None, V, n, S, nc, length, DIST, I, F, None) == _lib.BL_UNEXPECTED
    torch.cuda.synchronize()
    assert torch.all(oi == 7) and torch.all(ov == 3.5)
    hv = np.random.default_rng(9).standard_normal((n, 4)).astype(np.float32)
    hp = hv.ctypes.data_as(C.POINTER(_lib.ForceVector))
    hs = np.array([0, 5, 99], dtype=np.int32)
    sp = hs.ctypes.data_as(C.POINTER(C.c_int32))
    hi = np.full(nc * 2 * length, 7, dtype=np.int32)
    hf = np.full(nc * 2 * length, 3.5, dtype=np.float32)
    ip, fp = hi.ctypes.data_as(C.POINTER(C.c_int32)), hf.ctypes.data_as(C.POINTER(C.c_float))
    badseed = np.array([0, 100, 5], dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    for args in [(hp, n, sp, nc, 0, DIST, ip, fp), (hp, n, sp, nc, length, 5, ip, fp), (hp, 0, sp, nc, length, DIST, ip, fp),
                 (None, n, sp, nc, length, DIST, ip, fp), (hp, n, sp, nc, length, DIST, None, fp),
                 (hp, n, None, nc, length, DIST, ip, fp), (hp, n, badseed, nc, length, DIST, ip, fp)]:
        assert gpu_lib.bl_amd_chain_host(*args) == _lib.BL_UNEXPECTED, args
    assert np.all(hi == 7) and np.all(hf == 3.5)
    # h_value may be NULL
    assert gpu_lib.bl_amd_chain_host(hp, n, sp, nc, length, DIST, ip, None) == _lib.BL_OK
    assert np.array_equal(hi[:nc * length].reshape(nc, length), bliss_amd.chain(hv, hs, length)[0])
    assert np.all(hf == 3.5)
