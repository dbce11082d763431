"""Descriptors on the GPU (bl_amd_desc_*, bliss_amd.descriptor) against tests/desc_reference.py.  Every quantity is an
integer or a float with defined bits, so every comparison is ==.  Sizes are the smallest at which each path can go
wrong: one tile and its edges, more than one wave and workgroup, both list widths (k <= 64, k > 64), the column split."""
import ctypes as C

import numpy as np
import pytest

import bliss_amd
import bliss_amd.descriptor as D
from bliss_amd import _lib
from tests import desc_reference as R

pytestmark = pytest.mark.gpu

M, U, SENTINEL = R.SCALE_MAX, _lib.BL_UNEXPECTED, 0xA5


def _torch():
    import torch
    return torch


def dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


def range_record(lo, hi, cnt=None):
    rec = np.zeros(1, D.RANGE_DTYPE)
    rec["lo"], rec["hi"] = lo, hi
    rec["n_finite"] = 0 if cnt is None else cnt
    return rec


def dist2_u64(t):
    return t.cpu().numpy().view(np.uint64)


# ---- range and quantiser ---------------------------------------------------------------------------------------------

def feature_matrix(n, d, seed):
    """columns by kind (c + n) % 6: random, constant, all NaN, +-inf / NaN / +-0 among numbers, values within a few ulps
    of the column's ends, large magnitudes"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, d)) * 10.0).astype(np.float32)
    for c in range(d):
        kind = (c + n) % 6
        if kind == 1:
            x[:, c] = np.float32(-3.25)
        elif kind == 2:
            x[:, c] = np.nan
        elif kind == 3:
            x[:, c] = rng.choice(np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, 1.5, -2.5, 1e-30], np.float32), size=n)
        elif kind == 4:
            lo, hi = np.float32(-7.0), np.float32(9.0)
            ends = [lo, hi]
            for _ in range(3):
                ends += [np.nextafter(ends[-2], np.float32(np.inf)), np.nextafter(ends[-1], np.float32(-np.inf))]
            x[:, c] = rng.choice(np.array(ends, np.float32), size=n)
        elif kind == 5:
            x[:, c] = (rng.standard_normal(n) * 1e30).astype(np.float32)
    return x


@pytest.mark.parametrize("d", [1, 5, 25, 32])
def test_range_and_quantise(gpu_lib, d):
    torch = _torch()
    for n in (1, 2, 63, 64, 65, 257, 5000):
        x = feature_matrix(n, d, 100 * d + n)
        scale = [int(s) for s in np.random.default_rng(n).integers(0, M + 1, size=d)]
        lo, hi, cnt = R.desc_range(x)
        want = R.quantize(x, lo, hi, scale)
        desc_t, range_t = D.fit_device(dev(x), scale=scale)
        torch.cuda.synchronize()
        got_range = np.frombuffer(range_t.cpu().numpy().tobytes(), D.RANGE_DTYPE)[0]
        where = f"n {n} d {d}"
        assert got_range["lo"].tobytes() == lo.tobytes() and got_range["hi"].tobytes() == hi.tobytes(), where
        assert np.array_equal(got_range["n_finite"], cnt), where
        assert np.array_equal(desc_t.cpu().numpy(), want), where
        host_desc, host_range = D.fit(x, scale=scale)                     # device and host forms: identical bytes
        assert host_desc.tobytes() == want.tobytes() and host_range.tobytes() == got_range.tobytes(), where
        assert np.array_equal(D.fit(x)[0], R.quantize(x, lo, hi)), where  # NULL scale: all at the maximum


def test_quantise_ties_scales_and_the_clamp(gpu_lib):
    lo, hi = np.zeros(32, np.float32), np.ones(32, np.float32)
    # products u * scale that land exactly on .5: u = (m + .5) / scale for power-of-two scales, x = t = (u + 1) / 2
    for s in (1, 2, 64, 16384):
        ms = np.arange(-s, s, dtype=np.float64) if s <= 64 else np.arange(-s, s, 997, dtype=np.float64)
        x = (((ms + 0.5) / s + 1.0) / 2.0).astype(np.float32).reshape(-1, 1)
        assert np.array_equal(x.astype(np.float64)[:, 0], ((ms + 0.5) / s + 1.0) / 2.0)
        want = R.quantize(x, lo, hi, [s])
        assert not np.array_equal(want, R.quantize(x, lo, hi, [s], bugs={"half_away"}))    # they are ties
        assert np.array_equal(D.quantize(x, range_record(lo, hi), scale=s), want), s
    # t = 15/64 + 2^-55: u is a tie of its own, u * 112 the tie -59.5 (tests/test_desc_reference_host.py)
    lo2 = lo.copy()
    lo2[0] = -2.0 ** -55
    x = np.array([[0.234375]], np.float32)
    assert D.quantize(x, range_record(lo2, hi), scale=112)[0, 0] == R.quantize(x, lo2, hi, [112])[0, 0] == -60
    # scales 0, 1 and the maximum, over a library and over rows outside its range, which the clamp maps to +-scale
    rng = np.random.default_rng(3)
    x = rng.standard_normal((300, 3)).astype(np.float32)
    desc, fitted = D.fit(x, scale=[0, 1, M])
    flo, fhi, _ = R.desc_range(x)
    assert np.array_equal(desc, R.quantize(x, flo, fhi, [0, 1, M]))
    assert not desc[:, 0].any() and set(np.unique(desc[:, 1])) == {-1, 0, 1} and desc[:, 2].min() == -M and desc[:, 2].max() == M
    out = np.array([[9.0, 9.0, 9.0], [-9.0, -9.0, -9.0], [np.nan, np.inf, -np.inf]], np.float32)
    for scale in ([0, 1, M], [7, 300, 31000]):
        got = D.quantize(out, fitted, scale=scale)
        assert np.array_equal(got, R.quantize(out, flo, fhi, scale))
        assert list(got[0, :3]) == scale and list(got[1, :3]) == [-s for s in scale] and not got[2].any()
    # device form with a range fitted elsewhere
    torch = _torch()
    rt = torch.from_numpy(np.frombuffer(np.asarray(fitted).tobytes(), np.uint8).copy()).cuda()
    got = D.quantize_device(dev(out), rt, scale=[7, 300, 31000]).cpu().numpy()
    assert np.array_equal(got, R.quantize(out, flo, fhi, [7, 300, 31000]))


# ---- tile layout -----------------------------------------------------------------------------------------------------

def matrix_of(index, d2, n_cols):
    """the d^2 matrix a full-width kNN result lists, -1 where a column is missing"""
    m = np.full((index.shape[0], n_cols), -1, dtype=np.int64)
    for r in range(index.shape[0]):
        live = index[r] >= 0
        m[r, index[r][live]] = d2[r][live].astype(np.int64)
    return m


def test_tile_layout_one_hot(gpu_lib):
    a, b = R.one_hot_sets()
    # self form, k = n - 1: the whole matrix but its diagonal
    idx, d2 = D.knn(a, 31)
    want_i, want_d = R.knn(a, 31)
    assert np.array_equal(idx, want_i) and np.array_equal(d2, want_d)
    m = matrix_of(idx, d2, 32)
    full = R.d2_direct(a, a)
    np.fill_diagonal(full, -1)
    assert np.array_equal(m, full)
    # cross form against the second set, nothing excluded: every entry, the 32 where the dimensions meet included
    for k in (31, 32):
        idx, d2 = D.knn(b, k, queries=a)
        want_i, want_d = R.knn(b, k, queries=a)
        assert np.array_equal(idx, want_i) and np.array_equal(d2, want_d), k
    m = matrix_of(idx, d2, 32)
    assert np.array_equal(m, R.d2_direct(a, b))
    for bug in ("swap_rc", "cross_k", "hl_only", "unsigned_low"):   # each of them moves a named entry of this matrix
        wrong = R.d2_planes(a, b, {bug})
        cell = (0, 27) if bug == "hl_only" else (3, 0)
        assert wrong[cell] != m[cell], bug
    # and the other way round: b's rows as the queries
    idx, d2 = D.knn(a, 32, queries=b)
    assert np.array_equal(matrix_of(idx, d2, 32), R.d2_direct(b, a))


# ---- kNN -------------------------------------------------------------------------------------------------------------

def tied_library(n, seed):
    """rows drawn from a few distinct vectors, two of them at +-32512 in all 32 dimensions: most distances tie, and the
    largest is 32 * 65024^2"""
    rng = np.random.default_rng(seed)
    protos = rng.integers(-M, M + 1, size=(6, 32)).astype(np.int16)
    protos[3], protos[4] = M, -M
    protos[5] = (rng.integers(0, 2, size=32) * 2 - 1) * M
    return protos[rng.integers(0, 6, size=n)]


KS = (1, 2, 63, 64, 65, 128)


@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 31, 33, 64, 65, 129, 1000])
def test_knn_against_the_reference(gpu_lib, n):
    torch = _torch()
    lib = tied_library(n, n)
    d_lib = dev(lib)
    picks = np.random.default_rng(n + 1).integers(0, n, size=min(n, 21))
    queries = lib[picks]                               # copies of library rows: d^2 = 0 and nothing excluded
    d_q = dev(queries)
    row_begin = min(3, n - 1)
    n_rows = min(n - row_begin, 21)                    # not a multiple of 16 wherever n allows
    for k in KS:
        want_i, want_d = R.knn(lib, k)
        idx, d2 = D.knn_device(d_lib, k)
        ridx, rd2 = D.knn_device(d_lib, k, row_begin=row_begin, n_rows=n_rows)
        cidx, cd2 = D.knn_device(d_lib, k, queries=d_q)
        torch.cuda.synchronize()
        where = f"n {n} k {k}"
        assert np.array_equal(idx.cpu().numpy(), want_i) and np.array_equal(dist2_u64(d2), want_d), where
        assert np.array_equal(ridx.cpu().numpy(), want_i[row_begin:row_begin + n_rows]), where
        assert np.array_equal(dist2_u64(rd2), want_d[row_begin:row_begin + n_rows]), where
        cw_i, cw_d = R.knn(lib, k, queries=queries)
        assert np.array_equal(cidx.cpu().numpy(), cw_i) and np.array_equal(dist2_u64(cd2), cw_d), where
        assert (cw_d[:, 0] == 0).all() and (want_i[:, min(k, n - 1):] == -1).all()
        if n > 1:
            assert want_d.max() == np.uint64(R.EMPTY) if k > n - 1 else want_d.max() <= 32 * 65024 ** 2
    hi, hd = D.knn(lib, 5)                             # the host form: identical bytes
    wi, wd = R.knn(lib, 5)
    assert hi.tobytes() == wi.tobytes() and hd.tobytes() == wd.tobytes()
    hi, hd = D.knn(lib, 5, queries=queries)
    wi, wd = R.knn(lib, 5, queries=queries)
    assert hi.tobytes() == wi.tobytes() and hd.tobytes() == wd.tobytes()


def test_knn_untied_random_and_extreme(gpu_lib):
    torch = _torch()
    rng = np.random.default_rng(77)
    lib = rng.integers(-M, M + 1, size=(1000, 32)).astype(np.int16)
    lib[::50] = (rng.integers(0, 2, size=(20, 32)) * 2 - 1) * M        # d^2 up to 32 * 65024^2, near 2^37
    lib[7], lib[8] = M, -M
    d_lib = dev(lib)
    for k in (10, 128):
        want_i, want_d = R.knn(lib, k)
        idx, d2 = D.knn_device(d_lib, k)
        torch.cuda.synchronize()
        assert np.array_equal(idx.cpu().numpy(), want_i) and np.array_equal(dist2_u64(d2), want_d), k
    far_i, far_d = R.knn(lib, 999)
    assert far_d[7].max() == 32 * 65024 ** 2 > 2 ** 36 and not np.array_equal(R.knn(lib, 10, bugs={"trunc32"})[1], R.knn(lib, 10)[1])


# ---- split and ranges ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def split_case():
    n = 3 * 4096 + 5
    rng = np.random.default_rng(9)
    lib = rng.integers(-3000, 3001, size=(n, 32)).astype(np.int16)
    lib[rng.integers(0, n, size=400)] = lib[17]        # ties across the splits, far from row 17
    lib[n - 1] = lib[0]
    ref = {k: R.knn(lib, k, row_begin=0, n_rows=40) for k in (10, 100)}
    tail = R.knn(lib, 10, row_begin=n - 40, n_rows=40)
    return n, lib, ref, tail


def test_split_and_row_ranges(gpu_lib, split_case):
    torch = _torch()
    n, lib, ref, tail = split_case
    d_lib = dev(lib)
    took_split = []
    for k in (10, 100):
        full_i, full_d = D.knn_device(d_lib, k)
        torch.cuda.synchronize()
        full_i, full_d = full_i.cpu().numpy(), dist2_u64(full_d)
        took_split.append(gpu_lib.bl_amd_desc_knn_scratch_bytes(n, n, k) > 0)
        assert np.array_equal(full_i[:40], ref[k][0]) and np.array_equal(full_d[:40], ref[k][1]), k
        if k == 10:
            assert np.array_equal(full_i[n - 40:], tail[0]) and np.array_equal(full_d[n - 40:], tail[1])
        for b, r in ((0, 1), (5, 3), (0, 40)):
            idx, d2 = D.knn_device(d_lib, k, row_begin=b, n_rows=r)
            torch.cuda.synchronize()
            took_split.append(gpu_lib.bl_amd_desc_knn_scratch_bytes(n, r, k) > 0)
            where = f"k {k} rows [{b}, {b + r})"
            assert idx.cpu().numpy().tobytes() == full_i[b:b + r].tobytes(), where
            assert dist2_u64(d2).tobytes() == full_d[b:b + r].tobytes(), where
            assert np.array_equal(idx.cpu().numpy(), ref[k][0][b:b + r]), where
            assert np.array_equal(dist2_u64(d2), ref[k][1][b:b + r]), where
        cidx, cd2 = D.knn_device(d_lib, k, queries=dev(lib[5:8]))       # the cross form through the split
        torch.cuda.synchronize()
        cw_i, cw_d = R.knn(lib, k, queries=lib[5:8])
        assert np.array_equal(cidx.cpu().numpy(), cw_i) and np.array_equal(dist2_u64(cd2), cw_d)
    # the launch layer's plan is the witness: the workspace of a call is empty exactly when it is not split
    assert gpu_lib.bl_amd_desc_knn_scratch_bytes(n, 1, 10) == 8 * 1 * 3 * 10     # three splits of 4 096 columns at least
    assert any(took_split)
    assert gpu_lib.bl_amd_desc_knn_scratch_bytes(1000, 1000, 10) == 0            # fewer than 4 096 columns: never split


def test_contexts_give_the_same_bytes(gpu_lib, split_case):
    torch = _torch()
    n, lib, ref, _ = split_case
    d_lib, d_q = dev(lib), dev(lib[100:117])
    with bliss_amd.Context(0) as ctx:
        for kw in (dict(), dict(row_begin=5, n_rows=3), dict(queries=d_q)):
            a = D.knn_device(d_lib, 10, **kw)
            b = D.knn_device(d_lib, 10, ctx=ctx, **kw)
            torch.cuda.synchronize()
            assert a[0].cpu().numpy().tobytes() == b[0].cpu().numpy().tobytes(), kw
            assert a[1].cpu().numpy().tobytes() == b[1].cpu().numpy().tobytes(), kw
    assert np.array_equal(a[0].shape, (17, 10))


# ---- rejected arguments ----------------------------------------------------------------------------------------------

def test_rejected_arguments_leave_the_outputs_untouched(gpu_lib):
    torch = _torch()
    n, k = 40, 4
    lib = dev(tied_library(n, 1))
    x = dev(np.zeros((n, 5), np.float32))
    io = torch.full((n * 128 * 4,), SENTINEL, dtype=torch.uint8, device="cuda")
    do = torch.full((n * 128 * 8,), SENTINEL, dtype=torch.uint8, device="cuda")
    ro = torch.full((384,), SENTINEL, dtype=torch.uint8, device="cuda")
    qo = torch.full((n * 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    L, X, I, Dd, Rg, Q = (t.data_ptr() for t in (lib, x, io, do, ro, qo))
    knn, cross = gpu_lib.bl_amd_desc_knn_device, gpu_lib.bl_amd_desc_cross_knn_device
    for kk in (0, 129, -1):
        assert knn(L, n, 0, n, kk, I, Dd, None) == U and cross(L, 4, L, n, kk, I, Dd, None) == U
    for nn in (0, -1, 1 << 27, 2 ** 31 - 1):
        assert knn(L, nn, 0, 1, k, I, Dd, None) == U and cross(L, 4, L, nn, k, I, Dd, None) == U
    assert knn(L, n, 0, 0, k, I, Dd, None) == U and knn(L, n, -1, 2, k, I, Dd, None) == U
    assert knn(L, n, 39, 2, k, I, Dd, None) == U and knn(L, n, n, 1, k, I, Dd, None) == U
    assert cross(L, 0, L, n, k, I, Dd, None) == U
    assert knn(None, n, 0, n, k, I, Dd, None) == U and knn(L, n, 0, n, k, None, Dd, None) == U
    assert knn(L, n, 0, n, k, I, None, None) == U
    assert cross(None, 4, L, n, k, I, Dd, None) == U and cross(L, 4, None, n, k, I, Dd, None) == U
    assert gpu_lib.bl_amd_ctx_desc_knn_device(None, L, n, 0, n, k, I, Dd, None) == U
    assert gpu_lib.bl_amd_ctx_desc_cross_knn_device(None, L, 4, L, n, k, I, Dd, None) == U
    rng_fn, qz = gpu_lib.bl_amd_desc_range_device, gpu_lib.bl_amd_desc_quantize_device
    for d in (0, 33, -1):
        assert rng_fn(X, n, d, Rg, None) == U and qz(X, n, d, Rg, None, Q, None) == U
    assert rng_fn(X, 0, 5, Rg, None) == U and rng_fn(None, n, 5, Rg, None) == U and rng_fn(X, n, 5, None, None) == U
    assert qz(X, 0, 5, Rg, None, Q, None) == U and qz(None, n, 5, Rg, None, Q, None) == U
    assert qz(X, n, 5, None, None, Q, None) == U and qz(X, n, 5, Rg, None, None, None) == U
    over = (C.c_uint16 * 5)(1, 2, M + 1, 4, 5)                         # a scale above the maximum
    assert qz(X, n, 5, Rg, over, Q, None) == U
    # the host forms
    hx, hr, hq = np.zeros((n, 5), np.float32), np.zeros(1, D.RANGE_DTYPE), np.full((n, 32), 0x5A5A, np.int16)
    F32, RP, DP = C.POINTER(C.c_float), C.POINTER(_lib.DescRange), C.POINTER(_lib.Desc)
    build = gpu_lib.bl_amd_desc_build_host
    assert build(hx.ctypes.data_as(F32), n, 33, None, 1, hr.ctypes.data_as(RP), hq.ctypes.data_as(DP)) == U
    assert build(hx.ctypes.data_as(F32), n, 5, over, 1, hr.ctypes.data_as(RP), hq.ctypes.data_as(DP)) == U
    assert build(hx.ctypes.data_as(F32), n, 5, None, 1, None, hq.ctypes.data_as(DP)) == U
    assert (hq == 0x5A5A).all() and not hr.tobytes().strip(b"\0")
    hi, hl = np.full((n, k), 77, np.int32), np.zeros((n, 32), np.int16)
    kh = gpu_lib.bl_amd_desc_knn_host
    assert kh(None, 0, hl.ctypes.data_as(DP), n, 0, hi.ctypes.data_as(C.POINTER(C.c_int32)), None) == U
    assert kh(None, 0, hl.ctypes.data_as(DP), 1 << 27, k, hi.ctypes.data_as(C.POINTER(C.c_int32)), None) == U
    assert kh(None, 0, None, n, k, hi.ctypes.data_as(C.POINTER(C.c_int32)), None) == U and (hi == 77).all()
    assert kh(None, 0, hl.ctypes.data_as(DP), n, k, hi.ctypes.data_as(C.POINTER(C.c_int32)), None) == 0   # dist2 may be NULL
    assert gpu_lib.bl_amd_desc_knn_scratch_bytes(0, 1, 1) == 0 and gpu_lib.bl_amd_desc_knn_scratch_bytes(1 << 27, 1, 1) == 0
    torch.cuda.synchronize()
    for t in (io, do, ro, qo):
        assert bytes(t.cpu().numpy()) == bytes([SENTINEL]) * t.numel()


def test_from_the_analysis_to_neighbours(gpu_lib):
    """INTEGRATION.md's Python example: analyse, take levels, timbre, rhythm and chroma, then features, fit and knn"""
    import bliss_amd.chroma
    import bliss_amd.rhythm
    rate, n = 22050, 6
    lengths = [rate * 2 * 5 + 64 * i for i in range(n)]
    corpus = bliss_amd.DeviceCorpus(lengths, [2] * n, [5] * n, device="cuda:0")
    corpus.synth(seed_base=300, sample_rate=rate)
    corpus.analyze()
    corpus.levels()
    corpus.timbre(frames=False)
    bliss_amd.rhythm.rhythm_device(corpus, *bliss_amd.rhythm.lags_for_bpm(60, 200), onsets=False)
    bliss_amd.chroma.chroma_device(corpus)
    x, names = D.features(corpus.fetch(), levels=corpus.fetch_levels(), timbre=corpus.fetch_timbre()[0],
                          rhythm=bliss_amd.rhythm.fetch_rhythm(corpus)[0], chroma=bliss_amd.chroma.fetch_chroma(corpus)[0])
    assert x.shape == (n, 25) and len(names) == 25
    desc, rng = D.fit(x)
    lo, hi, cnt = R.desc_range(x)
    assert np.array_equal(desc, R.quantize(x, lo, hi)) and np.array_equal(rng["n_finite"], cnt)
    index, dist2 = D.knn(desc, 3)
    want_i, want_d = R.knn(desc, 3)
    assert np.array_equal(index, want_i) and np.array_equal(dist2, want_d)
    assert np.array_equal(D.distance(dist2), np.sqrt(want_d.astype(np.float64)) / M)
    outside = D.quantize(x[:2] * np.float32(3.0), rng)
    ci, cd = D.knn(desc, 3, queries=outside)
    wi, wd = R.knn(desc, 3, queries=R.quantize(x[:2] * np.float32(3.0), lo, hi))
    assert np.array_equal(ci, wi) and np.array_equal(cd, wd)


def test_profile_names(gpu_lib):
    torch = _torch()
    gpu_lib.bl_amd_profile(1)
    gpu_lib.bl_amd_profile_reset()
    x = dev(np.random.default_rng(2).standard_normal((5000, 25)).astype(np.float32))
    desc, _ = D.fit_device(x)
    D.knn_device(desc, 10)                       # all rows: no split
    D.knn_device(desc, 10, row_begin=0, n_rows=1)   # one row of 5 000 columns: no split either (4 096 at least per split)
    big = dev(tied_library(3 * 4096, 4))
    D.knn_device(big, 10, row_begin=0, n_rows=2)    # split: the merge runs
    torch.cuda.synchronize()
    n = C.c_int(0)
    for name, launches in ((b"desc_range", 1), (b"desc_quantize", 1), (b"desc_knn", 3), (b"desc_merge", 1)):
        ms = gpu_lib.bl_amd_profile_ms(name, C.byref(n))
        assert ms >= 0.0 and n.value == launches, name
    gpu_lib.bl_amd_profile(0)
