"""Playlist chains over descriptors on the GPU (bl_amd_desc_chain_*, bliss_amd.descriptor.chain_device) against
tests/desc_chain_reference.py.  Every comparison is ==, and every call runs under both launch shapes, forced through
bl_amd_chain_force_shape: the bytes are identical to each other and to the reference."""
import contextlib

import numpy as np
import pytest

import bliss_amd
import bliss_amd.descriptor as D
from bliss_amd import _lib
from tests import desc_chain_reference as R
from tests import desc_reference as DR

pytestmark = pytest.mark.gpu

PER_CHAIN, SPLIT = _lib.BL_AMD_CHAIN_PER_CHAIN, _lib.BL_AMD_CHAIN_SPLIT
U = _lib.BL_UNEXPECTED
EMPTY = np.uint64(DR.EMPTY)


def _torch():
    return pytest.importorskip("torch")


def dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


@contextlib.contextmanager
def forced(shape):
    lib = bliss_amd.load()
    prev = lib.bl_amd_chain_force_shape(shape)
    try:
        yield
    finally:
        lib.bl_amd_chain_force_shape(prev)


def run(lib, seeds=None, length=1, tags=None, gap=0, exclude=None, seed_desc=None, shape=None, d_lib=None, **kw):
    """(order int32, dist2 uint64) numpy arrays of chain_device on uploads of the arguments"""
    torch = _torch()
    d_lib = dev(lib) if d_lib is None else d_lib
    args = dict(tags=None if tags is None else dev(np.asarray(tags, dtype=np.int32)), gap=gap,
                exclude=None if exclude is None else dev(np.asarray(exclude)),
                seed_desc=None if seed_desc is None else (seed_desc if torch.is_tensor(seed_desc) else dev(seed_desc)))
    d_seeds = None if seeds is None else dev(np.asarray(seeds, dtype=np.int32).reshape(-1))
    with forced(shape) if shape else contextlib.nullcontext():
        order, dist2 = D.chain_device(d_lib, d_seeds, length, **args, **kw)
    torch.cuda.synchronize()
    return order.cpu().numpy(), dist2.cpu().numpy().view(np.uint64)


def check(want, where="", **kw):
    """both shapes give the bytes of `want`"""
    for shape in (PER_CHAIN, SPLIT):
        order, dist2 = run(shape=shape, **kw)
        assert order.dtype == np.int32 and order.shape == want[0].shape, (where, shape)
        assert np.array_equal(order, want[0]), (where, shape)
        assert np.array_equal(dist2, want[1]), (where, shape)


CASES = R.cases()


@pytest.mark.parametrize("name", list(CASES))
def test_named_cases(name):
    """the cases every switch of the reference changes a row of (tests/test_desc_chain_reference_host.py)"""
    check(R.chain(**CASES[name]), name, **CASES[name])


def test_a_descriptor_seed_equal_to_a_song_picks_it_at_zero():
    kw = CASES["seed_desc"]
    order, dist2 = run(**kw)
    assert (int(order[4, 0]), int(dist2[4, 0])) == (7, 0)


def _ruled(n, seed):
    rng = np.random.default_rng(seed)
    tags = rng.integers(-1, 4, size=n).astype(np.int32)
    ex = rng.random(n) < 0.15
    return tags, ex


@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 33, 257, 1025, 4099])
def test_shapes(n):
    """Full-scale descriptors (d2 up to 2^37) at every n, with 1 .. 33 chains (a partial group, more than one group) and
    every length around n.  The reference is computed once per n for 33 chains and the longest length: a chain's row
    depends neither on the number of chains nor on the length, by the reference's construction."""
    lib = R.random_lib(n, n)
    rng = np.random.default_rng(n)
    seeds = rng.integers(0, n, size=33).astype(np.int32)
    seeds[:2] = [0, n - 1]
    lengths = sorted({1, 2, max(1, n - 1), n, n + 3}) if n <= 257 else [6]
    tags, ex = _ruled(n, n + 1)
    for rules in (dict(), dict(tags=tags, gap=2, exclude=ex)):
        ref = R.chain(lib, seeds=seeds, length=lengths[-1], **rules)
        for nc in (1, 2, 15, 16, 17, 33):
            for length in lengths:
                want = (ref[0][:nc, :length], ref[1][:nc, :length])
                check(want, (n, nc, length, bool(rules)), lib=lib, seeds=seeds[:nc], length=length, **rules)


def test_the_largest_distances():
    """+32512 against -32512 in every column: d2 = 32 * 65024^2, just below 2^37"""
    lib = np.zeros((19, DR.DIMS), dtype=np.int16)
    lib[0], lib[18] = DR.SCALE_MAX, -DR.SCALE_MAX
    ex = np.ones(19, dtype=bool)
    ex[[0, 18]] = False
    kw = dict(lib=lib, seeds=[0, 18, 5], length=3, exclude=ex)
    want = R.chain(**kw)
    assert int(want[1][0, 1]) == 32 * 65024 ** 2 and list(want[0][2]) == [5, 0, 18]
    check(want, "extremes", **kw)


def test_ties_by_index_across_tiles_waves_slices_and_groups():
    n = 4099   # 257 tiles: 16 waves in the per-chain shape, nine slices in the split shape
    lib = R.tie_lib(n, 7)
    seeds = np.arange(0, n, 241, dtype=np.int32)[:18]
    kw = dict(lib=lib, seeds=seeds, length=48)
    check(R.chain(**kw), "ties", **kw)


def test_exact_duplicates_of_seeds_are_ordinary_candidates():
    lib = R.random_lib(100, 11)
    lib[[3, 50, 99]] = lib[10]
    lib[[0, 98]] = lib[20]
    kw = dict(lib=lib, seeds=[10, 20, 3, 99], length=8)
    want = R.chain(**kw)
    assert list(want[0][0, :4]) == [10, 3, 50, 99] and list(want[1][0, :4]) == [0, 0, 0, 0]
    check(want, "duplicates", **kw)
    sd = np.stack([lib[10], lib[20]])
    kw = dict(lib=lib, seed_desc=sd, length=5)
    want = R.chain(**kw)
    assert list(want[0][:, 0]) == [3, 0]
    check(want, "duplicate seeds", **kw)


def test_a_row_within_33_chains_is_the_same_seed_run_alone():
    n = 300
    lib = R.random_lib(n, 21)
    tags, ex = _ruled(n, 22)
    seeds = np.random.default_rng(23).integers(0, n, size=33).astype(np.int32)
    rules = dict(tags=tags, gap=3, exclude=ex)
    d_lib = dev(lib)
    for shape in (PER_CHAIN, SPLIT):
        order, dist2 = run(lib, seeds=seeds, length=20, shape=shape, d_lib=d_lib, **rules)
        for c in range(33):
            o1, d1 = run(lib, seeds=seeds[c:c + 1], length=20, shape=shape, d_lib=d_lib, **rules)
            assert np.array_equal(o1[0], order[c]) and np.array_equal(d1[0], dist2[c]), (shape, c)


def test_slot_one_is_the_nearest_neighbour_of_the_knn():
    torch = _torch()
    n = 1025
    lib = R.random_lib(n, 31)
    lib[500] = lib[4]
    d_lib = dev(lib)
    index, dist2 = D.knn_device(d_lib, 1)
    torch.cuda.synchronize()
    index, dist2 = index.cpu().numpy()[:, 0], dist2.cpu().numpy().view(np.uint64)[:, 0]
    seeds = np.arange(0, n, 31, dtype=np.int32)
    for shape in (PER_CHAIN, SPLIT):
        order, value = run(lib, seeds=seeds, length=2, shape=shape, d_lib=d_lib)
        assert np.array_equal(order[:, 1], index[seeds]) and np.array_equal(value[:, 1], dist2[seeds]), shape


def test_everything_excluded():
    lib = R.random_lib(40, 41)
    ex = np.ones(40, dtype=np.uint8)
    kw = dict(lib=lib, seeds=[3, 39], length=5, exclude=ex)
    want = R.chain(**kw)
    assert list(want[0][0]) == [3, -1, -1, -1, -1]
    check(want, "index seeds", **kw)
    kw = dict(lib=lib, seed_desc=lib[:3], length=5, exclude=ex)
    want = R.chain(**kw)
    assert (want[0] == -1).all() and (want[1] == EMPTY).all()
    check(want, "descriptor seeds", **kw)


@pytest.mark.parametrize("gap", [1, 16])
def test_gaps_and_negative_tags(gap):
    n = 120
    lib = R.random_lib(n, 50 + gap)
    rng = np.random.default_rng(gap)
    tags = rng.integers(0, 20, size=n).astype(np.int32)   # 20 tags, gap 16: a few are free at every slot
    tags[rng.random(n) < 0.2] = -3
    kw = dict(lib=lib, seeds=np.arange(0, 120, 7, dtype=np.int32), length=n, tags=tags, gap=gap)
    want = R.chain(**kw)
    plain = R.chain(lib=lib, seeds=kw["seeds"], length=n)
    assert not np.array_equal(want[0], plain[0])
    check(want, gap, **kw)


def test_rules_that_are_off_equal_the_plain_call():
    n = 77
    lib = R.random_lib(n, 61)
    seeds = [0, 5, 76]
    plain = run(lib, seeds=seeds, length=30)
    want = R.chain(lib, seeds=seeds, length=30)
    assert np.array_equal(plain[0], want[0]) and np.array_equal(plain[1], want[1])
    tags = np.zeros(n, dtype=np.int32)
    for kw in (dict(tags=tags, gap=0), dict(exclude=np.zeros(n, dtype=np.uint8)), dict(tags=tags, gap=0,
                                                                                     exclude=np.zeros(n, dtype=bool))):
        check(plain, sorted(kw), lib=lib, seeds=seeds, length=30, **kw)


def test_continuing_a_chain_reproduces_the_tail():
    n = 90
    lib = R.random_lib(n, 71)
    for shape in (PER_CHAIN, SPLIT):
        whole, wd = run(lib, seeds=[4, 50], length=40, shape=shape)
        for c in range(2):
            head = whole[c, :15]
            ex = np.zeros(n, dtype=np.uint8)
            ex[head] = 1
            tail, td = run(lib, seeds=[int(head[-1])], length=26, exclude=ex, shape=shape)
            assert np.array_equal(tail[0], whole[c, 14:]) and np.array_equal(td[0, 1:], wd[c, 15:]), (shape, c)


def test_descriptor_seeds_may_alias_the_library():
    n = 200
    lib = R.random_lib(n, 81)
    d_lib = dev(lib)
    tags, ex = _ruled(n, 82)
    kw = dict(lib=lib, length=12, tags=tags, gap=2, exclude=ex)
    want = R.chain(seed_desc=lib[40:59], **kw)
    for shape in (PER_CHAIN, SPLIT):
        order, dist2 = run(seed_desc=d_lib[40:59], d_lib=d_lib, shape=shape, **kw)
        assert np.array_equal(order, want[0]) and np.array_equal(dist2, want[1]), shape
    free = [c for c in range(19) if not ex[40 + c]]
    assert free and all(want[1][c, 0] == 0 for c in free)   # a song that is not excluded is its own nearest


def test_played_state_outside_lds():
    """200 000 songs are past 160 KiB at one bit per song and chain under any layout: the per-chain shape keeps the
    played words in the workspace"""
    n = 200_000
    lib = R.random_lib(n, 91)
    rng = np.random.default_rng(92)
    tags = rng.integers(0, 50, size=n).astype(np.int32)
    ex = rng.random(n) < 0.5
    kw = dict(lib=lib, seeds=[0, n - 1, 123_457], length=6, tags=tags, gap=2, exclude=ex)
    want = R.chain(**kw)
    order, dist2 = run(shape=PER_CHAIN, **kw)
    assert np.array_equal(order, want[0]) and np.array_equal(dist2, want[1])
    lib_c = bliss_amd.load()
    with forced(PER_CHAIN):
        assert lib_c.bl_amd_desc_chain_shape(n, 3) == PER_CHAIN
    with forced(SPLIT):
        assert lib_c.bl_amd_desc_chain_shape(n, 3) == SPLIT
    assert lib_c.bl_amd_desc_chain_shape(n, 3) in (PER_CHAIN, SPLIT)


def test_a_bad_device_seed_gives_an_empty_row_and_leaves_its_group_alone():
    n = 64
    lib = R.random_lib(n, 101)
    seeds = np.arange(20, dtype=np.int32)
    seeds[[2, 9, 17]] = [-1, n, 2 ** 31 - 1]
    kw = dict(lib=lib, seeds=seeds, length=10)
    want = R.chain(**kw)
    assert (want[0][[2, 9, 17]] == -1).all() and (want[1][[2, 9, 17]] == EMPTY).all() and (want[0][3] >= 0).all()
    check(want, "bad seeds", **kw)


def test_rejected_calls_leave_sentinels_untouched():
    torch = _torch()
    gpu_lib = bliss_amd.load()
    n, nc, length = 40, 3, 5
    lib = dev(R.random_lib(n, 111))
    seeds, tags = dev(np.array([0, 1, 2], dtype=np.int32)), dev(np.zeros(n, dtype=np.int32))
    oo = torch.full((nc * length * 4,), 0xA5, dtype=torch.uint8, device="cuda")
    do = torch.full((nc * length * 8,), 0xA5, dtype=torch.uint8, device="cuda")
    L, S, T, O, Dd = (t.data_ptr() for t in (lib, seeds, tags, oo, do))
    call, cctx = gpu_lib.bl_amd_desc_chain_device, gpu_lib.bl_amd_ctx_desc_chain_device
    bad = [(L, n, S, L, nc, length, T, 1, None, O, Dd), (L, n, None, None, nc, length, T, 1, None, O, Dd),
           (L, n, S, None, nc, length, T, 17, None, O, Dd), (L, n, S, None, nc, length, None, 1, None, O, Dd),
           (L, 0, S, None, nc, length, T, 1, None, O, Dd), (L, 1 << 27, S, None, nc, length, T, 1, None, O, Dd),
           (L, n, S, None, nc, 0, T, 1, None, O, Dd), (L, n, S, None, 0, length, T, 1, None, O, Dd),
           (L, n, S, None, nc, length, T, 1, None, None, Dd), (None, n, S, None, nc, length, T, 1, None, O, Dd)]
    for shape in (PER_CHAIN, SPLIT):
        with forced(shape):
            for args in bad:
                assert call(*args, None) == U, args
                assert cctx(None, *args, None) == U, args
    torch.cuda.synchronize()
    assert bool((oo == 0xA5).all()) and bool((do == 0xA5).all())


def test_two_calls_on_one_context_and_two_streams_are_ordered():
    """Both calls share the context's workspace (the split shape's state and played words): the second waits for the
    first on the device, whatever streams they are on"""
    torch = _torch()
    n = 4099
    lib = R.random_lib(n, 121)
    d_lib = dev(lib)
    a = dict(seeds=np.array([1, 2, 3], dtype=np.int32), length=40)
    b = dict(seeds=np.array([4000, 7], dtype=np.int32), length=30)
    want_a, want_b = R.chain(lib, **a), R.chain(lib, **b)
    sa, sb = dev(a["seeds"]), dev(b["seeds"])
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with bliss_amd.Context(0) as ctx:
        for shape in (PER_CHAIN, SPLIT):
            with forced(shape):
                ra = D.chain_device(d_lib, sa, a["length"], stream=s1, ctx=ctx)
                rb = D.chain_device(d_lib, sb, b["length"], stream=s2, ctx=ctx)
            torch.cuda.synchronize()
            for got, want in ((ra, want_a), (rb, want_b)):
                assert np.array_equal(got[0].cpu().numpy(), want[0]), shape
                assert np.array_equal(got[1].cpu().numpy().view(np.uint64), want[1]), shape
    dflt = D.chain_device(d_lib, sa, a["length"])
    torch.cuda.synchronize()
    assert np.array_equal(dflt[0].cpu().numpy(), want_a[0])


def test_the_host_forms_give_the_reference():
    """bl_amd_desc_chain_host through descriptor.chain (tags, mask and both kinds of seed uploaded, both outputs copied
    back) and called directly with h_dist2 NULL, which the header allows"""
    import ctypes as C
    n = 150
    lib = R.random_lib(n, 131)
    tags, ex = _ruled(n, 132)
    sd = R.random_lib(5, 133)
    sd[2] = lib[9]
    for kw in (dict(seeds=[0, 149, 77], length=25, tags=tags, gap=2, exclude=ex),
               dict(seed_desc=sd, length=25, tags=tags, gap=16, exclude=ex.astype(np.uint8)),
               dict(seeds=[5], length=n + 3)):
        want = R.chain(lib, **kw)
        seeds = kw.pop("seeds", None)
        for shape in (PER_CHAIN, SPLIT):
            with forced(shape):
                order, dist2 = D.chain(lib, seeds, **kw)
            assert order.dtype == np.int32 and dist2.dtype == np.uint64, shape
            assert np.array_equal(order, want[0]) and np.array_equal(dist2, want[1]), (sorted(kw), shape)
    want = R.chain(lib, seeds=[3, 4], length=7, tags=tags, gap=1, exclude=ex)
    seeds, order = np.array([3, 4], dtype=np.int32), np.full((2, 7), 99, dtype=np.int32)
    tg, mask = np.ascontiguousarray(tags, dtype=np.int32), np.ascontiguousarray(ex).view(np.uint8)
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    rc = bliss_amd.load().bl_amd_desc_chain_host(P(lib, _lib.Desc), n, P(seeds, C.c_int32), None, 2, 7, P(tg, C.c_int32), 1,
                                                 P(mask, C.c_uint8), P(order, C.c_int32), None)
    assert rc == _lib.BL_OK and np.array_equal(order, want[0])
