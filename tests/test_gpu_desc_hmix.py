"""Harmonic mixes on the GPU (bl_amd_desc_hmix_*, bliss_amd.descriptor.hmix_device / hmix) against
tests/desc_hmix_reference.py.  Every comparison is ==, and every call runs under both launch shapes, forced through
bl_amd_chain_force_shape: the bytes are identical to each other and to the reference."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import bliss_amd
import bliss_amd.descriptor as D
from bliss_amd import _lib
from tests import desc_chain_reference as R
from tests import desc_hmix_reference as H
from tests import desc_reference as DR

pytestmark = pytest.mark.gpu

PER_CHAIN, SPLIT = _lib.BL_AMD_CHAIN_PER_CHAIN, _lib.BL_AMD_CHAIN_SPLIT
U = _lib.BL_UNEXPECTED
EMPTY = np.uint64(DR.EMPTY)
ALL = H.KEY | H.TEMPO | H.HALF_DOUBLE


def _torch():
    return pytest.importorskip("torch")


def dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


def attr_records(attrs, reserved=0):
    """the (n, 2) integers of the reference as bl_amd_hmix_attr records; `reserved` is ignored by the calls"""
    a = np.asarray(attrs)
    out = np.zeros(a.shape[0], dtype=D.HMIX_ATTR_DTYPE)
    out["tempo"], out["key"], out["reserved"] = a[:, 0], a[:, 1], reserved
    return out


def rule_record(rule):
    out = np.zeros(1, dtype=D.HMIX_RULE_DTYPE)
    out["key_ok"][0], out["tempo_tol"], out["flags"] = rule["key_ok"], rule["tempo_tol"], rule["flags"]
    return out[0]


def dev_attrs(attrs, reserved=0):
    return None if attrs is None else dev(attr_records(attrs, reserved).view(np.uint8).reshape(-1, 4))


@contextlib.contextmanager
def forced(shape):
    lib = bliss_amd.load()
    prev = lib.bl_amd_chain_force_shape(shape)
    try:
        yield
    finally:
        lib.bl_amd_chain_force_shape(prev)


def run(lib, attrs, rule, seeds=None, length=1, tags=None, gap=0, exclude=None, seed_desc=None, shape=None, d_lib=None,
        d_attrs=None, **kw):
    """(order int32, dist2 uint64) numpy arrays of hmix_device on uploads of the arguments"""
    torch = _torch()
    d_lib = dev(lib) if d_lib is None else d_lib
    d_attrs = dev_attrs(attrs) if d_attrs is None else d_attrs
    args = dict(tags=None if tags is None else dev(np.asarray(tags, dtype=np.int32)), gap=gap,
                exclude=None if exclude is None else dev(np.asarray(exclude)),
                seed_desc=None if seed_desc is None else (seed_desc if torch.is_tensor(seed_desc) else dev(seed_desc)))
    d_seeds = None if seeds is None else dev(np.asarray(seeds, dtype=np.int32).reshape(-1))
    with forced(shape) if shape else contextlib.nullcontext():
        order, dist2 = D.hmix_device(d_lib, d_attrs, rule_record(rule), d_seeds, length, **args, **kw)
    torch.cuda.synchronize()
    return order.cpu().numpy(), dist2.cpu().numpy().view(np.uint64)


def check(want, where="", **kw):
    """both shapes give the bytes of `want`"""
    for shape in (PER_CHAIN, SPLIT):
        order, dist2 = run(shape=shape, **kw)
        assert order.dtype == np.int32 and order.shape == want[0].shape, (where, shape)
        assert np.array_equal(order, want[0]), (where, shape)
        assert np.array_equal(dist2, want[1]), (where, shape)


CASES = H.cases()


@pytest.mark.parametrize("name", list(CASES))
def test_named_cases(name):
    """the cases every switch of the reference changes a row of (tests/test_desc_hmix_reference_host.py)"""
    check(H.hmix(**CASES[name]), name, **CASES[name])


def _ruled(n, seed):
    rng = np.random.default_rng(seed)
    tags = rng.integers(-1, 4, size=n).astype(np.int32)
    ex = rng.random(n) < 0.15
    return tags, ex


@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 33, 257, 1025, 4099])
def test_shapes(n):
    """Full-scale descriptors at every n (the tile edges, the 4-wave / 16-wave boundary of the per-chain shape, the
    smallest n the split shape takes unforced), with 1 .. 33 chains and every length around n, under the rule alone and
    under the rule, tags and a mask.  The reference is computed once per n and set of rules, for 33 chains and the
    longest length: a chain's row depends neither on the number of chains nor on the length."""
    lib = R.random_lib(n, n)
    attrs = H.random_attrs(n, n + 7, unknown=0.15)
    rule = H.camelot(250, ALL)
    rng = np.random.default_rng(n)
    seeds = rng.integers(0, n, size=33).astype(np.int32)
    seeds[:2] = [0, n - 1]
    lengths = sorted({1, 2, max(1, n - 1), n, n + 3}) if n <= 257 else [6]
    tags, ex = _ruled(n, n + 1)
    d_lib, d_attrs = dev(lib), dev_attrs(attrs)
    for rules in (dict(), dict(tags=tags, gap=2, exclude=ex)):
        ref = H.hmix(lib, attrs, rule, seeds=seeds, length=lengths[-1], **rules)
        if n >= 257:   # the rule is at work: the plain chain differs
            plain = R.chain(lib, seeds=seeds, length=lengths[-1], **rules)
            assert not np.array_equal(ref[0], plain[0])
        for nc in (1, 15, 16, 17, 33):
            for length in lengths:
                want = (ref[0][:nc, :length], ref[1][:nc, :length])
                check(want, (n, nc, length, bool(rules)), lib=lib, attrs=attrs, rule=rule, seeds=seeds[:nc],
                      length=length, d_lib=d_lib, d_attrs=d_attrs, **rules)


def test_a_rule_that_is_off_and_attributes_all_unknown_give_the_bytes_of_chain_device():
    torch = _torch()
    n = 300
    lib = R.random_lib(n, 61)
    tags, ex = _ruled(n, 62)
    seeds = np.array([0, 5, 299, 77, 150], dtype=np.int32)
    attrs = H.random_attrs(n, 63)
    unknown = np.stack([np.zeros(n, dtype=np.int64), np.resize([24, 200, 255], n)], axis=1)
    d_lib, d_seeds = dev(lib), dev(seeds)
    for rules in (dict(), dict(tags=tags, gap=2, exclude=ex)):
        d_rules = dict(tags=None if not rules else dev(tags), gap=rules.get("gap", 0),
                       exclude=None if not rules else dev(ex))
        for shape in (PER_CHAIN, SPLIT):
            with forced(shape):
                order, dist2 = D.chain_device(d_lib, d_seeds, 30, **d_rules)
                plain_sd = D.chain_device(d_lib, None, 30, seed_desc=d_lib[40:45], **d_rules)
            torch.cuda.synchronize()
            plain = (order.cpu().numpy(), dist2.cpu().numpy().view(np.uint64))
            kw = dict(lib=lib, seeds=seeds, length=30, shape=shape, d_lib=d_lib, **rules)
            off = dict(H.camelot(60, 0), key_ok=[0] * 24)   # a table that would block every known pair
            for got in (run(attrs=None, rule=off, **kw), run(attrs=attrs, rule=off, **kw),
                        run(attrs=unknown, rule=dict(off, flags=ALL), **kw)):
                assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1]), (shape, bool(rules))
            got = run(lib, unknown, dict(off, flags=ALL), seed_desc=d_lib[40:45], length=30, shape=shape, d_lib=d_lib,
                      **rules)
            assert np.array_equal(got[0], plain_sd[0].cpu().numpy()), (shape, bool(rules))
            assert np.array_equal(got[1], plain_sd[1].cpu().numpy().view(np.uint64)), (shape, bool(rules))
        # and with the rule on and the attributes known the rows are others
        assert not np.array_equal(H.hmix(lib, attrs, H.camelot(60, ALL), seeds=seeds, length=30, **rules)[0], plain[0])


def test_the_reserved_byte_and_the_bits_past_23_are_ignored():
    kw = dict(CASES["wheel_rules"])
    want = H.hmix(**kw)
    rule = dict(kw["rule"], key_ok=[w | 0xFF000000 for w in kw["rule"]["key_ok"]])
    kw.pop("rule")
    attrs = kw.pop("attrs")
    d_attrs = dev_attrs(attrs, reserved=np.arange(attrs.shape[0]) % 256)
    check(want, "reserved", attrs=attrs, d_attrs=d_attrs, rule=rule, **kw)


def test_int32_attributes_are_the_same_bytes():
    kw = dict(CASES["keys"])
    want = H.hmix(**kw)
    d_attrs = dev(attr_records(kw["attrs"]).view(np.int32))
    check(want, "int32", d_attrs=d_attrs, **kw)


def test_a_row_within_33_chains_is_the_same_seed_run_alone():
    n = 300
    lib = R.random_lib(n, 21)
    attrs = H.random_attrs(n, 24)
    rule = H.camelot(250, ALL)
    tags, ex = _ruled(n, 22)
    seeds = np.random.default_rng(23).integers(0, n, size=33).astype(np.int32)
    rules = dict(tags=tags, gap=3, exclude=ex)
    d_lib, d_attrs = dev(lib), dev_attrs(attrs)
    for shape in (PER_CHAIN, SPLIT):
        order, dist2 = run(lib, attrs, rule, seeds=seeds, length=12, shape=shape, d_lib=d_lib, d_attrs=d_attrs, **rules)
        for c in range(33):
            o1, d1 = run(lib, attrs, rule, seeds=seeds[c:c + 1], length=12, shape=shape, d_lib=d_lib, d_attrs=d_attrs,
                         **rules)
            assert np.array_equal(o1[0], order[c]) and np.array_equal(d1[0], dist2[c]), (shape, c)


def test_chains_end_where_the_rule_leaves_nothing():
    """one key per half of the library and a table that lets nothing cross: a chain ends once its half is played, at a
    different slot per row, and the other rows of the group go on"""
    n = 40
    lib = R.random_lib(n, 31)
    attrs = np.stack([np.zeros(n, dtype=np.int64), (np.arange(n) >= 10).astype(np.int64)], axis=1)
    rule = dict(key_ok=[1, 2] + [0] * 22, tempo_tol=0, flags=H.KEY)
    kw = dict(lib=lib, attrs=attrs, rule=rule, seeds=np.array([0, 10, 5, 39], dtype=np.int32), length=n)
    want = H.hmix(**kw)
    assert [int((o >= 0).sum()) for o in want[0]] == [10, 30, 10, 30]
    check(want, "ends", **kw)


def test_descriptor_seeds_may_alias_the_library():
    n = 200
    lib = R.random_lib(n, 81)
    attrs = H.random_attrs(n, 83)
    rule = H.camelot(250, ALL)
    d_lib = dev(lib)
    tags, ex = _ruled(n, 82)
    kw = dict(lib=lib, attrs=attrs, rule=rule, length=12, tags=tags, gap=2, exclude=ex)
    want = H.hmix(seed_desc=lib[40:59], **kw)
    for shape in (PER_CHAIN, SPLIT):
        order, dist2 = run(seed_desc=d_lib[40:59], d_lib=d_lib, shape=shape, **kw)
        assert np.array_equal(order, want[0]) and np.array_equal(dist2, want[1]), shape
    free = [c for c in range(19) if not ex[40 + c]]
    assert free and all(want[1][c, 0] == 0 for c in free)   # slot 0 is under no pair rule: a free song is its own nearest


def test_played_state_outside_lds():
    """200 000 songs are past 160 KiB at one bit per song and chain: the per-chain shape keeps the played words in the
    workspace, and the rule's states in LDS"""
    n = 200_000
    lib = R.random_lib(n, 91)
    attrs = H.random_attrs(n, 93)
    rng = np.random.default_rng(92)
    tags = rng.integers(0, 50, size=n).astype(np.int32)
    ex = rng.random(n) < 0.5
    kw = dict(lib=lib, attrs=attrs, rule=H.camelot(60, ALL), seeds=[0, n - 1, 123_457], length=6, tags=tags, gap=2,
              exclude=ex)
    want = H.hmix(**kw)
    assert not np.array_equal(want[0], R.chain(lib, seeds=kw["seeds"], length=6, tags=tags, gap=2, exclude=ex)[0])
    order, dist2 = run(shape=PER_CHAIN, **kw)
    assert np.array_equal(order, want[0]) and np.array_equal(dist2, want[1])


def test_played_state_and_rule_in_more_lds_than_a_launch_gets_unasked():
    """40 000 songs: the per-chain shape keeps 80 000 bytes of played words in LDS behind the rule's states, past the
    64 KiB a launch may take without the kernel's attribute, which the launch layer sets for these kernels itself"""
    n = 40_000
    lib = R.random_lib(n, 95)
    attrs = H.random_attrs(n, 96)
    rng = np.random.default_rng(97)
    tags = rng.integers(0, 50, size=n).astype(np.int32)
    seeds = [0, n - 1, 23_457]
    for rules in (dict(), dict(tags=tags, gap=2, exclude=rng.random(n) < 0.5)):
        kw = dict(lib=lib, attrs=attrs, rule=H.camelot(60, ALL), seeds=seeds, length=5, **rules)
        want = H.hmix(**kw)
        assert (want[0] >= 0).all() and not np.array_equal(want[0], R.chain(lib, seeds=seeds, length=5, **rules)[0])
        order, dist2 = run(shape=PER_CHAIN, **kw)
        assert np.array_equal(order, want[0]) and np.array_equal(dist2, want[1]), bool(rules)


def test_a_bad_device_seed_gives_an_empty_row_and_leaves_its_group_alone():
    n = 64
    lib = R.random_lib(n, 101)
    attrs = H.random_attrs(n, 102)
    seeds = np.arange(20, dtype=np.int32)
    seeds[[2, 9, 17]] = [-1, n, 2 ** 31 - 1]
    kw = dict(lib=lib, attrs=attrs, rule=H.camelot(300, ALL), seeds=seeds, length=10)
    want = H.hmix(**kw)
    assert (want[0][[2, 9, 17]] == -1).all() and (want[1][[2, 9, 17]] == EMPTY).all() and (want[0][3, :3] >= 0).all()
    check(want, "bad seeds", **kw)


def test_rejected_calls_leave_sentinels_untouched():
    torch = _torch()
    gpu_lib = bliss_amd.load()
    n, nc, length = 40, 3, 5
    lib = dev(R.random_lib(n, 111))
    attrs = dev_attrs(H.random_attrs(n, 112))
    seeds, tags = dev(np.array([0, 1, 2], dtype=np.int32)), dev(np.zeros(n, dtype=np.int32))
    oo = torch.full((nc * length * 4,), 0xA5, dtype=torch.uint8, device="cuda")
    do = torch.full((nc * length * 8,), 0xA5, dtype=torch.uint8, device="cuda")
    L, A, S, T, O, Dd = (t.data_ptr() for t in (lib, attrs, seeds, tags, oo, do))

    def rule(tol, flags):
        r = _lib.HmixRule(tempo_tol=tol, flags=flags)
        for a in range(24):
            r.key_ok[a] = 0xFFFFFF
        return C.byref(r)

    ok = rule(60, ALL)
    call, cctx = gpu_lib.bl_amd_desc_hmix_device, gpu_lib.bl_amd_ctx_desc_hmix_device
    bad = [(L, A, n, ok, S, L, nc, length, T, 1, None, O, Dd), (L, A, n, ok, None, None, nc, length, T, 1, None, O, Dd),
           (L, A, n, ok, S, None, nc, length, T, 17, None, O, Dd), (L, A, n, ok, S, None, nc, length, None, 1, None, O, Dd),
           (L, A, 0, ok, S, None, nc, length, T, 1, None, O, Dd), (L, A, 1 << 27, ok, S, None, nc, length, T, 1, None, O, Dd),
           (L, A, n, ok, S, None, nc, 0, T, 1, None, O, Dd), (L, A, n, ok, S, None, 0, length, T, 1, None, O, Dd),
           (L, A, n, ok, S, None, nc, length, T, 1, None, None, Dd), (None, A, n, ok, S, None, nc, length, T, 1, None, O, Dd),
           (L, A, n, None, S, None, nc, length, T, 1, None, O, Dd),
           (L, A, n, rule(60, 8), S, None, nc, length, T, 1, None, O, Dd),
           (L, A, n, rule(60, H.HALF_DOUBLE), S, None, nc, length, T, 1, None, O, Dd),
           (L, A, n, rule(60, H.KEY | H.HALF_DOUBLE), S, None, nc, length, T, 1, None, O, Dd),
           (L, A, n, rule(1001, ALL), S, None, nc, length, T, 1, None, O, Dd),
           (L, A, n, rule(1001, 0), S, None, nc, length, T, 1, None, O, Dd),
           (L, None, n, rule(60, H.KEY), S, None, nc, length, T, 1, None, O, Dd),
           (L, None, n, rule(60, H.TEMPO), S, None, nc, length, T, 1, None, O, Dd)]
    for shape in (PER_CHAIN, SPLIT):
        with forced(shape):
            for args in bad:
                assert call(*args, None) == U, args
                assert cctx(None, *args, None) == U, args
    torch.cuda.synchronize()
    assert bool((oo == 0xA5).all()) and bool((do == 0xA5).all())


def test_two_calls_on_one_context_and_two_streams_are_ordered():
    """Both calls share the context's workspace (the split shape's state, pair states and played words): the second
    waits for the first on the device, whatever streams they are on"""
    torch = _torch()
    n = 4099
    lib = R.random_lib(n, 121)
    attrs = H.random_attrs(n, 122)
    rule = H.camelot(250, ALL)
    d_lib, d_attrs, rec = dev(lib), dev_attrs(attrs), rule_record(rule)
    a = dict(seeds=np.array([1, 2, 3], dtype=np.int32), length=20)
    b = dict(seeds=np.array([4000, 7], dtype=np.int32), length=15)
    want_a, want_b = H.hmix(lib, attrs, rule, **a), H.hmix(lib, attrs, rule, **b)
    sa, sb = dev(a["seeds"]), dev(b["seeds"])
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with bliss_amd.Context(0) as ctx:
        for shape in (PER_CHAIN, SPLIT):
            with forced(shape):
                ra = D.hmix_device(d_lib, d_attrs, rec, sa, a["length"], stream=s1, ctx=ctx)
                rb = D.hmix_device(d_lib, d_attrs, rec, sb, b["length"], stream=s2, ctx=ctx)
            torch.cuda.synchronize()
            for got, want in ((ra, want_a), (rb, want_b)):
                assert np.array_equal(got[0].cpu().numpy(), want[0]), shape
                assert np.array_equal(got[1].cpu().numpy().view(np.uint64), want[1]), shape
    dflt = D.hmix_device(d_lib, d_attrs, rec, sa, a["length"])
    torch.cuda.synchronize()
    assert np.array_equal(dflt[0].cpu().numpy(), want_a[0])


def test_the_host_forms_give_the_reference():
    """bl_amd_desc_hmix_host through descriptor.hmix (attributes, tags, mask and both kinds of seed uploaded, both outputs
    copied back) and called directly with h_dist2 NULL, which the header allows"""
    n = 150
    lib = R.random_lib(n, 131)
    attrs = H.random_attrs(n, 134)
    rule = H.camelot(250, ALL)
    rec, at = rule_record(rule), attr_records(attrs)
    tags, ex = _ruled(n, 132)
    sd = R.random_lib(5, 133)
    sd[2] = lib[9]
    for kw in (dict(seeds=[0, 149, 77], length=25, tags=tags, gap=2, exclude=ex),
               dict(seed_desc=sd, length=25, tags=tags, gap=16, exclude=ex.astype(np.uint8)),
               dict(seeds=[5], length=n + 3)):
        want = H.hmix(lib, attrs, rule, **kw)
        seeds = kw.pop("seeds", None)
        for shape in (PER_CHAIN, SPLIT):
            with forced(shape):
                order, dist2 = D.hmix(lib, at, rec, seeds, **kw)
            assert order.dtype == np.int32 and dist2.dtype == np.uint64, shape
            assert np.array_equal(order, want[0]) and np.array_equal(dist2, want[1]), (sorted(kw), shape)
    plain = D.chain(lib, [3, 4], 7, tags=tags, gap=1, exclude=ex)
    off = D.hmix(lib, None, D.camelot_rule(60, key=False, tempo=False), [3, 4], 7, tags=tags, gap=1, exclude=ex)
    assert np.array_equal(off[0], plain[0]) and np.array_equal(off[1], plain[1])
    want = H.hmix(lib, attrs, rule, seeds=[3, 4], length=7, tags=tags, gap=1, exclude=ex)
    seeds, order = np.array([3, 4], dtype=np.int32), np.full((2, 7), 99, dtype=np.int32)
    tg, mask = np.ascontiguousarray(tags, dtype=np.int32), np.ascontiguousarray(ex).view(np.uint8)
    one = np.zeros(1, dtype=D.HMIX_RULE_DTYPE)
    one[0] = rec
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    rc = bliss_amd.load().bl_amd_desc_hmix_host(P(lib, _lib.Desc), P(at, _lib.HmixAttr), n, P(one, _lib.HmixRule),
                                                P(seeds, C.c_int32), None, 2, 7, P(tg, C.c_int32), 1, P(mask, C.c_uint8),
                                                P(order, C.c_int32), None)
    assert rc == _lib.BL_OK and np.array_equal(order, want[0])
