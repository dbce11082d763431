"""Playlist chains over descriptors (bl_amd_desc_chain_*, bliss_amd.descriptor.chain / chain_device) without a
device: the reference of tests/desc_chain_reference.py against a brute-force loop, its switches against the cases the
GPU tests run, the checks the C entry points and the Python wrappers make before any device work, and the exports."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bliss_amd
import bliss_amd.descriptor as D
from bliss_amd import _lib
from tests import desc_chain_reference as R
from tests import desc_reference as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNX = _lib.BL_UNEXPECTED


# ---- 1. the reference

def _rows(order, dist2):
    """per chain the filled slots as [(song, d2)], once everything behind them is -1 / 2^64 - 1"""
    out = []
    for o, d in zip(order, dist2):
        k = int((o >= 0).sum())
        assert (o[:k] >= 0).all() and (o[k:] == -1).all() and (d[k:] == np.uint64(DR.EMPTY)).all()
        out.append([(int(a), int(b)) for a, b in zip(o[:k], d[:k])])
    return out


def _tiny(seed, n, tagged, masked):
    rng = np.random.default_rng(seed)
    lib = rng.integers(-3, 4, size=(n, DR.DIMS)).astype(np.int16)   # small entries: plenty of ties
    tags = rng.integers(-1, 3, size=n).astype(np.int32) if tagged else None
    ex = (rng.random(n) < 0.25) if masked else None
    return lib, tags, ex


@pytest.mark.parametrize("n", [1, 2, 5, 19])
@pytest.mark.parametrize("gap", [0, 1, 2, 16])
@pytest.mark.parametrize("masked", [False, True])
def test_reference_is_the_brute_force_loop(n, gap, masked):
    lib, tags, ex = _tiny(n * 31 + gap, n, gap > 0, masked)
    seeds = list(range(n)) + [-1, n]
    for length in (1, 2, max(1, n - 1), n, n + 3):
        got = _rows(*R.chain(lib, seeds=seeds, length=length, tags=tags, gap=gap, exclude=ex))
        for c, s in enumerate(seeds):
            assert got[c] == R.brute(lib, s, length, tags, gap, ex), (c, length)
        sd = np.concatenate([lib[:2], lib[-1:] + 1])
        got = _rows(*R.chain(lib, seed_desc=sd, length=length, tags=tags, gap=gap, exclude=ex))
        for c in range(sd.shape[0]):
            assert got[c] == R.brute(lib, None, length, tags, gap, ex, seed_vec=sd[c]), (c, length)


def test_reference_with_everything_excluded_is_empty_for_descriptor_seeds_only():
    lib, _, _ = _tiny(3, 6, False, False)
    ex = np.ones(6, dtype=bool)
    assert _rows(*R.chain(lib, seed_desc=lib[:2], length=4, exclude=ex)) == [[], []]
    assert _rows(*R.chain(lib, seeds=[4], length=4, exclude=ex)) == [[(4, 0)]]   # the seed takes slot 0 regardless


CASES = R.cases()
BASE = {name: R.chain(**kw) for name, kw in CASES.items()}


def test_every_switch_has_a_case():
    assert set(R.SWITCH_CASE) == set(R.BUGS)
    assert {case for case, _ in R.SWITCH_CASE.values()} <= set(CASES)


@pytest.mark.parametrize("bug", R.BUGS)
def test_every_switch_changes_its_row_of_its_case(bug):
    case, row = R.SWITCH_CASE[bug]
    order, dist2 = R.chain(**CASES[case], bugs=(bug,))
    want_o, want_d = BASE[case]
    assert not (np.array_equal(order[row], want_o[row]) and np.array_equal(dist2[row], want_d[row]))


def test_two_tag_chains_end_early_at_different_slots_of_one_group():
    order, _ = BASE["two_tags"]
    ends = {int((o >= 0).sum()) for o in order[:16]}
    assert len(ends) > 1 and max(ends) < CASES["two_tags"]["lib"].shape[0]


@pytest.mark.parametrize("name", ["ties", "one_hot"])
def test_a_chain_without_rules_is_repeated_knn_picks(name):
    """slot t + 1 = the first entry of the full kNN list of slot t's song that the chain has not played"""
    kw = CASES[name]
    lib, n = kw["lib"], kw["lib"].shape[0]
    index, dist2 = DR.knn(lib, n - 1)
    order, value = BASE[name]
    for c in range(0, order.shape[0], 5):
        played = {int(order[c, 0])}
        for t in range(1, min(kw["length"], n)):
            prev = int(order[c, t - 1])
            k = next(i for i in range(n - 1) if int(index[prev, i]) not in played)
            assert (int(order[c, t]), int(value[c, t])) == (int(index[prev, k]), int(dist2[prev, k])), (c, t)
            played.add(int(order[c, t]))


# ---- 2. the C entry points

def _buffers(n=16, nc=3, length=5):
    lib = (_lib.Desc * n)()
    seeds = (C.c_int32 * nc)(0, 5, 15)
    q = (_lib.Desc * nc)()
    tags = (C.c_int32 * n)(*range(n))
    ex = (C.c_uint8 * n)()
    order = (C.c_int32 * (nc * length))(*([7] * (nc * length)))
    dist2 = (C.c_uint64 * (nc * length))(*([35] * (nc * length)))
    return lib, seeds, q, tags, ex, order, dist2


def test_c_entry_points_refuse_bad_arguments_with_or_without_a_device():
    """Arguments and index seeds are checked before any device work: BL_UNEXPECTED and nothing written."""
    lib = bliss_amd.load()
    n, nc, length = 16, 3, 5
    v, good, q, tags, ex, order, dist2 = _buffers(n, nc, length)
    for bad in ((0, 16, 1), (-1, 2, 3), (0, 1, 2 ** 31 - 1)):
        seeds = (C.c_int32 * nc)(*bad)
        assert lib.bl_amd_desc_chain_host(v, n, seeds, None, nc, length, tags, 1, ex, order, dist2) == UNX
    host_bad = [
        (v, n, good, q, nc, length, tags, 1, ex, order, dist2),         # both kinds of seed
        (v, n, None, None, nc, length, tags, 1, ex, order, dist2),      # neither
        (v, n, good, None, nc, length, tags, 17, ex, order, dist2),
        (v, n, good, None, nc, length, tags, -1, ex, order, dist2),
        (v, n, good, None, nc, length, None, 1, ex, order, dist2),      # a gap without tags
        (v, n, None, q, nc, length, None, 16, None, order, dist2),
        (v, 0, good, None, nc, length, tags, 1, ex, order, dist2),
        (v, 2 ** 27, good, None, nc, length, tags, 1, ex, order, dist2),
        (v, -4, good, None, nc, length, tags, 1, ex, order, dist2),
        (v, n, good, None, nc, 0, tags, 1, ex, order, dist2),
        (v, n, good, None, nc, -7, tags, 1, ex, order, dist2),
        (v, n, good, None, 0, length, tags, 1, ex, order, dist2),
        (v, n, good, None, nc, length, tags, 1, ex, None, dist2),       # a NULL order
        (None, n, good, None, nc, length, tags, 1, ex, order, dist2),
    ]
    for args in host_bad:
        assert lib.bl_amd_desc_chain_host(*args) == UNX, args
    A = C.addressof
    V, S, Q, T, X, O, F = A(v), A(good), A(q), A(tags), A(ex), A(order), A(dist2)
    dev_bad = [
        (V, n, S, Q, nc, length, T, 1, X, O, F), (V, n, None, None, nc, length, T, 1, X, O, F),
        (V, n, S, None, nc, length, T, 17, X, O, F), (V, n, S, None, nc, length, T, -1, X, O, F),
        (V, n, S, None, nc, length, None, 3, X, O, F), (V, n, None, Q, nc, length, None, 1, None, O, F),
        (V, 0, S, None, nc, length, T, 1, X, O, F), (V, 2 ** 27, S, None, nc, length, T, 1, X, O, F),
        (V, n, S, None, nc, 0, T, 1, X, O, F), (V, n, S, None, 0, length, T, 1, X, O, F),
        (V, n, S, None, nc, length, T, 1, X, None, F), (V, n, S, None, nc, length, T, 1, X, O, None),
        (None, n, S, None, nc, length, T, 1, X, O, F),
    ]
    for args in dev_bad:
        assert lib.bl_amd_desc_chain_device(*args, None) == UNX, args
        assert lib.bl_amd_ctx_desc_chain_device(None, *args, None) == UNX, args
    assert list(order) == [7] * (nc * length) and list(dist2) == [35] * (nc * length)
    for n_bad, nc_bad in ((0, 1), (2 ** 27, 1), (-1, 1), (10, 0)):
        assert lib.bl_amd_desc_chain_shape(n_bad, nc_bad) == UNX


def test_symbols_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "bliss_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(bl_amd_(?:ctx_)?desc_chain_\w+)\s*\(", code))
    assert declared == {"bl_amd_desc_chain_device", "bl_amd_ctx_desc_chain_device", "bl_amd_desc_chain_host",
                        "bl_amd_desc_chain_shape"}
    assert declared <= set(_lib.SYMBOLS)
    lib = bliss_amd.load()
    for name in declared:
        assert hasattr(lib, name)
    assert "chain" in bliss_amd.__all__ and bliss_amd.chain is not D.chain   # the package's own namespace is unchanged
    assert callable(D.chain) and callable(D.chain_device)


# ---- 3. the Python wrappers

LIB = np.zeros((10, 32), dtype=np.int16)
TAGS = np.arange(10, dtype=np.int32)


def _t(a):
    return pytest.importorskip("torch").from_numpy(a)   # a CPU tensor: the checks come before anything touches a device


INT_ARGS = {
    ("chain", "length"): (1, None, lambda x: D.chain(LIB, 0, x)),
    ("chain", "gap"): (0, _lib.BL_AMD_MIX_MAX_GAP, lambda x: D.chain(LIB, 0, 3, tags=TAGS, gap=x)),
    ("chain_device", "length"): (1, None, lambda x: D.chain_device(_t(LIB), 0, x)),
    ("chain_device", "gap"): (0, _lib.BL_AMD_MIX_MAX_GAP, lambda x: D.chain_device(_t(LIB), 0, 3, tags=_t(TAGS), gap=x)),
}
NOT_AN_INTEGER = [True, 2.0, np.float32(2), "2", None]


def _refused(key, value):
    with pytest.raises(ValueError) as e:
        INT_ARGS[key][2](value)
    assert str(e.value).startswith(f"{key[1]} must be") and repr(value) in str(e.value), str(e.value)


@pytest.mark.parametrize("key", list(INT_ARGS), ids=".".join)
@pytest.mark.parametrize("value", NOT_AN_INTEGER, ids=repr)
def test_what_is_not_an_integer_is_refused(key, value):
    _refused(key, value)


@pytest.mark.parametrize("key", list(INT_ARGS), ids=".".join)
def test_integers_outside_the_range_are_refused(key):
    lo, hi, _ = INT_ARGS[key]
    _refused(key, lo - 1)
    _refused(key, np.int64(lo - 1))
    if hi is not None:
        _refused(key, hi + 1)


@pytest.mark.parametrize("fn", ["chain", "chain_device"])
def test_wrappers_refuse_bad_seeds_tags_and_masks(fn):
    call = getattr(D, fn)
    dev = fn == "chain_device"
    lib = _t(LIB) if dev else LIB
    wrap = _t if dev else (lambda a: a)
    with pytest.raises(ValueError):
        call(lib, None, 3)                                   # neither kind of seed
    with pytest.raises(ValueError):
        call(lib, 0, 3, seed_desc=lib[:2])                   # both
    with pytest.raises(ValueError):
        call(lib, 0, 3, gap=2)                               # a gap without tags
    with pytest.raises(ValueError):
        call(lib, [0.5], 3)
    for tags in (np.arange(9, dtype=np.int32), np.zeros(10, dtype=np.float32), np.zeros((10, 1), dtype=np.int32)):
        with pytest.raises(ValueError):
            call(lib, 0, 3, tags=wrap(tags), gap=1)
    for ex in (np.zeros(9, dtype=bool), np.zeros(10, dtype=np.int32)):
        with pytest.raises(ValueError):
            call(lib, 0, 3, exclude=wrap(ex))
    if not dev:
        for seeds in (-1, 10, [0, 10]):
            with pytest.raises(ValueError):
                call(lib, seeds, 3)                          # the host form refuses what the device form pads
        with pytest.raises(ValueError):
            call(lib.astype(np.int32), 0, 3)


ENTRY_POINTS = [
    ("bl_amd_desc_chain_host", lambda: D.chain(LIB, [0, 4], 3)),
    ("bl_amd_desc_chain_host", lambda: D.chain(LIB, [0, 4], 3, tags=TAGS, gap=1, exclude=TAGS > 7)),
    ("bl_amd_desc_chain_host", lambda: D.chain(LIB, None, 3, seed_desc=LIB[:2])),
    ("bl_amd_desc_chain_host", lambda: D.chain(LIB, np.int64(3), np.int32(4), tags=TAGS.astype(np.int64), gap=np.int64(16))),
]


@pytest.mark.parametrize("name, call", ENTRY_POINTS, ids=[f"{i}-{n}" for i, (n, _) in enumerate(ENTRY_POINTS)])
def test_a_well_formed_call_reaches_its_entry_point(name, call):
    """No ValueError.  Without a device the library refuses, which the wrapper reports as a RuntimeError that names
    the entry point; with one the call returns a row per seed."""
    try:
        order, dist2 = call()
    except RuntimeError as e:
        assert re.findall(r"bl_amd_\w+", str(e)) == [name]
    else:
        assert order.dtype == np.int32 and dist2.dtype == np.uint64 and order.shape == dist2.shape
