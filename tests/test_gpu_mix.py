"""Chains under rules on the device (bl_amd_mix_*, bliss_amd.mix / mix_device) against a numpy greedy that transcribes
the contract: the greedy of tests/test_gpu_chain.py with an allowed-mask per step (not played, not excluded, no tag of
the last `gap` slots).  Indices equal, values equal by their bits; no tolerance.  Every test runs with each launch
shape forced (bl_amd_chain_force_shape pins mix calls too)."""
import ctypes as C

import numpy as np
import pytest

import bliss_amd
from bliss_amd import _lib
from tests.test_gpu_chain import assert_chain, cpu, dist_rows, forced, mixed_set, ord_key

pytestmark = pytest.mark.gpu

PER_CHAIN, SPLIT = _lib.BL_AMD_CHAIN_PER_CHAIN, _lib.BL_AMD_CHAIN_SPLIT
SHAPES = [PER_CHAIN, SPLIT]
METRICS = ["distance", "cosine"]
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def greedy_mix(row_of, n, length, metric="distance", seed=None, seed_row=None, tags=None, gap=0, exclude=None):
    """the expected row: row_of(i) = row i of the matrix as float32; seed_row = the row of a vector seed"""
    order = np.full(length, -1, dtype=np.int32)
    value = np.full(length, np.nan, dtype=np.float32)
    idx = np.arange(n)
    never = np.zeros(n, dtype=bool) if exclude is None else np.asarray(exclude).astype(bool).copy()   # played or excluded
    slots_tags = []

    def pick(row, t):
        row = np.ascontiguousarray(row, dtype=np.float32)
        key = ord_key(-row if metric == "cosine" else row, idx)
        key[never] = EMPTY
        if gap > 0 and t > 0:
            recent = [x for x in slots_tags[-gap:] if x >= 0]
            key[np.isin(tags, recent)] = EMPTY
        j = int(np.argmin(key))
        return (j, row[j]) if key[j] != EMPTY else (-1, None)

    if seed_row is None:
        if not 0 <= seed < n:
            return order, value
        cur, val = int(seed), row_of(int(seed))[int(seed)]
    else:
        cur, val = pick(seed_row, 0)
        if cur < 0:
            return order, value
    for t in range(min(length, n)):
        if t > 0:
            cur, val = pick(row_of(cur), t)
            if cur < 0:
                break
        order[t], value[t] = cur, val
        never[cur] = True
        slots_tags.append(int(tags[cur]) if tags is not None else -1)
    return order, value


def dist_row_of(v):
    return lambda i: dist_rows(v, [i])[0]


def rows_of(v, metric, oracle):
    if metric == "distance":
        return dist_row_of(v)
    mat = oracle.cosine_matrix(v)
    return lambda i: mat[i]


def run(v, seeds, length, shape, lib, **kw):
    with forced(lib, shape):
        assert lib.bl_amd_chain_shape(len(v), 1) == shape
        return bliss_amd.mix(v, seeds, length, **kw)


def big_mixed_set(n):
    """the chain test's mixed-scale set, continued to n songs by vectors of the same mixture of scales"""
    base = mixed_set()
    rng = np.random.default_rng(12)
    more = (rng.standard_normal((n - len(base), 4)) * 10).astype(np.float32)
    more[::7] *= np.float32(1e-18)
    more[3::11] *= np.float32(1e17)
    return np.concatenate([base, more])


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n, length", [(3000, 3000), (20000, 150), (40000, 150)])
def test_no_rules_is_the_chain_byte_for_byte(gpu_lib, n, length, metric):
    """index seeds, no mask, gap 0 (with and without a tag array): bliss_amd.chain's bytes.  n = 3 000: 256 lanes per
    chain when that shape is forced; 20 000: 1 024 lanes; both larger sets take the split when left alone."""
    v = mixed_set() if n == 3000 else big_mixed_set(n)
    seeds = [0, 150, 250, 300, 5, 301, n - 1]
    tags = np.arange(n, dtype=np.int32) % 3
    assert gpu_lib.bl_amd_chain_shape(n, len(seeds)) == (PER_CHAIN if n == 3000 else SPLIT)
    for shape in (_lib.BL_AMD_CHAIN_AUTO, PER_CHAIN, SPLIT):
        with forced(gpu_lib, shape):
            want = bliss_amd.chain(v, seeds, length, metric=metric)
            got = bliss_amd.mix(v, seeds, length, metric=metric)
            got_tags = bliss_amd.mix(v, seeds, length, metric=metric, tags=tags, gap=0)
        for g in (got, got_tags):
            assert g[0].tobytes() == want[0].tobytes() and g[1].tobytes() == want[1].tobytes(), shape


@pytest.fixture(scope="module")
def albums(oracle):
    """400 albums of 8 songs each, 1e-3 around the album's centre, in shuffled order; tag = album"""
    rng = np.random.default_rng(41)
    centre = (rng.standard_normal((400, 4)) * 10).astype(np.float32)
    v = (np.repeat(centre, 8, axis=0) + rng.standard_normal((3200, 4)) * 1e-3).astype(np.float32)
    tags = np.repeat(np.arange(400, dtype=np.int32), 8)
    perm = rng.permutation(3200)
    v, tags = np.ascontiguousarray(v[perm]), np.ascontiguousarray(tags[perm])
    return v, tags, {"distance": oracle.distance_matrix(v), "cosine": oracle.cosine_matrix(v)}


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("metric", METRICS)
def test_albums(gpu_lib, albums, metric, shape):
    v, tags, mats = albums
    mat = mats[metric]
    n, length, seeds = len(v), 200, [0, 1234, 3199]
    plain = bliss_amd.chain(v, seeds, length, metric=metric)
    for c in range(len(seeds)):   # the unconstrained chain plays whole albums: a rule that does nothing would show
        t = tags[plain[0][c]]
        assert any(t[i] in t[max(0, i - 4):i] for i in range(1, length))
    got = run(v, seeds, length, shape, gpu_lib, metric=metric, tags=tags, gap=0)
    assert got[0].tobytes() == plain[0].tobytes() and got[1].tobytes() == plain[1].tobytes()
    for gap in (1, 4, 16):
        order, value = run(v, seeds, length, shape, gpu_lib, metric=metric, tags=tags, gap=gap)
        for c, s in enumerate(seeds):
            assert_chain(order[c], value[c], *greedy_mix(lambda i: mat[i], n, length, metric, seed=s, tags=tags, gap=gap))
            t = tags[order[c]]
            assert order[c].min() >= 0 and all(t[i] not in t[max(0, i - gap):i] for i in range(1, length))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("metric", METRICS)
def test_a_blocked_nearest_song_does_not_prune_the_allowed_one(gpu_lib, oracle, metric, shape):
    """The current song has an exact duplicate of its own tag, 256 columns ahead of the only allowed near song: both
    fall to one lane in either shape, the duplicate first.  A bound tightened by the blocked duplicate (distance 0)
    would skip the allowed song at distance 3 and pick a far one."""
    rng = np.random.default_rng(43)
    for n, cur, dup, near in ((600, 0, 1, 257), (2000, 1400, 1500, 1756)):
        v = (rng.standard_normal((n, 4)) + 100).astype(np.float32) * np.array([1, 0, 0, 1], dtype=np.float32)
        v[:, 1] = 50 + rng.standard_normal(n)
        v[cur] = [1, 2, 3, 4]
        v[dup] = v[cur]
        v[near] = [1, 2, 6, 4]
        tags = np.arange(n, dtype=np.int32) + 10
        tags[dup] = tags[cur]
        order, value = run(v, cur, 3, shape, gpu_lib, metric=metric, tags=tags, gap=1)
        want = greedy_mix(rows_of(v, metric, oracle), n, 3, metric, seed=cur, tags=tags, gap=1)
        assert_chain(order[0], value[0], *want)
        assert list(order[0][:2]) == [cur, near]
        if metric == "distance":
            assert value[0][1] == np.float32(3) and order[0][2] == dup   # the duplicate is free again one slot later


@pytest.mark.parametrize("shape", SHAPES)
def test_chains_that_end(gpu_lib, shape):
    rng = np.random.default_rng(44)
    n = 500
    v = (rng.standard_normal((n, 4)) * 5).astype(np.float32)
    row_of = dist_row_of(v)
    one = np.full(n, 7, dtype=np.int32)
    order, value = run(v, [3, 499], 6, shape, gpu_lib, tags=one, gap=1)
    for c, s in enumerate((3, 499)):
        assert list(order[c]) == [s, -1, -1, -1, -1, -1] and not np.isnan(value[c, 0]) and np.all(np.isnan(value[c, 1:]))
    for g, gap in ((3, 3), (3, 5), (5, 16)):   # g tags, gap >= g: every tag is in the window after g slots
        tags = (np.arange(n) % g).astype(np.int32)
        order, value = run(v, [0, 250], 40, shape, gpu_lib, tags=tags, gap=gap)
        for c, s in enumerate((0, 250)):
            assert_chain(order[c], value[c], *greedy_mix(row_of, n, 40, seed=s, tags=tags, gap=gap))
            assert np.all(order[c, :g] >= 0) and np.all(order[c, g:] == -1)
    for gap in (1, 3):   # gap + 1 tags: once the window is full exactly one tag is free, a round robin by nearness
        tags = (np.arange(n) % (gap + 1)).astype(np.int32)
        order, value = run(v, [0], n, shape, gpu_lib, tags=tags, gap=gap)
        assert_chain(order[0], value[0], *greedy_mix(row_of, n, n, seed=0, tags=tags, gap=gap))
        t = tags[order[0]]       # the first gap + 1 slots take the tags in order of nearness, then they repeat
        assert order[0].min() >= 0 and len(set(t[:gap + 1])) == gap + 1 and np.array_equal(t[gap + 1:], t[:-(gap + 1)])
    plain = bliss_amd.chain(v, [0, 77], 120)
    order, value = run(v, [0, 77], 120, shape, gpu_lib, tags=np.full(n, -1, dtype=np.int32), gap=16)
    assert order.tobytes() == plain[0].tobytes() and value.tobytes() == plain[1].tobytes()
    tags = np.where(rng.random(n) < 0.5, -3, 7).astype(np.int32)   # untagged songs and one tag
    order, value = run(v, [0, 77], 120, shape, gpu_lib, tags=tags, gap=2)
    for c, s in enumerate((0, 77)):
        assert_chain(order[c], value[c], *greedy_mix(row_of, n, 120, seed=s, tags=tags, gap=2))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("metric", METRICS)
def test_exclusion(gpu_lib, oracle, metric, shape):
    import torch
    rng = np.random.default_rng(45)
    n = 1007
    v = (rng.standard_normal((n, 4)) * 5).astype(np.float32)
    row_of = rows_of(v, metric, oracle)
    ex = np.zeros(n, dtype=bool)
    ex[[0, 31, 32, 63, 64, n - 1]] = True
    seeds = [5, 31, n - 1, 500]     # two of them excluded: they still take slot 0
    order, value = run(v, seeds, n, shape, gpu_lib, metric=metric, exclude=ex)
    for c, s in enumerate(seeds):
        assert_chain(order[c], value[c], *greedy_mix(row_of, n, n, metric, seed=s, exclude=ex))
        real = order[c][order[c] >= 0]
        assert real[0] == s and not ex[real[1:]].any() and len(real) == n - 6 + int(ex[s])
    only = np.ones(n, dtype=bool)
    only[77] = False
    order, value = run(v, [77, 78], 4, shape, gpu_lib, metric=metric, exclude=only)
    assert list(order[0]) == [77, -1, -1, -1] and list(order[1]) == [78, 77, -1, -1]
    assert np.all(np.isnan(value[0, 1:])) and np.all(np.isnan(value[1, 2:]))
    odd = (np.arange(n) % 2 == 1)
    order, value = run(v, [0], n, shape, gpu_lib, metric=metric, exclude=odd)
    assert_chain(order[0], value[0], *greedy_mix(row_of, n, n, metric, seed=0, exclude=odd))
    assert np.all(order[0, :(n + 1) // 2] % 2 == 0) and np.all(order[0, (n + 1) // 2:] == -1)
    d = torch.from_numpy(v).cuda()      # a mask is "non-zero": bytes of 1, bytes of 255, a bool tensor
    outs = []
    with forced(gpu_lib, shape):
        for mask in (torch.from_numpy(ex).cuda(), torch.from_numpy(ex.astype(np.uint8)).cuda(),
                     torch.from_numpy(ex.astype(np.uint8) * 255).cuda()):
            o, x = bliss_amd.mix_device(d, seeds, 60, metric=metric, exclude=mask)
            outs.append((cpu(o), cpu(x)))
    for o, x in outs:
        assert o.tobytes() == outs[0][0].tobytes() and x.tobytes() == outs[0][1].tobytes()
        assert np.array_equal(o[0], greedy_mix(row_of, n, 60, metric, seed=5, exclude=ex)[0])


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("n", [5000, 40000])
def test_continuing_a_chain(gpu_lib, n, shape):
    """40 songs, then 60 more from the last one with the 40 excluded: the single chain of 99, for gap 0 and gap 1"""
    rng = np.random.default_rng(46)
    v = (rng.standard_normal((n, 4)) * 8).astype(np.float32)
    tags = rng.integers(0, 40, size=n).astype(np.int32)
    for metric in METRICS:
        for gap in (0, 1):
            kw = dict(metric=metric, tags=tags, gap=gap)
            whole = run(v, [n // 3], 99, shape, gpu_lib, **kw)
            first = run(v, [n // 3], 40, shape, gpu_lib, **kw)
            played = np.zeros(n, dtype=bool)
            played[first[0][0]] = True
            second = run(v, [int(first[0][0, -1])], 60, shape, gpu_lib, exclude=played, **kw)
            assert np.array_equal(np.concatenate([first[0][0], second[0][0, 1:]]), whole[0][0])
            assert np.concatenate([first[1][0], second[1][0, 1:]]).tobytes() == whole[1][0].tobytes()
            if metric == "distance" and n == 5000:
                assert_chain(whole[0][0], whole[1][0], *greedy_mix(dist_row_of(v), n, 99, seed=n // 3, tags=tags, gap=gap))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("metric", METRICS)
def test_vector_seeds(gpu_lib, oracle, metric, shape):
    rng = np.random.default_rng(47)
    n, length = 1500, 30
    v = (rng.standard_normal((n, 4)) * 5).astype(np.float32)
    v[907] = v[7]
    tags = rng.integers(0, 100, size=n).astype(np.int32)
    tags[907] = tags[7]       # tags play no part at slot 0, and then block the duplicate
    q = np.stack([v[7], v[[10, 20, 30]].mean(axis=0, dtype=np.float32), np.full(4, np.nan, dtype=np.float32),
                  v[1499] * np.float32(2)]).astype(np.float32)
    both = np.concatenate([v, q])
    seed_rows = dist_rows(both, list(range(n, n + len(q))))[:, :n] if metric == "distance" \
        else oracle.cosine_matrix(both)[n:, :n]
    row_of = rows_of(v, metric, oracle)
    ex7 = np.zeros(n, dtype=bool)
    ex7[[7, 0]] = True
    for kw in (dict(), dict(tags=tags, gap=3), dict(exclude=ex7), dict(tags=tags, gap=16, exclude=ex7)):
        order, value = run(v, None, length, shape, gpu_lib, metric=metric, seed_vecs=q, **kw)
        for c in range(len(q)):
            assert_chain(order[c], value[c], *greedy_mix(row_of, n, length, metric, seed_row=seed_rows[c], **kw))
        first = 907 if "exclude" in kw else 7        # the smallest-index duplicate, or the next nearest
        assert order[0, 0] == first and order[2, 0] == (1 if "exclude" in kw else 0)
        if metric == "distance":
            assert value[0, 0].view(np.int32) == 0       # +0
        if "tags" in kw and "exclude" not in kw:
            assert order[0, 1] != 907
    order, value = run(v, None, 5, shape, gpu_lib, metric=metric, seed_vecs=q, exclude=np.ones(n, dtype=bool))
    assert np.all(order == -1) and np.all(np.isnan(value))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", [4096, 1 << 20])
def test_a_chain_does_not_depend_on_the_batch_or_the_shape(gpu_lib, n, metric):
    """one seed alone, in a batch of 2 and in a batch of 1 024, with tags and a mask: byte-identical; then both shapes
    forced on the single chain"""
    import torch
    length = 32
    rng = np.random.default_rng(48)
    v = (rng.standard_normal((n, 4)) * 8).astype(np.float32)
    d = torch.from_numpy(v).cuda()
    tags = torch.from_numpy(rng.integers(-1, 200, size=n).astype(np.int32)).cuda()
    ex = torch.from_numpy(rng.random(n) < 0.3).cuda()
    seed = n // 3
    others = rng.integers(0, n, size=1023).astype(np.int32)
    got = {}
    for batch in (1, 2, 1024):
        seeds = np.concatenate([others[:batch // 2], [seed], others[batch // 2:batch - 1]]).astype(np.int32)
        o, x = bliss_amd.mix_device(d, torch.from_numpy(seeds).cuda(), length, metric=metric, tags=tags, gap=4, exclude=ex)
        got[batch] = (cpu(o)[batch // 2], cpu(x)[batch // 2])
    for shape in SHAPES:
        with forced(gpu_lib, shape):
            assert gpu_lib.bl_amd_chain_shape(n, 1) == shape
            o, x = bliss_amd.mix_device(d, [seed], length, metric=metric, tags=tags, gap=4, exclude=ex)
            got[("forced", shape)] = (cpu(o)[0], cpu(x)[0])
    ref_o, ref_x = got[1]
    assert ref_o[0] == seed and len(set(ref_o)) == length and ref_o.min() >= 0
    assert not cpu(ex)[ref_o[1:]].any()
    for key, (o, x) in got.items():
        assert o.tobytes() == ref_o.tobytes(), key
        assert x.tobytes() == ref_x.tobytes(), key


@pytest.mark.parametrize("metric", METRICS)
def test_played_bits_in_the_workspace_beyond_what_lds_holds(gpu_lib, metric):
    """PER_CHAIN forced at n = 1.5 million with tags and a mask: the bits, initialised from the mask, live in the
    workspace; same bytes as SPLIT, and the distance chain equals the greedy"""
    import torch
    n, length = 1_500_000, 12
    rng = np.random.default_rng(49)
    v = (rng.standard_normal((n, 4)) * 8).astype(np.float32)
    tags = rng.integers(0, 6, size=n).astype(np.int32)
    ex = rng.random(n) < 0.5
    ex[[0, n - 1, n - 2]] = True
    d, dt, dx = torch.from_numpy(v).cuda(), torch.from_numpy(tags).cuda(), torch.from_numpy(ex).cuda()
    seeds = [n - 1, 64]
    out = {}
    for shape in SHAPES:
        with forced(gpu_lib, shape):
            o, x = bliss_amd.mix_device(d, seeds, length, metric=metric, tags=dt, gap=5, exclude=dx)
            out[shape] = (cpu(o), cpu(x))
    assert out[PER_CHAIN][0].tobytes() == out[SPLIT][0].tobytes()
    assert out[PER_CHAIN][1].tobytes() == out[SPLIT][1].tobytes()
    if metric == "distance":
        for c, s in enumerate(seeds):
            assert_chain(out[PER_CHAIN][0][c], out[PER_CHAIN][1][c],
                         *greedy_mix(dist_row_of(v), n, length, seed=s, tags=tags, gap=5, exclude=ex))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("n", [5000, 40000])
def test_side_stream_second_context_and_back_to_back_calls(gpu_lib, n, shape):
    """two calls enqueued back to back on one side stream with different rules (state, history and played bits are
    re-initialised by each call), then the same through a second context of the same device"""
    import torch
    length = 50
    rng = np.random.default_rng(50)
    v = (rng.standard_normal((n, 4)) * 8).astype(np.float32)
    tags = rng.integers(0, 30, size=n).astype(np.int32)
    ex = rng.random(n) < 0.4
    seeds = [17, n - 2]
    q = v[[3, 4]] + np.float32(0.25)
    with forced(gpu_lib, shape):
        want_a = bliss_amd.mix(v, seeds, length, tags=tags, gap=8, exclude=ex)
        want_b = bliss_amd.mix(v, None, length, seed_vecs=q, tags=tags, gap=1)
        assert_chain(want_a[0][0], want_a[1][0], *greedy_mix(dist_row_of(v), n, length, seed=17, tags=tags, gap=8, exclude=ex))
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            d, dt, dx = torch.from_numpy(v).cuda(), torch.from_numpy(tags).cuda(), torch.from_numpy(ex).cuda()
            dq = torch.from_numpy(q).cuda()
            ds = torch.tensor(seeds, dtype=torch.int32, device="cuda")
            oa, xa = bliss_amd.mix_device(d, ds, length, tags=dt, gap=8, exclude=dx, stream=s)
            ob, xb = bliss_amd.mix_device(d, None, length, seed_vecs=dq, tags=dt, gap=1, stream=s)
        s.synchronize()
        for (o, x), (wo, wx) in (((oa, xa), want_a), ((ob, xb), want_b)):
            assert cpu(o).tobytes() == wo.tobytes() and cpu(x).tobytes() == wx.tobytes()
        ctx = C.c_void_p()
        assert gpu_lib.bl_amd_ctx_create(0, C.byref(ctx)) == 0
        try:
            outs = []
            with torch.cuda.stream(s):
                for sd, sv, gap, mask in ((ds, None, 8, dx), (None, dq, 1, None)):
                    o = torch.full((2, length), 7, dtype=torch.int32, device="cuda")
                    x = torch.full((2, length), 3.5, dtype=torch.float32, device="cuda")
                    assert gpu_lib.bl_amd_ctx_mix_device(
                        ctx, d.data_ptr(), n, sd.data_ptr() if sd is not None else None,
                        sv.data_ptr() if sv is not None else None, 2, length, _lib.BL_AMD_KNN_DISTANCE, dt.data_ptr(), gap,
                        mask.data_ptr() if mask is not None else None, o.data_ptr(), x.data_ptr(),
                        C.c_void_p(s.cuda_stream)) == 0
                    outs.append((o, x))
            s.synchronize()
            for (o, x), (wo, wx) in zip(outs, (want_a, want_b)):
                assert cpu(o).tobytes() == wo.tobytes() and cpu(x).tobytes() == wx.tobytes()
        finally:
            gpu_lib.bl_amd_ctx_destroy(ctx)


def test_argument_errors_leave_the_outputs_untouched(gpu_lib):
    import torch
    n, nc, length = 100, 3, 8
    d = torch.randn((n, 4), dtype=torch.float32, device="cuda")
    ds = torch.tensor([0, 5, 99], dtype=torch.int32, device="cuda")
    dq = torch.randn((nc, 4), dtype=torch.float32, device="cuda")
    dt = torch.zeros(n, dtype=torch.int32, device="cuda")
    dx = torch.zeros(n, dtype=torch.uint8, device="cuda")
    oi = torch.full((nc, 2 * length), 7, dtype=torch.int32, device="cuda")
    ov = torch.full((nc, 2 * length), 3.5, dtype=torch.float32, device="cuda")
    V, S, Q, T, X, I, F = (t.data_ptr() for t in (d, ds, dq, dt, dx, oi, ov))
    DIST, COS = _lib.BL_AMD_KNN_DISTANCE, _lib.BL_AMD_KNN_COSINE
    bad = [
        (None, n, S, None, nc, length, DIST, T, 1, X, I, F), (V, n, None, None, nc, length, DIST, T, 1, X, I, F),
        (V, n, S, Q, nc, length, DIST, T, 1, X, I, F), (V, n, S, None, nc, length, DIST, T, 1, X, None, F),
        (V, n, S, None, nc, length, COS, T, 1, X, I, None), (V, 0, S, None, nc, length, DIST, T, 1, X, I, F),
        (V, -4, None, Q, nc, length, DIST, T, 1, X, I, F), (V, n, S, None, 0, length, DIST, T, 1, X, I, F),
        (V, n, None, Q, -1, length, COS, T, 1, X, I, F), (V, n, S, None, nc, 0, DIST, T, 1, X, I, F),
        (V, n, S, None, nc, length, 2, T, 1, X, I, F), (V, n, S, None, nc, length, -1, T, 1, X, I, F),
        (V, n, S, None, nc, length, DIST, T, -1, X, I, F), (V, n, S, None, nc, length, DIST, T, 17, X, I, F),
        (V, n, S, None, nc, length, DIST, None, 1, X, I, F), (V, n, None, Q, nc, length, COS, None, 16, None, I, F),
    ]
    for args in bad:
        assert gpu_lib.bl_amd_mix_device(*args, None) == _lib.BL_UNEXPECTED, args
    assert gpu_lib.bl_amd_ctx_mix_device(None, V, n, S, None, nc, length, DIST, T, 1, X, I, F, None) == _lib.BL_UNEXPECTED
    torch.cuda.synchronize()
    assert torch.all(oi == 7) and torch.all(ov == 3.5)
    hv = np.random.default_rng(9).standard_normal((n, 4)).astype(np.float32)
    hp = hv.ctypes.data_as(C.POINTER(_lib.ForceVector))
    hs = np.array([0, 5, 99], dtype=np.int32)
    sp = hs.ctypes.data_as(C.POINTER(C.c_int32))
    ht = (np.arange(n, dtype=np.int32) % 4)
    tp = ht.ctypes.data_as(C.POINTER(C.c_int32))
    hi = np.full(nc * 2 * length, 7, dtype=np.int32)
    hf = np.full(nc * 2 * length, 3.5, dtype=np.float32)
    ip, fp = hi.ctypes.data_as(C.POINTER(C.c_int32)), hf.ctypes.data_as(C.POINTER(C.c_float))
    badseed = np.array([0, 100, 5], dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    for args in [(hp, n, sp, None, nc, 0, DIST, tp, 1, None, ip, fp), (hp, n, sp, None, nc, length, 5, tp, 1, None, ip, fp),
                 (hp, n, sp, hp, nc, length, DIST, tp, 1, None, ip, fp), (hp, n, None, None, nc, length, DIST, tp, 1, None, ip, fp),
                 (hp, n, sp, None, nc, length, DIST, None, 2, None, ip, fp), (hp, n, sp, None, nc, length, DIST, tp, 17, None, ip, fp),
                 (hp, n, badseed, None, nc, length, DIST, tp, 1, None, ip, fp)]:
        assert gpu_lib.bl_amd_mix_host(*args) == _lib.BL_UNEXPECTED, args
    assert np.all(hi == 7) and np.all(hf == 3.5)
    # h_value may be NULL
    assert gpu_lib.bl_amd_mix_host(hp, n, sp, None, nc, length, DIST, tp, 2, None, ip, None) == _lib.BL_OK
    assert np.array_equal(hi[:nc * length].reshape(nc, length), bliss_amd.mix(hv, hs, length, tags=ht, gap=2)[0])
    assert np.all(hf == 3.5)


def test_mix_device_wants_aligned_seed_vectors(gpu_lib):
    """a contiguous view 4 bytes into a buffer is refused before the call; 16 bytes in, a view into d_vecs, is fine"""
    import torch
    d = torch.randn((64, 4), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        bliss_amd.mix_device(d, None, 4, seed_vecs=d.reshape(-1)[1:9].view(2, 4))
    order, value = bliss_amd.mix_device(d, None, 4, seed_vecs=d[5:7])
    assert cpu(order)[:, 0].tolist() == [5, 6] and cpu(value)[:, 0].view(np.int32).tolist() == [0, 0]
