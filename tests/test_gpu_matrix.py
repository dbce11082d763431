"""The oldest vector kernels on the device, each against a plain reference of the same operation: k_pairwise (the
N x N bl_distance / bl_cosine_similarity matrix, bl_amd_*_matrix_*) against the oracle's matrix, and k_seed_dist /
k_seed_dist_vec / k_rank_order (the seeded playlist, bl_amd_playlist_* and bl_amd_playlist_vec_*) against the oracle's
row and np.argsort(row, kind="stable").  The vector queries define their values as "the bits of the matrix entry", so
this is the ground they stand on.

One comparison rule everywhere: where the reference is NaN the result is NaN, everywhere else the int32 views are
equal.  No tolerance.

What the shapes are for (k_pairwise: a workgroup is 16 rows x 1024 columns, a wave 256 columns, a thread 4 columns;
16-byte stores only where n % 4 == 0 and the output is 16-byte aligned, per-element stores, a clamped load and a
partial last thread otherwise; the root of the distance is chosen per wave):
  a. ragged n, full matrix, both entry points            the per-element path at one, two and three column blocks
  b. planted tiny / huge / non-finite vectors, n = 1027  waves whose lanes are partly outside the fast root's domain
  c. row ranges into guarded buffers                     out is indexed relative to the range; unaligned outputs
  d. argument errors
  e. the playlist with NaN, infinite and tied distances  k_rank_order's 256-wide tile and its remainder

Not covered: blk_pairwise splits its launches at 65 535 x 16 rows.  A range that long needs an output of about 4 TB,
so that seam stays untested.
"""
import ctypes as C

import numpy as np
import pytest

import bliss_amd
from bliss_amd import _lib

pytestmark = pytest.mark.gpu

METRICS = ("distance", "cosine")
GUARD = 64                  # int32 / float slots in front of and behind every device output: 256 bytes, so the
                            # payload keeps the 16-byte alignment of the allocation
SENT = 0x7FA5C3E1           # fill of the matrix outputs: a NaN pattern no kernel writes (theirs are the default NaN
                            # or an input's), told apart by its bits
LO, HI = np.float32(2.0 ** -100), np.float32(2.0 ** 126)        # bl_sqrt.h: the domain of the five-instruction root


def assert_same(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), np.argwhere(np.isnan(got) != nan)[:5]
    bad = (got.view(np.int32) != want.view(np.int32)) & ~nan
    assert not bad.any(), (np.argwhere(bad)[:5], got[bad][:5], want[bad][:5])


class Guarded:
    """`count` 4-byte slots on the device holding `fill`, with GUARD + shift slots of `guard` in front (shift moves the
    payload off the 16-byte grid) and GUARD + tail slots behind"""

    def __init__(self, count, fill=SENT, guard=SENT, shift=0, tail=0):
        import torch
        self.lo, self.hi, self.guard, self.fill = GUARD + shift, GUARD + shift + count, guard, fill
        self.buf = torch.full((self.hi + tail + GUARD,), guard, dtype=torch.int32, device="cuda")
        self.buf[self.lo:self.hi] = fill
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = self.buf.data_ptr() + 4 * self.lo

    def payload(self):
        """the payload as int32 after a device synchronise; asserts that both guards are as they were"""
        import torch
        torch.cuda.synchronize()
        h = self.buf.cpu().numpy()
        assert np.all(h[:self.lo] == self.guard), np.flatnonzero(h[:self.lo] != self.guard)[:5]
        assert np.all(h[self.hi:] == self.guard), np.flatnonzero(h[self.hi:] != self.guard)[:5]
        return h[self.lo:self.hi]

    def floats(self, shape):
        """... as floats, every one of them written"""
        p = self.payload()
        assert not np.any(p == self.fill), np.flatnonzero(p == self.fill)[:5]
        return p.view(np.float32).reshape(shape)

    def untouched(self):
        return bool(np.all(self.payload() == self.fill))


def matrix_fn(lib, metric):
    return lib.bl_amd_distance_matrix_device if metric == "distance" else lib.bl_amd_cosine_matrix_device


def matrix_rows(lib, dv, n, row_begin, n_rows, metric, shift=0, tail=0, stream=None):
    out = Guarded(n_rows * n, shift=shift, tail=tail)
    s = None
    if stream is not None:
        import torch
        torch.cuda.synchronize()            # the fill of the buffer ran on the default stream
        s = C.c_void_p(stream.cuda_stream)
    assert matrix_fn(lib, metric)(dv.data_ptr(), n, row_begin, n_rows, out.ptr, s) == _lib.BL_OK
    if stream is not None:
        stream.synchronize()
    return out.floats((n_rows, n))


def ragged_vectors(n):
    """ordinary force vectors with an exact duplicate (an off-diagonal zero) where there is room for one"""
    v = (np.random.default_rng(500 + n).standard_normal((n, 4)) * 10).astype(np.float32)
    if n > 2:
        v[n - 1] = v[n // 3]
    v.setflags(write=False)
    return v


def planted_vectors():
    """n = 1027.  The specials are songs 8..64 and 1024..1026, so as rows they are a few, and as columns they lie in
    the wave spans 0..255 and 1024..1026; songs 256..1023 are ordinary."""
    n = 1027
    v = (np.random.default_rng(7).standard_normal((n, 4)) * 10).astype(np.float32)
    v[8:16] *= np.float32(1e-25)             # among themselves: every product underflows, the sums are exact zeros
    v[16:32] *= np.float32(1e-22)            # among themselves and against 8..15: subnormal sums
    v[32:40] *= np.float32(1e19)             # against anything: a product overflows, the sums are +inf
    # sums built exactly around both ends of the fast root's domain: song 40 and copies of it that differ in one
    # component, by t; the sum of the pair (40, 41 + k) is the f32 square of t[k] and nothing else
    t = [2.0 ** -50 * (1 - 2.0 ** -23), 2.0 ** -50, 2.0 ** -50 * (1 + 2.0 ** -23),
         2.0 ** 63 * (1 - 2.0 ** -23), 2.0 ** 63, 2.0 ** 63 * (1 + 2.0 ** -23)]
    v[40:47] = [1.5, -2, 0.25, 0]
    v[41:47, 3] = np.array(t, dtype=np.float64).astype(np.float32)
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    v[48] = [inf, 1, 2, 3]
    v[49] = [inf, -1, 0, 2]                  # against 48: inf - inf
    v[50] = [-inf, 0, 0, 0]
    v[51] = [1, nan, 2, 3]
    v[60] = v[300]; v[61] = v[300]           # exact duplicates of an ordinary song ...
    v[62] = [0.0, -0.0, 5, 0.0]
    v[63] = [-0.0, 0.0, 5, -0.0]             # ... and of each other up to the sign of zero
    v[64] = 0
    v[1024] = v[700]                         # the last, partial thread: a duplicate, a huge and a tiny song
    v[1025] *= np.float32(1e19)
    v[1026] *= np.float32(1e-22)
    v.setflags(write=False)
    return v


@pytest.fixture(scope="module")
def ref(oracle):
    """(vectors, oracle matrix) by name and metric, computed once and read-only.  Names: an int n for
    ragged_vectors(n), "planted" for planted_vectors()."""
    vecs, mats = {}, {}

    def get(name, metric):
        if name not in vecs:
            vecs[name] = planted_vectors() if name == "planted" else ragged_vectors(name)
        if (name, metric) not in mats:
            m = oracle.distance_matrix(vecs[name]) if metric == "distance" else oracle.cosine_matrix(vecs[name])
            m.setflags(write=False)
            mats[name, metric] = m
        return vecs[name], mats[name, metric]
    return get


# ---------------------------------------------------------------------------- a. ragged sizes

@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 15, 16, 17, 1021, 1024, 1025, 1027, 2051])
def test_ragged_sizes_against_the_oracle(gpu_lib, ref, n, metric):
    """one thread, one partial thread, a partial 16-row block, exactly one column block, one column past it, n % 4 of
    1 and 3 with two and three column blocks; n % 16 != 0 nearly throughout"""
    import torch
    v, want = ref(n, metric)
    host = bliss_amd.distance_matrix(v) if metric == "distance" else bliss_amd.cosine_matrix(v)
    assert_same(host, want)
    dv = torch.from_numpy(np.array(v)).cuda()       # a copy: the shared vectors are read-only
    assert_same(matrix_rows(gpu_lib, dv, n, 0, n, metric), want)
    if metric == "distance" and n > 2:
        assert want[n - 1, n // 3] == 0 and np.all(np.diag(want) == 0)


# ---------------------------------------------------------------------------- b. mixed scales, non-finite values

def test_planted_vectors_reach_both_roots_in_one_matrix(ref):
    """On the reference alone: the planted set does put waves with every lane inside the fast root's domain next to
    waves that mix lanes inside and outside it, and the matrix holds every kind of value the two roots differ on.
    A wave of k_pairwise is one row and the 256 columns of a span (the last span is one thread: columns 1024..1026)."""
    v, want = ref("planted", "distance")
    n = len(v)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        d = v[:, None, :] - v[None, :, :]
        s = d[..., 0] * d[..., 0]
        for c in (1, 2, 3):
            s = s + d[..., c] * d[..., c]                        # f32 throughout, left to right
        assert s.dtype == np.float32
        assert_same(np.sqrt(s), want)                            # these are the sums the oracle takes its roots of
        inside = (s >= LO) & (s <= HI)                           # false for NaN
    spans = [(0, 256), (256, 512), (512, 768), (768, 1024), (1024, n)]
    all_in = np.stack([inside[:, a:b].all(axis=1) for a, b in spans], axis=1)
    mixed = np.stack([inside[:, a:b].any(axis=1) for a, b in spans], axis=1) & ~all_in
    ordinary = np.arange(256, 1024)
    assert np.all(all_in[ordinary][:, 1:4].sum(axis=1) == 2)     # all but the span with the row's own diagonal
    assert mixed[ordinary, 0].all()                              # the specials among columns 0..255
    assert mixed[ordinary, 4].all()                              # the last thread: 1026 inside, 1025 outside
    assert mixed[8:65].any() and all_in[8:65].any()              # special rows have both kinds as well
    # the lanes outside are outside for every reason: in mixed waves of ordinary rows an infinite, a NaN and a finite
    # sum above the domain; in mixed waves of the tiny rows zeros, subnormals and normal sums below the domain
    sp = s[ordinary][:, :256]
    assert np.isinf(sp).any() and np.isnan(sp).any() and ((sp > HI) & np.isfinite(sp)).any()
    assert np.isinf(s[ordinary][:, 1024:]).any()
    sp = s[8:32, :256]
    assert mixed[8:32, 0].all() and (sp[:, 8:16] == 0).any() and ((sp > 0) & (sp < 2.0 ** -126)).any()
    assert mixed[40, 0] and 2.0 ** -126 < s[40, 41] < LO
    off = ~np.eye(n, dtype=bool)
    assert ((want == 0) & off).sum() >= 8 * 7                    # the underflowed pairs (and the duplicates)
    assert np.isinf(want).any() and np.isnan(want).any()
    assert ((want > 0) & (want < 2.0 ** -50)).any()
    assert ((s > 0) & (s < 2.0 ** -126)).sum() >= 16 * 15        # subnormal sums
    assert s[40, 41] == LO * np.float32(1 - 2.0 ** -22) and s[40, 42] == LO and s[40, 43] == LO * np.float32(1 + 2.0 ** -22)
    assert s[40, 44] == HI * np.float32(1 - 2.0 ** -22) and s[40, 45] == HI and s[40, 46] == HI * np.float32(1 + 2.0 ** -22)
    assert np.isfinite(s[40, 46])
    assert np.isnan(want[48, 49]) and np.isinf(want[48, 50]) and np.isnan(want[51]).all()
    assert want[62, 63] == 0 and want[60, 61] == 0 and want[1024, 700] == 0


@pytest.mark.parametrize("metric", METRICS)
def test_planted_vectors_against_the_oracle(gpu_lib, ref, metric):
    v, want = ref("planted", metric)
    got = bliss_amd.distance_matrix(v) if metric == "distance" else bliss_amd.cosine_matrix(v)
    assert_same(got, want)


# ---------------------------------------------------------------------------- c. row ranges

def ranges_of(n):
    return [(0, 1), (1, 1), (n - 1, 1), (7, 16), (15, 18), (16, 16), (n - 17, 17), (0, n)]


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", [1027, 1024])
def test_row_ranges_equal_the_full_matrix(gpu_lib, ref, n, metric):
    """Ranges that start and end inside a 16-row block, each into its own buffer: n_rows * n floats are written and
    nothing else.  The buffer goes on behind the range for as long as the full matrix would (still holding the guard
    value), so rows written at their matrix position instead of their position in the range are seen, not lost.
    At n = 1024 the output is also moved 4, 8 and 12 bytes off the 16-byte grid: legal, and the same bytes."""
    import torch
    v, want = ref(n, metric)
    full = bliss_amd.distance_matrix(v) if metric == "distance" else bliss_amd.cosine_matrix(v)
    assert_same(full, want)
    dv = torch.from_numpy(np.array(v)).cuda()       # a copy: the shared vectors are read-only
    for shift in (0, 1, 2, 3) if n == 1024 else (0,):
        for b, r in ranges_of(n):
            got = matrix_rows(gpu_lib, dv, n, b, r, metric, shift=shift, tail=(n - r) * n)
            assert np.array_equal(got.view(np.int32), full[b:b + r].view(np.int32)), (shift, b, r)
    torch.cuda.synchronize()
    side = matrix_rows(gpu_lib, dv, n, 15, 18, metric, tail=(n - 18) * n, stream=torch.cuda.Stream())
    assert np.array_equal(side.view(np.int32), full[15:33].view(np.int32))


# ---------------------------------------------------------------------------- d. argument errors

@pytest.mark.parametrize("metric", METRICS)
def test_matrix_argument_errors_leave_the_output_untouched(gpu_lib, metric):
    import torch
    n = 40
    dv = torch.randn((n, 4), dtype=torch.float32, device="cuda")
    out = Guarded(n * n)
    V, O = dv.data_ptr(), out.ptr
    fn = matrix_fn(gpu_lib, metric)
    for args in [(V, 0, 0, 1, O), (V, -5, 0, 1, O), (V, n, 0, 0, O), (V, n, 3, -2, O), (V, n, -1, 4, O),
                 (V, n, n, 1, O), (V, n, n - 3, 4, O), (V, n, 1, n, O), (None, n, 0, n, O), (V, n, 0, n, None)]:
        assert fn(*args, None) == _lib.BL_UNEXPECTED, args
    assert out.untouched()
    assert fn(V, n, n - 3, 3, O, None) == _lib.BL_OK             # the same buffer is a good one
    assert not np.any(out.payload()[:3 * n] == SENT) and np.all(out.payload()[3 * n:] == SENT)


# ---------------------------------------------------------------------------- e. playlist order

E = np.float32(2.0 ** -10)
SEED_SONG = 3


def playlist_library(n):
    """Songs far from the origin; song SEED_SONG is the origin itself.  Planted, where n has room: NaN songs (first
    and last among them), songs at infinite distance, exact duplicates of the seed, and two songs whose sums differ
    but whose roots round to the same float, the larger sum at the smaller index."""
    v = (np.random.default_rng(900 + n).standard_normal((n, 4)) * 8 + 20).astype(np.float32)
    if n > 250:
        v[SEED_SONG] = 0
        v[[50, 200]] = 0                                  # duplicates of the seed
        v[20] = [3, E, E, 0]                              # sum 9 + 2^-19
        v[120] = [3, E, 0, 0]                             # sum 9 + 2^-20: the same rounded root
        v[7] = [np.inf, 0, 0, 0]
        v[130] = [1, 2, -np.inf, 4]
        v[[0, 100, 101, n // 2, n - 1], [1, 0, 3, 2, 0]] = np.nan
    return v


def ref_row(oracle, v, seed_vec):
    """bl_distance(seed, v[j]) for every j with the seed the first operand: the last row of the oracle's matrix of
    v || seed"""
    m = oracle.distance_matrix(np.concatenate([v, np.asarray(seed_vec, dtype=np.float32)[None, :]]))
    return np.ascontiguousarray(m[len(v), :len(v)])


def playlist_forms(lib, v, seed_index, seed_vec):
    """(name, order, dist) of every form: device (d_order pre-filled with -1) and host, by index (if seed_index is not
    None) and by vector"""
    import torch
    n = len(v)
    dv = torch.from_numpy(v).cuda()
    sv = _lib.ForceVector(*(float(x) for x in seed_vec))
    forms = []
    for name in ("playlist_device", "playlist_vec_device"):
        if name == "playlist_device" and seed_index is None:
            continue
        order, dist = Guarded(n, fill=-1, guard=-7), Guarded(n)
        if name == "playlist_device":
            rc = lib.bl_amd_playlist_device(dv.data_ptr(), n, seed_index, order.ptr, dist.ptr, None)
        else:
            rc = lib.bl_amd_playlist_vec_device(dv.data_ptr(), n, sv, order.ptr, dist.ptr, None)
        assert rc == _lib.BL_OK
        forms.append((name, order.payload().copy(), dist.floats((n,)).copy()))
    if seed_index is not None:
        forms.append(("playlist", *bliss_amd.playlist(v, seed_index)))
    forms.append(("playlist_vec", *bliss_amd.playlist_vec(v, seed_vec)))
    return forms


def assert_playlist(forms, want_dist):
    n = len(want_dist)
    want_order = np.argsort(want_dist, kind="stable").astype(np.int32)
    for name, order, dist in forms:
        assert order.dtype == np.int32 and order.shape == (n,), name
        assert np.array_equal(np.sort(order), np.arange(n)), \
            (name, "not a permutation", "unwritten (-1) slots:", np.flatnonzero(order == -1)[:8],
             "songs missing:", np.setdiff1d(np.arange(n), order)[:8])
        assert np.array_equal(order, want_order), (name, np.flatnonzero(order != want_order)[:8])
        assert_same(dist, want_dist)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_playlist_order_with_nan_infinite_and_tied_distances(gpu_lib, oracle, n):
    v = playlist_library(n)
    s = SEED_SONG if n > 250 else 0
    want = ref_row(oracle, v, v[s])
    if n > 250:
        nan_songs = [0, 100, 101, n // 2, n - 1]
        assert np.flatnonzero(np.isnan(want)).tolist() == sorted(nan_songs)
        assert np.isinf(want[7]) and np.isinf(want[130]) and np.all(want[[3, 50, 200]] == 0)
        assert want[20] == want[120] == np.nextafter(np.float32(3), np.float32(4))
        o = np.argsort(want, kind="stable")
        assert o[:5].tolist() == [3, 50, 200, 20, 120] and o[-7:].tolist() == [7, 130] + sorted(nan_songs)
    assert_playlist(playlist_forms(gpu_lib, v, s, v[s]), want)
    # a seed that is no song of the library: no planted tie, the same NaN, infinite and duplicate songs
    outside = np.float32([1.5, -2, 0.25, 7])
    assert_playlist(playlist_forms(gpu_lib, v, None, outside), ref_row(oracle, v, outside))


@pytest.mark.parametrize("n", [1, 257])
def test_a_nan_seed_lists_the_songs_by_index(gpu_lib, oracle, n):
    v = playlist_library(n).copy()
    v[0, 2] = np.nan
    want = ref_row(oracle, v, v[0])
    assert np.isnan(want).all()
    forms = playlist_forms(gpu_lib, v, 0, v[0]) + playlist_forms(gpu_lib, v, None, np.float32([np.nan, 1, 2, 3]))
    assert_playlist(forms, want)
    for name, order, dist in forms:
        assert np.array_equal(order, np.arange(n)), name


@pytest.mark.parametrize("n", [256, 513])
def test_a_library_of_nan_songs_but_the_seed(gpu_lib, oracle, n):
    v = (np.random.default_rng(77).standard_normal((n, 4)) * 8).astype(np.float32)
    s = n - 2
    v[:, 1] = np.nan
    v[s, 1] = 0.5
    want = ref_row(oracle, v, v[s])
    assert want[s] == 0 and np.isnan(np.delete(want, s)).all()
    forms = playlist_forms(gpu_lib, v, s, v[s])
    assert_playlist(forms, want)
    for name, order, dist in forms:
        assert order[0] == s and np.array_equal(order[1:], np.delete(np.arange(n), s)), name
