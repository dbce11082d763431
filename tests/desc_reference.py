"""The descriptor definitions of include/bliss_amd.h (bl_amd_desc_*) in numpy float64 / int64 and Python integers: the
range, the quantiser, the digit split, d^2 both directly and through the four byte-plane products the kernel forms, and
the k nearest neighbours as a sort on (d^2, index).

`bugs` is a set of switches that make a kernel's plausible mistakes on purpose, so that the tests can show that their
cases tell the right arithmetic from each of them (tests/test_desc_reference_host.py):

  fused         the scale folded into 2t - 1 as one fused operation, q = rint(fma(t, 2 scale, -scale)).  (A literal
                fma(2, t, -1) cannot differ from the unfused expression: doubling is exact.)
  half_away     rounding half away from zero instead of to even
  no_clamp      u not clamped to [-1, 1] (the int16 conversion then wraps)
  unsigned_low  the digits h = q >> 8, l = (q & 255) - 128 (q = 256 h + l + 128) without the constant's terms
  hl_only       HL without LH
  swap_rc       row and column of every 16 x 16 tile swapped
  cross_k       the K halves of the mixed product paired crosswise: [h | l] against [h | l], HH + LL for HL + LH
  tie_larger    a tie in d^2 going to the larger index
  keep_self     the self form not excluding the query's own row
  trunc32       d^2 truncated to 32 bits
"""
from fractions import Fraction

import numpy as np

DIMS, SCALE_MAX, IDX_BITS = 32, 32512, 27
EMPTY = 2 ** 64 - 1
BUGS = ("fused", "half_away", "no_clamp", "unsigned_low", "hl_only", "swap_rc", "cross_k", "tie_larger", "keep_self",
        "trunc32")


def desc_range(x):
    """(lo, hi float32 (32,), n_finite uint32 (32,)) of the float32 matrix x[n][d]"""
    x = np.asarray(x, dtype=np.float32)
    lo, hi, cnt = np.zeros(DIMS, np.float32), np.zeros(DIMS, np.float32), np.zeros(DIMS, np.uint32)
    for c in range(x.shape[1]):
        col = x[:, c][np.isfinite(x[:, c])]
        cnt[c] = col.size
        if col.size:
            lo[c], hi[c] = col.min(), col.max()
    return lo + np.float32(0), hi + np.float32(0), cnt   # -0 + 0 = +0


def _rint_even(v):
    return np.rint(v)


def _rint_away(v):
    return np.where(v >= 0, np.floor(v + 0.5), np.ceil(v - 0.5))


def quantize(x, lo, hi, scale=None, bugs=()):
    """int16 (n, 32) descriptors of x[n][d] under the range (lo, hi) and the per-column scale (None: the maximum)"""
    x = np.asarray(x, dtype=np.float32)
    n, d = x.shape
    scale = [SCALE_MAX] * d if scale is None else [int(s) for s in scale]
    assert len(scale) == d and all(0 <= s <= SCALE_MAX for s in scale)
    out = np.zeros((n, DIMS), dtype=np.int16)
    rint = _rint_away if "half_away" in bugs else _rint_even
    for c in range(d):
        l, h = np.float64(lo[c]), np.float64(hi[c])
        if not (np.isfinite(l) and np.isfinite(h) and h > l):
            continue
        ok = np.isfinite(x[:, c])
        xs = x[ok, c].astype(np.float64)
        t = (xs - l) / (h - l)
        if "fused" in bugs:
            if "no_clamp" not in bugs:
                t = np.clip(t, 0.0, 1.0)
            p = np.array([float(Fraction(float(v)) * (2 * scale[c]) - scale[c]) for v in t], dtype=np.float64)
        else:
            u = 2.0 * t - 1.0
            if "no_clamp" not in bugs:
                u = np.clip(u, -1.0, 1.0)
            p = u * np.float64(scale[c])
        q = rint(p)
        out[ok, c] = (q.astype(np.int64) & 0xFFFF).astype(np.uint16).view(np.int16)   # the conversion wraps
    return out


def split(q, bugs=()):
    """(h, l) int64 digit planes of int16 q: q = 256 h + l, h in [-127, 127], l in [-128, 127]"""
    q = np.asarray(q).astype(np.int64)
    if "unsigned_low" in bugs:
        return q >> 8, (q & 255) - 128
    h = (q + 128) >> 8
    return h, q - 256 * h


def d2_direct(a, b):
    """int64 matrix [len(a)][len(b)] of sum_c (a_c - b_c)^2; exact in float64 products: every sum is below 2^53"""
    a64, b64 = np.asarray(a).astype(np.float64), np.asarray(b).astype(np.float64)
    na, nb = (a64 * a64).sum(axis=1), (b64 * b64).sum(axis=1)
    return (na[:, None] + nb[None, :] - 2.0 * (a64 @ b64.T)).astype(np.int64)


def d2_planes(a, b, bugs=()):
    """the same through the byte planes: a . b = 65536 HH + 256 (HL + LH) + LL, d^2 = |a|^2 + |b|^2 - 2 a . b"""
    a, b = np.asarray(a), np.asarray(b)
    (ha, la), (hb, lb) = split(a, bugs), split(b, bugs)
    f = lambda p, q: (p.astype(np.float64) @ q.astype(np.float64).T).astype(np.int64)   # exact: below 2^20
    hh, ll, hl, lh = f(ha, hb), f(la, lb), f(ha, lb), f(la, hb)
    assert max(np.abs(m).max() for m in (hh, ll, hl + lh)) < 2 ** 20
    mixed = hl if "hl_only" in bugs else hh + ll if "cross_k" in bugs else hl + lh
    dot = 65536 * hh + 256 * mixed + ll
    a64, b64 = a.astype(np.int64), b.astype(np.int64)
    d2 = (a64 * a64).sum(axis=1)[:, None] + (b64 * b64).sum(axis=1)[None, :] - 2 * dot
    if "swap_rc" in bugs:
        out = d2.copy()
        for i0 in range(0, d2.shape[0] - 15, 16):
            for j0 in range(0, d2.shape[1] - 15, 16):
                out[i0:i0 + 16, j0:j0 + 16] = d2[i0:i0 + 16, j0:j0 + 16].T
        d2 = out
    if "trunc32" in bugs:
        d2 = d2 & 0xFFFFFFFF
    return d2


def knn(lib, k, queries=None, row_begin=0, n_rows=None, bugs=(), chunk=512):
    """(index int32 (rows, k), d2 uint64 (rows, k)): per query the k candidates with the smallest (d^2, index)"""
    lib = np.asarray(lib)
    n = lib.shape[0]
    assert n < 2 ** IDX_BITS
    self_form = queries is None
    q = lib[row_begin:(n if n_rows is None else row_begin + n_rows)] if self_form else np.asarray(queries)
    rows = q.shape[0]
    index = np.full((rows, k), -1, dtype=np.int32)
    dist2 = np.full((rows, k), EMPTY, dtype=np.uint64)
    idx = np.arange(n, dtype=np.uint64)
    low = (np.uint64(2 ** IDX_BITS - 1) - idx) if "tie_larger" in bugs else idx
    plain = not ({"unsigned_low", "hl_only", "swap_rc", "cross_k", "trunc32"} & set(bugs))
    for r0 in range(0, rows, chunk):
        qq = q[r0:r0 + chunk]
        d2 = d2_direct(qq, lib) if plain else d2_planes(qq, lib, bugs)
        keys = (d2.astype(np.uint64) << np.uint64(IDX_BITS)) | low[None, :]
        if self_form and "keep_self" not in bugs:
            own = row_begin + r0 + np.arange(qq.shape[0])
            keys[np.arange(qq.shape[0]), own] = np.uint64(EMPTY)
        kk = min(k, n)
        part = np.sort(np.partition(keys, kk - 1, axis=1)[:, :kk], axis=1)
        live = part != np.uint64(EMPTY)
        lowbits = part & np.uint64(2 ** IDX_BITS - 1)
        cand = (np.uint64(2 ** IDX_BITS - 1) - lowbits) if "tie_larger" in bugs else lowbits
        index[r0:r0 + qq.shape[0], :kk] = np.where(live, cand.astype(np.int64), -1).astype(np.int32)
        dist2[r0:r0 + qq.shape[0], :kk] = np.where(live, part >> np.uint64(IDX_BITS), np.uint64(EMPTY))
    return index, dist2


def one_hot_sets():
    """The tile-layout case: (a, b), 32 descriptors each with one non-zero dimension and distinct values in both digits.
    a[i] carries dimension i with 257 i + 3 (h = i, l = i + 3); b[j] carries dimension (7 j + 3) % 32 with 259 j + 11.
    a[i] . b[j] is non-zero exactly where the dimensions meet, once per row and once per column and nowhere symmetric,
    so a swapped tile, a wrong K pairing or a dropped product moves a known entry of the cross matrix."""
    a, b = np.zeros((32, DIMS), np.int16), np.zeros((32, DIMS), np.int16)
    for i in range(32):
        a[i, i] = 257 * i + 3
        b[i, (7 * i + 3) % 32] = 259 * i + 11
    return a, b
