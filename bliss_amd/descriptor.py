"""Library-normalised descriptors and exact nearest neighbours over them (include/bliss_amd.h: bl_amd_desc,
bl_amd_desc_range, bl_amd_desc_*): up to 32 features per song, every column mapped onto the same int16 range by the
library's own minimum and maximum, and the squared Euclidean distance of two descriptors as an exact integer.

    x, names = features(results, levels=lv, timbre=tb, rhythm=rh, chroma=ch, mel=ml)
    desc, rng = fit(x)                      # the library
    index, dist2 = knn(desc, 10)            # its ten nearest songs per song
    q = quantize(x_new, rng)                # songs from outside, with the library's range
    index, dist2 = knn(desc, 10, queries=q)
    order, dist2 = chain(desc, seeds, 50, tags=artists, gap=3)   # playlists: no artist twice within 3 slots
    attrs, rule = hmix_attrs(rhythm=rh, chroma=ch), camelot_rule(60, half_double=True)
    order, dist2 = hmix(desc, attrs, rule, seeds, 50)            # harmonic mixes: compatible key, tempo within 6 %

This module is imported explicitly (`import bliss_amd.descriptor`): the package's own namespace is unchanged."""
import ctypes as C

import numpy as np

from . import _lib
from ._args import desc_scale, feature_matrix, int_in, seeds_array
from ._lib import check
from .records import (CHROMA_DTYPE, LEVELS_DTYPE, MEL_DTYPE, RESULT_DTYPE, RHYTHM_DTYPE, TIMBRE_SONG_DTYPE, levels_db,
                      timbre_hz)

DIMS, SCALE_MAX = _lib.BL_AMD_DESC_DIMS, _lib.BL_AMD_DESC_SCALE_MAX
MAX_N = 1 << 27          # a kNN library stays below it: the index bits of a key
EMPTY_DIST2 = 2 ** 64 - 1  # d2 of an empty slot (index -1)
DESC_DTYPE = np.dtype(_lib.Desc)            # one field q: int16 (32,)
RANGE_DTYPE = np.dtype(_lib.DescRange)      # lo, hi float32 (32,), n_finite uint32 (32,)
HMIX_ATTR_DTYPE = np.dtype(_lib.HmixAttr)   # tempo uint16 (1/100 BPM, 0 unknown), key uint8 (>= 24 unknown), reserved
HMIX_RULE_DTYPE = np.dtype(_lib.HmixRule)   # key_ok uint32 (24,), tempo_tol uint32, flags uint32

_I32, _U64 = C.POINTER(C.c_int32), C.POINTER(C.c_uint64)
_F32, _DESC, _RANGE = C.POINTER(C.c_float), C.POINTER(_lib.Desc), C.POINTER(_lib.DescRange)
_ATTR, _RULE = C.POINTER(_lib.HmixAttr), C.POINTER(_lib.HmixRule)


def _desc_array(name, desc):
    """desc as a contiguous int16 (n, 32) array, n >= 1"""
    a = np.ascontiguousarray(desc)
    if a.dtype == DESC_DTYPE and a.ndim == 1:
        a = a["q"]
    if a.dtype != np.int16 or a.ndim != 2 or a.shape[1] != DIMS or a.shape[0] < 1:
        raise ValueError(f"{name} must be int16 of shape (n, {DIMS}) with n >= 1, got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a)


def _range_record(rng):
    r = np.ascontiguousarray(rng)
    if r.dtype != RANGE_DTYPE or r.size != 1:
        raise ValueError("range must be one bl_amd_desc_range record, as fit() returns it")
    return r.reshape(1).copy()


def _build(x, scale, fit_range, rng):
    a = feature_matrix("x", x, DIMS)
    n, d = a.shape
    sc = desc_scale(scale, d, SCALE_MAX)
    out = np.empty((n, DIMS), dtype=np.int16)
    check(_lib.load().bl_amd_desc_build_host(a.ctypes.data_as(_F32), n, d, sc, 1 if fit_range else 0,
                                             rng.ctypes.data_as(_RANGE), out.ctypes.data_as(_DESC)),
          "bl_amd_desc_build_host")
    return out


def fit(x, scale=None):
    """Fit the per-column range on the (n, d) float32 feature matrix x, 1 <= d <= 32, and quantise x with it
    (bl_amd_desc_build_host): (desc int16 (n, 32), range record).  Non-finite entries are ignored by the range and
    quantise to 0, as does a constant column.  scale: None (every column at 32512), one integer for all columns or d of
    them in [0, 32512]: a column's weight in the distance."""
    rng = np.zeros(1, dtype=RANGE_DTYPE)
    return _build(x, scale, True, rng), rng[0]


def quantize(x, range, scale=None):
    """Quantise x with a range fitted elsewhere (fit()[1]): values outside it are clamped to -scale / +scale."""
    return _build(x, scale, False, _range_record(range))


def knn(desc, k, queries=None):
    """The k nearest descriptors of every row of desc (queries None: a row is no candidate of its own) or of every row
    of queries (nothing excluded): (index (rows, k) int32, dist2 (rows, k) uint64), ascending by (dist2, index).  Slots
    beyond the number of candidates hold -1 and 2^64 - 1.  k in [1, 128], fewer than 2^27 library rows."""
    lib = _desc_array("desc", desc)
    k = int_in("k", k, 1, _lib.BL_AMD_KNN_MAX_K)
    n = lib.shape[0]
    if n >= MAX_N:
        raise ValueError(f"desc must have fewer than {MAX_N} rows, got {n}")
    q = None if queries is None else _desc_array("queries", queries)
    rows = n if q is None else q.shape[0]
    index, dist2 = np.empty((rows, k), dtype=np.int32), np.empty((rows, k), dtype=np.uint64)
    check(_lib.load().bl_amd_desc_knn_host(None if q is None else q.ctypes.data_as(_DESC), rows, lib.ctypes.data_as(_DESC),
                                           n, k, index.ctypes.data_as(_I32), dist2.ctypes.data_as(_U64)),
          "bl_amd_desc_knn_host")
    return index, dist2


def _device_desc_check(name, t):
    import torch
    if t.dtype != torch.int16 or not t.is_cuda or not t.is_contiguous() or t.dim() != 2 or t.shape[1] != DIMS or \
            t.shape[0] < 1:
        raise ValueError(f"{name} must be a contiguous int16 CUDA tensor of shape (n, {DIMS}) with n >= 1")


def _on_device(lib, tensor, stream):
    from .queries import _on_device_of
    return _on_device_of(lib, tensor, stream)


def fit_device(d_x, scale=None, stream=None):
    """fit() on a contiguous float32 (n, d) CUDA tensor (bl_amd_desc_range_device, bl_amd_desc_quantize_device),
    asynchronously on `stream`: (desc int16 (n, 32) CUDA tensor, range as a uint8 CUDA tensor of 384 bytes)."""
    import torch
    rng = torch.empty(RANGE_DTYPE.itemsize, dtype=torch.uint8, device=d_x.device)
    return quantize_device(d_x, rng, scale, stream, _fit=True), rng


def quantize_device(d_x, d_range, scale=None, stream=None, _fit=False):
    """quantize() on the device: d_range the uint8 CUDA tensor fit_device() returned."""
    import torch
    if d_x.dtype != torch.float32 or not d_x.is_cuda or not d_x.is_contiguous() or d_x.dim() != 2 or \
            d_x.shape[0] < 1 or not 1 <= d_x.shape[1] <= DIMS:
        raise ValueError(f"d_x must be a contiguous float32 CUDA tensor of shape (n, d) with 1 <= d <= {DIMS}")
    if d_range.dtype != torch.uint8 or d_range.numel() != RANGE_DTYPE.itemsize or d_range.device != d_x.device or \
            not d_range.is_contiguous():
        raise ValueError("d_range must be the uint8 CUDA tensor of one bl_amd_desc_range on d_x's device")
    n, d = d_x.shape
    sc = desc_scale(scale, d, SCALE_MAX)
    lib = _lib.load()
    out = torch.empty((n, DIMS), dtype=torch.int16, device=d_x.device)
    with _on_device(lib, d_x, stream) as cur:
        s = C.c_void_p(cur.cuda_stream)
        if _fit:
            check(lib.bl_amd_desc_range_device(d_x.data_ptr(), n, d, d_range.data_ptr(), s), "bl_amd_desc_range_device")
        check(lib.bl_amd_desc_quantize_device(d_x.data_ptr(), n, d, d_range.data_ptr(), sc, out.data_ptr(), s),
              "bl_amd_desc_quantize_device")
    return out


def knn_device(d_desc, k, queries=None, row_begin=0, n_rows=None, stream=None, ctx=None):
    """knn() on torch tensors: d_desc a contiguous int16 (n, 32) CUDA tensor.  queries None: the rows
    [row_begin, row_begin + n_rows) of d_desc (default: all) are the queries; otherwise `queries` is a tensor like
    d_desc on the same device (row_begin and n_rows must be left alone).  Returns (index int32, dist2 as int64 bits of
    the uint64: an empty slot reads -1) CUDA tensors of shape (rows, k), asynchronously on `stream` (default: the
    current stream of that device).  ctx: an explicit Context."""
    import torch
    _device_desc_check("d_desc", d_desc)
    k = int_in("k", k, 1, _lib.BL_AMD_KNN_MAX_K)
    n = d_desc.shape[0]
    if n >= MAX_N:
        raise ValueError(f"d_desc must have fewer than {MAX_N} rows, got {n}")
    if queries is None:
        from .queries import _rows_check
        rows = _rows_check(n, int_in("row_begin", row_begin, 0), n_rows)
        name, args = "desc_knn_device", (d_desc.data_ptr(), n, int(row_begin), int(rows), k)
    else:
        _device_desc_check("queries", queries)
        if queries.device != d_desc.device or row_begin != 0 or n_rows is not None:
            raise ValueError("queries must be on d_desc's device, and a cross query takes no row range")
        rows = queries.shape[0]
        name, args = "desc_cross_knn_device", (queries.data_ptr(), int(rows), d_desc.data_ptr(), n, k)
    lib = _lib.load()
    index = torch.empty((rows, k), dtype=torch.int32, device=d_desc.device)
    dist2 = torch.empty((rows, k), dtype=torch.int64, device=d_desc.device)
    with _on_device(lib, d_desc, stream) as cur:
        tail = (index.data_ptr(), dist2.data_ptr(), C.c_void_p(cur.cuda_stream))
        if ctx is None:
            check(getattr(lib, "bl_amd_" + name)(*args, *tail), "bl_amd_" + name)
        else:
            check(getattr(lib, "bl_amd_ctx_" + name)(ctx.handle, *args, *tail), "bl_amd_ctx_" + name)
    return index, dist2


def _chain_seeds_check(seeds, seed_desc):
    if (seeds is None) == (seed_desc is None):
        raise ValueError("exactly one of seeds and seed_desc must be given")


def _chain_ints(length, gap, tags):
    length = int_in("length", length, 1)
    gap = int_in("gap", gap, 0, _lib.BL_AMD_MIX_MAX_GAP)
    if gap > 0 and tags is None:
        raise ValueError("gap > 0 needs tags")
    return length, gap


def _hmix_args(attrs, rule, n, device=None):
    """(attrs or None, the rule as a one-record array) of a hmix call after its checks: a rule that applies a test needs
    n attributes, as an array of HMIX_ATTR_DTYPE (device None) or a uint8 (n, 4) / int32 (n,) tensor on `device`"""
    r = np.ascontiguousarray(rule)
    if r.dtype != HMIX_RULE_DTYPE or r.size != 1:
        raise ValueError("rule must be one bl_amd_hmix_rule record, as camelot_rule() returns it")
    r = r.reshape(1).copy()
    flags, tol = int(r["flags"][0]), int(r["tempo_tol"][0])
    if flags & ~7 or (flags & _lib.BL_AMD_HMIX_HALF_DOUBLE and not flags & _lib.BL_AMD_HMIX_TEMPO) or tol > 1000:
        raise ValueError(f"rule has flags {flags} and tempo_tol {tol}: flags are KEY | TEMPO | HALF_DOUBLE (the last only "
                         "with TEMPO) and tempo_tol is 0 .. 1000 per mille")
    if attrs is None:
        if flags & (_lib.BL_AMD_HMIX_KEY | _lib.BL_AMD_HMIX_TEMPO):
            raise ValueError("a rule that applies a test needs attrs")
    elif device is None:
        attrs = np.ascontiguousarray(attrs)
        if attrs.dtype != HMIX_ATTR_DTYPE or attrs.shape != (n,):
            raise ValueError(f"attrs must be {n} bl_amd_hmix_attr records (hmix_attrs), got {attrs.dtype} {attrs.shape}")
    else:
        import torch
        if not isinstance(attrs, torch.Tensor) or not attrs.is_contiguous() or attrs.device != device or \
                (attrs.dtype, tuple(attrs.shape)) not in ((torch.uint8, (n, 4)), (torch.int32, (n,))):
            raise ValueError(f"attrs must be a contiguous uint8 ({n}, 4) or int32 ({n},) tensor on the device of d_desc")
    return attrs, r


def chain(desc, seeds, length, tags=None, gap=0, exclude=None, seed_desc=None):
    """Playlist chains over descriptors (bl_amd_desc_chain_host), one per seed: slot 0 is the seed and every next slot
    the allowed song nearest to the previous one by (dist2, index).  A song is allowed if the chain has not played it,
    exclude (n bools or bytes) does not mask it, and its tag (tags: n integers such as artist ids, negative = untagged)
    is not the tag of one of the last `gap` slots (0 <= gap <= 16; 0 ignores the tags).  seed_desc: (m, 32) int16
    descriptors instead of seeds (pass seeds=None): slot 0 is the nearest song not excluded.  An index seed takes slot 0
    even if it is excluded.  Returns (order (n_chains, length) int32, dist2 (n_chains, length) uint64): dist2[c, t] is the
    exact squared distance between the songs of slots t - 1 and t (slot 0: 0, or the seed descriptor's to its pick).  A
    chain with no allowed song left ends: the rest of its row, like the slots past n, holds -1 and 2^64 - 1.  To continue
    a chain, call again with seed = its last song and exclude = everything played so far."""
    return _chain_host(desc, seeds, length, tags, gap, exclude, seed_desc, None)


def hmix(desc, attrs, rule, seeds, length, tags=None, gap=0, exclude=None, seed_desc=None):
    """Harmonic mixes (bl_amd_desc_hmix_host): chain() with one more, hard, rule on consecutive songs.  attrs: n records
    of HMIX_ATTR_DTYPE (hmix_attrs()); rule: one record of HMIX_RULE_DTYPE (camelot_rule(), or a table of your own: bit b
    of key_ok[a] lets key b follow key a).  From slot 1 on a song is allowed only if chain() allows it and it passes
    against the song of the slot before: its key may follow that song's key (unknown keys pass), and its tempo is
    within tempo_tol per mille of that song's tempo, or of half or double of it with HALF_DOUBLE (unknown tempos
    pass).  Slot 0 is chain()'s; an index seed's attribute binds slot 1.  A chain with no allowed song ends; to go on
    without the rule, continue with chain() from its last song.  A rule with neither KEY nor TEMPO takes attrs=None and
    gives chain()'s arrays."""
    return _chain_host(desc, seeds, length, tags, gap, exclude, seed_desc, (attrs, rule))


def _chain_host(desc, seeds, length, tags, gap, exclude, seed_desc, pair):
    """chain() (pair None) and hmix() (pair = (attrs, rule))"""
    lib = _desc_array("desc", desc)
    _chain_seeds_check(seeds, seed_desc)
    length, gap = _chain_ints(length, gap, tags)
    n = lib.shape[0]
    if n >= MAX_N:
        raise ValueError(f"desc must have fewer than {MAX_N} rows, got {n}")
    s = q = None
    if seed_desc is not None:
        q = _desc_array("seed_desc", seed_desc)
    else:
        s = seeds_array(seeds, n)
    tg = None
    if tags is not None:
        tg = np.asarray(tags)
        if tg.dtype == np.bool_ or not np.issubdtype(tg.dtype, np.integer) or tg.shape != (n,):
            raise ValueError(f"tags must be {n} integers, got dtype {tg.dtype} and shape {tg.shape}")
        if tg.size and (tg.min() < -2 ** 31 or tg.max() >= 2 ** 31):
            raise ValueError("tags do not fit 32 bits")
        tg = np.ascontiguousarray(tg, dtype=np.int32)
    ex = None
    if exclude is not None:
        ex = np.asarray(exclude)
        if ex.dtype not in (np.bool_, np.uint8) or ex.shape != (n,):
            raise ValueError(f"exclude must be {n} bools or uint8, got dtype {ex.dtype} and shape {ex.shape}")
        ex = np.ascontiguousarray(ex).view(np.uint8)
    n_chains = q.shape[0] if q is not None else s.size
    order, dist2 = np.empty((n_chains, length), dtype=np.int32), np.empty((n_chains, length), dtype=np.uint64)
    args = (s.ctypes.data_as(_I32) if s is not None else None, q.ctypes.data_as(_DESC) if q is not None else None,
            n_chains, length, tg.ctypes.data_as(_I32) if tg is not None else None, gap,
            ex.ctypes.data_as(C.POINTER(C.c_uint8)) if ex is not None else None, order.ctypes.data_as(_I32),
            dist2.ctypes.data_as(_U64))
    if pair is None:
        check(_lib.load().bl_amd_desc_chain_host(lib.ctypes.data_as(_DESC), n, *args), "bl_amd_desc_chain_host")
    else:
        at, r = _hmix_args(*pair, n)
        check(_lib.load().bl_amd_desc_hmix_host(lib.ctypes.data_as(_DESC), at.ctypes.data_as(_ATTR) if at is not None else None,
                                                n, r.ctypes.data_as(_RULE), *args), "bl_amd_desc_hmix_host")
    return order, dist2


def chain_device(d_desc, d_seeds, length, tags=None, gap=0, exclude=None, seed_desc=None, stream=None, ctx=None):
    """chain() on torch tensors: d_desc a contiguous int16 (n, 32) CUDA tensor; d_seeds an int32 CUDA tensor on the same
    device (0-D or 1-D) or host integers, which are uploaded, or None with seed_desc, a tensor like d_desc that may be a
    view into it.  tags: an int32 CUDA tensor of n entries; exclude: a bool or uint8 CUDA tensor of n entries; both
    contiguous and on d_desc's device.  A seed outside [0, n) gives a row of -1.  Returns (order int32, dist2 as int64
    bits of the uint64: an empty slot reads -1) CUDA tensors of shape (n_chains, length), asynchronously on `stream`
    (default: the current stream of that device).  ctx: an explicit Context."""
    return _chain_device(d_desc, d_seeds, length, tags, gap, exclude, seed_desc, stream, ctx, None)


def hmix_device(d_desc, d_attrs, rule, d_seeds, length, tags=None, gap=0, exclude=None, seed_desc=None, stream=None,
                ctx=None):
    """hmix() on torch tensors (bl_amd_desc_hmix_device), the other arguments as chain_device() takes them.  d_attrs: the
    n attributes as a contiguous uint8 (n, 4) or int32 (n,) CUDA tensor on d_desc's device, the bytes of hmix_attrs()
    (torch.from_numpy(attrs.view(np.uint8).reshape(n, 4)).cuda()), or None with a rule that applies no test; rule: one
    record of HMIX_RULE_DTYPE in host memory, copied before the call returns."""
    return _chain_device(d_desc, d_seeds, length, tags, gap, exclude, seed_desc, stream, ctx, (d_attrs, rule))


def _chain_device(d_desc, d_seeds, length, tags, gap, exclude, seed_desc, stream, ctx, pair):
    """chain_device() (pair None) and hmix_device() (pair = (d_attrs, rule))"""
    import torch
    _chain_seeds_check(d_seeds, seed_desc)
    length, gap = _chain_ints(length, gap, tags)
    _device_desc_check("d_desc", d_desc)
    n = d_desc.shape[0]
    if n >= MAX_N:
        raise ValueError(f"d_desc must have fewer than {MAX_N} rows, got {n}")
    s = None
    if seed_desc is not None:
        _device_desc_check("seed_desc", seed_desc)
    elif isinstance(d_seeds, torch.Tensor):
        if d_seeds.dtype != torch.int32 or d_seeds.dim() > 1 or d_seeds.numel() < 1:
            raise ValueError("d_seeds must be an int32 tensor with 0 or 1 dimensions and at least one element")
        if not d_seeds.is_cuda:
            raise ValueError("d_seeds must be on the device of d_desc")
    else:
        s = seeds_array(d_seeds, None)
    for name, t, kinds in (("tags", tags, (torch.int32,)), ("exclude", exclude, (torch.bool, torch.uint8))):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype not in kinds or tuple(t.shape) != (n,)):
            raise ValueError(f"{name} must be a tensor of {n} entries of {' or '.join(str(k) for k in kinds)}")
    for name, t in (("d_seeds", d_seeds if s is None and seed_desc is None else None), ("seed_desc", seed_desc),
                    ("tags", tags), ("exclude", exclude)):
        if t is not None and (not t.is_cuda or t.device != d_desc.device or not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous tensor on the device of d_desc")
    name, head = "desc_chain_device", (d_desc.data_ptr(), n)
    if pair is not None:
        d_attrs, r = _hmix_args(*pair, n, d_desc.device)
        name = "desc_hmix_device"
        head = (d_desc.data_ptr(), d_attrs.data_ptr() if d_attrs is not None else None, n, r.ctypes.data_as(_RULE))
    lib = _lib.load()
    with _on_device(lib, d_desc, stream) as cur, torch.cuda.stream(cur):
        sd = None
        if s is not None:
            sd = torch.from_numpy(s).to(d_desc.device)
        elif seed_desc is None:
            sd = d_seeds.reshape(-1)
        n_chains = sd.numel() if sd is not None else seed_desc.shape[0]
        order = torch.empty((n_chains, length), dtype=torch.int32, device=d_desc.device)
        dist2 = torch.empty((n_chains, length), dtype=torch.int64, device=d_desc.device)
        args = (*head, sd.data_ptr() if sd is not None else None,
                seed_desc.data_ptr() if seed_desc is not None else None, n_chains, length,
                tags.data_ptr() if tags is not None else None, gap, exclude.data_ptr() if exclude is not None else None,
                order.data_ptr(), dist2.data_ptr(), C.c_void_p(cur.cuda_stream))
        if ctx is None:
            check(getattr(lib, "bl_amd_" + name)(*args), "bl_amd_" + name)
        else:
            check(getattr(lib, "bl_amd_ctx_" + name)(ctx.handle, *args), "bl_amd_ctx_" + name)
        if s is not None:
            sd.record_stream(cur)   # the uploaded seeds are freed when this returns
    return order, dist2


def hmix_attrs(rhythm=None, chroma=None, rate=22050):
    """The attributes of n songs for hmix() from their analysis records (bl_amd_hmix_attrs): a structured array of
    HMIX_ATTR_DTYPE.  rhythm: records of rhythm_to_numpy, tempo = round(100 * BPM) clamped to 1 .. 65535, 0 without a
    tempo; chroma: records of chroma_to_numpy, key as they hold it, 255 for key -1.  A group that is not passed is
    unknown for every song; at least one must be passed, and both must have the same length."""
    if rhythm is None and chroma is None:
        raise ValueError("at least one of rhythm and chroma must be given")
    first = np.asarray(rhythm if rhythm is not None else chroma)
    if first.ndim != 1 or first.size < 1:
        raise ValueError("the records must be a non-empty 1-D array")
    n = first.size
    rh = None if rhythm is None else _records("rhythm", rhythm, RHYTHM_DTYPE, n)
    ch = None if chroma is None else _records("chroma", chroma, CHROMA_DTYPE, n)
    out = np.zeros(n, dtype=HMIX_ATTR_DTYPE)
    check(_lib.load().bl_amd_hmix_attrs(
        rh.ctypes.data_as(C.POINTER(_lib.SongRhythm)) if rh is not None else None,
        ch.ctypes.data_as(C.POINTER(_lib.SongChroma)) if ch is not None else None, n, int_in("rate", rate, 1),
        out.ctypes.data_as(_ATTR)), "bl_amd_hmix_attrs")
    return out


def camelot_rule(tempo_tol, half_double=False, key=True, tempo=True):
    """The usual wheel as one record of HMIX_RULE_DTYPE (bl_amd_hmix_rule_camelot): after a key may follow the same key,
    the keys a fifth above and below in the same mode, and the relative key of the other mode.  tempo_tol: per mille of
    the previous song's tempo, 0 .. 1000; half_double: half and double time match too; key / tempo: whether that test
    is applied at all."""
    tempo_tol = int_in("tempo_tol", tempo_tol, 0, 1000)
    if half_double and not tempo:
        raise ValueError("half_double needs tempo")
    flags = (_lib.BL_AMD_HMIX_KEY if key else 0) | (_lib.BL_AMD_HMIX_TEMPO if tempo else 0) | \
        (_lib.BL_AMD_HMIX_HALF_DOUBLE if half_double else 0)
    out = np.zeros(1, dtype=HMIX_RULE_DTYPE)
    check(_lib.load().bl_amd_hmix_rule_camelot(out.ctypes.data_as(_RULE), tempo_tol, flags), "bl_amd_hmix_rule_camelot")
    return out[0]


def distance(dist2):
    """sqrt(dist2) / 32512 as float64: 2.0 is one column at full scale going from its minimum to its maximum.  Plain
    host arithmetic; an empty slot (2^64 - 1) gives inf."""
    d2 = np.asarray(dist2)
    out = np.sqrt(d2.astype(np.float64)) / float(SCALE_MAX)
    return np.where(d2.astype(np.uint64) == np.uint64(EMPTY_DIST2), np.inf, out)


_RATINGS = ("tempo", "amplitude", "frequency", "attack")


def _records(name, rec, dtype, n):
    a = np.ascontiguousarray(rec)
    if a.dtype != dtype or a.ndim != 1 or a.size != n:
        raise ValueError(f"{name} must be a 1-D array of {n} records of dtype {dtype.names}, got {a.dtype} {a.shape}")
    return a


def features(results, levels=None, timbre=None, rhythm=None, chroma=None, mel=None):
    """The float32 feature matrix of n songs from the records the other modules return, and its column names: (x, names).
    Host numpy only.  Groups that are not passed are left out; with all of them there are 32 columns, a full descriptor:

      ratings  tempo, amplitude, frequency, attack      the four ratings of `results` (results_to_numpy) as they are
      levels   rms_db, peak_db                          levels_db(): the louder channel's RMS and peak in dB (-inf for
                                                        silence, which the range ignores and the quantiser maps to 0)
               zcr                                      the larger of the channels' zero crossings per frame
      timbre   centroid_hz, centroid_std_hz,            timbre_hz(): mean and standard deviation over the used frames,
               rolloff_hz, rolloff_std_hz               in Hz; NaN for a song without a used frame
      rhythm   bpm, strength                            rhythm_bpm(): beats per minute (NaN without a tempo), r_lag / r0
      chroma   chroma_0 .. chroma_11                    chroma[k] / sum_k chroma[k] in float64, 0 when the sum is 0
      mel      flatness_db, mfcc_1 .. mfcc_6            mel_summary(): means over the used frames, NaN without one;
                                                        coefficient 0 is the overall level, which rms_db carries"""
    res = np.ascontiguousarray(results)
    if res.dtype != RESULT_DTYPE or res.ndim != 1 or res.size < 1:
        raise ValueError("results must be a non-empty 1-D array of bl_amd_song_result records (results_to_numpy)")
    n = res.size
    cols, names = [res[k].astype(np.float64) for k in _RATINGS], list(_RATINGS)
    if levels is not None:
        db = levels_db(_records("levels", levels, LEVELS_DTYPE, n))
        cols += [db["rms_db"].max(axis=1), db["peak_db"].max(axis=1), db["zcr"].max(axis=1)]
        names += ["rms_db", "peak_db", "zcr"]
    if timbre is not None:
        hz = timbre_hz(_records("timbre", timbre, TIMBRE_SONG_DTYPE, n))
        keys = ["centroid_hz", "centroid_std_hz", "rolloff_hz", "rolloff_std_hz"]
        cols += [hz[k] for k in keys]
        names += keys
    if rhythm is not None:
        from .rhythm import rhythm_bpm
        bpm, strength = rhythm_bpm(_records("rhythm", rhythm, RHYTHM_DTYPE, n))
        cols += [bpm, strength]
        names += ["bpm", "strength"]
    if chroma is not None:
        ch = _records("chroma", chroma, CHROMA_DTYPE, n)["chroma"].astype(np.float64)
        total = ch.sum(axis=1, keepdims=True)
        share = np.divide(ch, total, out=np.zeros_like(ch), where=total > 0)
        cols += [share[:, k] for k in range(12)]
        names += [f"chroma_{k}" for k in range(12)]
    if mel is not None:
        from .mel import mel_summary
        ms = mel_summary(_records("mel", mel, MEL_DTYPE, n))
        cols += [ms["flatness_db"]] + [ms["mfcc"][:, k] for k in range(1, 7)]
        names += ["flatness_db"] + [f"mfcc_{k}" for k in range(1, 7)]
    with np.errstate(over="ignore"):
        return np.stack(cols, axis=1).astype(np.float32), names
