"""Queries over (n, 4) force vectors: matrices, playlists, nearest neighbours, chains, mixes, radius lists, duplicate
groups and the cross forms, each from host memory and, as `*_device`, on torch CUDA tensors."""
import contextlib
import ctypes as C

import numpy as np

from . import _lib
from ._args import int_in, seeds_array, vecs_shape_check
from ._lib import check, libc_free

_FV, _I32, _F32 = C.POINTER(_lib.ForceVector), C.POINTER(C.c_int32), C.POINTER(C.c_float)


def _matrix(fn_name, vecs):
    lib = _lib.load()
    v = np.ascontiguousarray(vecs, dtype=np.float32).reshape(-1, 4)
    n = v.shape[0]
    out = np.empty((n, n), dtype=np.float32)
    check(getattr(lib, fn_name)(v.ctypes.data_as(_FV), n, out.ctypes.data_as(_F32)), fn_name)
    return out


def distance_matrix(vecs):
    """N x N bl_distance matrix (ref src/analyze.c:96-100) of (N, 4) force vectors."""
    return _matrix("bl_amd_distance_matrix_host", vecs)


def cosine_matrix(vecs):
    """N x N bl_cosine_similarity matrix (ref src/analyze.c:135-140)."""
    return _matrix("bl_amd_cosine_matrix_host", vecs)


def _playlist_host_call(name, v, seed):
    """(order, dist) over the n vectors of v from the playlist host entry point `name`, which takes `seed`"""
    lib = _lib.load()
    n = v.shape[0]
    order = np.empty(n, dtype=np.int32)
    dist = np.empty(n, dtype=np.float32)
    check(getattr(lib, name)(v.ctypes.data_as(_FV), n, seed, order.ctypes.data_as(_I32), dist.ctypes.data_as(_F32)), name)
    return order, dist


def playlist(vecs, seed_index):
    """Song indices ordered by increasing bl_distance from song `seed_index`, and the
    distances (ref python/examples/make_m3u_playlist.py:62-72).  Stable for ties.  NaN distances after every
    number, in index order: numpy's stable argsort."""
    v = np.ascontiguousarray(vecs, dtype=np.float32).reshape(-1, 4)
    return _playlist_host_call("bl_amd_playlist_host", v, int(seed_index))


def playlist_vec(vecs, seed_vec):
    """playlist() from a seed that need not be a song of `vecs`: the song indices by increasing bl_distance from the
    4-component `seed_vec`, and the distances.  Stable for ties; a seed equal to a song lists it at distance 0.  NaN
    distances after every number, in index order: numpy's stable argsort."""
    v = np.ascontiguousarray(vecs, dtype=np.float32)
    vecs_shape_check("vecs", v.shape)
    sv = np.asarray(seed_vec, dtype=np.float32)
    if sv.shape != (4,):
        raise ValueError(f"the seed must be one force vector of 4 components, got shape {sv.shape}")
    return _playlist_host_call("bl_amd_playlist_vec_host", v, _lib.ForceVector(*(float(x) for x in sv)))


_KNN_METRICS = {"distance": _lib.BL_AMD_KNN_DISTANCE, "cosine": _lib.BL_AMD_KNN_COSINE}


def _metric_check(metric, shape):
    """the metric's code, for a known metric over (n, 4) force vectors"""
    if metric not in _KNN_METRICS:
        raise ValueError(f"metric must be one of {sorted(_KNN_METRICS)}, got {metric!r}")
    vecs_shape_check("force vectors", shape)
    return _KNN_METRICS[metric]


def _device_vecs_check(d_vecs):
    import torch
    if d_vecs.dtype != torch.float32 or not d_vecs.is_cuda or not d_vecs.is_contiguous():
        raise ValueError("d_vecs must be a contiguous float32 CUDA tensor")


def _rows_check(n, row_begin, n_rows):
    """n_rows (None: all rows from row_begin) once [row_begin, row_begin + n_rows) lies inside [0, n)"""
    if n_rows is None:
        n_rows = n - row_begin
    if not (0 <= row_begin < n and 1 <= n_rows <= n - row_begin):
        raise ValueError(f"rows [{row_begin}, {row_begin + n_rows}) are not inside [0, {n})")
    return n_rows


@contextlib.contextmanager
def _on_device_of(lib, tensor, stream):
    """The tensor's device current and the library initialised on it; yields the torch stream to launch on (`stream`,
    else that device's current one) without entering it: the caller decides under which stream it allocates."""
    import torch
    cur = stream if stream is not None else torch.cuda.current_stream(tensor.device)
    idx = tensor.device.index or 0
    with torch.cuda.device(idx):
        check(lib.bl_amd_init(idx), "bl_amd_init")
        yield cur


def _knn_check(k, metric, shape):
    int_in("k", k, 1, _lib.BL_AMD_KNN_MAX_K)
    return _metric_check(metric, shape)


def _host_pair(rows, cols):
    """the (rows, cols) int32 and float32 outputs of the kNN, chain and mix host entry points"""
    return np.empty((rows, cols), dtype=np.int32), np.empty((rows, cols), dtype=np.float32)


def _knn_host_call(name, args, rows, k):
    """(index, value) of shape (rows, k) from the kNN host entry point `name`, called with `args` and the two outputs"""
    lib = _lib.load()
    index, value = _host_pair(rows, k)
    check(getattr(lib, name)(*args, index.ctypes.data_as(_I32), value.ctypes.data_as(_F32)), name)
    return index, value


def _knn_device_call(name, args, v, rows, k, stream):
    """The same for a device entry point, on the device of the library tensor v and on `stream`"""
    import torch
    lib = _lib.load()
    index = torch.empty((rows, k), dtype=torch.int32, device=v.device)
    value = torch.empty((rows, k), dtype=torch.float32, device=v.device)
    with _on_device_of(lib, v, stream) as cur:
        check(getattr(lib, name)(*args, index.data_ptr(), value.data_ptr(), C.c_void_p(cur.cuda_stream)), name)
    return index, value


def knn(vecs, k, metric="distance"):
    """The k nearest songs of every song of (n, 4) force vectors: (index (n, k) int32, value (n, k) float32).
    Values have the bits of bl_distance ("distance", nearest = smallest) or bl_cosine_similarity ("cosine",
    nearest = largest); ties go to the smaller index and the song itself is never listed
    (ref python/examples/make_m3u_playlist.py:62-72 for every seed).  Slots past n - 1 hold -1 and NaN."""
    v = np.ascontiguousarray(vecs, dtype=np.float32)
    m = _knn_check(k, metric, v.shape)
    n = v.shape[0]
    return _knn_host_call("bl_amd_knn_host", (v.ctypes.data_as(_FV), n, int(k), m), n, k)


def knn_device(d_vecs, k, metric="distance", row_begin=0, n_rows=None, stream=None):
    """knn() for the queries d_vecs[row_begin:row_begin + n_rows] against all of d_vecs, a float32 (n, 4) CUDA
    tensor; returns (index, value) CUDA tensors of shape (n_rows, k) on its device, asynchronously on `stream`
    (default: the current stream of that device)."""
    m = _knn_check(k, metric, tuple(d_vecs.shape))
    _device_vecs_check(d_vecs)
    n = d_vecs.shape[0]
    n_rows = _rows_check(n, row_begin, n_rows)
    return _knn_device_call("bl_amd_knn_device", (d_vecs.data_ptr(), n, int(row_begin), int(n_rows), int(k), m), d_vecs,
                            n_rows, k, stream)


def _chain_check(seeds, length, metric, shape, n_limit):
    """(metric code, seeds as a contiguous 1-D int32 numpy array or None for a tensor); n_limit: reject seeds outside
    [0, n_limit) (None: leave them to the device, which answers with a -1 / NaN row)"""
    int_in("length", length, 1)
    m = _metric_check(metric, shape)
    if hasattr(seeds, "is_cuda"):   # a torch tensor: _device_seeds_check checks it
        return m, None
    return m, seeds_array(seeds, n_limit)


def _device_seeds_check(d_seeds, d_vecs):
    import torch
    if d_seeds.dtype != torch.int32 or d_seeds.dim() > 1 or d_seeds.numel() < 1:
        raise ValueError("d_seeds must be an int32 tensor with 0 or 1 dimensions and at least one element")
    if not d_seeds.is_cuda or d_seeds.device != d_vecs.device:
        raise ValueError("d_seeds must be on the device of d_vecs")


def _chain_device_call(name, args, v, s, d_seeds, n_vec_seeds, length, stream):
    """(order, value) of shape (n_chains, length) from the chain or mix device entry point `name`, on the device of the
    library tensor v and on `stream`.  The chains start from the host seeds s, which are uploaded, else from the tensor
    d_seeds, flattened, else (both None) from n_vec_seeds vectors; args(seeds pointer or None, n_chains) gives the
    arguments in front of the two outputs."""
    import torch
    lib = _lib.load()
    with _on_device_of(lib, v, stream) as cur, torch.cuda.stream(cur):
        sd = None
        if s is not None:
            sd = torch.from_numpy(s).to(v.device)
        elif d_seeds is not None:
            sd = d_seeds.reshape(-1).contiguous()
        n_chains = sd.numel() if sd is not None else n_vec_seeds
        order = torch.empty((n_chains, length), dtype=torch.int32, device=v.device)
        value = torch.empty((n_chains, length), dtype=torch.float32, device=v.device)
        check(getattr(lib, name)(*args(sd.data_ptr() if sd is not None else None, n_chains), order.data_ptr(),
                                 value.data_ptr(), C.c_void_p(cur.cuda_stream)), name)
        if s is not None:
            sd.record_stream(cur)   # the uploaded seeds are freed when this returns
    return order, value


def chain(vecs, seeds, length, metric="distance"):
    """Song-to-song chains over (n, 4) force vectors, one per seed (a scalar seed gives one chain): slot 0 is the
    seed and every next slot the song nearest to the previous one that the chain has not played yet, nearest as in
    knn().  Returns (order (n_chains, length) int32, value (n_chains, length) float32); value[c, t] has the bits of
    bl_distance / bl_cosine_similarity between the songs of slots t - 1 and t (slot 0: the seed with itself).
    Slots past n hold -1 and NaN."""
    v = np.ascontiguousarray(vecs, dtype=np.float32)
    m, s = _chain_check(seeds, length, metric, v.shape, v.shape[0] if v.ndim == 2 else 0)
    lib = _lib.load()
    order, value = _host_pair(s.size, length)
    check(lib.bl_amd_chain_host(v.ctypes.data_as(_FV), v.shape[0], s.ctypes.data_as(_I32), s.size, int(length), m,
                                order.ctypes.data_as(_I32), value.ctypes.data_as(_F32)), "bl_amd_chain_host")
    return order, value


def chain_device(d_vecs, d_seeds, length, metric="distance", stream=None):
    """chain() on the device: d_vecs a contiguous float32 (n, 4) CUDA tensor, d_seeds an int32 CUDA tensor on the same
    device (0-D or 1-D) or host integers, which are uploaded.  Returns (order, value) CUDA tensors of shape
    (n_chains, length), asynchronously on `stream` (default: the current stream of that device).  A seed outside
    [0, n) gives a row of -1 / NaN."""
    m, s = _chain_check(d_seeds, length, metric, tuple(d_vecs.shape), None)
    _device_vecs_check(d_vecs)
    if s is None:
        _device_seeds_check(d_seeds, d_vecs)
    v, n = d_vecs, d_vecs.shape[0]
    return _chain_device_call("bl_amd_chain_device", lambda sd, n_chains: (v.data_ptr(), n, sd, n_chains, int(length), m),
                              v, s, d_seeds, 0, length, stream)


def _mix_gap_check(gap, tags):
    gap = int_in("gap", gap, 0, _lib.BL_AMD_MIX_MAX_GAP)
    if gap > 0 and tags is None:
        raise ValueError("gap > 0 needs tags")
    return gap


def _mix_seeds_check(seeds, seed_vecs):
    if (seeds is None) == (seed_vecs is None):
        raise ValueError("exactly one of seeds and seed_vecs must be given")


def mix(vecs, seeds, length, metric="distance", tags=None, gap=0, exclude=None, seed_vecs=None):
    """chain() under rules.  tags: n integers (artist, album ...; negative = untagged) of which no value may repeat
    within `gap` slots (0 <= gap <= 16; 0 ignores the tags).  exclude: n bools or bytes, non-zero = never picked.
    seed_vecs: (m, 4) float32 vectors instead of seeds (pass seeds=None): slot 0 is the song nearest to the vector
    among the songs not excluded.  An index seed takes slot 0 even if it is excluded.  A chain with no allowed song
    left ends: the rest of its row holds -1 and NaN.  To continue a chain, call again with seed = its last song and
    exclude = everything played so far.  Returns (order, value) as chain() does."""
    v = np.ascontiguousarray(vecs, dtype=np.float32)
    _mix_seeds_check(seeds, seed_vecs)
    gap = _mix_gap_check(gap, tags)
    n = v.shape[0] if v.ndim == 2 else 0
    q = None
    if seed_vecs is not None:
        if hasattr(seed_vecs, "dtype") and seed_vecs.dtype != np.float32:
            raise ValueError(f"seed_vecs must be float32, got {seed_vecs.dtype}")
        q = np.ascontiguousarray(seed_vecs, dtype=np.float32)
        vecs_shape_check("seed_vecs", q.shape)
        m, s = _chain_check(0, length, metric, v.shape, None)[0], None
    else:
        m, s = _chain_check(seeds, length, metric, v.shape, n)
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
    lib = _lib.load()
    n_chains = q.shape[0] if q is not None else s.size
    order, value = _host_pair(n_chains, length)
    check(lib.bl_amd_mix_host(v.ctypes.data_as(_FV), n, s.ctypes.data_as(_I32) if s is not None else None,
                              q.ctypes.data_as(_FV) if q is not None else None, n_chains, int(length), m,
                              tg.ctypes.data_as(_I32) if tg is not None else None, gap,
                              ex.ctypes.data_as(C.POINTER(C.c_uint8)) if ex is not None else None,
                              order.ctypes.data_as(_I32), value.ctypes.data_as(_F32)), "bl_amd_mix_host")
    return order, value


def mix_device(d_vecs, d_seeds, length, metric="distance", tags=None, gap=0, exclude=None, seed_vecs=None, stream=None):
    """mix() on the device: d_vecs as chain_device() takes it, d_seeds as chain_device() takes them or None with
    seed_vecs, a contiguous, 16-byte aligned float32 (m, 4) CUDA tensor that may be a view into d_vecs.  tags: an
    int32 CUDA tensor of n entries; exclude: a bool or uint8 CUDA tensor of n entries; both contiguous and on the
    device of d_vecs.
    Returns (order, value) CUDA tensors of shape (n_chains, length), asynchronously on `stream`."""
    import torch
    _mix_seeds_check(d_seeds, seed_vecs)
    gap = _mix_gap_check(gap, tags)
    shape = tuple(d_vecs.shape)
    if seed_vecs is not None:
        m, s = _chain_check(0, length, metric, shape, None)[0], None
        if not isinstance(seed_vecs, torch.Tensor) or seed_vecs.dtype != torch.float32:
            raise ValueError("seed_vecs must be a float32 tensor of shape (m, 4) with m >= 1")
        vecs_shape_check("seed_vecs", seed_vecs.shape)
    else:
        m, s = _chain_check(d_seeds, length, metric, shape, None)
    n = shape[0]
    for name, t, kinds in (("tags", tags, (torch.int32,)), ("exclude", exclude, (torch.bool, torch.uint8))):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype not in kinds or tuple(t.shape) != (n,)):
            raise ValueError(f"{name} must be a tensor of {n} entries of {' or '.join(str(k) for k in kinds)}")
    _device_vecs_check(d_vecs)
    if seed_vecs is None and s is None:
        _device_seeds_check(d_seeds, d_vecs)
    for name, t in (("seed_vecs", seed_vecs), ("tags", tags), ("exclude", exclude)):
        if t is not None and (not t.is_cuda or t.device != d_vecs.device or not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous tensor on the device of d_vecs")
    if seed_vecs is not None and seed_vecs.data_ptr() % 16:   # a view such as flat[1:9].view(2, 4) is contiguous
        raise ValueError("seed_vecs must be 16-byte aligned")
    v = d_vecs
    return _chain_device_call(
        "bl_amd_mix_device",
        lambda sd, n_chains: (v.data_ptr(), n, sd, seed_vecs.data_ptr() if seed_vecs is not None else None, n_chains,
                              int(length), m, tags.data_ptr() if tags is not None else None, gap,
                              exclude.data_ptr() if exclude is not None else None),
        v, s, d_seeds, seed_vecs.shape[0] if seed_vecs is not None else 0, length, stream)


def _radius_check(r, metric, shape):
    """(metric code, the radius as a Python float that is an exact f32)"""
    if isinstance(r, bool) or not isinstance(r, (int, float, np.integer, np.floating)):
        raise ValueError(f"the radius must be a real number, got {r!r}")
    m = _metric_check(metric, shape)
    with np.errstate(over="ignore"):
        r32 = np.float32(r)
    if np.isnan(r32):
        raise ValueError("the radius must not be NaN")
    return m, float(r32)


def _radius_host_call(name, args, rows):
    """(offsets, index, value) of `rows` queries from the radius host entry point `name`, called with `args` and the
    three outputs; the two blocks the library allocates are copied and freed"""
    lib = _lib.load()
    offsets = np.empty(rows + 1, dtype=np.int64)
    p_index, p_value = _I32(), _F32()
    check(getattr(lib, name)(*args, offsets.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(p_index), C.byref(p_value)),
          name)
    try:
        total = int(offsets[rows])
        index = np.ctypeslib.as_array(p_index, shape=(total,)).copy() if total else np.empty(0, dtype=np.int32)
        value = np.ctypeslib.as_array(p_value, shape=(total,)).copy() if total else np.empty(0, dtype=np.float32)
    finally:
        libc_free(p_index)
        libc_free(p_value)
    return offsets, index, value


def _radius_device_call(count, fill, args, v, rows, values, stream):
    """The same from the device entry points `count` and `fill`, both called with `args` and their outputs on the
    device of the library tensor v: count, read the total back (the one synchronisation), fill"""
    import torch
    lib = _lib.load()
    with _on_device_of(lib, v, stream) as cur, torch.cuda.stream(cur):
        s = C.c_void_p(cur.cuda_stream)
        offsets = torch.empty(rows + 1, dtype=torch.int64, device=v.device)
        check(getattr(lib, count)(*args, offsets.data_ptr(), s), count)
        total = int(offsets[-1].item())
        # one slot at least: an empty result still goes through the fill call, which then writes nothing
        index = torch.empty(max(total, 1), dtype=torch.int32, device=v.device)
        value = torch.empty(max(total, 1), dtype=torch.float32, device=v.device) if values else None
        check(getattr(lib, fill)(*args, offsets.data_ptr(), index.data_ptr(), value.data_ptr() if values else None, s),
              fill)
    return offsets, index[:total], value[:total] if values else None


def radius(vecs, r, metric="distance"):
    """The songs within radius r of every song of (n, 4) force vectors, as compressed sparse row lists:
    (offsets int64 (n + 1,), index int32 (total,), value float32 (total,)); row i is index[offsets[i]:offsets[i + 1]],
    in ascending song index, and never lists i.  Within means bl_distance <= r ("distance") or bl_cosine_similarity
    >= r ("cosine") on the f32 matrix entry, whose bits `value` holds; a NaN entry is never within."""
    v = np.ascontiguousarray(vecs, dtype=np.float32)
    m, r = _radius_check(r, metric, v.shape)
    n = v.shape[0]
    return _radius_host_call("bl_amd_radius_host", (v.ctypes.data_as(_FV), n, m, r), n)


def radius_device(d_vecs, r, metric="distance", row_begin=0, n_rows=None, values=True, stream=None):
    """radius() for the queries d_vecs[row_begin:row_begin + n_rows] against all of d_vecs, a contiguous float32
    (n, 4) CUDA tensor.  Returns (offsets int64 (n_rows + 1,), index int32 (total,), value float32 (total,) or None
    without `values`) as CUDA tensors on its device.  Count and fill run on `stream` (default: the current stream of
    that device); between them the total is read back, which is the one synchronisation."""
    m, r = _radius_check(r, metric, tuple(d_vecs.shape))
    _device_vecs_check(d_vecs)
    n = d_vecs.shape[0]
    n_rows = _rows_check(n, row_begin, n_rows)
    return _radius_device_call("bl_amd_radius_count_device", "bl_amd_radius_fill_device",
                               (d_vecs.data_ptr(), n, int(row_begin), int(n_rows), m, r), d_vecs, n_rows, values, stream)


def duplicate_groups(vecs, r, metric="distance"):
    """A group label per song of (n, 4) force vectors, int32 (n,): the smallest song index among the songs connected
    to it by steps of at most radius r (bl_distance <= r, or bl_cosine_similarity >= r), as radius() defines "within".
    The same recording under two names gets one label; a song with no neighbour is its own group."""
    v = np.ascontiguousarray(vecs, dtype=np.float32)
    m, r = _radius_check(r, metric, v.shape)
    lib = _lib.load()
    n = v.shape[0]
    group = np.empty(n, dtype=np.int32)
    check(lib.bl_amd_groups_host(v.ctypes.data_as(_FV), n, m, r, group.ctypes.data_as(_I32)), "bl_amd_groups_host")
    return group


def duplicate_groups_device(d_vecs, r, metric="distance", stream=None):
    """duplicate_groups() on the device: d_vecs a contiguous float32 (n, 4) CUDA tensor; returns an int32 (n,) CUDA
    tensor on its device, asynchronously on `stream` (default: the current stream of that device)."""
    import torch
    m, r = _radius_check(r, metric, tuple(d_vecs.shape))
    _device_vecs_check(d_vecs)
    lib = _lib.load()
    v = d_vecs
    n = v.shape[0]
    with _on_device_of(lib, v, stream) as cur, torch.cuda.stream(cur):
        group = torch.empty(n, dtype=torch.int32, device=v.device)
        check(lib.bl_amd_groups_device(v.data_ptr(), n, m, r, group.data_ptr(), C.c_void_p(cur.cuda_stream)),
              "bl_amd_groups_device")
    return group


def _cross_shapes_check(q_shape, v_shape):
    vecs_shape_check("queries", q_shape)
    vecs_shape_check("vecs", v_shape)


def _cross_host_vecs(queries, vecs):
    """(queries, vecs) as contiguous float32 numpy arrays.  Plain sequences are converted; an array that says what it
    holds must hold float32, so that the two sides cannot silently differ in precision."""
    for name, x in (("queries", queries), ("vecs", vecs)):
        if hasattr(x, "dtype") and x.dtype != np.float32:
            raise ValueError(f"{name} must be float32, got {x.dtype}")
    q, v = np.ascontiguousarray(queries, dtype=np.float32), np.ascontiguousarray(vecs, dtype=np.float32)
    _cross_shapes_check(q.shape, v.shape)
    return q, v


def _cross_device_check(d_queries, d_vecs):
    import torch
    for name, t in (("d_queries", d_queries), ("d_vecs", d_vecs)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch tensor")
    _cross_shapes_check(tuple(d_queries.shape), tuple(d_vecs.shape))
    if d_queries.dtype != torch.float32 or d_vecs.dtype != torch.float32:
        raise ValueError(f"d_queries and d_vecs must both be float32, got {d_queries.dtype} and {d_vecs.dtype}")
    if d_queries.device != d_vecs.device:
        raise ValueError(f"d_queries ({d_queries.device}) and d_vecs ({d_vecs.device}) must be on the same device")
    if not d_vecs.is_cuda:
        raise ValueError("d_queries and d_vecs must be CUDA tensors")
    if not d_queries.is_contiguous() or not d_vecs.is_contiguous():
        raise ValueError("d_queries and d_vecs must be contiguous")


def knn_cross(queries, vecs, k, metric="distance"):
    """The k nearest songs of the library `vecs` (n, 4) to each of `queries` (m, 4), vectors that need not be songs of
    it: (index (m, k) int32, value (m, k) float32), ordered and valued as knn() does.  Unlike knn() nothing is left
    out: a query equal to library song 7 lists song 7 first, at distance 0.  Slots past n hold -1 and NaN."""
    m_code = _knn_check(k, metric, (1, 4))   # the shapes are checked per side below
    q, v = _cross_host_vecs(queries, vecs)
    m = q.shape[0]
    return _knn_host_call("bl_amd_cross_knn_host",
                          (q.ctypes.data_as(_FV), m, v.ctypes.data_as(_FV), v.shape[0], int(k), m_code), m, k)


def knn_cross_device(d_queries, d_vecs, k, metric="distance", stream=None):
    """knn_cross() on the device: d_queries (m, 4) and d_vecs (n, 4) contiguous float32 CUDA tensors on one device;
    d_queries may be a view into d_vecs and needs 16-byte alignment only.  Returns (index, value) CUDA tensors of
    shape (m, k), asynchronously on `stream` (default: the current stream of that device).  Queries are independent:
    shard by slicing d_queries."""
    m_code = _knn_check(k, metric, (1, 4))
    _cross_device_check(d_queries, d_vecs)
    q, v = d_queries, d_vecs
    m = q.shape[0]
    return _knn_device_call("bl_amd_cross_knn_device", (q.data_ptr(), m, v.data_ptr(), v.shape[0], int(k), m_code), v, m,
                            k, stream)


def _radius_cross_check(r, metric):
    return _radius_check(r, metric, (1, 4))   # the shapes are checked per side


def radius_cross(queries, vecs, r, metric="distance"):
    """The songs of the library `vecs` (n, 4) within radius r of each of `queries` (m, 4), as compressed sparse row
    lists: (offset int64 (m + 1,), index int32 (total,), value float32 (total,)), as radius() defines "within" and
    orders a row.  Unlike radius() nothing is left out: with r = 0 a query that is in the library finds its copy."""
    m_code, r = _radius_cross_check(r, metric)
    q, v = _cross_host_vecs(queries, vecs)
    m = q.shape[0]
    return _radius_host_call("bl_amd_cross_radius_host",
                             (q.ctypes.data_as(_FV), m, v.ctypes.data_as(_FV), v.shape[0], m_code, r), m)


def radius_cross_device(d_queries, d_vecs, r, metric="distance", values=True, stream=None):
    """radius_cross() on the device, tensors as for knn_cross_device().  Returns (offset int64 (m + 1,), index int32
    (total,), value float32 (total,) or None without `values`) as CUDA tensors.  Count and fill run on `stream`;
    between them the total is read back, which is the one synchronisation."""
    m_code, r = _radius_cross_check(r, metric)
    _cross_device_check(d_queries, d_vecs)
    q, v = d_queries, d_vecs
    m, n = q.shape[0], v.shape[0]
    return _radius_device_call("bl_amd_cross_radius_count_device", "bl_amd_cross_radius_fill_device",
                               (q.data_ptr(), m, v.data_ptr(), n, m_code, r), v, m, values, stream)
