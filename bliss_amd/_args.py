"""The argument checks and conversions the wrappers share.  Every refusal is a ValueError that names the argument and
shows the offending value."""
import ctypes as C

import numpy as np


def per_song(x, n):
    """x for each of n songs as a list: a scalar stands for all of them, a sequence is taken as it is"""
    return [x] * n if np.isscalar(x) else list(x)


def int_in(name, x, lo, hi=None):
    """int(x), once x is a Python or numpy integer (no bool, no float however integral) in [lo, hi]; hi None: no upper
    bound"""
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or x < lo or (hi is not None and x > hi):
        raise ValueError(f"{name} must be an integer in [{lo}, {'inf' if hi is None else hi}], got {x!r}")
    return int(x)


def songs_check(lengths, channels, shortest):
    """per-song channel list, once there is a song and every song has 1 or 2 channels and at least shortest[channels - 1]
    interleaved samples"""
    n = len(lengths)
    if n < 1:
        raise ValueError("at least one song is needed")
    channels = per_song(channels, n)
    if len(channels) != n:
        raise ValueError(f"{n} songs but {len(channels)} channel counts")
    for i, (ln, ch) in enumerate(zip(lengths, channels)):
        channels[i] = int_in("channels", ch, 1, 2)
        if int(ln) < shortest[channels[i] - 1]:
            raise ValueError(f"a song of {channels[i]} channels needs at least {shortest[channels[i] - 1]} samples, "
                             f"got {int(ln)}")
    return channels


def seeds_array(seeds, n_limit):
    """the seeds of chains (a scalar or a non-empty 1-D sequence of integers) as a contiguous 1-D int32 array; n_limit:
    reject seeds outside [0, n_limit) (None: leave them to the device, which answers with an empty row)"""
    s = np.asarray(seeds)
    if s.dtype == np.bool_ or not np.issubdtype(s.dtype, np.integer):
        raise ValueError(f"seeds must be integers, got dtype {s.dtype}")
    if s.ndim > 1 or s.size < 1:
        raise ValueError(f"seeds must be a scalar or a non-empty 1-D sequence, got shape {s.shape}")
    s = s.reshape(-1)
    if n_limit is not None and (s.min() < 0 or s.max() >= n_limit):
        raise ValueError(f"seeds must lie in [0, {n_limit})")
    if s.min() < -2 ** 31 or s.max() >= 2 ** 31:
        raise ValueError("seeds do not fit 32 bits")
    return np.ascontiguousarray(s, dtype=np.int32)


def vecs_shape_check(name, shape):
    if len(shape) != 2 or shape[1] != 4 or shape[0] < 1:
        raise ValueError(f"{name} must have shape (n, 4) with n >= 1, got {tuple(shape)}")


def host_pcm(pcm_list, dtype):
    """(arrays, pointers, sizes) of a list of host PCM arrays: contiguous arrays of `dtype`, which keep alive what the
    c_void_p array points to, and the c_int32 array of their sample counts"""
    arrs = [np.ascontiguousarray(p, dtype=dtype) for p in pcm_list]
    n = len(arrs)
    return arrs, (C.c_void_p * n)(*[a.ctypes.data for a in arrs]), (C.c_int32 * n)(*[a.size for a in arrs])


def desc_scale(scale, d, scale_max):
    """the ctypes uint16 array of a descriptor's d scales (None: NULL, all at the maximum), once every one is an
    integer in [0, scale_max]; a scalar stands for all columns"""
    if scale is None:
        return None
    vals = per_song(scale, d)
    if len(vals) != d:
        raise ValueError(f"{d} columns but {len(vals)} scales")
    return (C.c_uint16 * d)(*[int_in("scale", v, 0, scale_max) for v in vals])


def feature_matrix(name, x, dims_max):
    """x as a contiguous float32 (n, d) array with n >= 1 and 1 <= d <= dims_max"""
    a = np.ascontiguousarray(x, dtype=np.float32)
    if a.ndim != 2 or a.shape[0] < 1 or not 1 <= a.shape[1] <= dims_max:
        raise ValueError(f"{name} must have shape (n, d) with n >= 1 and 1 <= d <= {dims_max}, got {a.shape}")
    return a
