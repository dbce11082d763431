"""Spectral timbre without a device.  tests/timbre_reference.py, the Python-int restatement the GPU test compares with,
is run on designed spectra (the transform is skipped, P is fed directly) whose answers are known in closed form, and
every plausible misreading of the definitions — an exclusive prefix, > for >=, bin 0 taking part, rounding for floor —
is shown to change the answer on them.  Then what is plain host arithmetic in the library: bl_amd_timbre_frames, the
*_hz helpers against numpy, the argument checks of the device entry points (which come before any device is touched),
and the layout of the two records."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import bliss_amd
from bliss_amd import _lib
from bliss_amd.batch import TIMBRE_FRAME_DTYPE, TIMBRE_SONG_DTYPE
from tests import timbre_reference as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = _lib.BL_UNEXPECTED

NEW_SYMBOLS = {
    "bl_amd_timbre_frames": C.c_int, "bl_amd_timbre_batch_device": C.c_int, "bl_amd_ctx_timbre_batch_device": C.c_int,
    "bl_amd_timbre_batch_host": C.c_int, "bl_amd_timbre_centroid_hz": C.c_double,
    "bl_amd_timbre_rolloff_hz": C.c_double, "bl_amd_timbre_peak_hz": C.c_double,
}
FRAME_OFFSETS = dict(energy=0, moment=8, rolloff=16, peak=20)
SONG_OFFSETS = dict(centroid_sum=0, centroid_sumsq=8, rolloff_sum=16, rolloff_sumsq=24, peak_sum=32, peak_sumsq=40,
                    energy_max=48, frames=56, used=60, status=64, reserved=68)


def spectrum(values):
    """256 power values from {bin: P}"""
    p = np.zeros(256, dtype=np.float64)
    for d, v in values.items():
        p[d] = v
    return p


# ---- the reference on designed spectra ---------------------------------------------------------------------------

@pytest.mark.parametrize("pct", [1, 50, 85, 100])
def test_one_hot_bin_at_every_d(pct):
    for d in range(1, 256):
        e, m, roll, peak = tr.frame_record(spectrum({d: 3.0 + d}), pct)
        assert e == 16 * (3 + d) and m == d * e
        assert roll == d and peak == d
        assert tr.centroid(e, m) == 4096 * d


def test_two_equal_maxima_the_smaller_bin_wins():
    for lo, hi in ((1, 2), (1, 255), (31, 32), (100, 200), (254, 255)):
        _, _, _, peak = tr.frame_record(spectrum({lo: 7.0, hi: 7.0, 50: 6.5}), 85)
        assert peak == lo
    # ... and a larger value further up still wins
    assert tr.frame_record(spectrum({3: 7.0, 9: 7.0625}), 85)[3] == 9


def test_pct_100_is_the_last_non_zero_bin():
    assert tr.frame_record(spectrum({4: 1.0, 17: 2.0, 200: 0.0625}), 100)[2] == 200
    assert tr.frame_record(spectrum({4: 1.0, 17: 2.0, 200: 0.0624}), 100)[2] == 17   # floor(16 * 0.0624) = 0
    assert tr.frame_record(spectrum({255: 1.0}), 100)[2] == 255


def test_rolloff_exactly_on_the_threshold():
    # Q = 16 * (1, 1, 1, 1) in bins 10, 20, 30, 40: the prefix reaches exactly 50 % at bin 20 and 75 % at bin 30
    p = spectrum({10: 1.0, 20: 1.0, 30: 1.0, 40: 1.0})
    assert tr.frame_record(p, 50)[2] == 20
    assert tr.frame_record(p, 51)[2] == 30
    assert tr.frame_record(p, 75)[2] == 30
    assert tr.frame_record(p, 25)[2] == 10
    assert tr.frame_record(p, 1)[2] == 10


def test_all_zero():
    assert tr.frame_record(np.zeros(256), 85) == (0, 0, 1, 1)
    assert tr.frame_record(np.full(256, 0.06), 1) == (0, 0, 1, 1)   # below one sixteenth everywhere
    rec = tr.song_record([(0, 0, 1, 1)] * 3, 0)
    assert rec["used"] == 0 and rec["frames"] == 3 and rec["energy_max"] == 0
    assert rec["centroid_sum"] == rec["rolloff_sumsq"] == rec["peak_sum"] == 0


def test_song_record_sums_and_min_energy():
    frames = [(100, 250, 3, 2), (0, 0, 1, 1), (10, 10, 1, 1), (1 << 49, 255 << 49, 255, 255)]
    rec = tr.song_record(frames, 0)
    cs = [(250 << 12) // 100, 4096, 255 * 4096]
    assert rec["used"] == 3 and rec["centroid_sum"] == sum(cs) and rec["centroid_sumsq"] == sum(c * c for c in cs)
    assert rec["rolloff_sum"] == 3 + 1 + 255 and rec["peak_sumsq"] == 4 + 1 + 255 ** 2 and rec["energy_max"] == 1 << 49
    assert tr.song_record(frames, 1)["used"] == 3
    assert tr.song_record(frames, 11)["used"] == 2
    assert tr.song_record(frames, 100)["used"] == 2
    assert tr.song_record(frames, 1 << 63) == dict(tr.song_record([], 0), frames=4, energy_max=1 << 49)


# ---- mutations: each must change the answer on these inputs ------------------------------------------------------------

ON_THRESHOLD = {10: 1.0, 20: 1.0, 30: 1.0, 40: 1.0}


def test_mutation_exclusive_prefix():
    assert tr.frame_record(spectrum(ON_THRESHOLD), 50)[2] == 20
    assert tr.frame_record(spectrum(ON_THRESHOLD), 50, exclusive=True)[2] != 20
    assert tr.frame_record(spectrum({77: 5.0}), 85, exclusive=True)[2] != 77


def test_mutation_strict_compare():
    assert tr.frame_record(spectrum(ON_THRESHOLD), 50, strict=True)[2] == 30      # not 20
    assert tr.frame_record(spectrum({9: 2.0}), 100, strict=True)[2] != 9
    assert tr.frame_record(np.zeros(256), 85, strict=True)[2] != 1


def test_mutation_bin_zero_included():
    p = spectrum({0: 100.0, 40: 1.0})
    good, bad = tr.frame_record(p, 85), tr.frame_record(p, 85, bin0=True)
    assert good == (16, 640, 40, 40)
    assert bad[0] != good[0] and bad[2] != good[2] and bad[3] != good[3]
    assert tr.centroid(bad[0], bad[1]) != tr.centroid(good[0], good[1])


def test_mutation_rounding_instead_of_floor():
    p = spectrum({5: 0.99 / 16, 6: 1.5 / 16, 7: 1.0 / 16})     # Q = 0, 1, 1 by floor; 1, 2, 1 to nearest
    good, bad = tr.frame_record(p, 85), tr.frame_record(p, 85, round_q=True)
    assert good == (2, 13, 7, 6)
    assert bad[0] == 4 and bad[3] == 6 and bad[1] != good[1]
    assert tr.centroid(2, 13) == 26624 and tr.centroid(3, 20) == 27306 and tr.centroid(3, 20, rounded=True) == 27307


# ---- host arithmetic of the library ------------------------------------------------------------------------------

def test_header_bindings_exports_and_package_agree():
    text = open(os.path.join(ROOT, "include", "bliss_amd.h")).read()
    declared = set(re.findall(r"\b(?:int|double) (bl_amd_(?:ctx_)?timbre_\w+)\(", text))
    assert declared == set(NEW_SYMBOLS)
    lib = bliss_amd.load()
    for name, res in NEW_SYMBOLS.items():
        assert name in _lib.SYMBOLS, name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == _lib.SYMBOLS[name][1]
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, stdout=subprocess.PIPE,
                         text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert set(NEW_SYMBOLS) <= exported
    for name in ("timbre_batch_host", "timbre_to_numpy", "timbre_hz", "SongTimbre", "FrameTimbre"):
        assert name in bliss_amd.__all__ and getattr(bliss_amd, name) is not None
    assert callable(bliss_amd.DeviceCorpus.timbre) and callable(bliss_amd.DeviceCorpus.fetch_timbre)


def test_record_layouts():
    for S, dt, offsets, size, cname in ((_lib.FrameTimbre, TIMBRE_FRAME_DTYPE, FRAME_OFFSETS, 24, "bl_amd_frame_timbre"),
                                        (_lib.SongTimbre, TIMBRE_SONG_DTYPE, SONG_OFFSETS, 72, "bl_amd_song_timbre")):
        assert C.sizeof(S) == size and dt.itemsize == size
        assert [f[0] for f in S._fields_] == list(offsets) == list(dt.names)
        for name, off in offsets.items():
            assert getattr(S, name).offset == off and dt.fields[name][1] == off, name
        src = "#include <stddef.h>\n#include \"bliss_amd.h\"\n" + "".join(
            f"_Static_assert(offsetof({cname}, {k}) == {v}, \"{k}\");\n" for k, v in offsets.items()) + \
            f"_Static_assert(sizeof({cname}) == {size}, \"size\");\n"
        subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"],
                       input=src, text=True, check=True)
    songs, frames = bliss_amd.timbre_to_numpy(bytes(range(72)) * 2, bytes(range(24)) * 5)
    assert songs.shape == (2,) and frames.shape == (5,) and int(frames["peak"][0]) == 0x17161514
    assert int(songs["used"][1]) == 0x3F3E3D3C


def test_timbre_frames():
    lib = bliss_amd.load()
    f = lib.bl_amd_timbre_frames
    assert [f(n, 1) for n in (0, 1, 511, 512, 513, 1023, 1024, 5120)] == [0, 0, 0, 1, 1, 1, 2, 10]
    assert [f(n, 2) for n in (0, 1023, 1024, 1025, 2047, 2048, 2049)] == [0, 0, 1, 1, 1, 2, 2]
    assert f(2 ** 31 - 1, 1) == (2 ** 31 - 1) // 512 and f(2 ** 31 - 1, 2) == (2 ** 31 - 1) // 1024
    assert [f(-1, 1), f(1024, 0), f(1024, 3), f(1024, -1)] == [-1, -1, -1, -1]


def _song_records(rows):
    st = np.zeros(len(rows), dtype=TIMBRE_SONG_DTYPE)
    for i, (cs, rs, ps) in enumerate(rows):
        st["centroid_sum"][i], st["centroid_sumsq"][i] = sum(cs), sum(c * c for c in cs)
        st["rolloff_sum"][i], st["rolloff_sumsq"][i] = sum(rs), sum(r * r for r in rs)
        st["peak_sum"][i], st["peak_sumsq"][i] = sum(ps), sum(p * p for p in ps)
        st["used"][i] = st["frames"][i] = len(cs)
    return st


def test_hz_helpers_against_numpy():
    rng = np.random.default_rng(7)
    rows = []
    for n in (1, 2, 17, 300, 4000):
        rows.append(([int(x) for x in rng.integers(4096, 255 * 4096 + 1, n)], [int(x) for x in rng.integers(1, 256, n)],
                     [int(x) for x in rng.integers(1, 256, n)]))
    rows.append(([255 * 4096] * 1000, [255] * 1000, [1] * 1000))     # no spread: the variance is exactly 0
    rows.append(([4096, 255 * 4096] * 2000, [1, 255] * 2000, [128, 129] * 2000))
    st = _song_records(rows)
    for rate in (22050, 44100):
        hz = bliss_amd.timbre_hz(st, rate)
        for i, (cs, rs, ps) in enumerate(rows):
            for name, vals, unit in (("centroid", cs, rate / 512 / 4096), ("rolloff", rs, rate / 512),
                                     ("peak", ps, rate / 512)):
                v = np.array(vals, dtype=np.float64) * unit
                assert hz[name + "_hz"][i] == pytest.approx(v.mean(), rel=1e-12)
                assert hz[name + "_std_hz"][i] == pytest.approx(v.std(), rel=1e-9, abs=1e-9 * v.mean())
    assert hz["centroid_std_hz"][5] == 0 and hz["peak_std_hz"][5] == 0
    lib = bliss_amd.load()
    rec = st.ctypes.data_as(C.POINTER(_lib.SongTimbre))
    assert lib.bl_amd_timbre_rolloff_hz(rec, 22050, None) == hz_of(rows[0][1], 22050)   # std_hz may be NULL


def hz_of(vals, rate):
    return pytest.approx(float(np.mean(vals)) * rate / 512, rel=1e-12)


def test_hz_helpers_without_a_used_frame():
    st = np.zeros(1, dtype=TIMBRE_SONG_DTYPE)
    st["frames"] = 9
    hz = bliss_amd.timbre_hz(st)
    assert all(math.isnan(hz[name][0]) for name in hz.dtype.names)
    lib = bliss_amd.load()
    std = C.c_double(1.0)
    assert math.isnan(lib.bl_amd_timbre_centroid_hz(None, 22050, C.byref(std))) and math.isnan(std.value)
    for bad in (np.zeros(0, TIMBRE_SONG_DTYPE), np.zeros((2, 2), TIMBRE_SONG_DTYPE), np.zeros(72, np.uint8)):
        with pytest.raises(ValueError):
            bliss_amd.timbre_hz(bad)


# ---- argument checks: all of them come before the first touch of a device ----------------------------------------

def _desc(items):
    d = (_lib.SongDesc * len(items))()
    for i, (off, n, ch) in enumerate(items):
        d[i].pcm_offset, d[i].n_samples, d[i].channels = off, n, ch
    return d


def test_device_entry_points_reject_bad_arguments_and_write_nothing():
    lib = bliss_amd.load()
    buf = np.zeros(8192, np.int16)
    pcm = buf.ctypes.data + (-buf.ctypes.data) % 16
    good = [(0, 2048, 2), (2048, 1030, 1)]          # F = 2 and 2
    songs = (_lib.SongTimbre * 2)()
    frames = (_lib.FrameTimbre * 4)()
    C.memset(songs, 0xA5, C.sizeof(songs))
    C.memset(frames, 0xA5, C.sizeof(frames))
    so, fo = C.addressof(songs), C.addressof(frames)

    def both(pcm_, desc, n, pct, so_, fo_, nrec):
        a = lib.bl_amd_timbre_batch_device(pcm_, desc, n, pct, 0, so_, fo_, nrec, None)
        b = lib.bl_amd_ctx_timbre_batch_device(None, pcm_, desc, n, pct, 0, so_, fo_, nrec, None)
        return a, b

    d = _desc(good)
    cases = [
        (pcm, d, 2, 0, so, fo, 4), (pcm, d, 2, 101, so, fo, 4), (pcm, d, 2, -1, so, fo, 4),     # pct
        (pcm, _desc([(0, 2048, 3), good[1]]), 2, 85, so, fo, 4),                               # channels 3
        (pcm, _desc([(0, 2048, 0), good[1]]), 2, 85, so, fo, 4),
        (pcm, _desc([good[0], (2048, 511, 1)]), 2, 85, so, fo, 2),                             # F = 0
        (pcm, _desc([good[0], (2048, 1023, 2)]), 2, 85, so, None, 0),                          # F = 0, no frame output
        (pcm, _desc([(0, -1, 1), good[1]]), 2, 85, so, None, 0),
        (pcm, _desc([good[0], (2049, 1030, 1)]), 2, 85, so, fo, 4),                            # an odd pcm_offset
        (pcm, _desc([good[0], (2052, 1030, 1)]), 2, 85, so, fo, 4),                            # no multiple of 8
        (pcm, d, 2, 85, so, fo, 3), (pcm, d, 2, 85, so, fo, 5), (pcm, d, 2, 85, so, fo, 0),    # n_frame_records
        (pcm, d, 0, 85, so, fo, 0), (pcm, d, -1, 85, so, fo, 0),                               # n_songs
        (None, d, 2, 85, so, fo, 4), (pcm, None, 2, 85, so, fo, 4), (pcm, d, 2, 85, None, fo, 4),   # NULL pointers
        (pcm + 2, d, 2, 85, so, fo, 4), (pcm + 8, d, 2, 85, so, fo, 4),                        # d_pcm not 16-byte aligned
    ]
    for case in cases:
        assert both(*case) == (U, U), case
    assert bytes(songs) == b"\xa5" * C.sizeof(songs) and bytes(frames) == b"\xa5" * C.sizeof(frames)


def test_host_entry_point_rejects_bad_arguments():
    lib = bliss_amd.load()
    a = np.ones(2048, np.int16)
    ptrs = (C.c_void_p * 2)(a.ctypes.data, a.ctypes.data)
    out = (_lib.SongTimbre * 2)()
    C.memset(out, 0xA5, C.sizeof(out))
    i32 = C.c_int32 * 2

    def call(ptrs_, ns, chs, n, pct, out_):
        return lib.bl_amd_timbre_batch_host(ptrs_, ns, chs, n, pct, 0, out_, None)
    assert call(ptrs, i32(2048, 2048), i32(1, 2), 2, 0, out) == U
    assert call(ptrs, i32(2048, 2048), i32(1, 2), 2, 101, out) == U
    assert call(ptrs, i32(2048, 2048), i32(1, 3), 2, 85, out) == U
    assert call(ptrs, i32(2048, 1023), i32(1, 2), 2, 85, out) == U
    assert call(ptrs, i32(2048, 2048), i32(1, 2), 0, 85, out) == U
    assert call(None, i32(2048, 2048), i32(1, 2), 2, 85, out) == U
    assert call(ptrs, None, i32(1, 2), 2, 85, out) == U
    assert call(ptrs, i32(2048, 2048), None, 2, 85, out) == U
    assert call(ptrs, i32(2048, 2048), i32(1, 2), 2, 85, None) == U
    assert call((C.c_void_p * 2)(a.ctypes.data, None), i32(2048, 2048), i32(1, 2), 2, 85, out) == U
    assert bytes(out) == b"\xa5" * C.sizeof(out)


@pytest.mark.parametrize("kwargs", [dict(pct=0), dict(pct=101), dict(pct=85.0), dict(pct=True), dict(min_energy=-1),
                                    dict(min_energy=2 ** 64), dict(min_energy=1.5)])
def test_python_wrappers_reject_bad_parameters(kwargs):
    with pytest.raises(ValueError):
        bliss_amd.timbre_batch_host([np.zeros(1024, np.int16)], 1, **kwargs)


@pytest.mark.parametrize("pcm, channels", [
    ([np.zeros(1024, np.int16)], 3), ([np.zeros(1024, np.int16)], [1, 2]), ([], 1),
    ([np.zeros(511, np.int16)], 1), ([np.zeros(2048, np.int16), np.zeros(1023, np.int16)], 2),   # no whole frame
])
def test_python_wrapper_rejects_bad_songs(pcm, channels):
    with pytest.raises(ValueError):
        bliss_amd.timbre_batch_host(pcm, channels)
