"""Signal levels (bl_amd_levels_*, bl_amd_gapless_host, bliss_amd.levels_batch_host / gapless_links / levels_db /
DeviceCorpus.levels) without a device: the header, the bindings, the export list and the package agree on the names and
on the record's layout, the wrappers check their arguments before anything touches the library, the device and host
entry points have no CPU path, and what is plain host arithmetic — the gapless rule and the dB helpers — is held against
numpy restatements."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bliss_amd
from bliss_amd import _lib
from bliss_amd.batch import LEVELS_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = {
    "bl_amd_levels_batch_device": C.c_int, "bl_amd_ctx_levels_batch_device": C.c_int,
    "bl_amd_levels_batch_host": C.c_int, "bl_amd_gapless_host": C.c_int,
    "bl_amd_levels_peak_db": C.c_double, "bl_amd_levels_rms_db": C.c_double,
}
OFFSETS = dict(sum=0, sum_sq=16, peak=32, zero_cross=40, clipped=48, lead=56, trail=60, frames=64, status=68, head=72,
               tail=76)


def test_header_bindings_exports_and_package_agree():
    text = open(os.path.join(ROOT, "include", "bliss_amd.h")).read()
    declared = set(re.findall(r"\b(?:int|double) (bl_amd_(?:(?:ctx_)?levels_|gapless_)\w+)\(", text))
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
    for name in ("levels_batch_host", "levels_to_numpy", "levels_db", "gapless_links", "SongLevels"):
        assert name in bliss_amd.__all__ and getattr(bliss_amd, name) is not None
    assert callable(bliss_amd.DeviceCorpus.levels) and callable(bliss_amd.DeviceCorpus.fetch_levels)


def test_record_layout():
    S = _lib.SongLevels
    assert C.sizeof(S) == 80 and LEVELS_DTYPE.itemsize == 80
    assert [f[0] for f in S._fields_] == list(OFFSETS) == list(LEVELS_DTYPE.names)
    for name, off in OFFSETS.items():
        assert getattr(S, name).offset == off, name
        assert LEVELS_DTYPE.fields[name][1] == off, name
    # the C compiler lays the struct of the header out the same way
    src = "#include <stddef.h>\n#include \"bliss_amd.h\"\n" + "".join(
        f"_Static_assert(offsetof(bl_amd_song_levels, {k}) == {v}, \"{k}\");\n" for k, v in OFFSETS.items()) + \
        "_Static_assert(sizeof(bl_amd_song_levels) == 80, \"size\");\n"
    subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"],
                   input=src, text=True, check=True)
    raw = bytes(range(80)) * 3
    a = bliss_amd.levels_to_numpy(raw)
    assert a.shape == (3,) and a.tobytes() == raw and a["head"][1].tolist() == [0x4948, 0x4B4A]


@pytest.mark.parametrize("silence", [-1, 32768, True, 1.0, "0", None, 2 ** 40])
def test_wrappers_reject_a_bad_silence(silence):
    pcm = [np.zeros(16, np.int16)]
    with pytest.raises(ValueError):
        bliss_amd.levels_batch_host(pcm, 1, silence=silence)


@pytest.mark.parametrize("pcm, channels", [
    ([np.zeros(16, np.int16)], 3), ([np.zeros(16, np.int16)], 0), ([np.zeros(16, np.int16)], [1, 2]),
    ([np.zeros(16, np.int16), np.zeros(16, np.int16)], [1, 4]), ([np.zeros(16, np.int16)], True),
    ([np.zeros(16, np.int16)], 2.0),
    ([], 1),                                                              # no song
    ([np.zeros(1, np.int16)], 1), ([np.zeros(16, np.int16), np.zeros(0, np.int16)], 2),   # shorter than 2 samples
])
def test_host_wrapper_rejects_bad_songs(pcm, channels):
    with pytest.raises(ValueError):
        bliss_amd.levels_batch_host(pcm, channels)


def _corpus_without_a_device(lengths, channels):
    """a DeviceCorpus as far as DeviceCorpus.levels() looks before it touches the library"""
    c = object.__new__(bliss_amd.DeviceCorpus)
    n = len(lengths)
    c.n_songs = n
    c.desc = (_lib.SongDesc * n)()
    for i in range(n):
        c.desc[i].n_samples, c.desc[i].channels = lengths[i], channels[i]

    class _Never:
        def __getattr__(self, name):
            raise AssertionError(f"the wrapper reached for .{name} before checking its arguments")
    c.lib = c.torch = c.pcm = _Never()
    c.levels_raw = None
    return c


@pytest.mark.parametrize("lengths, channels, silence", [
    ([16], [1], -1), ([16], [1], 32768), ([16], [1], True), ([16], [1], 0.0),
    ([16, 16], [1, 3], 0), ([16, 1], [1, 1], 0), ([], [], 0),
])
def test_device_wrapper_rejects_bad_arguments(lengths, channels, silence):
    with pytest.raises(ValueError):
        _corpus_without_a_device(lengths, channels).levels(silence=silence)


@pytest.mark.parametrize("fn", [bliss_amd.gapless_links, bliss_amd.levels_db])
def test_record_consumers_reject_what_is_no_record_array(fn):
    for bad in (np.zeros(0, LEVELS_DTYPE), np.zeros((2, 2), LEVELS_DTYPE), np.zeros(80, np.uint8), [1, 2, 3]):
        with pytest.raises(ValueError):
            fn(bad)


def test_entry_points_fail_loudly_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present: tests/test_gpu_levels.py runs these calls")
    lib = bliss_amd.load()
    n = 2
    desc = (_lib.SongDesc * n)()
    for i in range(n):
        desc[i].pcm_offset, desc[i].n_samples, desc[i].channels = 64 * i, 40, 1 + i
    out = (_lib.SongLevels * n)()
    C.memset(out, 0xAB, C.sizeof(out))
    pcm = np.zeros(128, np.int16)
    aligned = pcm.ctypes.data + (-pcm.ctypes.data) % 16   # the argument checks pass: it is the device that is missing
    U = _lib.BL_UNEXPECTED
    assert lib.bl_amd_levels_batch_device(aligned, desc, n, 0, C.addressof(out), None) == U
    assert lib.bl_amd_ctx_levels_batch_device(None, aligned, desc, n, 0, C.addressof(out), None) == U
    songs = [np.ones(40, np.int16), np.ones(40, np.int16)]
    ptrs = (C.c_void_p * n)(*[s.ctypes.data for s in songs])
    assert lib.bl_amd_levels_batch_host(ptrs, (C.c_int32 * n)(40, 40), (C.c_int32 * n)(1, 2), n, 0, out) == U
    assert bytes(out) == b"\xab" * C.sizeof(out)
    with pytest.raises(RuntimeError):
        bliss_amd.levels_batch_host(songs, [1, 2], silence=32767)   # the limits pass the Python checks


def _records(pairs):
    """records whose tail / head are the given ((t0, t1), (h0, h1)) pairs"""
    lv = np.zeros(len(pairs), dtype=LEVELS_DTYPE)
    for i, (tail, head) in enumerate(pairs):
        lv["tail"][i], lv["head"][i] = tail, head
    return lv


def _gapless_f32(lv):
    """ref examples/detect-gapless.c:35-54 with numpy's float32: the quotient is an f32, the compare a double's"""
    out = []
    for i in range(lv.size - 1):
        ok = False
        for k in (0, 1):
            t, h = int(lv["tail"][i][k]), int(lv["head"][i + 1][k])
            if abs(t) >= 5 and abs(h) >= 5:
                diff = np.abs((np.float32(t) - np.float32(h)) / np.float32(32767))
                assert diff.dtype == np.float32
                ok |= bool(np.float64(diff) < 0.01)
        out.append(ok)
    return out


def test_gapless_rule():
    z = (0, 0)
    # link i -> i + 1 compares the tail of record i with the head of record i + 1
    lv = _records([
        ((1000, 0), z),
        ((1000, 0), (1327, 0)),           # 0 -> 1: |1000 - 1327| = 327, linked through slot 0
        ((-5, 0), (1328, 0)),             # 1 -> 2: 328, not linked
        ((4, 4), (5, 0)),                 # 2 -> 3: magnitude 5 on both sides, linked
        ((3, -20000), (4, 4)),            # 3 -> 4: magnitude 4 never links, however close
        ((0, -20000), (9, -20327)),       # 4 -> 5: slot 1 only, 327 apart
        ((-32768, 32767), (0, -20328)),   # 5 -> 6: slot 1, 328
        ((-32768, 5), (-32441, 32440)),   # 6 -> 7: the extremes, 327 apart in both slots
        ((-200, 200), (-32441, -4)),      # 7 -> 8: slot 0 at the negative end; slot 1 meets a 4
        (z, (200, -200)),                 # 8 -> 9: opposite signs, 400 apart
    ])
    got = bliss_amd.gapless_links(lv)
    assert got.dtype == np.bool_ and got.shape == (lv.size - 1,)
    assert got.tolist() == _gapless_f32(lv) == [True, False, True, False, True, False, True, True, False]
    # every difference around the boundary, at a few levels and both signs: |a - b| <= 327 in integers
    pairs = []
    for base in (5, 400, 20000, 32767 - 330, -32768 + 330, -5):
        for d in range(320, 336):
            for sign in (1, -1):
                b = base + sign * d
                if -32768 <= b <= 32767:
                    pairs.append(((base, 0), z))
                    pairs.append((z, (b, 0)))
    lv = _records(pairs)
    got = bliss_amd.gapless_links(lv)
    assert got.tolist() == _gapless_f32(lv)
    for i in range(0, lv.size - 1, 2):
        a, b = int(lv["tail"][i][0]), int(lv["head"][i + 1][0])
        assert bool(got[i]) == (abs(a) >= 5 and abs(b) >= 5 and abs(a - b) <= 327), (a, b)
    # one song: nothing to write, BL_OK
    lib = bliss_amd.load()
    one = _records([(z, z)])
    guard = (C.c_uint8 * 4)(7, 7, 7, 7)
    assert lib.bl_amd_gapless_host(one.ctypes.data_as(C.POINTER(_lib.SongLevels)), 1, guard) == _lib.BL_OK
    assert lib.bl_amd_gapless_host(one.ctypes.data_as(C.POINTER(_lib.SongLevels)), 1, None) == _lib.BL_OK
    assert list(guard) == [7, 7, 7, 7] and bliss_amd.gapless_links(one).shape == (0,)
    assert lib.bl_amd_gapless_host(one.ctypes.data_as(C.POINTER(_lib.SongLevels)), 0, guard) == _lib.BL_UNEXPECTED
    assert lib.bl_amd_gapless_host(None, 2, guard) == _lib.BL_UNEXPECTED


def test_db_helpers():
    """against numpy, to an absolute 1e-9 dB: two correctly working log10s differ by a few ulp of a double, about 3e-14
    at 100 dB, far below 1e-9, which is far below anything that matters"""
    lib = bliss_amd.load()
    lv = np.zeros(5, dtype=LEVELS_DTYPE)
    lv["frames"] = [1000, 3, 7_938_000, 44100, 10]
    lv["peak"] = [(32768, 1), (12345, 0), (32767, 20000), (1, 0), (0, 0)]
    lv["sum_sq"] = [(1000 * 2 ** 30, 1000), (3 * 12345 ** 2, 0), (2 ** 61 + 12345, 7_938_000 * 9), (1, 0), (0, 0)]
    lv["sum"] = [(-32768 * 1000, 31), (5, 0), (-(2 ** 40), 2 ** 40), (1, 0), (0, 0)]
    lv["zero_cross"] = [(999, 0), (2, 0), (123456, 654321), (0, 0), (0, 0)]
    P = C.POINTER(_lib.SongLevels)
    db = bliss_amd.levels_db(lv)
    for i in range(lv.size):
        rec = lv[i:i + 1].ctypes.data_as(P)
        for c in (0, 1):
            with np.errstate(divide="ignore"):
                peak = 20.0 * np.log10(np.float64(lv["peak"][i][c]) / 32768.0)
                rms = 10.0 * np.log10(np.float64(lv["sum_sq"][i][c]) / (np.float64(lv["frames"][i]) * 2.0 ** 30))
            for got in (lib.bl_amd_levels_peak_db(rec, c), db["peak_db"][i][c]):
                assert got == peak if np.isinf(peak) else abs(got - peak) <= 1e-9, (i, c, got, peak)
            for got in (lib.bl_amd_levels_rms_db(rec, c), db["rms_db"][i][c]):
                assert got == rms if np.isinf(rms) else abs(got - rms) <= 1e-9, (i, c, got, rms)
        for c in (-1, 2, 100):
            assert np.isnan(lib.bl_amd_levels_peak_db(rec, c)) and np.isnan(lib.bl_amd_levels_rms_db(rec, c))
    assert lib.bl_amd_levels_peak_db(lv[0:1].ctypes.data_as(P), 0) == 0.0        # full scale
    assert lib.bl_amd_levels_rms_db(lv[0:1].ctypes.data_as(P), 0) == 0.0         # nothing but -32768
    assert lib.bl_amd_levels_peak_db(lv[1:2].ctypes.data_as(P), 1) == -np.inf    # mono: channel 1
    assert lib.bl_amd_levels_rms_db(lv[4:5].ctypes.data_as(P), 0) == -np.inf     # silence
    assert np.isnan(lib.bl_amd_levels_peak_db(None, 0))
    assert db["dc"][0].tolist() == [-32768.0, 0.031] and db["zcr"][0].tolist() == [1.0, 0.0]
    assert db["zcr"][1][0] == 1.0 and db["dc"][2][1] == 2 ** 40 / 7_938_000
    one = np.zeros(1, dtype=LEVELS_DTYPE)
    one["frames"] = 1
    assert bliss_amd.levels_db(one)["zcr"].tolist() == [[0.0, 0.0]]              # max(frames - 1, 1)
