"""The mel call (bl_amd_mel_*, bliss_amd.mel) without a device.  tests/mel_reference.py, the Python-int restatement the
GPU test compares with, rebuilds the three tables on its own and must land on the library's, entry for entry; the
integer logarithm of bl_ilog2.h (through tests/host/test_ilog2_host.cpp) equals the restatement on the self-test's
values, is monotone and stays within 1 + 2^-10 units below 4096 log2 x; every plausible misreading of the definitions
(mel_reference.SWITCHES) changes a named frame or song of designed spectra (the transform is skipped, P is fed
directly); the host arithmetic of the library agrees with numpy; descriptor.features() takes the new group."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import bliss_amd
import bliss_amd.descriptor as D
import bliss_amd.mel as M
from bliss_amd import _lib
from bliss_amd.records import (CHROMA_DTYPE, FRAME_MEL_DTYPE, LEVELS_DTYPE, MEL_DTYPE, RESULT_DTYPE, RHYTHM_DTYPE,
                               TIMBRE_SONG_DTYPE)
from tests import mel_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = _lib.BL_UNEXPECTED

NEW_SYMBOLS = {
    "bl_amd_mel_frames": C.c_int, "bl_amd_mel_batch_device": C.c_int, "bl_amd_ctx_mel_batch_device": C.c_int,
    "bl_amd_mel_batch_host": C.c_int, "bl_amd_mel_table": C.c_int, "bl_amd_mel_mfcc": C.c_double,
    "bl_amd_mel_flatness_db": C.c_double, "bl_amd_selftest_ilog2": C.c_int,
}
FRAME_OFFSETS = dict(mfcc=0, flat=52)
SONG_OFFSETS = dict(mfcc_sum=0, mfcc_sumsq=104, flat_sum=208, flat_sumsq=216, band_sum=224, frames=480, used=484,
                    status=488, reserved=492)


# ---- the tables --------------------------------------------------------------------------------------------------

def test_edges_come_out_of_the_mel_formula():
    assert mr.edges() == mr.EDGES and len(mr.EDGES) == 34
    margin = min(abs(x - math.floor(x) - 0.5) for x in mr.edges_exact())
    print("nearest rounding boundary:", margin)
    assert margin > 0.05        # 0.056, as bl_mel_table.h says: no libm moves an edge


def test_library_tables_equal_the_reference_entry_for_entry():
    edges, weights, dct = M.mel_table()
    assert [int(v) for v in edges] == list(mr.edges())
    assert weights.shape == (32, 256) and weights.astype(np.int64).tolist() == [list(r) for r in mr.weights()]
    assert dct.shape == (13, 32) and dct.astype(np.int64).tolist() == [list(r) for r in mr.dct()]
    lib = bliss_amd.load()
    assert lib.bl_amd_mel_table(None, None, None) == 0          # any pointer may be NULL
    only = np.zeros(34, np.int32)
    assert lib.bl_amd_mel_table(only.ctypes.data, None, None) == 0 and only.tolist() == list(mr.EDGES)


def test_what_the_kernel_bounds_rest_on():
    w = np.array(mr.weights())
    width = (w > 0).sum(axis=1)
    assert width.min() == 3 and width.max() == 41
    for row in w:                                                # contiguous
        nz = np.nonzero(row)[0]
        assert nz[-1] - nz[0] + 1 == nz.size
    assert (w > 0).sum(axis=0).max() == 2 and w.sum(axis=0).max() == 64 and w.max() == 64
    assert w[:, 0].sum() == 0 and w[:, 1].sum() == 0
    assert w.sum(axis=1).min() == 90 and w.sum(axis=1).max() == 1320
    d = np.array(mr.dct())
    assert (d[0] == 16384).all() and abs(d).max() == 16384 and d[1][0] == 16364 and d[1][31] == -16364
    assert (d[:, ::-1] == d * np.array([(-1) ** k for k in range(13)])[:, None]).all()   # cos(pi k - x) = (-1)^k cos x


# ---- the integer logarithm ---------------------------------------------------------------------------------------

def sweep_value(i):
    """bl_ilog2_sweep_value restated"""
    if i < 192:
        return (1 << (i // 3)) - 1 + i % 3
    v = (0x9E3779B97F4A7C15 * (i - 191)) % (1 << 64)
    return (v >> (i & 63)) | 1


def test_ilog2_header_on_the_cpu_equals_the_restatement(tmp_path):
    exe = str(tmp_path / "test_ilog2_host.bin")
    cc = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                         os.path.join(ROOT, "tests", "host", "test_ilog2_host.cpp"), "-o", exe],
                        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert cc.returncode == 0, "g++ failed:\n" + cc.stdout
    out = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    lines = out.stdout.split("\n")
    assert out.returncode == 0 and lines[-2] == "OK", lines[-5:]
    got = np.array([ln.split() for ln in lines[:-2]], dtype=np.uint64)
    n = 192 + 2 ** 17
    want_x = np.array([sweep_value(i) for i in range(1, n)], dtype=np.uint64)
    assert got.shape == (n - 1, 2) and np.array_equal(got[:, 0], want_x)
    assert len(set(want_x.tolist())) > 2 ** 16 and int(want_x.max()) > 2 ** 63 and int(want_x.min()) == 1
    assert {int(x).bit_length() for x in want_x.tolist()} == set(range(1, 65))      # every magnitude
    assert np.array_equal(got[:, 1], mr.ilog2_np(want_x))
    for x, l in got[:400].tolist() + got[::997].tolist():       # the vectorised form is the int form
        assert mr.ilog2(x) == l


def test_ilog2_known_values_powers_and_monotony():
    assert [mr.ilog2(x) for x in (1, 2, 3, 2 ** 63)] == [0, 4096, 6492, 258048]
    assert all(mr.ilog2(1 << e) == 4096 * e for e in range(64))
    a = mr.ilog2_np(np.arange(1, 2 ** 20 + 1, dtype=np.uint64)).astype(np.int64)
    assert (np.diff(a) >= 0).all() and a[0] == 0 and a[-1] == 20 * 4096
    assert mr.ilog2(2 ** 64 - 1) == 64 * 4096 - 1 or mr.ilog2(2 ** 64 - 1) < 64 * 4096


def test_ilog2_error_bound():
    """0 <= 4096 log2 x - L(x) < 1 + 2^-10 on 200 000 random values of every magnitude up to 2^63"""
    rng = np.random.default_rng(5)
    xs = rng.integers(1, 2 ** 63, 200000, dtype=np.uint64) >> rng.integers(0, 63, 200000).astype(np.uint64)
    xs = xs[xs >= 1]
    ls = mr.ilog2_np(xs)
    err = [4096.0 * math.log2(int(x)) - int(l) for x, l in zip(xs.tolist(), ls.tolist())]
    print("4096 log2 x - L(x): min", min(err), "max", max(err), "over", len(err), "values")
    assert min(err) >= 0.0 and max(err) < 1.0 + 2.0 ** -10


# ---- the reference on designed spectra, and what every wrong form does to them -------------------------------------

def spectrum(values):
    p = np.zeros(256, dtype=np.float64)
    for d, v in values.items():
        p[d] = v
    return p


DESIGNED = {
    "silence": np.zeros(256),
    "q1_bin27": spectrum({27: 1 / 16}),                      # Q = 1 on an edge that is a whole bin (432 = 16 * 27)
    "bin27": spectrum({27: 1000.0}),
    "bin163": spectrum({163: 2.0 ** 40}),                    # the other such edge (2608 = 16 * 163)
    "bin250": spectrum({250: 12345.0}),                      # band 31 alone
    "flat": np.r_[0.0, np.full(255, 64.0)],
    "loud": np.r_[0.0, np.full(255, 2.0 ** 37)],             # energy 2^49.0: the largest S
    "slope": np.r_[0.0, 1e6 / np.arange(1, 256) ** 2],
    "two": spectrum({5: 3.0, 200: 7e5}),
}
# the frames a wrong form must change, and one it must leave alone (None: there is none)
CHANGES = {
    "closed_left": (("q1_bin27", "bin27", "bin163", "flat"), "bin250"),
    "round_w": (("bin250", "flat", "slope", "two"), "bin27"),
    "no_plus1": (("q1_bin27", "two"), "loud"),
    "iters11": (("q1_bin27", "bin27", "flat", "loud"), "silence"),
    "norm31": (("q1_bin27", "bin27", "bin163", "flat", "loud", "slope"), None),
    "even_dct": (("q1_bin27", "bin163", "flat", "two"), "silence"),
    "trunc_shift": (("bin27", "bin163", "flat", "loud"), "silence"),
    "bands31": (("silence", "bin250", "flat", "loud"), "two"),
}


def test_designed_frames_have_the_answers_the_definitions_give():
    f = {k: mr.frame_record(v) for k, v in DESIGNED.items()}
    z = f["silence"]
    assert z["energy"] == 0 and z["S"] == [0] * 32 and z["E"] == [0] * 32 and z["mfcc"] == [0] * 13 and z["flat"] == 0
    q1 = f["q1_bin27"]                                       # S[10] = 64, everything else 0
    assert q1["energy"] == 1 and q1["S"] == [64 if b == 10 else 0 for b in range(32)]
    assert q1["E"][10] == mr.ilog2(65) and q1["flat"] == 32 * mr.ilog2(64 + 32) - 160 * 4096 - mr.ilog2(65)
    assert q1["mfcc"][0] == mr.ilog2(65) and q1["mfcc"][1] == (mr.dct()[1][10] * mr.ilog2(65)) >> 14
    flat, loud = f["flat"], f["loud"]
    assert flat["energy"] == 255 * 1024 and loud["energy"] == 255 * 2 ** 41 and 2 ** 48 < loud["energy"] < 2 ** 50
    assert max(loud["S"]) == 1320 * 2 ** 41 and max(loud["S"]) < 2 ** 56 and max(loud["E"]) < 2 ** 18
    assert abs(loud["mfcc"][0]) < 2 ** 23 and loud["mfcc"][0] == sum(loud["E"])
    # the same shape 2^31 times louder: the levels move by 31 * 4096 (up to L's last unit), the flatness hardly at all
    assert all(abs(a - b - 31 * 4096) <= 1 for a, b in zip(loud["E"], flat["E"]))
    assert abs(loud["flat"] - flat["flat"]) <= 33 and 0 < flat["flat"] < f["bin27"]["flat"] < f["bin163"]["flat"]
    assert any(v < 0 for v in f["bin27"]["mfcc"]) and f["two"]["mfcc"][1] < 0


@pytest.mark.parametrize("switch", sorted(CHANGES))
def test_every_wrong_form_changes_a_named_frame(switch):
    changed, unchanged = CHANGES[switch]
    for name in changed:
        good, bad = mr.frame_record(DESIGNED[name]), mr.frame_record(DESIGNED[name], **{switch: True})
        assert (good["E"], good["mfcc"], good["flat"]) != (bad["E"], bad["mfcc"], bad["flat"]), (switch, name)
    if unchanged is not None:
        assert mr.frame_record(DESIGNED[unchanged]) == mr.frame_record(DESIGNED[unchanged], **{switch: True})


def test_the_wrong_forms_in_detail():
    w, wc, wr = np.array(mr.weights()), np.array(mr.weights(closed_left=True)), np.array(mr.weights(round_w=True))
    assert np.argwhere(w != wc).tolist() == [[10, 27], [27, 163]] and w[10][27] == w[27][163] == 64
    assert (w != wr).sum() == 249 and (wr >= w).all() and wr.sum(axis=0).max() > 64     # rounding breaks the column bound
    good, bad = mr.frame_record(DESIGNED["q1_bin27"]), mr.frame_record(DESIGNED["q1_bin27"], no_plus1=True)
    assert good["E"][10] == mr.ilog2(65) > bad["E"][10] == 6 * 4096
    assert mr.ilog2(3, iters11=True) == 6492 and mr.ilog2(11, iters11=True) == mr.ilog2(11) - 1   # the twelfth digit
    assert mr.dct(even_dct=True)[1][0] == 16384 != mr.dct()[1][0]
    acc = -5 * 16384 - 1                                      # floor: -6, towards zero: -5
    assert acc >> 14 == -6 and -((-acc) >> 14) == -5
    good, bad = mr.frame_record(DESIGNED["bin27"]), mr.frame_record(DESIGNED["bin27"], trunc_shift=True)
    assert [b - g for g, b in zip(good["mfcc"], bad["mfcc"])] == [1 if g < 0 else 0 for g in good["mfcc"]]


def test_song_record_and_the_used_rule():
    names = list(DESIGNED)
    frames, rec = mr.from_power([DESIGNED[k] for k in names])
    assert rec["frames"] == 9 and rec["used"] == 8 and rec["status"] == 0 and rec["reserved"] == 0     # not the silence
    used = [f for f in frames if f["energy"] > 0]
    assert rec["mfcc_sum"][3] == sum(f["mfcc"][3] for f in used) and rec["mfcc_sum"][3] < 0 < rec["mfcc_sumsq"][3]
    assert rec["flat_sumsq"] == sum(f["flat"] ** 2 for f in used) and rec["band_sum"][31] == sum(f["E"][31] for f in used)
    e = frames[names.index("bin27")]["energy"]
    assert e == 16000
    at, above = mr.from_power([DESIGNED[k] for k in names], e)[1], mr.from_power([DESIGNED[k] for k in names], e + 1)[1]
    assert at["used"] == above["used"] + 1 == 7
    # the mutation: > for >= drops the frame whose energy equals the threshold
    wrong = mr.from_power([DESIGNED[k] for k in names], e, strict_used=True)[1]
    assert wrong["used"] == at["used"] - 1 and wrong["mfcc_sum"] != at["mfcc_sum"] and wrong == above
    assert mr.from_power([DESIGNED[k] for k in names], 1 << 62)[1] == dict(mr.song_record([], 0), frames=9)


# ---- header, bindings, exports, layouts --------------------------------------------------------------------------

def test_header_bindings_exports_and_package_agree():
    text = open(os.path.join(ROOT, "include", "bliss_amd.h")).read()
    declared = set(re.findall(r"\b(?:int|double) (bl_amd_(?:(?:ctx_)?mel_|selftest_ilog2)\w*)\(", text))
    assert declared == set(NEW_SYMBOLS)
    lib = bliss_amd.load()
    for name, res in NEW_SYMBOLS.items():
        assert name in _lib.SYMBOLS, name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == _lib.SYMBOLS[name][1]
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, stdout=subprocess.PIPE,
                         text=True).stdout
    assert set(NEW_SYMBOLS) <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in ("mel_device", "fetch_mel", "mel_batch_host", "mel_table", "mel_summary", "mel_to_numpy"):
        assert callable(getattr(M, name)) and name not in bliss_amd.__all__     # imported explicitly


def test_record_layouts():
    for S, dt, offsets, size, cname in ((_lib.FrameMel, FRAME_MEL_DTYPE, FRAME_OFFSETS, 56, "bl_amd_frame_mel"),
                                        (_lib.SongMel, MEL_DTYPE, SONG_OFFSETS, 496, "bl_amd_song_mel")):
        assert C.sizeof(S) == size and dt.itemsize == size
        assert [f[0] for f in S._fields_] == list(offsets) == list(dt.names)
        for name, off in offsets.items():
            assert getattr(S, name).offset == off and dt.fields[name][1] == off, name
        src = "#include <stddef.h>\n#include \"bliss_amd.h\"\n" + "".join(
            f"_Static_assert(offsetof({cname}, {k}) == {v}, \"{k}\");\n" for k, v in offsets.items()) + \
            f"_Static_assert(sizeof({cname}) == {size}, \"size\");\n"
        subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"],
                       input=src, text=True, check=True)
    songs, frames, bands = M.mel_to_numpy(bytes(496 * 2), bytes(range(56)) * 3, bytes(128 * 3))
    assert songs.shape == (2,) and frames.shape == (3,) and bands.shape == (3, 32) and bands.dtype == np.uint32
    assert int(frames["flat"][0]) == 0x37363534 and int(frames["mfcc"][1][12]) == 0x33323130


def test_mel_frames_is_the_timbre_frame_count():
    lib = bliss_amd.load()
    for n, ch in ((0, 1), (511, 1), (512, 1), (1023, 2), (1024, 2), (5120, 1), (2 ** 31 - 1, 2), (-1, 1), (1024, 3)):
        assert lib.bl_amd_mel_frames(n, ch) == lib.bl_amd_timbre_frames(n, ch)
    assert lib.bl_amd_mel_frames(1024, 2) == 1 and lib.bl_amd_mel_frames(1024, 0) == -1


# ---- host arithmetic of the library ------------------------------------------------------------------------------

def _mel_records(rows):
    """rows: per song the list of per-frame (mfcc[13], flat) of its used frames"""
    rec = np.zeros(len(rows), dtype=MEL_DTYPE)
    for i, frames in enumerate(rows):
        for k in range(13):
            rec["mfcc_sum"][i][k] = sum(f[0][k] for f in frames)
            rec["mfcc_sumsq"][i][k] = sum(f[0][k] ** 2 for f in frames)
        rec["flat_sum"][i], rec["flat_sumsq"][i] = sum(f[1] for f in frames), sum(f[1] ** 2 for f in frames)
        rec["used"][i] = rec["frames"][i] = len(frames)
    return rec


def test_summary_against_numpy():
    rng = np.random.default_rng(7)
    rows = []
    for n in (1, 2, 17, 300, 4000):
        rows.append([([int(v) for v in rng.integers(-2 ** 22, 2 ** 22, 13)], int(rng.integers(-40, 2 ** 22)))
                     for _ in range(n)])
    rows.append([([-12345] * 13, 777)] * 1000)                 # no spread: the variance is exactly 0
    rows.append([([2 ** 23 - 1] * 13, -(2 ** 22))] * 5 + [([-(2 ** 23) + 1] * 13, 2 ** 22)] * 5)
    rec = _mel_records(rows)
    s = M.mel_summary(rec)
    unit = 10.0 * math.log10(2.0) / (32 * 4096)
    for i, frames in enumerate(rows):
        m = np.array([f[0] for f in frames], dtype=np.float64) / 4096.0
        fl = np.array([f[1] for f in frames], dtype=np.float64)
        assert s["mfcc"][i] == pytest.approx(m.mean(axis=0), rel=1e-12, abs=1e-12)
        assert s["mfcc_std"][i] == pytest.approx(m.std(axis=0), rel=1e-9, abs=1e-9 * abs(m).max())
        assert s["flatness_db"][i] == pytest.approx(-fl.mean() * unit, rel=1e-12)
        assert s["flatness_std_db"][i] == pytest.approx(fl.std() * unit, rel=1e-9, abs=1e-9 * abs(fl).max() * unit)
    assert (s["mfcc_std"][5] == 0).all() and s["flatness_std_db"][5] == 0 and s["flatness_db"][5] < 0
    assert s["mfcc"][6] == pytest.approx(np.zeros(13), abs=1e-12) and s["mfcc_std"][6][0] == pytest.approx((2 ** 23 - 1) / 4096)
    lib = bliss_amd.load()
    ptr = rec.ctypes.data_as(C.POINTER(_lib.SongMel))
    assert lib.bl_amd_mel_mfcc(ptr, 3, None) == s["mfcc"][0][3]             # std may be NULL
    assert lib.bl_amd_mel_flatness_db(ptr, None) == s["flatness_db"][0]


def test_summary_without_a_used_frame_and_bad_arguments():
    rec = np.zeros(1, dtype=MEL_DTYPE)
    rec["frames"] = 9
    s = M.mel_summary(rec)
    assert np.isnan(s["mfcc"]).all() and np.isnan(s["mfcc_std"]).all() and np.isnan(s["flatness_db"][0])
    lib = bliss_amd.load()
    std = C.c_double(1.0)
    good = _mel_records([[([4096] * 13, 0)]])
    ptr = good.ctypes.data_as(C.POINTER(_lib.SongMel))
    assert lib.bl_amd_mel_mfcc(ptr, 0, C.byref(std)) == 1.0 and std.value == 0.0
    for k in (-1, 13):
        std.value = 1.0
        assert math.isnan(lib.bl_amd_mel_mfcc(ptr, k, C.byref(std))) and math.isnan(std.value)
    assert math.isnan(lib.bl_amd_mel_mfcc(None, 0, C.byref(std))) and math.isnan(lib.bl_amd_mel_flatness_db(None, None))
    for bad in (np.zeros(0, MEL_DTYPE), np.zeros((2, 2), MEL_DTYPE), np.zeros(496, np.uint8)):
        with pytest.raises(ValueError):
            M.mel_summary(bad)


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
    songs, frames, bands = (_lib.SongMel * 2)(), (_lib.FrameMel * 4)(), (C.c_uint32 * 128)()
    for b in (songs, frames, bands):
        C.memset(b, 0xA5, C.sizeof(b))
    so, fo, bo = C.addressof(songs), C.addressof(frames), C.addressof(bands)

    def both(pcm_, desc, n, so_, fo_, bo_, nrec):
        a = lib.bl_amd_mel_batch_device(pcm_, desc, n, 0, so_, fo_, bo_, nrec, None)
        b = lib.bl_amd_ctx_mel_batch_device(None, pcm_, desc, n, 0, so_, fo_, bo_, nrec, None)
        return a, b

    d = _desc(good)
    cases = [
        (pcm, _desc([(0, 2048, 3), good[1]]), 2, so, fo, bo, 4),                               # channels 3
        (pcm, _desc([(0, 2048, 0), good[1]]), 2, so, fo, bo, 4),
        (pcm, _desc([good[0], (2048, 511, 1)]), 2, so, fo, bo, 2),                             # F = 0
        (pcm, _desc([good[0], (2048, 1023, 2)]), 2, so, None, None, 0),                        # F = 0, no frame output
        (pcm, _desc([(0, -1, 1), good[1]]), 2, so, None, None, 0),
        (pcm, _desc([good[0], (2049, 1030, 1)]), 2, so, fo, bo, 4),                            # an odd pcm_offset
        (pcm, _desc([good[0], (2052, 1030, 1)]), 2, so, fo, bo, 4),                            # no multiple of 8
        (pcm, d, 2, so, fo, bo, 3), (pcm, d, 2, so, fo, bo, 5), (pcm, d, 2, so, fo, None, 3),  # n_frame_records
        (pcm, d, 2, so, None, bo, 5), (pcm, d, 2, so, fo, bo, 0),
        (pcm, d, 0, so, fo, bo, 0), (pcm, d, -1, so, fo, bo, 0),                               # n_songs
        (None, d, 2, so, fo, bo, 4), (pcm, None, 2, so, fo, bo, 4), (pcm, d, 2, None, fo, bo, 4),   # NULL pointers
        (pcm + 2, d, 2, so, fo, bo, 4), (pcm + 8, d, 2, so, fo, bo, 4),                        # d_pcm not 16-byte aligned
    ]
    for case in cases:
        assert both(*case) == (U, U), case
    for b in (songs, frames, bands):
        assert bytes(b) == b"\xa5" * C.sizeof(b)


def test_host_entry_point_and_wrappers_reject_bad_arguments():
    lib = bliss_amd.load()
    a = np.ones(2048, np.int16)
    ptrs = (C.c_void_p * 2)(a.ctypes.data, a.ctypes.data)
    out = (_lib.SongMel * 2)()
    C.memset(out, 0xA5, C.sizeof(out))
    i32 = C.c_int32 * 2

    def call(ptrs_, ns, chs, n, out_):
        return lib.bl_amd_mel_batch_host(ptrs_, ns, chs, n, 0, out_, None, None)
    assert call(ptrs, i32(2048, 2048), i32(1, 3), 2, out) == U
    assert call(ptrs, i32(2048, 1023), i32(1, 2), 2, out) == U
    assert call(ptrs, i32(2048, 2048), i32(1, 2), 0, out) == U
    assert call(None, i32(2048, 2048), i32(1, 2), 2, out) == U
    assert call(ptrs, None, i32(1, 2), 2, out) == U
    assert call(ptrs, i32(2048, 2048), None, 2, out) == U
    assert call(ptrs, i32(2048, 2048), i32(1, 2), 2, None) == U
    assert call((C.c_void_p * 2)(a.ctypes.data, None), i32(2048, 2048), i32(1, 2), 2, out) == U
    assert bytes(out) == b"\xa5" * C.sizeof(out)
    for kw in (dict(min_energy=-1), dict(min_energy=2 ** 64), dict(min_energy=1.5), dict(min_energy=True)):
        with pytest.raises(ValueError):
            M.mel_batch_host([np.zeros(1024, np.int16)], 1, **kw)
    for pcm, ch in (([np.zeros(1024, np.int16)], 3), ([np.zeros(1024, np.int16)], [1, 2]), ([], 1),
                    ([np.zeros(511, np.int16)], 1), ([np.zeros(2048, np.int16), np.zeros(1023, np.int16)], 2)):
        with pytest.raises(ValueError):
            M.mel_batch_host(pcm, ch)


def test_selftest_needs_a_device_or_passes():
    """without a device the self-test reports BL_UNEXPECTED and leaves the counts alone; tests/test_gpu_mel.py runs it"""
    import torch
    if torch.cuda.is_available():
        return
    counts = (C.c_uint64 * 2)(7, 7)
    assert bliss_amd.load().bl_amd_selftest_ilog2(counts) == U and list(counts) == [7, 7]


# ---- descriptors -------------------------------------------------------------------------------------------------

def _records(n):
    res = np.zeros(n, RESULT_DTYPE)
    res["tempo"], res["amplitude"] = np.arange(n) - 1.5, 2.0
    res["frequency"], res["attack"] = -np.arange(n), 0.25
    lv = np.zeros(n, LEVELS_DTYPE)
    lv["frames"] = 1000
    lv["peak"] = [[1000 * (i + 1), 500] for i in range(n)]
    lv["sum_sq"] = [[10 ** 9 * (i + 1), 10 ** 7] for i in range(n)]
    lv["zero_cross"] = [[10 * i, 3] for i in range(n)]
    tb = np.zeros(n, TIMBRE_SONG_DTYPE)
    tb["used"] = 4
    tb["centroid_sum"], tb["centroid_sumsq"] = 4 * 40 * 65536, 4 * (40 * 65536) ** 2
    tb["rolloff_sum"], tb["rolloff_sumsq"] = [4 * (60 + i) for i in range(n)], [4 * (60 + i) ** 2 for i in range(n)]
    rh = np.zeros(n, RHYTHM_DTYPE)
    rh["lag"], rh["r0"], rh["r_lag"], rh["r_prev"], rh["r_next"] = 40, 1000, 500, 400, 400
    ch = np.zeros(n, CHROMA_DTYPE)
    ch["chroma"][1:] = np.arange(1, 13, dtype=np.uint64)
    ml = _mel_records([[([4096 * (k + i) * (-1) ** k for k in range(13)], 1000 * (i + 1))] * 3 for i in range(n - 1)] + [[]])
    return res, lv, tb, rh, ch, ml


def test_features_take_the_mel_group():
    n = 4
    res, lv, tb, rh, ch, ml = _records(n)
    x, names = D.features(res, levels=lv, timbre=tb, rhythm=rh, chroma=ch, mel=ml)
    assert x.shape == (n, 32) and x.dtype == np.float32 and len(names) == len(set(names)) == 32 == D.DIMS
    assert names[25:] == ["flatness_db", "mfcc_1", "mfcc_2", "mfcc_3", "mfcc_4", "mfcc_5", "mfcc_6"]
    s = M.mel_summary(ml)
    assert np.array_equal(x[:, 25], s["flatness_db"].astype(np.float32), equal_nan=True)
    for k in range(1, 7):
        assert np.array_equal(x[:, 25 + k], s["mfcc"][:, k].astype(np.float32), equal_nan=True)
    assert x[1, 26] == -2.0 and x[1, 27] == 3.0 and x[0, 25] == np.float32(-1000 * 10 * math.log10(2) / 131072)
    assert np.isnan(x[n - 1, 25:]).all() and not np.isnan(x[:n - 1]).any()      # a song without a used frame
    alone, alone_names = D.features(res, mel=ml)
    assert alone.shape == (n, 11) and alone_names == names[:4] + names[25:]
    assert alone[:, 4:].tobytes() == x[:, 25:].tobytes()
    with pytest.raises(ValueError):
        D.features(res, mel=ml[:2])
    with pytest.raises(ValueError):
        D.features(res, mel=tb)


def test_the_25_column_call_is_unchanged():
    """the features of these records without the mel group, as the parent commit gave them: tests/golden"""
    res, lv, tb, rh, ch, ml = _records(4)
    x, names = D.features(res, levels=lv, timbre=tb, rhythm=rh, chroma=ch)
    gold = np.load(os.path.join(ROOT, "tests", "golden", "desc_features25.npy"))
    assert x.shape == (4, 25) and x.dtype == gold.dtype == np.float32 and x.tobytes() == gold.tobytes()
    x32, names32 = D.features(res, levels=lv, timbre=tb, rhythm=rh, chroma=ch, mel=ml)
    assert names32[:25] == names and x32[:, :25].tobytes() == x.tobytes()
