"""The true-peak reference (tests/tpeak_reference.py) and the host arithmetic of bl_amd_tpeak_* (bl_api.c), without a
GPU: the table from its formula, the numpy reference against the Python-integer one, every deliberate mistake changing a
named song, the metering accuracy against analytic peaks inside EBU Tech 3341's tolerance, the dB arithmetic, and
header / bindings / exports agreement and the wrappers' argument checks."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import bliss_amd.truepeak as tp
from bliss_amd import _lib
from bliss_amd.records import LOUD_DTYPE, TPEAK_DTYPE
from tests import tpeak_reference as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TPEAK_SYMBOLS = ("bl_amd_tpeak_batch_device", "bl_amd_ctx_tpeak_batch_device", "bl_amd_tpeak_batch_host",
                 "bl_amd_tpeak_table", "bl_amd_tpeak_shape", "bl_amd_tpeak_dbtp", "bl_amd_tpeak_song_dbtp",
                 "bl_amd_tpeak_gain_db", "bl_amd_tpeak_profile_ms")


# ---- the table ----------------------------------------------------------------------------------------------------------

def test_table_is_its_formula_and_the_librarys(lib):
    g = tr.generate_table()
    assert np.array_equal(g, tr.TABLE)
    assert np.array_equal(tp.table(), tr.TABLE)
    text = open(os.path.join(ROOT, "bliss_amd", "csrc", "bl_tpeak_table.h")).read()
    rows = re.findall(r"\{((?:\s*-?\d+\s*,){11}\s*-?\d+\s*)\}", text)
    assert [[int(v) for v in r.split(",")] for r in rows] == tr.TABLE.tolist()


def test_table_sums_and_range():
    assert tr.TABLE.sum(axis=1).tolist() == [16384, 16392, 16400, 16392]
    l1 = np.abs(tr.TABLE).sum(axis=1)
    assert l1.max() == 30544 and 30544 * 32768 == 1000865792 < 1 << 30
    assert np.array_equal(tr.TABLE[1], tr.TABLE[3][::-1]) and np.array_equal(tr.TABLE[2], tr.TABLE[2][::-1])
    assert np.abs(tr.TABLE).max() < 32768   # a tap fits an int16


def test_shape_is_a_lane_and_a_group(lib):
    lane, group = tp.shape()
    assert 1 <= lane <= group and group % lane == 0


# ---- the two references -------------------------------------------------------------------------------------------------

def test_numpy_reference_equals_the_python_integer_one():
    rng = np.random.default_rng(11)
    for k in range(40):
        ch = 1 + k % 2
        n = int(rng.integers(1, 60))
        x = rng.integers(-32768, 32768, n).astype(np.int16)
        if k % 5 == 0:
            x[:] = rng.choice([-32768, 32767], n)
        ceiling = int(rng.choice([0, 1000, 20000, 32767, 65535]))
        block = int(rng.choice([1, 2, 3, 7, 16, 65536]))
        a, ab = tr.song(x, ch, ceiling, block)
        b, bb = tr.song_slow(x, ch, ceiling, block)
        assert a.tobytes() == b.tobytes(), (k, a, b)
        assert np.array_equal(ab, bb), k
    a, ab = tr.song(np.array([7], dtype=np.int16), 2, 0, 1)
    assert a["frames"][0] == 0 and a["at"].tolist() == [[-1, -1]] and ab.shape == (0, 2)
    m, _ = tr.song(np.array([7, -9], dtype=np.int16), 1, 0, 1)
    assert m["at"][0, 1] == -1 and m["tpeak"][0, 1] == 0 and m["peak"][0].tolist() == [9, 0]


def _noise(frames, ch, seed):
    return np.random.default_rng(seed).integers(-32768, 32768, frames * ch).astype(np.int16)


def named_songs(lane=16):
    """(pcm, channels, ceiling, block) by name: the songs the switches are shown on"""
    lean = np.zeros(40, dtype=np.int16)
    lean[20], lean[21] = 32767, 16384                     # the largest point lies in phase 1
    twin = np.zeros(3 * lane, dtype=np.int16)
    twin[5], twin[2 * lane + 3] = 12345, -12345           # two equal maxima, both in phase 0
    worst = np.zeros(2 * 40, dtype=np.int16)
    for j in range(-5, 7):
        worst[2 * (20 + j)] = 32767 if tr.TABLE[2][j + 5] > 0 else -32767
    worst[1::2] = -32768
    return {
        "noise": (_noise(3 * lane + 5, 2, 1), 2, 9000, 1),
        "noise, blocks of 7": (_noise(3 * lane + 5, 2, 1), 2, 9000, 7),
        "noise, nothing under the ceiling": (_noise(3 * lane + 5, 2, 2), 2, 0, 1),
        "lean": (lean, 1, 32767, 1),
        "twin": (twin, 1, 12345, 1),
        "negative": (np.full(50, -20000, dtype=np.int16), 1, 32767, 1),
        "odd": (_noise(21, 1, 3)[:21], 2, 100, 1),
        "worst": (worst, 2, 32767, 1),
    }


SHOWN_ON = {
    "halo_swapped": "noise", "phases_exchanged": "lean", "last_frame_dropped": "noise, nothing under the ceiling",
    "front_from_memory": "noise", "last_index": "twin", "overs_ge": "twin", "pair_across_channels": "noise",
    "signed_max": "negative", "block_at_tile": "noise, blocks of 7", "odd_tail_frame": "odd",
    "pair_saturated": "worst", "seam_twice": "noise",
}


def test_every_switch_changes_a_named_song():
    assert set(SHOWN_ON) == set(tr.SWITCHES) and len(tr.SWITCHES) >= 12
    songs = named_songs()
    for sw, name in SHOWN_ON.items():
        x, ch, ceiling, block = songs[name]
        rec, blocks = tr.song(x, ch, ceiling, block)
        bad, bad_blocks = tr.song(x, ch, ceiling, block, sw=(sw,))
        assert rec.tobytes() != bad.tobytes() or not np.array_equal(blocks, bad_blocks), (sw, name)
    # what the named songs are meant to be
    x, ch, ceiling, block = songs["lean"]
    assert tr.song(x, ch)[0]["at"][0, 0] % 4 == 1
    x, ch, ceiling, block = songs["twin"]
    r = tr.song(x, ch, ceiling)[0]
    assert r["at"][0, 0] == 4 * 5 and r["tpeak"][0, 0] == 12345 << 14 and r["overs"][0, 0] == 0
    assert tr.song(x, ch, ceiling, sw=("overs_ge",))[0]["overs"][0, 0] == 2
    x, ch, ceiling, block = songs["worst"]
    r = tr.song(x, ch)[0]
    assert r["tpeak"][0, 0] == 30544 * 32767 and r["at"][0, 0] == 4 * 20 + 2
    assert r["tpeak"][0, 1] >= 16400 * 32768 and r["peak"][0].tolist() == [32767, 32768]


# ---- metering accuracy ------------------------------------------------------------------------------------------------------

SINES = [  # amplitude, period in frames, phase in degrees
    (0.5, 4.0, 0.0), (0.5, 4.0, 45.0), (0.5, 6.0, 60.0), (0.5, 8.0, 67.5), (0.5, 3.0, 30.0), (0.5, 2.5, 10.0),
    (1.41, 4.0, 45.0)]


@pytest.mark.parametrize("amplitude,period,phase", SINES)
def test_reading_is_within_tech_3341_of_the_analytic_peak(amplitude, period, phase):
    """48 kHz, 4 800 frames with a linear fade of 480 frames at both ends (an abrupt start is a real inter-sample
    transient and reads high); +0.2 / -0.4 dB is the tolerance of EBU Tech 3341's true-peak cases"""
    x = tr.faded_sine(4800, period, phase, amplitude)
    rec, _ = tr.song(x, 1)
    got = tr.dbtp(int(rec["tpeak"][0, 0]))
    want = 20.0 * math.log10(amplitude * 32767.0 / 32768.0)
    print(f"A {amplitude} period {period} phase {phase}: {got:.4f} dBTP, analytic {want:.4f}, off {got - want:+.4f}")
    assert -0.4 <= got - want <= 0.2
    if (amplitude, period, phase) == (0.5, 4.0, 45.0):   # the sample peak is 3 dB short
        assert 20.0 * math.log10(int(rec["peak"][0, 0]) / 32768.0) < want - 2.9
    if amplitude > 1.0:                                    # above full scale between samples that all fit
        assert got > 2.8 and int(rec["peak"][0, 0]) < 32768 and int(rec["overs"][0, 0]) > 0


# ---- host arithmetic --------------------------------------------------------------------------------------------------------

def _tpeak_record(t0, t1):
    rec = np.zeros(1, dtype=TPEAK_DTYPE)
    rec["tpeak"][0] = (t0, t1)
    return rec


def _loud_record(gated_sum, count):
    rec = np.zeros(1, dtype=LOUD_DTYPE)
    rec["gated_sum"][0] = (gated_sum, 0)
    rec["gated_count"] = count
    return rec


def test_figures_follow_the_records(lib):
    rec = _tpeak_record(1 << 29, 1 << 28)
    per, song = tp.dbtp(rec)
    assert per[0, 0] == 0.0 and per[0, 1] == pytest.approx(-20.0 * math.log10(2.0), abs=1e-12) and song[0] == 0.0
    rec = _tpeak_record(0, 1000865792)
    per, song = tp.dbtp(rec)
    assert per[0, 0] == -math.inf and song[0] == per[0, 1] == pytest.approx(tr.dbtp(1000865792), abs=1e-12)
    per, song = tp.dbtp(_tpeak_record(0, 0))
    assert per[0].tolist() == [-math.inf, -math.inf] and song[0] == -math.inf
    ptr = rec.ctypes.data_as(C.POINTER(_lib.SongTpeak))
    for ch in (-1, 2, 100):
        assert math.isnan(lib.bl_amd_tpeak_dbtp(ptr, ch))
    assert math.isnan(lib.bl_amd_tpeak_dbtp(None, 0)) and math.isnan(lib.bl_amd_tpeak_song_dbtp(None))


def test_gain_is_the_smaller_of_loudness_gain_and_headroom(lib):
    import bliss_amd.loudness as ld
    hop = 4800
    loud = _loud_record(int(10 * 4 * hop * 2 ** 30 * 10 ** -3.0), 10)   # about -30.7 LUFS
    lufs = ld.lufs(loud, hop)[0][0]
    plain = ld.gain_db(loud, hop, -18.0)[0]
    assert plain == -18.0 - lufs > 12.0
    quiet, hot = _tpeak_record(1 << 20, 1 << 18), _tpeak_record(1 << 28, 1 << 29)
    assert tp.gain_db(loud, hop, quiet, -18.0, -1.0)[0] == plain               # headroom to spare
    assert tp.gain_db(loud, hop, hot, -18.0, -1.0)[0] == -1.0                  # 0 dBTP already: one dB down
    assert tp.gain_db(loud, hop, _tpeak_record(0, 0), -18.0, -1.0)[0] == plain  # nothing to hold the gain back
    silent = _loud_record(0, 0)
    assert tp.gain_db(silent, hop, quiet, -18.0, -1.0)[0] == 0.0
    assert tp.gain_db(silent, hop, hot, -18.0, -1.0)[0] == -1.0
    lp, tq = loud.ctypes.data_as(C.POINTER(_lib.SongLoud)), hot.ctypes.data_as(C.POINTER(_lib.SongTpeak))
    assert math.isnan(lib.bl_amd_tpeak_gain_db(None, hop, -18.0, tq, -1.0))
    assert math.isnan(lib.bl_amd_tpeak_gain_db(lp, 0, -18.0, tq, -1.0))
    assert math.isnan(lib.bl_amd_tpeak_gain_db(lp, hop, -18.0, None, -1.0))


# ---- header, bindings, exports ----------------------------------------------------------------------------------------------

def _struct_fields(text, name):
    body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            out += [re.sub(r"\[.*\]", "", part.strip().split()[-1]) for part in decl.split(",")]
    return out


def test_header_bindings_and_exports_agree(lib):
    text = open(os.path.join(ROOT, "include", "bliss_amd.h")).read()
    declared = set(re.findall(r"\b(bl_amd_(?:ctx_)?tpeak_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == set(TPEAK_SYMBOLS)
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], stdout=subprocess.PIPE, text=True,
                              check=True).stdout
    for name in TPEAK_SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
        assert re.search(r"\b" + name + r"$", exported, flags=re.M), name
    assert [f[0] for f in _lib.SongTpeak._fields_] == _struct_fields(text, "bl_amd_song_tpeak")
    assert C.sizeof(_lib.SongTpeak) == 56 == TPEAK_DTYPE.itemsize == tr.RECORD_DTYPE.itemsize
    assert [(n, TPEAK_DTYPE.fields[n][1]) for n in TPEAK_DTYPE.names] == \
        [(n, tr.RECORD_DTYPE.fields[n][1]) for n in tr.RECORD_DTYPE.names]
    assert "True peak (4x oversampling) is not computed" not in text
    assert "True peak is not computed" not in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_package_namespace_is_unchanged():
    import bliss_amd
    assert "truepeak" not in bliss_amd.__all__ and not any("tpeak" in n for n in bliss_amd.__all__)


# ---- argument checks ----------------------------------------------------------------------------------------------------------

def test_wrappers_refuse_bad_arguments_before_the_library(lib, monkeypatch):
    x = np.zeros(100, dtype=np.int16)

    def unreachable(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", unreachable)
    for kw in (dict(ceiling=-1), dict(ceiling=65536), dict(ceiling=1.0), dict(ceiling=True), dict(block=0),
               dict(block=65537), dict(block=2.0)):
        with pytest.raises(ValueError):
            tp.tpeak_host([x], 1, **kw)
    with pytest.raises(ValueError):
        tp.tpeak_host([x], 3)
    with pytest.raises(ValueError):
        tp.tpeak_host([], 1)
    with pytest.raises(ValueError):
        tp.tpeak_host([x[:0]], 1)
    with pytest.raises(ValueError):
        tp.tpeak_host([x, x], [1])
    with pytest.raises(ValueError):
        tp.dbtp(np.zeros(1, dtype=LOUD_DTYPE))
    with pytest.raises(ValueError):
        tp.dbtp(np.zeros(0, dtype=TPEAK_DTYPE))
    with pytest.raises(ValueError):
        tp.gain_db(np.zeros(2, dtype=LOUD_DTYPE), 4800, np.zeros(1, dtype=TPEAK_DTYPE))
    with pytest.raises(ValueError):
        tp.gain_db(np.zeros(1, dtype=LOUD_DTYPE), 0, np.zeros(1, dtype=TPEAK_DTYPE))
    with pytest.raises(ValueError):
        tp.gain_db(np.zeros(1, dtype=LOUD_DTYPE), 4800, np.zeros(1, dtype=TPEAK_DTYPE), target_lufs=math.nan)


def test_library_refuses_before_it_looks_for_a_device(lib):
    x = np.zeros(64, dtype=np.int16)
    out = (_lib.SongTpeak * 1)()
    ptrs, ns, chs = (C.c_void_p * 1)(x.ctypes.data), (C.c_int32 * 1)(64), (C.c_int32 * 1)(1)
    U = _lib.BL_UNEXPECTED
    for ceiling, block in ((-1, 1), (65536, 1), (0, 0), (0, 65537)):
        assert lib.bl_amd_tpeak_batch_host(ptrs, ns, chs, 1, ceiling, block, out, None) == U
    assert lib.bl_amd_tpeak_batch_host(ptrs, ns, chs, 0, 0, 1, out, None) == U
    assert lib.bl_amd_tpeak_batch_host(None, ns, chs, 1, 0, 1, out, None) == U
    assert lib.bl_amd_tpeak_batch_host(ptrs, ns, chs, 1, 0, 1, None, None) == U
    assert lib.bl_amd_tpeak_batch_host(ptrs, ns, (C.c_int32 * 1)(3), 1, 0, 1, out, None) == U
    assert lib.bl_amd_tpeak_batch_host(ptrs, (C.c_int32 * 1)(0), chs, 1, 0, 1, out, None) == U
    desc = (_lib.SongDesc * 1)(_lib.SongDesc(0, 64, 1, 0))
    dev = C.c_void_p(4096)   # never dereferenced: every call below is refused on its arguments
    for ceiling, block in ((-1, 1), (65536, 1), (0, 0), (0, 65537)):
        assert lib.bl_amd_tpeak_batch_device(dev, desc, 1, ceiling, block, dev, None, 0, None) == U
    assert lib.bl_amd_tpeak_batch_device(None, desc, 1, 0, 1, dev, None, 0, None) == U
    assert lib.bl_amd_tpeak_batch_device(dev, None, 1, 0, 1, dev, None, 0, None) == U
    assert lib.bl_amd_tpeak_batch_device(dev, desc, 1, 0, 1, None, None, 0, None) == U
    assert lib.bl_amd_tpeak_batch_device(dev, desc, 0, 0, 1, dev, None, 0, None) == U
    assert lib.bl_amd_tpeak_batch_device(C.c_void_p(4104), desc, 1, 0, 1, dev, None, 0, None) == U
    assert lib.bl_amd_tpeak_batch_device(dev, desc, 1, 0, 1, C.c_void_p(4100), None, 0, None) == U
    assert lib.bl_amd_tpeak_batch_device(dev, desc, 1, 0, 1, dev, C.c_void_p(4098), 64, None) == U
    assert lib.bl_amd_tpeak_batch_device(dev, desc, 1, 0, 1, dev, dev, 63, None) == U
    bad = (_lib.SongDesc * 1)(_lib.SongDesc(4, 64, 1, 0))
    assert lib.bl_amd_tpeak_batch_device(dev, bad, 1, 0, 1, dev, None, 0, None) == U
    assert lib.bl_amd_tpeak_profile_ms(b"loud_filter", None) == -1.0
    n = C.c_int(5)
    assert lib.bl_amd_tpeak_profile_ms(b"tpeak_scan", C.byref(n)) == 0.0 and n.value == 0
