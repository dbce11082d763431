"""The tempo (bl_amd_rhythm_*, bliss_amd.rhythm) without a device: the reference of tests/rhythm_reference.py meets the
header's bounds on the extreme songs and behaves as the definitions say on designed ones; each of its deliberate
mistakes changes a named song of the corpus tests/test_gpu_rhythm.py runs, so that test would catch a kernel that made
it; the header, the bindings and the export list agree; the host arithmetic of the library (bpm, strength, hops)
equals the documented double expressions; the entry points that need a device fail loudly; the wrappers check their
arguments; and bl_isqrt.h passes the selftest's sweep on the CPU (tests/host/test_isqrt_host.cpp)."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import bliss_amd
import bliss_amd.rhythm as rh
from bliss_amd import _lib
from bliss_amd.records import RHYTHM_DTYPE
from tests import rhythm_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {
    "bl_amd_rhythm_hops": C.c_int, "bl_amd_rhythm_batch_device": C.c_int, "bl_amd_ctx_rhythm_batch_device": C.c_int,
    "bl_amd_rhythm_batch_host": C.c_int, "bl_amd_rhythm_from_onsets": C.c_int, "bl_amd_rhythm_bpm": C.c_double,
    "bl_amd_rhythm_strength": C.c_double, "bl_amd_selftest_isqrt": C.c_int,
}
OFFSETS = dict(r0=0, r_prev=8, r_lag=16, r_next=24, r_peak=32, onset_sum=40, onset_max=48, hops=52, terms=56, lag=60,
               lag_peak=64, status=68)
LO, HI = rr.LAG_MIN, rr.LAG_MAX


@pytest.fixture(scope="module")
def corpus():
    return rr.corpus()


# ---- the reference -----------------------------------------------------------------------------------------------

def test_the_extreme_songs_meet_the_bounds(corpus):
    pcm, ch = corpus["all_min_stereo"]
    n, a, b, A, B = rr.novelty(pcm, ch)
    assert int(rr.mix(pcm, ch).min()) == -2 ** 16 and int(A.max()) == 128 * 2 ** 32 == 2 ** 39   # m^2 = 2^32
    assert max(a) == 2 ** 16 and a[3:] == [2 ** 16] * (len(a) - 3) and max(b) == 0
    pcm, ch = corpus["nyquist_hops"]
    n, a, b, A, B = rr.novelty(pcm, ch)
    m = rr.mix(pcm, ch)
    assert int(np.abs(np.diff(m)).max()) == 2 ** 17 - 2                     # the largest |d| there is
    assert int(B.max()) < 2 ** 41 and int(B.max()) > 2 ** 40 and max(b) < 2 ** 17 and max(b) > 2 ** 16
    for name in ("nyquist_hops", "nyquist_hops_stereo", "all_min_stereo", "noise_H1500_2ch"):
        rec, o, R = rr.song(*corpus[name], LO, HI)
        assert max(rr.novelty(*corpus[name])[0]) < 2 ** 18 and int(o.max()) < 2 ** 18 and max(R) < 2 ** 60
    assert rr.song(*corpus["nyquist_hops"], LO, HI)[0]["lag"] % 2 == 0      # the hops alternate


def test_mono_equals_dual_mono(corpus):
    for name in ("noise_H640_1ch", "click_43", "nyquist_hops", "dc_3", "noise_H19_1ch"):
        pcm, ch = corpus[name]
        assert ch == 1
        a, b = rr.song(pcm, 1, LO, HI), rr.song(rr.dual_mono(pcm), 2, LO, HI)
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2], name
    a, b = rr.song(*corpus["nyquist_hops"], LO, HI), rr.song(*corpus["nyquist_hops_stereo"], LO, HI)
    assert a[0] == b[0] and a[2] == b[2]


@pytest.mark.parametrize("c", rr.DC)
def test_dc_songs_sit_on_perfect_squares(corpus, c):
    pcm, ch = corpus[f"dc_{c}"]
    n, a, b, A, B = rr.novelty(pcm, ch)
    assert a[3:] == [2 * abs(c)] * (len(a) - 3) and int(A[5]) == 128 * 4 * c * c
    assert max(b) == 0 and n[4:] == [0] * (len(n) - 4)
    rec, o, R = rr.song(pcm, ch, LO, HI)
    assert rec["status"] == 0 and rec["hops"] == 600 and rec["terms"] == 89


@pytest.mark.parametrize("period, hops, ch", rr.CLICKS)
def test_click_tracks_return_their_period(corpus, period, hops, ch):
    rec, o, R = rr.song(*corpus[f"click_{period}"], LO, HI)
    assert rec["lag"] == period and rec["hops"] == hops and rec["terms"] == hops - 511
    assert rr.bpm(rec) == pytest.approx(60 * 22050 / (128 * period), rel=0.01)
    assert 0.8 < rr.strength(rec) < 1.1


def test_silence_and_short_songs(corpus):
    rec, o, R = rr.song(*corpus["silence"], LO, HI)
    assert rec["lag"] == rec["lag_peak"] == 0 and rec["r0"] == 0 and rec["status"] == 0 and not o.any()
    assert math.isnan(rr.bpm(rec)) and rr.strength(rec) == 0.0
    rec, o, R = rr.song(*corpus["noise_H511_1ch"], LO, HI)
    assert rec == dict(dict.fromkeys(rr.FIELDS, 0), hops=511, status=rr.BL_UNEXPECTED) and R == [0] * 512 and o.any()
    rec, o, R = rr.song(*corpus["noise_H512_2ch"], LO, HI)
    assert rec["terms"] == 1 and R == [int(o[0]) * int(o[t]) for t in range(512)]
    rec, o, R = rr.song(*corpus["late"], LO, HI)
    assert not o[:890].any() and o[905:].any() and rec["status"] == 0


SWITCHES = [
    ("trunc32", dict(trunc32=True), "all_min_stereo"),
    ("across_start", dict(across_start=2 * rr.ARENA_FILL), "noise_H640_1ch"),
    ("across_start stereo", dict(across_start=2 * rr.ARENA_FILL), "noise_H19_2ch"),
    ("forget_at", dict(forget_at=64), "noise_H640_1ch"),
    ("forget_at 1024", dict(forget_at=1024), "noise_H1500_2ch"),
    ("float_isqrt", dict(float_isqrt=True), "noise_H1500_1ch"),
    ("lag_terms", dict(lag_terms=True), "noise_H513_1ch"),
    ("argmax", dict(argmax=True), "click_43"),
]


@pytest.mark.parametrize("what, switch, name", SWITCHES, ids=[s[0] for s in SWITCHES])
def test_every_switch_changes_a_song_of_the_corpus(corpus, what, switch, name):
    good, bad = rr.song(*corpus[name], LO, HI), rr.song(*corpus[name], LO, HI, **switch)
    assert good[0] != bad[0] or not np.array_equal(good[1], bad[1]) or good[2] != bad[2], (what, name)


def test_the_forgetful_window_also_shows_in_the_long_song():
    pcm = rr.long_song(1)[:128 * 4096]
    good, bad = rr.onsets(pcm, 1), rr.onsets(pcm, 1, forget_at=2048)
    assert np.array_equal(good[:2030], bad[:2030]) and not np.array_equal(good[2040:2060], bad[2040:2060])


def test_float64_sums_show_on_the_big_curve():
    o = rr.big_curve()
    assert o.size == 140000 and int(o.min()) >= 2 ** 17 and int(o.max()) < 2 ** 18
    R = rr.lag_products(o)
    assert 2 ** 53 < min(R) and max(R) < 2 ** 60
    assert R[7] == sum(int(x) * int(y) for x, y in zip(o[:139489].tolist(), o[7:7 + 139489].tolist()))
    assert rr.lag_products(o, float_acf=True) != R
    assert [r & 0xFFFFFFFF for r in R] != R                                   # what a 32-bit sum would keep


def test_the_pick_takes_each_branch():
    flat = [0] + [100] * 511
    # the local-maximum rule fires: 30 is within 1/16 of the best (at 90) and is the first such local maximum
    R = list(flat)
    R[30], R[60], R[90] = 960, 500, 1000
    assert rr.pick(R, 10, 200) == (30, 90, 1000)
    R[30] = 937                                   # 16 * 937 < 15 * 1000: no longer within 1/16
    assert rr.pick(R, 10, 200) == (90, 90, 1000)
    # the maximum at the edge of the range on a slope, and nothing else qualifies: the fallback to lag_peak
    R = [1000 - t for t in range(512)]
    assert rr.pick(R, 10, 200) == (10, 10, 990)
    R = [t for t in range(512)]
    assert rr.pick(R, 10, 200) == (200, 200, 200)
    # ties go to the smaller lag
    R = list(flat)
    R[40] = R[80] = R[120] = 700
    assert rr.pick(R, 10, 200) == (40, 40, 700)
    assert rr.pick([5] * 512, 10, 200) == (10, 10, 5)
    assert rr.pick([9] + [0] * 511, 1, 510) == (0, 0, 0)


# ---- the library without a device ----------------------------------------------------------------------------------

def test_header_bindings_and_exports_agree():
    text = open(os.path.join(ROOT, "include", "bliss_amd.h")).read()
    declared = set(re.findall(r"\b(?:int|double) (bl_amd_(?:(?:ctx_)?rhythm_|selftest_isqrt)\w*)\(", text))
    assert declared == set(NEW_SYMBOLS)
    lib = bliss_amd.load()
    for name, res in NEW_SYMBOLS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == _lib.SYMBOLS[name][1]
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, stdout=subprocess.PIPE,
                         text=True).stdout
    assert set(NEW_SYMBOLS) <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert "#define BL_AMD_RHYTHM_HOP 128" in text and "#define BL_AMD_RHYTHM_LAGS 512" in text
    assert (rh.HOP, rh.LAGS) == (rr.HOP, rr.LAGS) == (128, 512)
    assert not any("rhythm" in name.lower() for name in bliss_amd.__all__)     # the package's own names are unchanged


def test_record_layout():
    S = _lib.SongRhythm
    assert C.sizeof(S) == 72 == RHYTHM_DTYPE.itemsize
    assert [f[0] for f in S._fields_] == list(OFFSETS) == list(RHYTHM_DTYPE.names) == list(rr.FIELDS)
    for name, off in OFFSETS.items():
        assert getattr(S, name).offset == off == RHYTHM_DTYPE.fields[name][1], name
    src = "#include <stddef.h>\n#include \"bliss_amd.h\"\n" + "".join(
        f"_Static_assert(offsetof(bl_amd_song_rhythm, {k}) == {v}, \"{k}\");\n" for k, v in OFFSETS.items()) + \
        "_Static_assert(sizeof(bl_amd_song_rhythm) == 72, \"size\");\n"
    inc = os.path.join(ROOT, "include")
    subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", inc, "-x", "c", "-"], input=src, text=True, check=True)
    # the header stays C99
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-fsyntax-only", "-I", inc, "-x", "c", "-"],
                   input="#include \"bliss_amd.h\"\nint bl_test_unit;\n", text=True, check=True)
    raw = bytes(range(72)) * 2
    a = rh.rhythm_to_numpy(raw)
    assert a.shape == (2,) and a.tobytes() == raw and int(a["hops"][0]) == 0x37363534


def test_hops_is_plain_arithmetic():
    lib = bliss_amd.load()
    for n, ch, want in ((0, 1, 0), (127, 1, 0), (128, 1, 1), (255, 2, 0), (256, 2, 1), (257, 2, 1), (2 ** 31 - 1, 1, 2 ** 24 - 1),
                        (-1, 1, -1), (1000, 0, -1), (1000, 3, -1)):
        assert lib.bl_amd_rhythm_hops(n, ch) == want, (n, ch)


def _record(**kw):
    rec = np.zeros(1, dtype=RHYTHM_DTYPE)
    for k, v in kw.items():
        rec[k] = v
    return rec


def test_bpm_and_strength_are_the_documented_arithmetic():
    """to 1e-12 relative: a handful of double operations on exact integers"""
    lib = bliss_amd.load()
    P = C.POINTER(_lib.SongRhythm)
    cases = [
        dict(lag=43, r_prev=900, r_lag=1000, r_next=950, r0=1100),           # a vertex right of the lag
        dict(lag=86, r_prev=2 ** 59 + 12345, r_lag=2 ** 59 + 99999, r_next=2 ** 59 - 7, r0=2 ** 60 - 1),
        dict(lag=130, r_prev=1000, r_lag=1000, r_next=1000, r0=999),         # flat: den = 0, delta = 0; strength > 1
        dict(lag=10, r_prev=1200, r_lag=1000, r_next=800, r0=5000),          # on a slope (the fallback): delta = 0
        dict(lag=200, r_prev=500, r_lag=1000, r_next=1000, r0=2000),         # a tie with the neighbour: delta = +0.5
        dict(lag=200, r_prev=1000, r_lag=1000, r_next=0, r0=2000),           # delta = -0.5
        dict(lag=1, r_prev=7, r_lag=9, r_next=8, r0=0),                      # r0 = 0: strength 0
        dict(lag=0, r0=12345),                                               # no beat
    ]
    for kw in cases:
        rec = _record(**kw)
        want = dict.fromkeys(rr.FIELDS, 0)
        want.update(kw)
        for rate in (22050, 44100):
            got, w = lib.bl_amd_rhythm_bpm(rec.ctypes.data_as(P), rate), rr.bpm(want, rate)
            assert (math.isnan(got) and math.isnan(w)) or abs(got - w) <= 1e-12 * w, (kw, got, w)
        got, w = lib.bl_amd_rhythm_strength(rec.ctypes.data_as(P)), rr.strength(want)
        assert abs(got - w) <= 1e-12 * w, (kw, got, w)
        bpm, strength = rh.rhythm_bpm(rec)
        assert strength[0] == got and (bpm[0] == lib.bl_amd_rhythm_bpm(rec.ctypes.data_as(P), 22050) or kw["lag"] == 0)
    assert rr.bpm(dict.fromkeys(rr.FIELDS, 0) | cases[4]) == 60 * 22050 / (128 * 200.5)
    assert rr.bpm(dict.fromkeys(rr.FIELDS, 0) | cases[5]) == 60 * 22050 / (128 * 199.5)
    assert rr.bpm(dict.fromkeys(rr.FIELDS, 0) | cases[0]) < 60 * 22050 / (128 * 43)
    assert math.isnan(lib.bl_amd_rhythm_bpm(None, 22050)) and math.isnan(lib.bl_amd_rhythm_strength(None))
    assert math.isnan(lib.bl_amd_rhythm_bpm(_record(lag=5, r_lag=3).ctypes.data_as(P), 0))
    for bad in (np.zeros(0, RHYTHM_DTYPE), np.zeros((2, 2), RHYTHM_DTYPE), np.zeros(72, np.uint8)):
        with pytest.raises(ValueError):
            rh.rhythm_bpm(bad)


def test_lags_for_bpm():
    assert rh.lags_for_bpm(60, 180) == (math.ceil(60 * 22050 / (128 * 180)), math.floor(60 * 22050 / (128 * 60))) == (58, 172)
    lo, hi = rh.lags_for_bpm(21, 10000)
    assert (lo, hi) == (2, 492)
    for bad in ((20, 100), (1, 20000), (0, 100), (100, 60), (-5, 60), (120, 120)):
        with pytest.raises(ValueError):
            rh.lags_for_bpm(*bad)
    with pytest.raises(ValueError):
        rh.lags_for_bpm(60, 180, rate=0)


PCM = [np.zeros(512 * 128, np.int16)]
NOT_AN_INTEGER = [True, 2.0, np.float32(2), "2", None]


@pytest.mark.parametrize("value", NOT_AN_INTEGER + [0, 511, -1, np.int64(0)], ids=repr)
def test_lag_arguments_are_refused_with_the_usual_message(value):
    calls = {
        "lag_min": [lambda: rh.rhythm_batch_host(PCM, 1, value, 100), lambda: rh.rhythm_from_onsets([np.arange(600)], value, 100)],
        "lag_max": [lambda: rh.rhythm_batch_host(PCM, 1, 1, value), lambda: rh.rhythm_from_onsets([np.arange(600)], 1, value)],
    }
    for name, fns in calls.items():
        for fn in fns:
            with pytest.raises(ValueError) as e:
                fn()
            assert str(e.value).startswith(f"{name} must be an integer in [") and repr(value) in str(e.value)
    with pytest.raises(ValueError) as e:
        rh.rhythm_batch_host(PCM, 1, 100, 99)
    assert str(e.value).startswith("lag_max must be an integer in [100, 510]")


def test_wrappers_reject_bad_songs_and_curves():
    for pcm, ch in (([], 1), ([np.zeros(127, np.int16)], 1), ([np.zeros(255, np.int16)], 2), (PCM, 3), (PCM, [1, 2])):
        with pytest.raises(ValueError):
            rh.rhythm_batch_host(pcm, ch, 1, 510)
    for curves in ([], [np.zeros(0, np.int64)], [np.array([1 << 18])], [np.array([-1, 5])], [np.zeros(5)],
                   [np.zeros((2, 2), np.int64)]):
        with pytest.raises(ValueError):
            rh.rhythm_from_onsets(curves, 1, 510)

    class NoCorpus:
        rhythm_raw = None
    with pytest.raises(RuntimeError):
        rh.fetch_rhythm(NoCorpus())


def test_entry_points_fail_loudly_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present: tests/test_gpu_rhythm.py runs these calls")
    lib = bliss_amd.load()
    U = _lib.BL_UNEXPECTED
    n = 2
    desc = (_lib.SongDesc * n)()
    for i in range(n):
        desc[i].pcm_offset, desc[i].n_samples, desc[i].channels = 1024 * i, 600, 1 + i
    out = (_lib.SongRhythm * n)()
    C.memset(out, 0xAB, C.sizeof(out))
    pcm = np.zeros(4096, np.int16)
    aligned = pcm.ctypes.data + (-pcm.ctypes.data) % 16       # the argument checks pass: it is the device that is missing
    assert lib.bl_amd_rhythm_batch_device(aligned, desc, n, 1, 510, C.addressof(out), None, 0, None, None) == U
    assert lib.bl_amd_ctx_rhythm_batch_device(None, aligned, desc, n, 1, 510, C.addressof(out), None, 0, None, None) == U
    songs = [np.ones(600, np.int16), np.ones(600, np.int16)]
    ptrs = (C.c_void_p * n)(*[s.ctypes.data for s in songs])
    assert lib.bl_amd_rhythm_batch_host(ptrs, (C.c_int32 * n)(600, 600), (C.c_int32 * n)(1, 2), n, 1, 510, out, None,
                                        None) == U
    curve = np.arange(1200, dtype=np.uint32)
    assert lib.bl_amd_rhythm_from_onsets(curve.ctypes.data_as(C.POINTER(C.c_uint32)), (C.c_int32 * n)(600, 600), n, 1,
                                         510, out, None) == U
    counts = (C.c_uint64 * 2)(7, 7)
    assert lib.bl_amd_selftest_isqrt(counts) == U and list(counts) == [7, 7]
    assert bytes(out) == b"\xab" * C.sizeof(out)
    for name, call in (("bl_amd_rhythm_batch_host", lambda: rh.rhythm_batch_host(songs, [1, 2], 1, 510, acf=True)),
                       ("bl_amd_rhythm_from_onsets", lambda: rh.rhythm_from_onsets([curve[:600], curve], 1, 510))):
        with pytest.raises(RuntimeError) as e:
            call()
        assert re.findall(r"bl_amd_\w+", str(e.value)) == [name]


def test_isqrt_header_on_the_cpu(tmp_path):
    exe = str(tmp_path / "test_isqrt_host.bin")
    cc = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                         os.path.join(ROOT, "tests", "host", "test_isqrt_host.cpp"), "-o", exe],
                        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert cc.returncode == 0, "g++ failed:\n" + cc.stdout
    out = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout
    assert f"sweep: checked {3 * 2 ** 17 + 1} wrong 0" in out.stdout
