"""Chroma and key (bl_amd_chroma_*, bliss_amd.chroma) without a device: the library's bank equals the table
tests/chroma_reference.py generates, entry for entry; the polynomial sine and cosine stay within 1e-9 of numpy's; the
bank meets the header's bounds and finds a tone at its own pitch; the reference names the keys of designed progressions;
each of its deliberate mistakes changes a named song of the corpus tests/test_gpu_chroma.py runs, so that test would
catch a kernel that made it; the header, the bindings and the export list agree; bl_amd_chroma_frames and
bl_amd_chroma_key_name are covered at their edges; the entry points that need a device fail loudly; and
bl_chroma_table.h passes its own checks on the CPU (tests/host/test_chroma_table_host.cpp)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bliss_amd
import bliss_amd.chroma as ch
from bliss_amd import _lib
from bliss_amd.records import CHROMA_DTYPE, FRAME_CHROMA_DTYPE
from tests import chroma_reference as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("bl_amd_chroma_frames", "bl_amd_chroma_batch_device", "bl_amd_ctx_chroma_batch_device",
               "bl_amd_chroma_batch_host", "bl_amd_chroma_table", "bl_amd_chroma_key_name")
OFFSETS = dict(chroma=0, score=96, score_next=104, frames=112, key=116, status=120, reserved=124)
# the song of the corpus each deliberate mistake shows on
SHOWS_ON = dict(trunc_shift="noise_T3_1ch", class_p="tone_13", hop4096="noise_T3_2ch", no_128="noise_T70_1ch",
                swap_rows="tone_0", tie_last="tie", s_off="c_major")


@pytest.fixture(scope="module")
def corpus():
    return cr.corpus()


# ---- the table ---------------------------------------------------------------------------------------------------

def test_the_library_s_table_is_the_reference_s():
    re_, im_, gain, length = ch.chroma_table()
    want = cr.table()
    assert re_.dtype == np.int8 and re_.shape == (48, 4096) and gain.dtype == np.uint32 and length.dtype == np.int32
    for got, w, name in zip((re_, im_, gain, length), want, ("re", "im", "gain", "len")):
        assert got.dtype == w.dtype and np.array_equal(got, w), name
    assert (int(length[0]), int(length[47]), int(gain[0]), int(gain[47])) == (3406, 224, 283, 65536)
    # any pointer may be NULL
    lib = bliss_amd.load()
    only = np.zeros(48, np.uint32)
    assert lib.bl_amd_chroma_table(None, None, only.ctypes.data, None) == 0 and np.array_equal(only, gain)
    assert lib.bl_amd_chroma_table(None, None, None, None) == 0


def test_sine_and_cosine_are_within_1e_9_of_numpy_s():
    rng = np.random.default_rng(4801)
    t = np.concatenate([rng.random(400000), np.linspace(0.0, 1.0, 100001), np.arange(9) / 8.0])
    c, s = cr.cossin(t)
    assert np.abs(c - np.cos(2.0 * np.pi * t)).max() <= 1e-9 and np.abs(s - np.sin(2.0 * np.pi * t)).max() <= 1e-9
    for p in (0, 11, 29, 47):               # the unquantised entries themselves
        a, b, tt = cr.entries(p)
        n = np.arange(cr.length(p))
        w = 0.5 - 0.5 * np.cos(2.0 * np.pi * (n + 0.5) / cr.length(p))
        assert np.abs(a - 127.0 * w * np.cos(2.0 * np.pi * tt)).max() <= 127e-9
        assert np.abs(b - 127.0 * w * np.sin(2.0 * np.pi * tt)).max() <= 127e-9


def test_the_table_meets_the_header_s_bounds():
    re_, im_, gain, length = cr.table()
    for t in (re_, im_):
        sums = np.abs(t.astype(np.int64)).sum(axis=1)
        assert sums.max() <= 140000 and sums.min() > 0
        assert np.abs(t.astype(np.int64)).max() <= 127
    for p in range(48):
        n0 = (4096 - int(length[p])) // 2
        assert not re_[p, :n0].any() and not re_[p, n0 + length[p]:].any()
        assert not im_[p, :n0].any() and not im_[p, n0 + length[p]:].any()
    assert [cr.pitch_class(p) for p in (0, 3, 47)] == [9, 0, 8]
    # the extreme songs: |Re| < 2^33.1, e < 2^37.2, chroma of T frames below T 2^39.2
    for name in ("all_min_stereo", "all_max_stereo", "all_max_mono"):
        pcm, chn = cr.corpus()[name]
        Re, Im = cr.pitch_sums(pcm, chn)
        assert max(int(np.abs(Re).max()), int(np.abs(Im).max())) < 2 ** 33.1
        rec, X = cr.song(pcm, chn)
        assert int(X.max()) < 2 ** 39.2 and max(rec["chroma"]) < X.shape[0] * 2 ** 39.2 and abs(rec["score"]) < 2 ** 29
    assert int(np.abs(cr.mix(*cr.corpus()["all_min_stereo"])).max()) == 2 ** 16


def test_a_tone_scores_highest_at_its_own_pitch_and_alike_at_every_pitch():
    gain = cr.table()[2].astype(np.int64)
    peak = []
    for p in range(48):
        Re, Im = cr.pitch_sums(cr.tone([cr.freq(p)], 4096, amp=16384.0), 1)
        a, b = Re[0] >> 15, Im[0] >> 15
        E = ((a * a + b * b) * gain) >> 16
        assert int(E.argmax()) == p, p
        peak.append(int(E[p]))
    assert max(peak) / min(peak) < 1.02        # the gain levels the window lengths


@pytest.mark.parametrize("tonic,minor,key", [(0, False, 0), (2, False, 2), (7, False, 7), (9, True, 21), (11, True, 23),
                                              (4, True, 16)])
def test_keys_of_triad_progressions(tonic, minor, key):
    rec, _ = cr.song(cr.progression(tonic, minor), 1)
    assert rec["key"] == key and rec["score"] > rec["score_next"] > 0
    assert cr.key_name(key) == cr.NAMES[tonic] + ("m" if minor else "")


def test_mono_equals_dual_mono(corpus):
    for name in ("noise_T3_1ch", "tone_13", "alternating", "tie"):
        pcm, chn = corpus[name]
        assert chn == 1
        a, b = cr.song(pcm, 1), cr.song(cr.dual_mono(pcm), 2)
        assert a[0] == b[0] and np.array_equal(a[1], b[1]), name


def test_designed_songs(corpus):
    rec, X = cr.song(*corpus["silence"])
    assert (rec["key"], rec["score"], rec["score_next"], rec["frames"], rec["status"]) == (-1, 0, 0, 3, 0) and not X.any()
    for name in ("short_Fr1_1ch", "short_Fr1_2ch", "short_Fr4095_1ch", "short_Fr4095_2ch"):
        rec, X = cr.song(*corpus[name])
        assert rec["status"] == cr.BL_UNEXPECTED and rec["frames"] == 0 and rec["key"] == -1 and X.shape == (0, 12)
    rec, _ = cr.song(*corpus["tie"])
    assert rec["score"] == rec["score_next"] > 0 and cr.song(*corpus["tie"], tie_last=True)[0]["key"] > rec["key"]
    assert sorted(cr.frames_of(p.size, c) for n, (p, c) in corpus.items() if n.startswith("noise_T") and "dual" not in n) \
        == sorted(list(cr.SHAPES_T) * 2 + [70, 71])
    assert any(p.size % 2 for p, c in corpus.values() if c == 2)                   # odd n_samples in stereo
    assert any((p.size // c) % 2048 for p, c in corpus.values())                   # Fr no multiple of 2 048


@pytest.mark.parametrize("mistake", cr.MISTAKES)
def test_every_deliberate_mistake_changes_a_named_song(corpus, mistake):
    pcm, chn = corpus[SHOWS_ON[mistake]]
    right, wrong = cr.song(pcm, chn), cr.song(pcm, chn, **{mistake: True})
    assert right[0] != wrong[0], mistake
    assert set(SHOWS_ON) == set(cr.MISTAKES)


# ---- the library without a device ----------------------------------------------------------------------------------

def test_header_bindings_and_exports_agree():
    text = open(os.path.join(ROOT, "include", "bliss_amd.h")).read()
    declared = set(re.findall(r"\bint (bl_amd_(?:ctx_)?chroma_\w*)\(", text))
    assert declared == set(NEW_SYMBOLS)
    lib = bliss_amd.load()
    for name in NEW_SYMBOLS:
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == _lib.SYMBOLS[name][1]
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, stdout=subprocess.PIPE,
                         text=True).stdout
    assert set(NEW_SYMBOLS) <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for line in ("#define BL_AMD_CHROMA_FRAME 4096", "#define BL_AMD_CHROMA_HOP 2048", "#define BL_AMD_CHROMA_PITCHES 48"):
        assert line in text
    assert (ch.FRAME, ch.HOP, ch.PITCHES) == (cr.FRAME, cr.HOP, cr.PITCHES) == (4096, 2048, 48)
    for q in (cr.QM, cr.Qm):                               # the profiles as the header prints them
        assert "{" + ", ".join(str(v) for v in q) + "}" in re.sub(r"\s*\n \*\s*", " ", text)
    assert not any("chroma" in name.lower() for name in bliss_amd.__all__)     # the package's own names are unchanged


def test_record_layout():
    S, F = _lib.SongChroma, _lib.FrameChroma
    assert C.sizeof(S) == 128 == CHROMA_DTYPE.itemsize and C.sizeof(F) == 96 == FRAME_CHROMA_DTYPE.itemsize
    assert [f[0] for f in S._fields_] == list(OFFSETS) == list(CHROMA_DTYPE.names)
    for name, off in OFFSETS.items():
        assert getattr(S, name).offset == off == CHROMA_DTYPE.fields[name][1], name
    src = "#include <stddef.h>\n#include \"bliss_amd.h\"\n" + "".join(
        f"_Static_assert(offsetof(bl_amd_song_chroma, {k}) == {v}, \"{k}\");\n" for k, v in OFFSETS.items()) + \
        "_Static_assert(sizeof(bl_amd_song_chroma) == 128, \"size\");\n" \
        "_Static_assert(sizeof(bl_amd_frame_chroma) == 96, \"size\");\n"
    inc = os.path.join(ROOT, "include")
    subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", inc, "-x", "c", "-"], input=src, text=True, check=True)
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-fsyntax-only", "-I", inc, "-x", "c", "-"],
                   input="#include \"bliss_amd.h\"\nint bl_test_unit;\n", text=True, check=True)
    raw = bytes(range(128)) * 2
    a = ch.chroma_to_numpy(raw)
    assert a.shape == (2,) and a.tobytes() == raw and int(a["frames"][0]) == 0x73727170
    s, f = ch.chroma_to_numpy(raw, bytes(range(96)) * 3)
    assert f.shape == (3,) and f["x"].shape == (3, 12) and int(f["x"][0][1]) == 0x0F0E0D0C0B0A0908


def test_frames_is_plain_arithmetic():
    lib = bliss_amd.load()
    for n, chn, want in ((0, 1, 0), (1, 1, 0), (4095, 1, 0), (4096, 1, 1), (6143, 1, 1), (6144, 1, 2), (8191, 2, 0),
                         (8192, 2, 1), (8193, 2, 1), (12287, 2, 1), (12288, 2, 2), (2 ** 31 - 1, 1, 2 ** 20 - 2),
                         (2 ** 31 - 1, 2, 2 ** 19 - 2), (-1, 1, -1), (1000, 0, -1), (1000, 3, -1)):
        assert lib.bl_amd_chroma_frames(n, chn) == want, (n, chn)
        if want >= 0:
            assert cr.frames_of(n, chn) == want


def test_key_names():
    lib = bliss_amd.load()
    buf = C.create_string_buffer(b"zzzzzzz", 8)
    for key in range(24):
        assert lib.bl_amd_chroma_key_name(key, buf) == 0 and buf.value.decode() == cr.key_name(key)
    assert [cr.key_name(k) for k in (0, 6, 10, 12, 21, 22)] == ["C", "F#", "A#", "Cm", "Am", "A#m"]
    for key in (-1, 24, -2 ** 31, 2 ** 31 - 1):
        buf.value = b"zzzzzzz"
        assert lib.bl_amd_chroma_key_name(key, buf) == _lib.BL_UNEXPECTED and buf.value == b""
    assert lib.bl_amd_chroma_key_name(3, None) == _lib.BL_UNEXPECTED
    rec = np.zeros(4, CHROMA_DTYPE)
    rec["key"] = [-1, 0, 18, 23]
    assert ch.key_names(rec) == ["", "C", "F#m", "Bm"]
    for bad in (np.zeros((2, 2), CHROMA_DTYPE), np.zeros(128, np.uint8)):
        with pytest.raises(ValueError):
            ch.key_names(bad)


def test_wrappers_reject_bad_songs():
    pcm = [np.zeros(8192, np.int16)]
    for songs, chn in (([], 1), ([np.zeros(0, np.int16)], 1), ([np.zeros(1, np.int16)], 2), (pcm, 3), (pcm, [1, 2])):
        with pytest.raises(ValueError):
            ch.chroma_batch_host(songs, chn)

    class NoCorpus:
        chroma_raw = None
    with pytest.raises(RuntimeError):
        ch.fetch_chroma(NoCorpus())


def test_entry_points_fail_loudly_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present: tests/test_gpu_chroma.py runs these calls")
    lib = bliss_amd.load()
    U = _lib.BL_UNEXPECTED
    n = 2
    desc = (_lib.SongDesc * n)()
    for i in range(n):
        desc[i].pcm_offset, desc[i].n_samples, desc[i].channels = 16384 * i, 9000, 1 + i
    out = (_lib.SongChroma * n)()
    C.memset(out, 0xAB, C.sizeof(out))
    pcm = np.zeros(40000, np.int16)
    aligned = pcm.ctypes.data + (-pcm.ctypes.data) % 16       # the argument checks pass: it is the device that is missing
    assert lib.bl_amd_chroma_batch_device(aligned, desc, n, C.addressof(out), None, 0, None) == U
    assert lib.bl_amd_ctx_chroma_batch_device(None, aligned, desc, n, C.addressof(out), None, 0, None) == U
    songs = [np.ones(9000, np.int16), np.ones(9000, np.int16)]
    ptrs = (C.c_void_p * n)(*[s.ctypes.data for s in songs])
    assert lib.bl_amd_chroma_batch_host(ptrs, (C.c_int32 * n)(9000, 9000), (C.c_int32 * n)(1, 2), n, out, None) == U
    assert bytes(out) == b"\xab" * C.sizeof(out)
    with pytest.raises(RuntimeError) as e:
        ch.chroma_batch_host(songs, [1, 2], frames=True)
    assert re.findall(r"bl_amd_\w+", str(e.value)) == ["bl_amd_chroma_batch_host"]


def test_table_header_on_the_cpu(tmp_path):
    exe = str(tmp_path / "test_chroma_table_host.bin")
    cc = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                         os.path.join(ROOT, "tests", "host", "test_chroma_table_host.cpp"), "-o", exe],
                        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert cc.returncode == 0, "g++ failed:\n" + cc.stdout
    out = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout
    assert "sum L 56880, largest sum |c| 137690" in out.stdout
