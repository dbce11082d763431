"""The fingerprint reference (tests/fprint_reference.py) and the host arithmetic of bl_amd_fprint_* (bl_api.c,
bl_amd_fprint_shape), without a GPU: the numpy words against the Python-integer ones, every deliberate mistake changing a
named input's words or record, the symmetry of the match, the robustness table of DESIGN.md 4.22 regenerated from
tests/chroma_reference.py's chromagram of seeded melodies, and the wrappers' argument checks."""
import ctypes as C
import math

import numpy as np
import pytest

import bliss_amd.fingerprint as fp
from bliss_amd import _lib
from bliss_amd.records import FPRINT_MATCH_DTYPE
from tests import chroma_reference as cr
from tests import fprint_reference as fr

FPRINT_SYMBOLS = ("bl_amd_fprint_words", "bl_amd_fprint_words_device", "bl_amd_ctx_fprint_words_device",
                  "bl_amd_fprint_words_host", "bl_amd_fprint_match_device", "bl_amd_ctx_fprint_match_device",
                  "bl_amd_fprint_match_host", "bl_amd_fprint_shape", "bl_amd_fprint_ber",
                  "bl_amd_fprint_offset_seconds", "bl_amd_fprint_profile_ms")


def test_symbols_and_record_layout(lib):
    for name in FPRINT_SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert C.sizeof(_lib.FprintMatch) == 24 == FPRINT_MATCH_DTYPE.itemsize == fr.MATCH_DTYPE.itemsize
    assert [f[0] for f in _lib.FprintMatch._fields_] == list(fr.MATCH_DTYPE.names)
    assert [FPRINT_MATCH_DTYPE.fields[k][1] for k in fr.MATCH_DTYPE.names] == [0, 4, 8, 12, 16, 20]


# ---- words -------------------------------------------------------------------------------------------------------

def test_numpy_words_equal_the_python_integer_ones():
    for seed, T, hi in ((1, 16, 1 << 30), (2, 40, fr.X_MAX), (3, 33, 4), (4, 17, 2)):
        X = fr.random_frames(seed, T, hi)
        w = fr.words(X)
        assert w.size == T - 15
        assert [int(v) for v in w] == [fr.words_slow(X, t) for t in range(T - 15)]
    top = np.full((20, 12), fr.X_MAX - 1, dtype=np.int64)   # every sum at its bound: 16 X_MAX < 2^45
    top[8:, ::2] -= 1
    assert [int(v) for v in fr.words(top)] == [fr.words_slow(top, t) for t in range(5)]
    assert 16 * fr.X_MAX < 2 ** 45 and fr.X_MAX > 2 ** 39.19


def test_word_counts(lib):
    for T in (0, 1, 15, 16, 17, 31, 32, 33, 1000, (1 << 20) - 1):
        assert fp.words_count(T) == fr.words_count(T) == max(0, T - 15)
    assert lib.bl_amd_fprint_words(-1) == -1
    assert fr.words(np.zeros((15, 12))).size == 0


def test_silence_and_ties_give_zero_bits():
    assert fr.words(np.zeros((20, 12))).tolist() == [0] * 5
    flat = np.full((16, 12), 7, dtype=np.int64)             # every comparison a tie
    assert fr.words(flat).tolist() == [0]
    assert fr.words(flat, {"ge"}).tolist() == [0xFFFFFFFF]


def word_inputs():
    """named chromagrams on which the word mistakes show"""
    ramp = np.arange(12, dtype=np.int64)[None, :] * np.ones((24, 1), np.int64) + 1      # classes rise with k, flat in t
    last = np.zeros((16, 12), np.int64)
    last[7, 0] = 5                                                                      # S1's eighth frame, class 0
    return {"flat": np.full((16, 12), 7, np.int64), "ramp": ramp, "fall": 13 - ramp, "eighth frame": last,
            "random": fr.random_frames(5, 40)}


@pytest.mark.parametrize("switch,name", [("ge", "flat"), ("half7", "eighth frame"), ("next_down", "ramp"),
                                         ("no_wrap", "fall"), ("count16", "random")])
def test_every_word_mistake_changes_a_named_input(switch, name):
    X = word_inputs()[name]
    good, bad = fr.words(X), fr.words(X, {switch})
    assert good.size != bad.size or not np.array_equal(good, bad), (switch, name)


# ---- match -------------------------------------------------------------------------------------------------------

def match_inputs():
    """named (a, b, D, min_overlap) on which the match mistakes show, each with the offset the definition gives"""
    w = fr.random_words(7, 60)
    four = np.tile(fr.random_words(8, 4), 10)                  # period 4
    two = np.tile(fr.random_words(9, 2), 6)                    # period 2
    ones = np.ones(8, np.uint32)
    return {
        "trimmed": ((w, w[5:], 16, 1), -5),                    # b = a without its first 5 words
        "edge": ((w, w[5:], 16, 55), -5),                      # the largest overlap is exactly min_overlap
        "far tie": ((four, four[4:], 8, 1), 0),                # zero errors at d = -8, -4, 0, 4, 8
        "sign tie": ((two[1:11], two, 1, 1), -1),              # zero errors at d = -1 and +1, not at 0
        "thirds": ((np.array([3, 0, 0], np.uint32), np.zeros(3, np.uint32), 0, 1), 0),   # e 2, n 3: 43690.67
        "short b": ((ones, np.zeros(4, np.uint32), 0, 1), 0),  # n = 4 of Wa = 8
        "high bits": ((w, w ^ np.uint32(0xFFFF0000), 2, 1), 0),   # all errors in the high half
    }


@pytest.mark.parametrize("switch,name", [("d_sign", "trimmed"), ("overlap_gt", "edge"), ("tie_far", "far tie"),
                                         ("tie_pos", "sign tie"), ("round_score", "thirds"), ("full_len", "short b"),
                                         ("pop16", "high bits")])
def test_every_match_mistake_changes_a_named_input(switch, name):
    args, offset = match_inputs()[name]
    good, bad = fr.match(*args)[0], fr.match(*args, {switch})[0]
    assert good["status"] == fr.BL_OK and good["offset"] == offset
    assert good != bad, (switch, name)


def test_named_inputs_are_what_their_names_say():
    m = {k: fr.match(*v[0]) for k, v in match_inputs().items()}
    assert m["trimmed"][0]["errors"] == 0 and m["trimmed"][0]["overlap"] == 55
    assert m["edge"][0]["overlap"] == 55 and max(m["edge"][2]) == 55
    assert [e for e, n in zip(m["far tie"][1], m["far tie"][2])][0::4] == [0] * 5
    assert m["sign tie"][1] == [0, m["sign tie"][1][1], 0] and m["sign tie"][1][1] > 0
    assert m["thirds"][0]["score"] == 43690 and m["short b"][0]["score"] == 65536
    assert m["high bits"][0]["errors"] == 16 * 60
    assert set(fr.SWITCHES) == {"ge", "half7", "next_down", "no_wrap", "count16", "d_sign", "overlap_gt", "tie_far",
                                "tie_pos", "round_score", "full_len", "pop16"}


def test_swapping_a_and_b_negates_a_unique_offset():
    rng = np.random.default_rng(21)
    seen = 0
    for k in range(30):
        wa, wb = int(rng.integers(1, 50)), int(rng.integers(1, 50))
        a = fr.random_words(100 + k, wa)
        b = fr.noisy_copy(np.concatenate([fr.random_words(200 + k, 7), a])[:wb], 300 + k) if k % 2 else \
            fr.random_words(400 + k, wb)
        D, mo = int(rng.integers(0, 20)), int(rng.integers(1, 6))
        ab, e_ab, n_ab = fr.match(a, b, D, mo)
        ba, e_ba, n_ba = fr.match(b, a, D, mo)
        assert e_ab == e_ba[::-1] and n_ab == n_ba[::-1]
        if ab["status"] != fr.BL_OK:
            assert ba["status"] != fr.BL_OK
            continue
        scores = [e * 65536 // n for e, n in zip(e_ab, n_ab) if n >= mo]
        if scores.count(min(scores)) == 1:
            seen += 1
            assert ba["offset"] == -ab["offset"] and ba["errors"] == ab["errors"] and ba["overlap"] == ab["overlap"]
    assert seen >= 10


def test_batch_reference_answers_bad_indices_with_the_failed_record():
    w = fr.random_words(31, 30)
    rec, prof = fr.match_batch(w, [10, 20], w, [10, 20], [(0, 1), (-1, 0), (0, 2), (1, 1)], 3)
    assert rec["status"].tolist() == [0, -2, -2, 0] and rec["score"][1] == fr.NO_SCORE
    assert not prof[1].any() and not prof[2].any() and prof[3, 3].tolist() == [0, 20]
    assert rec.tobytes()[24:48] == np.array([(0, 0, 0, fr.NO_SCORE, -2, 0)], dtype=fr.MATCH_DTYPE).tobytes()


# ---- host arithmetic through ctypes --------------------------------------------------------------------------------

def test_ber_and_offset_seconds(lib):
    rec = np.zeros(3, dtype=FPRINT_MATCH_DTYPE)
    rec[0] = (48, 100, -5, 31457, 0, 0)
    rec[1] = (0, 0, 0, fr.NO_SCORE, _lib.BL_UNEXPECTED, 0)
    rec[2] = (0, 7, 14, 0, 0, 0)
    b, s = fp.ber(rec), fp.offset_seconds(rec, 22050)
    assert b[0] == 48 / 3200.0 and math.isnan(b[1]) and b[2] == 0.0
    assert s[0] == -5 * 2048 / 22050 and math.isnan(s[1]) and s[2] == 14 * 2048 / 22050
    assert abs(fp.offset_seconds(rec, 22050)[2] - 1.3) < 0.001          # "starts 1.3 s later"
    assert fp.offset_seconds(rec, 44100)[2] == 14 * 2048 / 44100
    assert math.isnan(lib.bl_amd_fprint_ber(None)) and math.isnan(lib.bl_amd_fprint_offset_seconds(None, 22050))
    one = _lib.FprintMatch(1, 1, 1, 65536, 0, 0)
    assert math.isnan(lib.bl_amd_fprint_offset_seconds(C.byref(one), 0))
    assert lib.bl_amd_fprint_ber(C.byref(one)) == 1 / 32.0


def test_shape_describes_the_tiling(lib):
    for D in (0, 1, 2, 63, 64, 127, 128, 511, 512, 1024):
        block, strip, tile, chunk = fp.shape(D)
        assert block == 256 and strip == 64
        assert tile % strip == 0 and 64 <= tile <= 2048
        assert chunk % 4 == 0 and 4 <= chunk <= 1024
        chunks = -(-(2 * D + 1) // chunk)
        assert (chunks - 1) * chunk < 2 * D + 1 <= chunks * chunk + 3 * chunks   # the chunks tile the offsets
        assert (tile // strip) * (chunk // 4) <= 256                             # a lane per (strip, 4 offsets)
    assert fp.shape(64)[2:] == (448, 132) and fp.shape(0)[2:] == (2048, 4) and fp.shape(1024)[2:] == (64, 684)


def test_pairs_from_knn():
    idx = np.array([[1, 2], [0, -1], [0, 1]], dtype=np.int32)
    assert fp.pairs_from_knn(idx).tolist() == [[0, 1], [0, 2], [1, 0], [1, -1], [2, 0], [2, 1]]
    assert fp.pairs_from_knn(idx).dtype == np.int32
    for bad in (np.zeros(3, np.int32), np.zeros((2, 2), np.float32), np.zeros((2, 2), bool)):
        with pytest.raises(ValueError):
            fp.pairs_from_knn(bad)


def test_wrappers_refuse_bad_arguments_before_the_library(lib):
    w = fr.random_words(1, 10)
    pairs = np.array([[0, 0]], np.int32)
    for kw in (dict(max_shift=-1), dict(max_shift=1025), dict(max_shift=1.0), dict(min_overlap=0),
               dict(min_overlap=True)):
        with pytest.raises(ValueError):
            fp.match_host(w, [10], pairs, **kw)
    for counts in ([], [-1], [1 << 20], [11]):
        with pytest.raises(ValueError):
            fp.match_host(w, counts, pairs)
    for p in (np.zeros((0, 2), np.int32), np.zeros((3,), np.int32), np.zeros((2, 3), np.int32)):
        with pytest.raises(ValueError):
            fp.match_host(w, [10], p)
    with pytest.raises(ValueError):
        fp.words_host(np.zeros((5, 11), np.uint64), [5])
    with pytest.raises(ValueError):
        fp.words_host(np.zeros((5, 12), np.uint64), [6])
    with pytest.raises(ValueError):
        fp.words_count(-1)
    with pytest.raises(ValueError):
        fp.shape(2000)


def test_no_device_fails_loudly(lib):
    import torch
    if torch.cuda.is_available():
        return
    w = fr.random_words(1, 10)
    with pytest.raises(RuntimeError):
        fp.match_host(w, [10], np.array([[0, 0]], np.int32))
    with pytest.raises(RuntimeError):
        fp.words_host(np.zeros((16, 12), np.uint64), [16])


# ---- the robustness table ------------------------------------------------------------------------------------------

SAME_BELOW, OTHER_ABOVE = 0.33, 0.40


def test_robustness_table_of_seeded_melodies():
    """The table of DESIGN.md 4.22, regenerated: the bit-error rate at the best offset (max_shift 64, min_overlap 200)
    of variants of melody 1 against it, and of seven other melodies.  Measured on this reference with this generator:
    the worst same-recording case 0.2605 (trimmed by 5.5 hops, half a hop off any grid), the best unrelated pair
    0.4593.  The bounds keep the margins the definition was proposed with (0.08 above the worst same-recording case,
    0.06 below the best unrelated pair) and leave 0.07 between them."""
    x = fr.melody(1)
    wa = fr.words(cr.chromagram(x, 1))
    assert wa.size == 414
    got = {}
    for name, (pcm, ch, offset) in fr.variants(x, 99).items():
        r = fr.match(wa, fr.words(cr.chromagram(pcm, ch)), 64, 200)[0]
        got[name] = (round(fr.ber(r), 4), r["offset"])
        assert r["status"] == fr.BL_OK and fr.ber(r) < SAME_BELOW, (name, got[name])
        assert offset is None or r["offset"] == offset, (name, got[name])
    assert got["trimmed 5 hops"] == (0.0, -5)
    assert got["trimmed 3.25 hops"][1] == -3 and got["trimmed 5.5 hops"][1] in (-5, -6)
    assert got["half gain"][0] < 0.01 and got["stereo, unequal channels"][0] < 0.01
    for seed in range(2, 9):
        r = fr.match(wa, fr.words(cr.chromagram(fr.melody(seed), 1)), 64, 200)[0]
        assert fr.ber(r) > OTHER_ABOVE, (seed, fr.ber(r), r["offset"])
