"""The loudness reference (tests/loud_reference.py) and the host arithmetic of bl_amd_loud_* (bl_api.c), without a GPU:
the K-weighting table, the chunked filter against an unchunked scipy.signal.lfilter, the EBU Tech 3341 / 3342 sequences
inside the standards' own tolerances, every deliberate mistake changing a named input, and header / bindings / exports
agreement and the wrappers' argument checks."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import bliss_amd.loudness as ld
from bliss_amd import _lib
from bliss_amd.records import LOUD_DTYPE
from tests import loud_reference as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# ITU-R BS.1770-4, tables 1 and 2 (48 kHz): b0 b1 b2 a1 a2 of the shelf, a1 a2 of the high-pass
TABLE_48K = (1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
             -1.99004745483398, 0.99007225036621)


def coefs(p):
    return [float(x) for x in (*p.s1_b, *p.s1_a, *p.s2_a)]


# ---- K-weighting -----------------------------------------------------------------------------------------------------

def test_kweight_reproduces_the_48k_table():
    p = ld.kweight(48000)
    assert max(abs(a - b) for a, b in zip(coefs(p), TABLE_48K)) <= 1e-12
    assert (p.hop, p.warm) == (4800, 4096)
    assert p.abs_gate == math.floor(4 * 4800 * 2 ** 30 * 10 ** -6.9309)
    # -70 LUFS: a block exactly on the gate reads -70 to the gate's own rounding
    assert abs(-0.691 + 10 * math.log10(p.abs_gate / (4 * 4800 * 2 ** 30)) + 70.0) < 1e-5


@pytest.mark.parametrize("rate", [8000, 22050, 32000, 44100, 48000])
def test_kweight_is_the_references_design(rate):
    p, q = ld.kweight(rate), lr.kweight(rate)
    assert np.allclose(coefs(p), coefs(q), rtol=4e-16, atol=0)
    assert (p.hop, p.warm, p.abs_gate) == (q.hop, q.warm, q.abs_gate) and p.hop == rate // 10


def test_kweight_rejects_other_rates(lib):
    p = _lib.LoudParams()
    for rate in (7990, 48010, 96000, 44101, 0, -44100):
        assert lib.bl_amd_loud_kweight(rate, C.byref(p)) == _lib.BL_UNEXPECTED
        with pytest.raises(ValueError):
            ld.kweight(rate)
    assert lib.bl_amd_loud_kweight(44100, None) == _lib.BL_UNEXPECTED


# ---- the chunked filter against the unchunked one -------------------------------------------------------------------

def test_chunked_hop_energies_agree_with_lfilter():
    """warm = 4096 at 44.1 kHz: noise plus a 50 Hz tone plus DC, the slowest-decaying input of the high-pass.  The bound
    of 1e-8 relative is the issue's; the figure measured here is printed."""
    from scipy.signal import lfilter
    rate = 44100
    p = lr.kweight(rate)
    rng = np.random.default_rng(5)
    F = p.hop * 33 + 100
    t = np.arange(F)
    x = (rng.integers(-3000, 3000, F) + 12000 * np.sin(2 * np.pi * 50 * t / rate) + 6000).astype(np.int16)
    Z = lr.hop_energies([x], [1], p)[0][:, 0].astype(np.float64)
    v = lfilter(p.s1_b, [1.0] + p.s1_a, x.astype(np.float64))
    y = lfilter([1.0, -2.0, 1.0], [1.0] + p.s2_a, v)
    want = (y[:33 * p.hop] ** 2).reshape(33, p.hop).sum(axis=1)
    rel = np.abs(Z - np.floor(want)) / want
    print("largest relative difference", rel.max())
    assert rel.max() <= 1e-8


# ---- the EBU sequences ------------------------------------------------------------------------------------------------

sine, EBU_3341, EBU_3342, ORDER = lr.sine, lr.EBU_3341, lr.EBU_3342, lr.ORDER


@pytest.fixture(scope="module")
def ebu():
    """the nine sequences as 1 kHz stereo sines at 22 050 Hz through the reference, in one vectorised run"""
    p = lr.kweight(22050)
    keys = [("3341", k) for k in EBU_3341] + [("3342", k) for k in EBU_3342]
    pcm = [sine(22050, (EBU_3341 if s == "3341" else EBU_3342)[k][0]) for s, k in keys]
    recs, _ = lr.loud(pcm, [2] * len(pcm), p)
    return p, dict(zip(keys, recs))


@pytest.mark.parametrize("case", sorted(EBU_3341))
def test_tech_3341_programme_loudness(ebu, case):
    p, recs = ebu
    got = lr.lufs(recs[("3341", case)], p.hop)
    print("case", case, got)
    assert abs(got - EBU_3341[case][1]) <= 0.1


@pytest.mark.parametrize("case", sorted(EBU_3342))
def test_tech_3342_loudness_range(ebu, case):
    p, recs = ebu
    got = lr.range_lu(recs[("3342", case)])
    print("case", case, got)
    assert abs(got - EBU_3342[case][1]) <= 1.0


# ---- the deliberate mistakes ------------------------------------------------------------------------------------------

SMALL = lr.plain(lr.kweight(22050), hop=7, warm=5, abs_gate=1000)
def noise(frames, ch, seed):
    return np.random.default_rng(seed).integers(-20000, 20000, frames * ch).astype(np.int16)


def _pcm_case(pcm, ch, p):
    return lambda m: lr.loud([pcm], [ch], p, m)


def _hops_case(z, gate, mono=False):
    return lambda m: lr.gates(z, gate, m, mono=mono)


def _levels(*runs):
    return np.concatenate([np.full(n, v, dtype=np.int64) for n, v in runs])


NAMED_INPUT = {
    # a stereo song of 40 hops and 3 frames: three chunks, the warm-up of chunk 0 clipped to nothing
    "warm_wraps": _pcm_case(noise(7 * 40 + 3, 2, 1), 2, SMALL),
    "state_carried": _pcm_case(noise(7 * 40 + 3, 2, 1), 2, SMALL),
    "count_from_warm": _pcm_case(noise(7 * 40 + 3, 2, 1), 2, SMALL),
    "a_swapped": _pcm_case(noise(7 * 40 + 3, 2, 1), 2, SMALL),
    "sum_order": _pcm_case(np.full(8, 4, dtype=np.int16), 1, ORDER),
    "z_rounded": _pcm_case(noise(7 * 40 + 3, 2, 1), 2, SMALL),
    "partial_hop": _pcm_case(noise(7 * 40 + 3, 2, 1), 2, SMALL),
    "mono_dual": _pcm_case(noise(7 * 40 + 3, 1, 2), 1, SMALL),
    "abs_ge": _hops_case(_levels((12, 250)), 1000),                       # every block exactly on the gate
    "rel_ge": _hops_case(np.array([100, 0, 0, 0, 1900]), 0),              # P0 10 N1 == S1
    "rel_over_all": _hops_case(_levels((12, 1), (4, 40), (12, 400)), 100),
    "block_stride4": _hops_case(_levels((12, 250)), 0),
    "st_gate_unscaled": _hops_case(_levels((60, 125)), 1000),             # ST = 3.75 gates: above 1, below 7.5
    "pct_truncated": _hops_case(_levels((30, 100), (10, 200)), 0),        # M = 2
    # both channels at the largest accepted value: S1 = 39 997 * 8 * (2^46 - 1) > 2^64
    "carry_dropped": _hops_case(np.full((40000, 2), (1 << 46) - 1, dtype=np.int64), 0),
}


def test_every_mistake_has_a_named_input():
    assert set(NAMED_INPUT) == set(lr.MISTAKES)


@pytest.mark.parametrize("mistake", lr.MISTAKES)
def test_mistake_changes_its_named_input(mistake):
    run = NAMED_INPUT[mistake]
    right, wrong = run(()), run((mistake,))
    if isinstance(right, tuple):   # (records, Z)
        same = right[0] == wrong[0] and all(np.array_equal(a, b) for a, b in zip(right[1], wrong[1]))
    else:
        same = right == wrong
    assert not same, f"{mistake} leaves its named input unchanged"


def test_carry_is_needed_for_accepted_input():
    rec = NAMED_INPUT["carry_dropped"](())
    assert rec["abs_sum"] >= 1 << 64 and rec["abs_count"] == 39997


def test_percentile_indices():
    """M = 1, 2 and 101 survivors: the nearest-rank rule of Tech 3342's reference code"""
    one = lr.gates(_levels((30, 100)), 0)
    assert (one["st_gated"], one["lra_lo"], one["lra_hi"]) == (1, 3000, 3000)
    two = lr.gates(_levels((30, 100), (10, 200)), 0)
    assert (two["st_gated"], two["lra_lo"], two["lra_hi"]) == (2, 3000, 4000)
    ramp = np.repeat(np.arange(1000, 1103), 10)   # 1030 hops: 101 starts, each window a level higher than the last
    many = lr.gates(ramp, 0)
    st = sorted(int(ramp[j:j + 30].sum()) for j in range(0, 1001, 10))
    assert (many["st_gated"], many["lra_lo"], many["lra_hi"]) == (101, st[10], st[95])


# ---- header, bindings, exports -------------------------------------------------------------------------------------------

LOUD_SYMBOLS = ("bl_amd_loud_batch_device", "bl_amd_ctx_loud_batch_device", "bl_amd_loud_batch_host",
                "bl_amd_loud_from_hops", "bl_amd_loud_kweight", "bl_amd_loud_lufs", "bl_amd_loud_momentary_max_lufs",
                "bl_amd_loud_short_max_lufs", "bl_amd_loud_range_lu", "bl_amd_loud_gain_db", "bl_amd_loud_profile_ms")


def _struct_fields(name):
    text = open(os.path.join(ROOT, "include", "bliss_amd.h")).read()
    body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        names += [re.sub(r"\[.*", "", w.strip()) for w in re.sub(r"^\s*\w+\s", "", decl.strip() + " ").split(",")
                  if w.strip()]
    return names


def test_header_bindings_and_exports_agree(lib):
    text = open(os.path.join(ROOT, "include", "bliss_amd.h")).read()
    for name in LOUD_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    declared = set(re.findall(r"\b(bl_amd_(?:ctx_)?loud_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == set(LOUD_SYMBOLS)
    assert [f[0] for f in _lib.LoudParams._fields_] == _struct_fields("bl_amd_loud_params")
    assert [f[0] for f in _lib.SongLoud._fields_] == _struct_fields("bl_amd_song_loud")
    assert C.sizeof(_lib.LoudParams) == 72 and C.sizeof(_lib.SongLoud) == 88 == LOUD_DTYPE.itemsize
    assert re.search(r"#define BL_AMD_LOUD_CHUNK 16\b", text) and ld.CHUNK == lr.CHUNK == 16


def test_package_namespace_is_unchanged():
    import bliss_amd
    assert "loudness" not in bliss_amd.__all__ and not any("loud" in n for n in bliss_amd.__all__)


# ---- host arithmetic ------------------------------------------------------------------------------------------------------

def _record(d):
    rec = np.zeros(1, dtype=LOUD_DTYPE)
    for f in lr.FIELDS:
        if f in ("gated_sum", "abs_sum"):
            rec[f][0] = (d[f] & ((1 << 64) - 1), d[f] >> 64)
        else:
            rec[f][0] = d[f]
    return rec


def test_figures_follow_the_records():
    hop = 2205
    d = lr.gates(_levels((200, 3 << 40), (200, 3 << 37)), 1000)
    rec = _record(d)
    assert lr.rec_ints(rec, 0) == d
    integrated, momentary, short = ld.lufs(rec, hop)
    assert integrated[0] == pytest.approx(lr.lufs(d, hop), abs=1e-12)
    assert momentary[0] == pytest.approx(-0.691 + 10 * math.log10(d["momentary_max"] / (4 * hop * 2 ** 30)), abs=1e-12)
    assert short[0] == pytest.approx(-0.691 + 10 * math.log10(d["st_max"] / (30 * hop * 2 ** 30)), abs=1e-12)
    assert ld.range_lu(rec)[0] == pytest.approx(lr.range_lu(d), abs=1e-12) and 8.9 < ld.range_lu(rec)[0] < 9.1
    assert ld.gain_db(rec, hop, -18.0)[0] == pytest.approx(-18.0 - lr.lufs(d, hop), abs=1e-12)
    big = _record(NAMED_INPUT["carry_dropped"](()))   # the high limb counts
    assert ld.lufs(big, hop)[0] == pytest.approx(lr.lufs(NAMED_INPUT["carry_dropped"](()), hop), abs=1e-9)
    silent = _record(lr.gates(_levels((50, 0)), 1000))
    assert ld.lufs(silent, hop)[0] == -math.inf and ld.range_lu(silent)[0] == 0.0 and ld.gain_db(silent, hop)[0] == 0.0


def test_figures_reject_bad_arguments(lib):
    rec = _record(lr.gates(_levels((50, 1 << 30)), 1000))
    assert math.isnan(lib.bl_amd_loud_lufs(None, 2205)) and math.isnan(lib.bl_amd_loud_range_lu(None))
    ptr = rec.ctypes.data_as(C.POINTER(_lib.SongLoud))
    assert math.isnan(lib.bl_amd_loud_lufs(ptr, 0)) and math.isnan(lib.bl_amd_loud_gain_db(ptr, 0, -18.0))
    with pytest.raises(ValueError):
        ld.lufs(np.zeros(1, dtype=np.uint8), 2205)
    with pytest.raises(ValueError):
        ld.lufs(rec, 0)
    with pytest.raises(ValueError):
        ld.gain_db(rec, 2205, math.nan)


# ---- the wrappers' argument checks -----------------------------------------------------------------------------------------

def test_params_are_checked():
    p = ld.kweight(44100)
    for kw in (dict(hop=0), dict(hop=4801), dict(warm=-1), dict(warm=8193), dict(abs_gate=1 << 56), dict(abs_gate=-1),
               dict(hop=4410.0), dict(s1_b=(1.0, math.inf, 0.0)), dict(s2_a=(math.nan, 0.0)), dict(s1_a=(1.0,))):
        args = dict(s1_b=tuple(p.s1_b), s1_a=tuple(p.s1_a), s2_a=tuple(p.s2_a), hop=p.hop, warm=p.warm,
                    abs_gate=p.abs_gate)
        args.update(kw)
        with pytest.raises(ValueError):
            ld.params(**args)
    q = ld.params(p.s1_b, p.s1_a, p.s2_a, 7, 5, 1000)
    assert (q.hop, q.warm, q.abs_gate) == (7, 5, 1000) and coefs(q) == coefs(p)


def test_host_wrappers_check_their_arguments(lib):
    p = ld.kweight(44100)
    x = np.zeros(100, dtype=np.int16)
    with pytest.raises(ValueError):
        ld.loud_host([x], 3, p)
    with pytest.raises(ValueError):
        ld.loud_host([], 1, p)
    with pytest.raises(ValueError):
        ld.loud_host([x[:0]], 1, p)
    with pytest.raises(ValueError):
        ld.loud_host([x], 1, "44100")
    with pytest.raises(ValueError):
        ld.from_hops([], p)
    with pytest.raises(ValueError):
        ld.from_hops([np.array([1 << 46])], p)
    with pytest.raises(ValueError):
        ld.from_hops([np.array([-1])], p)
    with pytest.raises(ValueError):
        ld.from_hops([np.array([1.5])], p)
    with pytest.raises(ValueError):
        ld.from_hops([np.zeros((4, 3), dtype=np.int64)], p)
    # the library's own refusals come before it looks for a device
    out = (_lib.SongLoud * 1)()
    z = (C.c_uint64 * 8)(*([5] * 7 + [1 << 46]))
    hops = (C.c_int32 * 1)(4)
    assert lib.bl_amd_loud_from_hops(z, hops, 1, C.byref(p), out) == _lib.BL_UNEXPECTED
    assert lib.bl_amd_loud_from_hops(z, hops, 0, C.byref(p), out) == _lib.BL_UNEXPECTED
    assert lib.bl_amd_loud_from_hops(None, hops, 1, C.byref(p), out) == _lib.BL_UNEXPECTED
    assert lib.bl_amd_loud_from_hops(z, hops, 1, None, out) == _lib.BL_UNEXPECTED
    assert lib.bl_amd_loud_from_hops(z, (C.c_int32 * 1)(-1), 1, C.byref(p), out) == _lib.BL_UNEXPECTED
    desc = (_lib.SongDesc * 1)(_lib.SongDesc(0, 100, 3, 1))
    assert lib.bl_amd_loud_batch_device(C.c_void_p(4096), desc, 1, C.byref(p), C.c_void_p(4096), None, 0,
                                        None) == _lib.BL_UNEXPECTED
    assert bytes(out) == bytes(88)
