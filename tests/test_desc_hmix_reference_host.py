"""Harmonic mixes (bl_amd_desc_hmix_*, bl_amd_hmix_*, bliss_amd.descriptor.hmix / hmix_device) without a device: the
reference of tests/desc_hmix_reference.py against a brute-force loop, its switches against the cases the GPU tests
run, what keeps those cases from passing vacuously, the host arithmetic of the wheel and of the attributes, and the
checks the C entry points and the Python wrappers make before any device work.  Part 1 needs no library."""
import ctypes as C

import numpy as np
import pytest

import bliss_amd
import bliss_amd.descriptor as D
from bliss_amd import _lib
from bliss_amd.records import CHROMA_DTYPE, RHYTHM_DTYPE
from tests import desc_chain_reference as R
from tests import desc_hmix_reference as H
from tests import desc_reference as DR


# ---- 1. the reference

def _rows(order, dist2):
    """per chain the filled slots as [(song, d2)], once everything behind them is -1 / 2^64 - 1"""
    out = []
    for o, d in zip(order, dist2):
        k = int((o >= 0).sum())
        assert (o[:k] >= 0).all() and (o[k:] == -1).all() and (d[k:] == np.uint64(DR.EMPTY)).all()
        out.append([(int(a), int(b)) for a, b in zip(o[:k], d[:k])])
    return out


CASES = H.cases()
BASE = {name: H.hmix(**kw) for name, kw in CASES.items()}
RULED = [name for name, kw in CASES.items() if kw["rule"]["flags"] & (H.KEY | H.TEMPO)]


def _plain(kw):
    return {k: v for k, v in kw.items() if k not in ("attrs", "rule")}


@pytest.mark.parametrize("name", list(CASES))
def test_brute_force_equals_the_walker_on_every_case(name):
    kw = CASES[name]
    got = _rows(*BASE[name])
    rest = dict(tags=kw.get("tags"), gap=kw.get("gap", 0), exclude=kw.get("exclude"))
    for c in range(len(got)):
        if "seeds" in kw:
            want = H.brute(kw["lib"], kw["attrs"], kw["rule"], int(kw["seeds"][c]), kw["length"], **rest)
        else:
            want = H.brute(kw["lib"], kw["attrs"], kw["rule"], None, kw["length"], seed_vec=kw["seed_desc"][c], **rest)
        assert got[c] == want, c


@pytest.mark.parametrize("n", [1, 2, 5, 19])
@pytest.mark.parametrize("flags", [1, 2, 3, 6, 7])
def test_brute_force_equals_the_walker_on_tiny_libraries(n, flags):
    """small entries, so plenty of ties; bad seeds; every length around n; tags and a mask"""
    rng = np.random.default_rng(n * 8 + flags)
    lib = rng.integers(-3, 4, size=(n, DR.DIMS)).astype(np.int16)
    attrs = H.random_attrs(n, n + flags, unknown=0.2, tempos=H.EDGE_TEMPOS)
    rule = dict(key_ok=H.asymmetric_table(flags), tempo_tol=50, flags=flags)
    tags, ex = rng.integers(-1, 3, size=n).astype(np.int32), rng.random(n) < 0.2
    seeds = list(range(n)) + [-1, n]
    for length in (1, 2, n, n + 3):
        got = _rows(*H.hmix(lib, attrs, rule, seeds=seeds, length=length, tags=tags, gap=1, exclude=ex))
        for c, s in enumerate(seeds):
            assert got[c] == H.brute(lib, attrs, rule, s, length, tags, 1, ex), (c, length)
        sd = np.concatenate([lib[:2], lib[-1:] + 1])
        got = _rows(*H.hmix(lib, attrs, rule, seed_desc=sd, length=length, tags=tags, gap=1, exclude=ex))
        for c in range(sd.shape[0]):
            assert got[c] == H.brute(lib, attrs, rule, None, length, tags, 1, ex, seed_vec=sd[c]), (c, length)


def test_every_switch_has_a_case():
    assert set(H.SWITCH_CASE) == set(H.BUGS)
    assert {case for case, _ in H.SWITCH_CASE.values()} <= set(CASES)


@pytest.mark.parametrize("bug", H.BUGS)
def test_every_switch_changes_its_row_of_its_case(bug):
    case, row = H.SWITCH_CASE[bug]
    order, dist2 = H.hmix(**CASES[case], bugs=(bug,))
    want_o, want_d = BASE[case]
    assert not (np.array_equal(order[row], want_o[row]) and np.array_equal(dist2[row], want_d[row]))


@pytest.mark.parametrize("name", list(CASES))
def test_a_rule_that_is_off_or_finds_nothing_known_is_the_plain_chain(name):
    kw = CASES[name]
    want = R.chain(**_plain(kw))
    off = dict(kw, rule=dict(kw["rule"], flags=0))
    unknown = np.stack([np.zeros(kw["lib"].shape[0], dtype=np.int64),
                        np.resize([24, 200, 255], kw["lib"].shape[0])], axis=1)
    for got in (H.hmix(**off), H.hmix(**dict(off, attrs=None)), H.hmix(**dict(kw, attrs=unknown))):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("name", RULED)
def test_no_case_passes_vacuously(name):
    """the rule changes at least a quarter of the slots it could change, and at least half of the chains go on for
    four slots or more under it"""
    assert RULED == list(CASES)
    order = BASE[name][0]
    plain = R.chain(**_plain(CASES[name]))[0]
    filled = order[:, 1:] >= 0
    assert 4 * int(((order[:, 1:] != plain[:, 1:]) & filled).sum()) >= int(filled.sum()) > 0
    assert 2 * int(((order >= 0).sum(axis=1) >= 4).sum()) >= order.shape[0]


def test_the_cases_hold_what_they_are_named_for():
    keys = CASES["keys"]
    table = keys["rule"]["key_ok"]
    assert any((table[a] >> b & 1) != (table[b] >> a & 1) for a in range(24) for b in range(24))
    assert {24, 200, 255} <= set(keys["attrs"][:, 1].tolist())
    for name in ("tempo_edges", "half_double"):
        kw = CASES[name]
        assert set(H.EDGE_TEMPOS) | {0} <= set(kw["attrs"][:, 0].tolist())
        # a consecutive pair with equality on a boundary, for every window the rule has
        order, tol, at = BASE[name][0], kw["rule"]["tempo_tol"], kw["attrs"]
        pairs = {(int(at[p, 0]), int(at[j, 0])) for row in order for p, j in zip(row[:-1], row[1:]) if j >= 0}
        assert any(a and b and 1000 * abs(b - a) == tol * a for a, b in pairs)
        if name == "half_double":
            assert any(a and b and 1000 * abs(2 * b - a) == tol * a for a, b in pairs)
            assert any(a and b and 1000 * abs(b - 2 * a) == 2 * tol * a for a, b in pairs)
    # one unit past each boundary of 120.00 BPM at 50 per mille is blocked, the boundary itself passes
    attrs = np.array([[t, 0] for t in H.EDGE_TEMPOS])
    ok = H.pair_ok((12000, 0), attrs, dict(key_ok=[0] * 24, tempo_tol=50, flags=H.TEMPO | H.HALF_DOUBLE))
    assert ok.tolist() == [True, True, False, True, False, True, False, True, False, True, False, True, False]
    wheel = CASES["wheel_rules"]
    assert wheel["gap"] > 0 and wheel["exclude"].any() and wheel["exclude"][wheel["seeds"][3]]


# ---- 2. the host arithmetic and the C entry points

UNX, OK = _lib.BL_UNEXPECTED, _lib.BL_OK
NAMES = ["C", "C#", "D", "D#", "E", "F", "F#", "G", "G#", "A", "A#", "B"]


def test_struct_layouts():
    assert C.sizeof(_lib.HmixAttr) == 4 and C.sizeof(_lib.HmixRule) == 104
    assert (_lib.HmixAttr.tempo.offset, _lib.HmixAttr.key.offset, _lib.HmixAttr.reserved.offset) == (0, 2, 3)
    assert (_lib.HmixRule.key_ok.offset, _lib.HmixRule.tempo_tol.offset, _lib.HmixRule.flags.offset) == (0, 96, 100)


def test_the_camelot_table_is_the_formula():
    lib = bliss_amd.load()
    rule = _lib.HmixRule()
    assert lib.bl_amd_hmix_rule_camelot(C.byref(rule), 60, 7) == OK
    want = H.camelot(60, 7)
    assert list(rule.key_ok) == want["key_ok"] and (rule.tempo_tol, rule.flags) == (60, 7)
    # written out: after a major key the same, a fifth up, a fifth down, the relative minor; likewise after a minor
    for k in range(12):
        assert rule.key_ok[k] == sum(1 << b for b in {k, (k + 7) % 12, (k + 5) % 12, 12 + (k + 9) % 12})
        assert rule.key_ok[12 + k] == sum(1 << b for b in {12 + k, 12 + (k + 7) % 12, 12 + (k + 5) % 12, (k + 3) % 12})
    name = lambda b: NAMES[b % 12] + ("m" if b >= 12 else "")
    after = lambda a: {name(b) for b in range(24) if rule.key_ok[a] >> b & 1}
    assert after(0) == {"C", "G", "F", "Am"} and after(12 + 9) == {"Am", "Em", "Dm", "C"}
    for a in range(24):
        assert bin(rule.key_ok[a]).count("1") == 4
        assert all((rule.key_ok[a] >> b & 1) == (rule.key_ok[b] >> a & 1) for b in range(24))
    sentinel = _lib.HmixRule(tempo_tol=77, flags=5)
    for tol, flags in ((-1, 3), (1001, 3), (60, 8), (60, 4), (60, 5), (60, -1)):
        assert lib.bl_amd_hmix_rule_camelot(C.byref(sentinel), tol, flags) == UNX, (tol, flags)
    assert lib.bl_amd_hmix_rule_camelot(None, 60, 3) == UNX
    assert (sentinel.tempo_tol, sentinel.flags, list(sentinel.key_ok)) == (77, 5, [0] * 24)
    for tol, flags in ((0, 0), (1000, 1), (5, 2), (5, 6)):
        assert lib.bl_amd_hmix_rule_camelot(C.byref(sentinel), tol, flags) == OK
        assert (sentinel.tempo_tol, sentinel.flags) == (tol, flags)
    r = D.camelot_rule(60, half_double=True)
    assert r.dtype == D.HMIX_RULE_DTYPE and r["key_ok"].tolist() == want["key_ok"] and int(r["flags"]) == 7
    assert int(D.camelot_rule(0, key=False)["flags"]) == 2 and int(D.camelot_rule(0, tempo=False)["flags"]) == 1
    for bad in (lambda: D.camelot_rule(1001), lambda: D.camelot_rule(-1), lambda: D.camelot_rule(60.0),
                lambda: D.camelot_rule(60, half_double=True, tempo=False)):
        with pytest.raises(ValueError):
            bad()


def test_attributes_from_records():
    lib = bliss_amd.load()
    rate = 22050
    # (lag, r_prev, r_lag, r_next): no tempo; a parabola's vertex; flat; faster than 655.35 BPM; slower than 0.005 BPM
    lags = [(0, 0, 0, 0), (80, 900, 1000, 950), (86, 5, 5, 5), (1, 0, 9, 3), (12, 7, 9, 8), (3_000_000, 1, 2, 1),
            (20_000, 3, 4, 3)]
    rh = np.zeros(len(lags), dtype=RHYTHM_DTYPE)
    for i, (lag, p, c, nx) in enumerate(lags):
        rh[i]["lag"], rh[i]["r_prev"], rh[i]["r_lag"], rh[i]["r_next"] = lag, p, c, nx
    ch = np.zeros(len(lags), dtype=CHROMA_DTYPE)
    ch["key"] = [-1, 0, 23, 12, 5, -1, 11]
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    bpm = np.array([lib.bl_amd_rhythm_bpm(C.byref(r), rate) for r in (_lib.SongRhythm * len(lags)).from_buffer(rh)])
    assert np.isnan(bpm[0]) and bpm[3] > 655.35 and 100 * bpm[5] < 0.5 and np.isfinite(bpm[1:]).all()
    with np.errstate(invalid="ignore"):
        want_tempo = np.where(np.isnan(bpm), 0, np.clip(np.rint(100 * bpm), 1, 65535)).astype(np.int64)
    assert want_tempo[0] == 0 and want_tempo[3] == 65535 and want_tempo[5] == 1 and 1 < want_tempo[1] < 65535
    want_key = [255, 0, 23, 12, 5, 255, 11]
    out = np.full(len(lags), 0xA5, dtype=np.uint8).repeat(4).view(D.HMIX_ATTR_DTYPE)
    assert lib.bl_amd_hmix_attrs(P(rh, _lib.SongRhythm), P(ch, _lib.SongChroma), len(lags), rate, P(out, _lib.HmixAttr)) == OK
    assert out["tempo"].tolist() == want_tempo.tolist() and out["key"].tolist() == want_key
    assert (out["reserved"] == 0).all()
    got = D.hmix_attrs(rhythm=rh, chroma=ch)
    assert got.dtype == D.HMIX_ATTR_DTYPE and np.array_equal(got, out)
    only_rh, only_ch = D.hmix_attrs(rhythm=rh), D.hmix_attrs(chroma=ch)
    assert only_rh["tempo"].tolist() == want_tempo.tolist() and (only_rh["key"] == 255).all()
    assert (only_ch["tempo"] == 0).all() and only_ch["key"].tolist() == want_key
    other = D.hmix_attrs(rhythm=rh, rate=44100)["tempo"].astype(np.int64)
    assert other[1] in (2 * want_tempo[1] - 1, 2 * want_tempo[1], 2 * want_tempo[1] + 1)
    sentinel = out.copy()
    assert lib.bl_amd_hmix_attrs(P(rh, _lib.SongRhythm), None, 0, rate, P(out, _lib.HmixAttr)) == UNX
    assert lib.bl_amd_hmix_attrs(P(rh, _lib.SongRhythm), None, len(lags), rate, None) == UNX
    assert np.array_equal(out, sentinel)
    for bad in (lambda: D.hmix_attrs(), lambda: D.hmix_attrs(rhythm=rh, chroma=ch[:3]), lambda: D.hmix_attrs(rhythm=ch),
                lambda: D.hmix_attrs(chroma=ch, rate=0)):
        with pytest.raises(ValueError):
            bad()


def _buffers(n=16, nc=3, length=5):
    lib = (_lib.Desc * n)()
    attr = (_lib.HmixAttr * n)()
    seeds = (C.c_int32 * nc)(0, 5, 15)
    q = (_lib.Desc * nc)()
    tags = (C.c_int32 * n)(*range(n))
    ex = (C.c_uint8 * n)()
    order = (C.c_int32 * (nc * length))(*([7] * (nc * length)))
    dist2 = (C.c_uint64 * (nc * length))(*([35] * (nc * length)))
    return lib, attr, seeds, q, tags, ex, order, dist2


def _rule(tol, flags):
    r = _lib.HmixRule(tempo_tol=tol, flags=flags)
    for a in range(24):
        r.key_ok[a] = 0xFFFFFF
    return r


def test_c_entry_points_refuse_bad_arguments_with_or_without_a_device():
    """Arguments, the rule and index seeds are checked before any device work: BL_UNEXPECTED and nothing written."""
    lib = bliss_amd.load()
    n, nc, length = 16, 3, 5
    v, at, good, q, tags, ex, order, dist2 = _buffers(n, nc, length)
    ok = C.byref(_rule(60, 7))
    for bad in ((0, 16, 1), (-1, 2, 3), (0, 1, 2 ** 31 - 1)):
        seeds = (C.c_int32 * nc)(*bad)
        assert lib.bl_amd_desc_hmix_host(v, at, n, ok, seeds, None, nc, length, tags, 1, ex, order, dist2) == UNX
    host_bad = [
        # everything bl_amd_desc_chain_host rejects
        (v, at, n, ok, good, q, nc, length, tags, 1, ex, order, dist2),         # both kinds of seed
        (v, at, n, ok, None, None, nc, length, tags, 1, ex, order, dist2),      # neither
        (v, at, n, ok, good, None, nc, length, tags, 17, ex, order, dist2),
        (v, at, n, ok, good, None, nc, length, tags, -1, ex, order, dist2),
        (v, at, n, ok, good, None, nc, length, None, 1, ex, order, dist2),      # a gap without tags
        (v, at, 0, ok, good, None, nc, length, tags, 1, ex, order, dist2),
        (v, at, 2 ** 27, ok, good, None, nc, length, tags, 1, ex, order, dist2),
        (v, at, n, ok, good, None, nc, 0, tags, 1, ex, order, dist2),
        (v, at, n, ok, good, None, 0, length, tags, 1, ex, order, dist2),
        (v, at, n, ok, good, None, nc, length, tags, 1, ex, None, dist2),       # a NULL order
        (None, at, n, ok, good, None, nc, length, tags, 1, ex, order, dist2),
        # and the rule's own
        (v, at, n, None, good, None, nc, length, tags, 1, ex, order, dist2),                        # a NULL rule
        (v, at, n, C.byref(_rule(60, 8)), good, None, nc, length, tags, 1, ex, order, dist2),      # an unknown flag
        (v, at, n, C.byref(_rule(60, 0x80000001)), good, None, nc, length, tags, 1, ex, order, dist2),
        (v, at, n, C.byref(_rule(60, 4)), good, None, nc, length, tags, 1, ex, order, dist2),      # HALF_DOUBLE alone
        (v, at, n, C.byref(_rule(60, 5)), good, None, nc, length, tags, 1, ex, order, dist2),      # ... with KEY only
        (v, at, n, C.byref(_rule(1001, 3)), good, None, nc, length, tags, 1, ex, order, dist2),    # tempo_tol
        (v, at, n, C.byref(_rule(1001, 0)), good, None, nc, length, tags, 1, ex, order, dist2),
        (v, None, n, C.byref(_rule(60, 1)), good, None, nc, length, tags, 1, ex, order, dist2),    # KEY, no attributes
        (v, None, n, C.byref(_rule(60, 2)), good, None, nc, length, tags, 1, ex, order, dist2),    # TEMPO, none
        (v, None, n, C.byref(_rule(60, 6)), None, q, nc, length, tags, 1, ex, order, dist2),
    ]
    for args in host_bad:
        assert lib.bl_amd_desc_hmix_host(*args) == UNX, args
    A = C.addressof
    V, AT, S, Q, T, X, O, F = A(v), A(at), A(good), A(q), A(tags), A(ex), A(order), A(dist2)
    dev_bad = [
        (V, AT, n, ok, S, Q, nc, length, T, 1, X, O, F), (V, AT, n, ok, None, None, nc, length, T, 1, X, O, F),
        (V, AT, n, ok, S, None, nc, length, T, 17, X, O, F), (V, AT, n, ok, S, None, nc, length, T, -1, X, O, F),
        (V, AT, n, ok, S, None, nc, length, None, 3, X, O, F), (V, AT, 0, ok, S, None, nc, length, T, 1, X, O, F),
        (V, AT, 2 ** 27, ok, S, None, nc, length, T, 1, X, O, F), (V, AT, n, ok, S, None, nc, 0, T, 1, X, O, F),
        (V, AT, n, ok, S, None, 0, length, T, 1, X, O, F), (V, AT, n, ok, S, None, nc, length, T, 1, X, None, F),
        (V, AT, n, ok, S, None, nc, length, T, 1, X, O, None), (None, AT, n, ok, S, None, nc, length, T, 1, X, O, F),
        (V, AT, n, None, S, None, nc, length, T, 1, X, O, F),
        (V, AT, n, C.byref(_rule(60, 8)), S, None, nc, length, T, 1, X, O, F),
        (V, AT, n, C.byref(_rule(60, 16 + 3)), S, None, nc, length, T, 1, X, O, F),
        (V, AT, n, C.byref(_rule(60, 4)), S, None, nc, length, T, 1, X, O, F),
        (V, AT, n, C.byref(_rule(60, 5)), S, None, nc, length, T, 1, X, O, F),
        (V, AT, n, C.byref(_rule(1001, 7)), S, None, nc, length, T, 1, X, O, F),
        (V, AT, n, C.byref(_rule(2 ** 32 - 1, 0)), S, None, nc, length, T, 1, X, O, F),
        (V, None, n, C.byref(_rule(60, 1)), S, None, nc, length, T, 1, X, O, F),
        (V, None, n, C.byref(_rule(60, 2)), S, None, nc, length, T, 1, X, O, F),
        (V, None, n, C.byref(_rule(60, 7)), None, Q, nc, length, T, 1, X, O, F),
    ]
    for args in dev_bad:
        assert lib.bl_amd_desc_hmix_device(*args, None) == UNX, args
        assert lib.bl_amd_ctx_desc_hmix_device(None, *args, None) == UNX, args
    assert list(order) == [7] * (nc * length) and list(dist2) == [35] * (nc * length)


def test_symbols_are_bound_and_the_package_namespace_is_unchanged():
    names = {"bl_amd_desc_hmix_device", "bl_amd_ctx_desc_hmix_device", "bl_amd_desc_hmix_host",
             "bl_amd_hmix_rule_camelot", "bl_amd_hmix_attrs"}
    assert names <= set(_lib.SYMBOLS)
    lib = bliss_amd.load()
    for name in names:
        assert hasattr(lib, name)
    assert not hasattr(bliss_amd, "hmix") and "hmix" not in bliss_amd.__all__
    for fn in ("hmix", "hmix_device", "hmix_attrs", "camelot_rule"):
        assert callable(getattr(D, fn))
    assert (_lib.BL_AMD_HMIX_KEY, _lib.BL_AMD_HMIX_TEMPO, _lib.BL_AMD_HMIX_HALF_DOUBLE) == (H.KEY, H.TEMPO, H.HALF_DOUBLE)


# ---- 3. the Python wrappers

LIB = np.zeros((10, 32), dtype=np.int16)
TAGS = np.arange(10, dtype=np.int32)


def _t(a):
    return pytest.importorskip("torch").from_numpy(a)   # a CPU tensor: the checks come before anything touches a device


@pytest.mark.parametrize("fn", ["hmix", "hmix_device"])
def test_wrappers_refuse_bad_attributes_and_rules_and_what_chain_refuses(fn):
    call = getattr(D, fn)
    dev = fn == "hmix_device"
    ATTRS = np.zeros(10, dtype=D.HMIX_ATTR_DTYPE)
    lib = _t(LIB) if dev else LIB
    attrs = _t(ATTRS.view(np.uint8).reshape(10, 4)) if dev else ATTRS
    wrap = _t if dev else (lambda a: a)
    rule = D.camelot_rule(60, half_double=True)
    off = D.camelot_rule(60, key=False, tempo=False)
    bad_rules = [None, rule.tobytes(), np.zeros(2, dtype=D.HMIX_RULE_DTYPE), np.zeros(26, dtype=np.uint32)]
    for flags, tol in ((8, 60), (4, 60), (5, 60), (3, 1001)):
        r = np.zeros(1, dtype=D.HMIX_RULE_DTYPE)
        r[0] = rule
        r["flags"], r["tempo_tol"] = flags, tol
        bad_rules.append(r)
    for r in bad_rules:
        with pytest.raises((ValueError, TypeError)):
            call(lib, attrs, r, 0, 3)
    with pytest.raises(ValueError):
        call(lib, None, rule, 0, 3)                                  # a rule that tests needs attributes
    bad_attrs = [ATTRS[:9], np.zeros(10, dtype=np.uint32), np.zeros((10, 2), dtype=np.int64)]
    for a in bad_attrs:
        with pytest.raises(ValueError):
            call(lib, wrap(a) if dev and a.dtype.names is None else a, rule, 0, 3)
    # chain's own checks are made here too
    with pytest.raises(ValueError):
        call(lib, attrs, rule, None, 3)
    with pytest.raises(ValueError):
        call(lib, attrs, rule, 0, 3, seed_desc=lib[:2])
    with pytest.raises(ValueError):
        call(lib, attrs, rule, 0, 3, gap=2)
    with pytest.raises(ValueError):
        call(lib, attrs, rule, 0, 0)
    with pytest.raises(ValueError):
        call(lib, attrs, rule, 0, 3, tags=wrap(TAGS[:9]), gap=1)
    with pytest.raises(ValueError):
        call(lib, attrs, rule, 0, 3, exclude=wrap(np.zeros(9, dtype=bool)))
    if not dev:
        with pytest.raises(ValueError):
            call(lib, attrs, rule, [0, 10], 3)
        # well-formed calls reach their entry point: a RuntimeError that names it without a device, rows with one
        for args in ((lib, attrs, rule, [0, 4], 3), (lib, None, off, [0, 4], 3),
                     (lib, attrs, rule, None, 3, TAGS, 1, TAGS > 7, LIB[:2])):
            try:
                order, dist2 = call(*args)
            except RuntimeError as e:
                assert "bl_amd_desc_hmix_host" in str(e)
            else:
                assert order.dtype == np.int32 and dist2.dtype == np.uint64 and order.shape == dist2.shape
