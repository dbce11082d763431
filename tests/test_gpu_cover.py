"""Cover and version matching on the GPU (bl_amd_cover_units_device, bl_amd_cover_match_device, their context and host
forms, bliss_amd.cover): every byte of the units and of bl_amd_cover_match is compared with == against
tests/cover_reference.py.  There is no tolerance anywhere.

The outputs are filled with 0xA5 before the call and carry 16 guard bytes, so a byte the kernels do not write, or one
they write too far, shows.  The alignment gets crafted units: lengths around a strip of 64 columns and a block of 64
rows (bl_amd_cover_shape), a three-letter alphabet so that ties are the rule, rotated copies, constant songs, a short
song between two copies of a longer one, and the longest song the call takes."""
import ctypes as C

import numpy as np
import pytest

import bliss_amd
import bliss_amd.cover as cover
from bliss_amd import _lib
from bliss_amd.records import COVER_MATCH_DTYPE
from tests import cover_reference as cr
from tests import form_reference as fr

pytestmark = pytest.mark.gpu

UNEXPECTED = _lib.BL_UNEXPECTED
SENTINEL, GUARD = 0xA5, 16


def filled(nbytes):
    import torch
    return torch.full((nbytes + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")


def fetch(t, nbytes):
    import torch
    torch.cuda.synchronize()
    raw = t.cpu().numpy()
    assert (raw[nbytes:] == SENTINEL).all(), "written past the end"
    return raw[:nbytes].tobytes()


def to_device(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


class Match:
    """one device call over the sets (lists of (U, 12) unit arrays; set_b None: the self form, one pointer twice); the
    records were filled with 0xA5.  A unit of 0x7F bytes follows each set, so a read past a set's end would show."""

    def __init__(self, lib, set_a, set_b, pairs, p, ctx=None, bad=None):
        self.set_a, self.set_b, self.p = set_a, set_a if set_b is None else set_b, dict(p)
        self.pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
        guard = np.full((1, 16), 0x7F, np.uint8)
        self.ua = to_device(np.concatenate([cr.cat(set_a), guard]))
        self.ub = self.ua if set_b is None else to_device(np.concatenate([cr.cat(set_b), guard]))
        self.dp = to_device(self.pairs)
        self.n = self.pairs.shape[0]
        self.rec = filled(40 * self.n)
        self.params = _lib.CoverParams(*[p[k] for k in ("thr", "gap", "transpose", "reserved")])
        ca, cb = [len(x) for x in self.set_a], [len(x) for x in self.set_b]
        ptr = lambda t: C.c_void_p(t.data_ptr())
        arg = dict(a=ptr(self.ua), ca=(C.c_int32 * len(ca))(*ca), na=len(ca), b=ptr(self.ub),
                   cb=(C.c_int32 * len(cb))(*cb), nb=len(cb), pairs=ptr(self.dp), n=self.n, p=C.byref(self.params),
                   rec=ptr(self.rec))
        for k, v in (bad or {}).items():
            arg[k] = v(self) if callable(v) else v
        args = tuple(arg[k] for k in ("a", "ca", "na", "b", "cb", "nb", "pairs", "n", "p", "rec"))
        if ctx is None:
            self.rc = lib.bl_amd_cover_match_device(*args, None)
        else:
            self.rc = lib.bl_amd_ctx_cover_match_device(ctx.handle, *args, None)

    def read(self):
        assert self.rc == 0
        return np.frombuffer(fetch(self.rec, 40 * self.n), dtype=COVER_MATCH_DTYPE)

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return bool((self.rec == SENTINEL).all())

    def reference(self):
        return cr.match_batch(self.set_a, self.set_b, self.pairs, self.p)


def assert_match(m, what=""):
    rec, want = m.read(), m.reference()
    for n in range(m.n):
        for k in COVER_MATCH_DTYPE.names:
            assert int(rec[k][n]) == int(want[k][n]), (f"{what}: pair {n} {m.pairs[n].tolist()} {k} {int(rec[k][n])}, "
                                                       f"want {int(want[k][n])}; record {rec[n]}, want {want[n]}")
    assert rec.tobytes() == want.tobytes(), what
    return rec


# ---- units -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", [1, 3, 16])
def test_units_equal_the_structure_calls_bytes_and_the_reference(gpu_lib, P):
    import torch
    import bliss_amd.form as form
    counts = [0, P, 255 * P + P - 1, 256 * P, 257 * P + P // 2]
    assert [t // P for t in counts] == [0, 1, 255, 256, 257]
    songs = [fr.random_frames(700 + i, t, fr.X_MAX if i % 2 else 1 << 19) for i, t in enumerate(counts)]
    songs[2][:P] = 0                                                  # a silent unit
    X = np.concatenate(songs + [np.zeros((1, 12), np.int64)]).astype(np.uint64)
    n = sum(t // P for t in counts)
    want = np.concatenate([fr.unit_bytes(fr.units(x, P)) for x in songs])
    frames, out = to_device(X), filled(16 * n)
    rc = gpu_lib.bl_amd_cover_units_device(C.c_void_p(frames.data_ptr()), (C.c_int32 * 5)(*counts), 5, P,
                                           C.c_void_p(out.data_ptr()), n, None)
    assert rc == 0 and fetch(out, 16 * n) == want.tobytes()
    f = form.form_device(frames, counts, form.params(pool=P, seg=8, min_lag=4, nov=4), units=True)
    torch.cuda.synchronize()
    assert f["unit_bytes"].cpu().numpy().tobytes() == want.tobytes()
    with bliss_amd.Context(0) as ctx:
        u, uc = cover.units_device(frames, counts, pool=P, ctx=ctx)
        torch.cuda.synchronize()
        assert uc == [0, 1, 255, 256, 257] and u.cpu().numpy().tobytes() == want.tobytes()
    h, hc = cover.units_host(X[:-1], counts, pool=P)
    assert hc == uc and h.tobytes() == want.tobytes()
    e, ec = cover.units_host(np.zeros((0, 12), np.uint64), [0], pool=P)
    assert ec == [0] and e.shape == (0, 16)


# ---- alignment -------------------------------------------------------------------------------------------------------

LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 191, 193)


@pytest.mark.parametrize("thr,gap", [(12000, 0), (9000, 2500)])
def test_all_pairs_of_lengths_around_a_strip(gpu_lib, thr, gap):
    assert cover.shape() == (64, 64)
    abc = cr.alphabet(31, 3)
    set_a = [cr.letters_song(40 + i, n, abc) for i, n in enumerate(LENGTHS)]
    set_b = [cr.letters_song(60 + i, n, abc) for i, n in enumerate(LENGTHS)]
    pairs = [(i, j) for i in range(len(LENGTHS)) for j in range(len(LENGTHS))]
    assert len(pairs) == 121
    rec = assert_match(Match(gpu_lib, set_a, set_b, pairs, cr.params(thr=thr, gap=gap, transpose=0)), f"{thr} {gap}")
    assert (rec["status"] == 0).sum() >= 90 and (rec["status"][:11] == cr.NO_MATCH).all()
    assert_match(Match(gpu_lib, set_a, set_b, pairs, cr.params(thr=thr, gap=gap)), f"{thr} {gap}, r found")


def test_rotated_copies_at_every_transposition(gpu_lib):
    X = cr.chord_song(5, n_chords=15, hold=5)
    a = cr.units(X, 1)
    set_b = [cr.units(cr.transposed(X, r), 1) for r in range(12)]
    pairs = [(0, r) for r in range(12)]
    rec = assert_match(Match(gpu_lib, [a], set_b, pairs, cr.params()), "r found")
    assert rec["transpose"].tolist() == list(range(12)) and (rec["a_end"] == 74).all() and (rec["b_start"] == 0).all()
    assert len(set(rec["score"].tolist())) == 1 and cover.score(rec)[0] > 0.9
    for r in range(12):
        got = assert_match(Match(gpu_lib, [a], set_b, pairs, cr.params(transpose=r)), f"r {r}")
        assert got["score"][r] == rec["score"][r] and got["score"].argmax() == r and (got["transpose"] == r).all()
    base = cr.alphabet(9, 1)[0]
    flat = np.stack([np.roll(base, k) for k in range(12)] * 3)        # every C(r) ties: r = 0
    got = assert_match(Match(gpu_lib, [flat, a], set_b[3:5], [(0, 0), (0, 1), (1, 0)], cr.params()), "flat profile")
    assert got["transpose"].tolist() == [0, 0, 3]


def test_constant_songs_pin_the_origin_precedence_and_the_best_cell(gpu_lib):
    c = np.repeat(cr.alphabet(12, 1), 130, axis=0)
    sets = [c[:5], c[:3], c[:70], c[:130], c[:65]]
    pairs = [(i, j) for i in range(len(sets)) for j in range(len(sets))]
    w = int((c[0] * c[0]).sum()) - 12000
    for gap in (0, 5000):
        rec = assert_match(Match(gpu_lib, sets, None, pairs, cr.params(gap=gap, transpose=0)), f"gap {gap}")
        for (i, j), r in zip(pairs, rec):                           # H = (min(i, j) + 1) w: the first cell to reach it
            n = min(len(sets[i]), len(sets[j]))
            assert (r["score"], r["a_start"], r["a_end"], r["b_start"], r["b_end"]) == (n * w, 0, n - 1, 0, n - 1)
    p = cr.params(gap=0, transpose=0)
    good = cr.match_batch(sets, sets, pairs, p).tobytes()
    for sw in ("origin_prev", "best_late_i", "strip_diag_row"):
        assert cr.match_batch(sets, sets, pairs, p, frozenset([sw])).tobytes() != good, sw
    # two letters, no gap cost: up and diagonal tie at most cells away from the main diagonal
    abc = cr.alphabet(21, 2)
    two = [cr.letters_song(80 + i, n, abc) for i, n in enumerate((7, 5, 66, 131))]
    pairs2 = [(i, j) for i in range(4) for j in range(4)]
    assert_match(Match(gpu_lib, two, None, pairs2, p), "two letters")
    assert cr.match_batch(two, two, pairs2, p, frozenset(["up_first"])).tobytes() != cr.match_batch(two, two, pairs2, p).tobytes()


@pytest.mark.parametrize("sw", cr.SWITCHES)
def test_the_input_that_would_show_each_mistake(gpu_lib, sw):
    """the named input of each switch (tests/test_cover_reference_host.py shows that the switch changes its record);
    the unit that row_overrun would read follows the song in set a"""
    a, b, p, tail = cr.switch_inputs()[sw]
    set_a = [a] if tail is None else [a, np.asarray(tail).reshape(1, 12)]
    rec = assert_match(Match(gpu_lib, set_a, [b], [(0, 0)], p), sw)
    assert rec["status"][0] == 0


def test_a_short_song_between_two_copies_of_a_longer_one(gpu_lib):
    """the unit behind the short song is the one that would extend its alignment: a row or a column that ran over the
    song's end would raise the score and move the end"""
    abc = cr.alphabet(33, 3)
    long_ = cr.letters_song(1, 150, abc)
    short = long_[20:60]
    sets = [long_[60:], short, long_[60:]]                        # behind `short` comes long_[60], its continuation
    other = [long_[:61], long_, short]
    p = cr.params(gap=3000, transpose=0)
    pairs = [(1, 0), (1, 1), (0, 2), (2, 1), (1, 2)]
    bad = cr.match_batch(sets, other, pairs, p, frozenset(["row_overrun"]))
    good = cr.match_batch(sets, other, pairs, p)
    assert bad["score"][0] > good["score"][0] and bad["a_end"][0] == 40 and good["a_end"][0] == 39
    rec = assert_match(Match(gpu_lib, sets, other, pairs, p), "rows")
    assert rec["a_end"][0] == 39 and rec["b_end"][0] == 59
    # the same with the sets swapped: the short song on the columns, its continuation behind it in set b
    swapped = [(j, i) for i, j in pairs]
    rec2 = assert_match(Match(gpu_lib, other, sets, swapped, p), "columns")
    assert rec2["b_end"][0] == 39 and rec2["score"][0] == rec["score"][0]
    assert_match(Match(gpu_lib, sets, None, [(1, 1), (1, 0), (0, 1), (2, 2)], p), "self form")


def test_the_longest_song_both_ways_and_one_unit_more(gpu_lib):
    abc = cr.alphabet(35, 3)
    long_ = cr.letters_song(2, cr.UNITS_MAX + 1, abc)
    side = np.concatenate([cr.letters_song(3, 57, abc), long_[4000:4200]])          # 257 units
    sets = [long_[:cr.UNITS_MAX], side, long_]
    p = cr.params(gap=3000, transpose=0)
    rec = assert_match(Match(gpu_lib, sets, None, [(0, 1), (1, 0), (2, 1), (1, 2), (1, 1), (2, 2)], p), "8192 x 257")
    assert rec["status"].tolist() == [0, 0, cr.TOO_LONG, cr.TOO_LONG, 0, cr.TOO_LONG]
    assert rec["units_a"].tolist() == [8192, 257, 8193, 257, 257, 8193] and rec["a_end"][0] >= 4199 and rec["b_end"][1] >= 4199
    assert not rec["score"][2] and rec["score"][4] == sum(int((q * q).sum()) - 12000 for q in side)


# ---- independence, forms, rejection ----------------------------------------------------------------------------------

def test_a_pairs_record_does_not_depend_on_its_call(gpu_lib):
    import torch
    abc = cr.alphabet(37, 3)
    set_a = [cr.letters_song(100 + i, n, abc) for i, n in enumerate((90, 0, 64, 131, 17, 300))]
    set_b = [cr.letters_song(200 + i, n, abc) for i, n in enumerate((70, 129, 1, 65))]
    p = cr.params(gap=2000)
    pairs = [(i, j) for i in range(6) for j in range(4)]
    rec = assert_match(Match(gpu_lib, set_a, set_b, pairs, p), "all")
    at = {pr: n for n, pr in enumerate(pairs)}
    assert_match(Match(gpu_lib, set_a, set_b, pairs[::-1], p), "reversed")
    assert Match(gpu_lib, set_a, set_b, pairs[::-1], p).read()[::-1].tobytes() == rec.tobytes()
    for pr in ((3, 1), (5, 0), (1, 2), (2, 3)):
        alone = Match(gpu_lib, set_a, set_b, [pr], p).read()
        assert alone[0].tobytes() == rec[at[pr]].tobytes(), pr
        only = Match(gpu_lib, [set_a[pr[0]]], [set_b[pr[1]]], [(0, 0)], p).read()
        assert only[0].tobytes() == rec[at[pr]].tobytes(), pr
    with bliss_amd.Context(0) as ctx:
        assert Match(gpu_lib, set_a, set_b, pairs, p, ctx=ctx).read().tobytes() == rec.tobytes()
    cp = cover.params(gap=2000)
    h = cover.match_host(cr.cat(set_a), [len(x) for x in set_a], pairs, cp, cr.cat(set_b), [len(x) for x in set_b])
    assert h.tobytes() == rec.tobytes()
    d = cover.match_device(to_device(cr.cat(set_a)), [len(x) for x in set_a], np.array(pairs, np.int32), cp,
                           to_device(cr.cat(set_b)), [len(x) for x in set_b])
    torch.cuda.synchronize()
    assert cover.match_to_numpy(d.cpu().numpy()).tobytes() == rec.tobytes()
    # the self form: one set given twice reads what the cross form reads from two copies
    both = set_a + set_b
    cross = [(i, 6 + j) for i, j in pairs]
    self_rec = assert_match(Match(gpu_lib, both, None, cross, p), "self")
    assert self_rec.tobytes() == rec.tobytes()
    hs = cover.match_host(cr.cat(both), [len(x) for x in both], cross, cp)
    assert hs.tobytes() == rec.tobytes()


def test_pair_indices_outside_their_sets(gpu_lib):
    abc = cr.alphabet(39, 3)
    sets = [cr.letters_song(1, 40, abc), cr.letters_song(2, 30, abc)]
    pairs = [(-1, 0), (0, -1), (2, 0), (0, 2), (1 << 30, 1), (0, 1), (-(1 << 31), -(1 << 31))]
    rec = assert_match(Match(gpu_lib, sets, None, pairs, cr.params()), "bad indices")
    assert rec["status"].tolist() == [cr.BAD_INDEX] * 5 + [0, cr.BAD_INDEX]
    assert not any(rec[k][n] for n in (0, 1, 2, 3, 4, 6) for k in COVER_MATCH_DTYPE.names if k != "status")


def test_rejected_arguments_write_nothing(gpu_lib):
    abc = cr.alphabet(41, 3)
    sets = [cr.letters_song(1, 40, abc), cr.letters_song(2, 30, abc)]
    good = cr.params()
    shifted = lambda name, by: (lambda m: C.c_void_p(getattr(m, name).data_ptr() + by))
    bad = [dict(a=None), dict(ca=None), dict(b=None), dict(cb=None), dict(pairs=None), dict(p=None), dict(rec=None),
           dict(na=0), dict(nb=-1), dict(n=0), dict(n=-1), dict(ca=(C.c_int32 * 2)(40, -1)),
           dict(cb=(C.c_int32 * 2)(1 << 20, 30)), dict(a=shifted("ua", 8)), dict(b=shifted("ub", 4)),
           dict(pairs=shifted("dp", 4)), dict(rec=shifted("rec", 2))]
    for kw in bad:
        m = Match(gpu_lib, sets, None, [(0, 1), (1, 0)], good, bad=kw)
        assert m.rc == UNEXPECTED and m.untouched(), list(kw)
    for kw in (dict(thr=0), dict(thr=16129), dict(gap=-1), dict(gap=(1 << 20) + 1), dict(transpose=-2),
               dict(transpose=12), dict(reserved=1), dict(reserved=-1)):
        m = Match(gpu_lib, sets, None, [(0, 1)], dict(good, **kw))
        assert m.rc == UNEXPECTED and m.untouched(), kw
    import torch
    frames, out = to_device(fr.random_frames(1, 12).astype(np.uint64)), filled(16 * 5)
    for counts, n, P, n_units in (((6, 5), 2, 2, 4), ((6, 5), 2, 0, 5), ((6, 5), 2, 17, 5), ((6, -1), 2, 2, 3), ((6, 5), 0, 2, 5)):
        rc = gpu_lib.bl_amd_cover_units_device(C.c_void_p(frames.data_ptr()), (C.c_int32 * 2)(*counts), n, P,
                                               C.c_void_p(out.data_ptr()), n_units, None)
        torch.cuda.synchronize()
        assert rc == UNEXPECTED and bool((out == SENTINEL).all())
    assert_match(Match(gpu_lib, sets, None, [(0, 1), (1, 0)], good), "after the rejections")
    assert_match(Match(gpu_lib, sets, None, [(0, 1)], cr.params(thr=16128, gap=1 << 20, transpose=11)), "upper ends")
    assert_match(Match(gpu_lib, sets, None, [(0, 0)], cr.params(thr=1, gap=0, transpose=0)), "lower ends")


def test_profile_ms_names_both_kernels(gpu_lib):
    n = C.c_int(-1)
    names = (b"cover_profile", b"cover_align")
    assert gpu_lib.bl_amd_cover_profile_ms(b"nothing", C.byref(n)) == -1.0 and n.value == 0
    abc = cr.alphabet(43, 3)
    gpu_lib.bl_amd_profile(1)
    try:
        for name in names:
            gpu_lib.bl_amd_cover_profile_ms(name, C.byref(n))
        Match(gpu_lib, [cr.letters_song(1, 100, abc)], None, [(0, 0)], cr.params()).read()
        for name in names:
            ms = gpu_lib.bl_amd_cover_profile_ms(name, C.byref(n))
            assert n.value == 1 and 0.0 < ms < 1000.0, name
            assert gpu_lib.bl_amd_cover_profile_ms(name, C.byref(n)) == 0.0 and n.value == 0
    finally:
        gpu_lib.bl_amd_profile(0)


# ---- end to end ------------------------------------------------------------------------------------------------------

def test_from_pcm_through_the_chroma_call(gpu_lib):
    """a melody of the chroma tests (tests/fprint_reference.py's, seed 1, 20 s), the same three semitones up and 12 %
    slower, and an unrelated one (seed 2).  The CPU reference over the chroma reference's frames (chroma_reference.
    chromagram) reads 0.850 for the version and 0.056 / 0.063 for the two unrelated pairs at pool 1 (0.704 against 0.046 /
    0.065 at pool 2); the bound is midway between the two readings at pool 1, (0.850 + 0.063) / 2 = 0.456."""
    import bliss_amd.chroma as ch
    from tests import fprint_reference as fpr
    assert np.array_equal(cr.melody(1, seconds=3.0), fpr.melody(1, seconds=3.0))
    pcm = [cr.melody(1), cr.melody(1, semitones=3, slow=1.12), cr.melody(2)]
    units, counts = cover.from_pcm(pcm, 1)
    songs, frames = ch.chroma_batch_host(pcm, 1, frames=True)
    T = [int(t) for t in songs["frames"]]
    assert counts == T == [214, 240, 214]
    at = np.cumsum([0] + T)
    q = [fr.units(frames["x"][at[i]:at[i + 1]].astype(np.int64), 1) for i in range(3)]
    assert units.tobytes() == cr.cat(q).tobytes()
    pairs = [(0, 1), (0, 2), (1, 2)]
    rec = cover.match_host(units, counts, pairs)
    assert rec.tobytes() == cr.match_batch(q, q, pairs, cr.params()).tobytes()
    s = cover.score(rec)
    assert s[0] > 0.456 > max(s[1], s[2]) and rec["transpose"][0] == 3 and rec["status"].tolist() == [0, 0, 0]
    assert abs(cover.tempo_ratio(rec)[0] - 1.12) < 0.03
    assert cover.seconds(int(rec["a_end"][0])) > 18.0
