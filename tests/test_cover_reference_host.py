"""tests/cover_reference.py against itself, without a device: the anti-diagonal alignment equals the per-cell one on
small inputs where ties are the rule, every switch changes the record of a named input (so the GPU tests' inputs, which
are built the same way, would catch that mistake), and the definition separates synthetic chord songs from their
versions.

The synthetic figures, measured here with chord_song() at thr 12000 and gap 4000 (bl_amd_cover_score of the reference's
records): versions (three semitones up; 25 % slower; 20 % faster and five semitones up; noise of 2^29 under chords of
2^30 .. 2^32; 20 frames of foreign lead-in) read 0.711 .. 0.949 at pool 1 and 0.593 .. 0.948 at pool 2, unrelated songs
0.019 .. 0.022 at pool 1 and 0.022 .. 0.023 at pool 2.  The bound is midway between the two groups' extremes:
(0.593 + 0.023) / 2 = 0.308.  The transposition is found in every case.  This is evidence on synthetic material; nothing
is tuned on recorded music."""
import numpy as np
import pytest

from tests import cover_reference as cr

BOUND = 0.308        # midway between the weakest version (0.593) and the strongest unrelated song (0.023)


def test_params_and_switch_names():
    assert cr.params() == dict(thr=12000, gap=4000, transpose=-1, reserved=0)
    assert len(set(cr.SWITCHES)) == len(cr.SWITCHES) == 14 and cr.COVER_DTYPE.itemsize == 40


def test_antidiagonals_equal_the_definition_on_small_alphabets():
    """300 pairs of 1 .. 19 units from alphabets of 2 to 4 letters: most cells tie with a neighbour"""
    rng = np.random.default_rng(1)
    matched = 0
    for n in range(300):
        abc = cr.alphabet(100 + n % 7, int(rng.integers(2, 5)))
        a = cr.letters_song(2 * n, int(rng.integers(1, 20)), abc)
        b = cr.letters_song(2 * n + 1, int(rng.integers(1, 20)), abc)
        thr, gap = int(rng.choice([9000, 12000, 15000, 16000][:3 + n % 2])), int(rng.choice([0, 100, 4000]))
        r = int(rng.integers(0, 12)) if n % 4 == 3 else cr.pick_r(a, b)
        want = cr.align_slow(a, b, thr, gap, r)
        assert cr.align(a, b, thr, gap, r) == want, (n, thr, gap, r)
        matched += want is not None
    assert matched > 200
    a, b = cr.lettered(10, 3, 79, 85)                                # across a strip of 64, both ways round
    p = cr.params(gap=3000, transpose=0)
    assert cr.match_one(a, b, p) == cr.match_one(a, b, p, slow=True)
    assert cr.match_one(b, a, p) == cr.match_one(b, a, p, slow=True)


def test_batch_statuses_and_the_record_of_a_copy():
    abc = cr.alphabet(3, 3)
    a = cr.letters_song(1, 30, abc)
    sets = [a, np.zeros((0, 12), np.int64), np.zeros((cr.UNITS_MAX + 1, 12), np.int64)]
    rec = cr.match_batch(sets, sets, [(0, 0), (0, 1), (1, 0), (2, 0), (0, 2), (-1, 0), (0, 3)], cr.params())
    assert rec["status"].tolist() == [0, cr.NO_MATCH, cr.NO_MATCH, cr.TOO_LONG, cr.TOO_LONG, cr.BAD_INDEX,
                                      cr.BAD_INDEX]
    assert tuple(rec[0])[1:8] == (0, 29, 0, 29, 0, 30, 30) and rec["units_b"][3] == 30 and rec["units_a"][3] == 8193
    assert rec["score"][0] == sum(int((q * q).sum()) - 12000 for q in a) and not any(tuple(rec[5])[:8])
    assert 0.9 < cr.score(rec[0], 12000) <= 1.0 and np.isnan(cr.score(rec[1], 12000))


@pytest.mark.parametrize("sw", cr.SWITCHES)
def test_every_switch_changes_the_record_of_its_input(sw):
    a, b, p, tail = cr.switch_inputs()[sw]
    good = cr.match_one(a, b, p, tail_a=tail)
    assert good == cr.match_one(a, b, p, slow=True) and good[8] == 0
    assert cr.match_one(a, b, p, frozenset([sw]), tail) != good, sw


def test_named_ties_read_as_the_definition_says():
    ins = cr.switch_inputs()
    a, b, p, _ = ins["best_late_i"]                               # constant songs, 5 x 3: H = (min(i, j) + 1) w
    w = int((a[0] * a[0]).sum()) - p["thr"]
    assert cr.match_one(a, b, p)[:5] == (3 * w, 0, 2, 0, 2)
    assert cr.match_one(a, b, p, frozenset(["best_late_i"]))[:5] == (3 * w, 2, 4, 0, 2)
    a, b, p, _ = ins["best_j_first"]                              # cells (0, 1) and (1, 0) tie: the smaller i wins
    assert cr.match_one(a, b, p)[1:5] == (0, 0, 1, 1)
    assert cr.match_one(a, b, p, frozenset(["best_j_first"]))[1:5] == (1, 1, 0, 0)
    a, b, p, _ = ins["oti_tie_large"]
    assert cr.match_one(a, b, p)[5] == 0 and cr.match_one(a, b, p, frozenset(["oti_tie_large"]))[5] == 11
    a, b, p, _ = ins["profile_short"]
    assert cr.match_one(a, b, p)[5] == 7


def versions_of(X, seed):
    return {"transposed": (cr.transposed(X, 3), 3), "slower": (cr.stretched(X, 1.25), 0),
            "faster, transposed": (cr.transposed(cr.stretched(X, 1 / 1.2), 5), 5), "noisy": (cr.noisy(X, 77 + seed), 0),
            "lead-in": (cr.with_lead_in(X, 500 + seed), 0)}


@pytest.mark.parametrize("pool", [1, 2])
def test_versions_lie_above_and_unrelated_songs_below_the_bound(pool):
    p = cr.params()
    covers, others = [], []
    for seed in range(4):
        X = cr.chord_song(10 + seed)
        qa = cr.units(X, pool)
        for name, (V, semitones) in versions_of(X, seed).items():
            rec = cr.match_batch([qa], [cr.units(V, pool)], [(0, 0)], p)[0]
            assert rec["transpose"] == semitones, (seed, name)
            covers.append(cr.score(rec, p["thr"]))
        for other in range(3):
            rec = cr.match_batch([qa], [cr.units(cr.chord_song(200 + 10 * seed + other), pool)], [(0, 0)], p)[0]
            others.append(cr.score(rec, p["thr"]))
    print(f"pool {pool}: versions {min(covers):.3f} .. {max(covers):.3f}, unrelated {min(others):.3f} .. {max(others):.3f}")
    assert min(covers) > BOUND > max(others)
    lead = cr.match_batch([cr.units(cr.chord_song(10), pool)],
                          [cr.units(cr.with_lead_in(cr.chord_song(10), 500), pool)], [(0, 0)], p)[0]
    assert (lead["a_start"], lead["b_start"]) == (0, 20 // pool)
