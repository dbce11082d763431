"""tests/chords_reference.py against itself, without a device: the Viterbi equals a brute-force search over all label
paths under the tie rule the header's definitions amount to, every mistake switch changes the result on its named input
(which tests/test_gpu_chords.py runs on the device), and the definition does what it is for: it labels three synthetic
progressions, silence and noise correctly where picking the best template per unit does not."""
import numpy as np
import pytest

from tests import chords_reference as cr


def test_viterbi_is_the_brute_force_maximum_with_the_smallest_reversed_path():
    """Among the paths of the largest score the definition picks the one whose reversed label sequence is the
    lexicographically smallest: L_{U-1} is the smallest end of a best path, and B_t[L_t] the smallest label before the
    suffix already fixed.  Alphabets and tables on which many paths tie."""
    zero = np.zeros((25, 25), dtype=np.int64)
    two = (np.arange(625).reshape(25, 25) % 2) * 30                 # many equal costs
    cases = [(cr.letters_song(s, U, cr.alphabet(s)), none, cost)
             for s, U in ((1, 1), (2, 2), (3, 3), (4, 3), (5, 2))
             for none, cost in ((150, cr.costs()), (0, zero), (381, two), (90, cr.asymmetric_cost(s)))]
    cases.append((cr.letters_song(6, 4, cr.alphabet(6)), 120, cr.costs(40, 20)))
    ties = 0
    for q, none, cost in cases:
        E = cr.emissions(q, none)
        L, score, _ = cr.viterbi(E, cost)
        want, want_score = cr.brute_force(E, cost)
        assert (L.tolist(), score) == (want, want_score), (q.tolist(), none)
        late, _, _ = cr.viterbi(E, cost, frozenset(["pred_tie_last", "end_tie_last"]))
        ties += late.tolist() != want
    assert ties >= len(cases) // 4                                  # the ties are there: the other rule gives other paths


@pytest.mark.parametrize("sw", cr.SWITCHES)
def test_every_switch_changes_its_named_input(sw):
    songs, none, cost = cr.switch_inputs()[sw]
    good = cr.chords_batch(songs, none, cost)
    bad = cr.chords_batch(songs, none, cost, frozenset([sw]))
    assert any(g.tobytes() != b.tobytes() for g, b in zip(good, bad)), sw
    assert len(cr.SWITCHES) == 14 and set(cr.switch_inputs()) == set(cr.SWITCHES)


def test_records_of_a_batch_by_hand():
    C, G = cr.triad_unit(0), cr.triad_unit(7)
    songs = [np.stack([C, C, G, G, G]), np.zeros((0, 12), np.int64), np.zeros((2, 12), np.int64)]
    rec, labels, hist = cr.chords_batch(songs, 150, cr.costs())
    # C C G G G: 5 x 300 less one change between chords that share one class (G): 60 - 15
    assert rec[0].tolist() == (5, 0, 1500 - 45, 1, 7, 3, 0, 0) and labels[:5].tolist() == [0, 0, 7, 7, 7]
    assert rec[1].tolist() == (0, cr.EMPTY, 0, 0, -1, 0, 0, 0)
    assert rec[2].tolist() == (2, 0, 300, 0, 24, 2, 2, 0) and labels[5:].tolist() == [24, 24]
    assert hist[0, 0] == 2 and hist[0, 7] == 3 and hist[1].sum() == 0 and hist[2, 24] == 2
    assert cr.segments(labels) == ([0, 2, 5], [0, 7, 24]) and cr.segments([]) == ([], [])
    assert [cr.name(k) for k in (0, 1, 11, 12, 21, 23, 24, 25, -1)] == ["C", "C#", "B", "Cm", "Am", "Bm", "N", "", ""]
    c = cr.costs(60, 15)
    assert (c[0, 21], c[0, 5], c[0, 6], c[0, 24], c[24, 3], c[4, 4]) == (30, 45, 60, 60, 60, 0)
    assert cr.emissions(np.full((1, 12), 127), 381).max() == cr.EMISSION_MAX


@pytest.mark.parametrize("tonic,minor", cr.PROGRESSIONS)
@pytest.mark.parametrize("pool", [1, 2])
def test_progressions_decode_to_the_chords_played_and_per_unit_picking_does_not(tonic, minor, pool):
    """a condition on the definition, not a tolerance: every unit whose frames lie wholly inside one chord gets that
    chord, every unit wholly inside the silence or the noise gets N; with all costs 0 (the best template of each unit)
    some unit is mislabelled"""
    q = cr.progression_units(tonic, minor, pool)
    want = cr.progression_want(tonic, minor, pool, len(q))
    assert sum(w >= 0 for w in want) >= len(q) * 2 // 3 and {w for w in want if w >= 0} >= {cr.NONE}
    rec, labels, _ = cr.chords_batch([q], 150, cr.costs(60, 15))
    assert all(w < 0 or int(l) == w for l, w in zip(labels, want)), ([cr.name(int(l)) for l in labels], want)
    runs = [cr.name(c) for c in cr.segments([l for l, w in zip(labels, want) if w >= 0 and w != cr.NONE])[1]]
    root = lambda d: cr.name((12 if minor else 0) + (tonic + d) % 12)
    assert runs == [root(0), root(5), root(7), root(0)]
    _, raw, _ = cr.chords_batch([q], 150, np.zeros((25, 25), dtype=np.int64))
    assert any(w >= 0 and int(l) != w for l, w in zip(raw, want))
    assert rec["none_units"][0] >= sum(w == cr.NONE for w in want)
