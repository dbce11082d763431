"""The reference of the song structure (tests/form_reference.py) on the CPU: its vectorised forms agree with the
definition written out in Python integers, every switch that makes a kernel's plausible mistake changes the result on a
named input (the inputs the GPU tests use), and the correct reference satisfies the two claims of the issue on seeded
songs: the thumbnail of an A-B-A song and the boundaries of homogeneous sections."""
import numpy as np
import pytest

from tests import form_reference as fr

NONE = frozenset()


def sw(*names):
    assert all(n in fr.SWITCHES for n in names)
    return frozenset(names)


def test_there_are_at_least_ten_switches_and_they_are_distinct():
    assert len(fr.SWITCHES) >= 10 and len(set(fr.SWITCHES)) == len(fr.SWITCHES)


def test_vectorised_forms_agree_with_the_definition():
    X = fr.random_frames(1, 61, fr.X_MAX)
    X[6:9] = 0
    for P in (1, 3, 16):
        q = fr.units(X, P)
        assert q.shape == (61 // P, 12) and 0 <= q.min() and q.max() <= 127
        for u in range(q.shape[0]):
            assert q[u].tolist() == fr.unit_slow(X, u, P)
    q = fr.units(fr.random_frames(2, 40), 1)
    M, lag = 6, 4
    th, rep = fr.thumb(q, M, lag)
    F = {(u, l): fr.f_slow(q, u, l, M) for l in range(lag, 40 - M + 1) for u in range(0, 40 - M - l + 1)}
    best = max(F.items(), key=lambda kv: (kv[1], -kv[0][1], -kv[0][0]))
    assert (th["thumb_start"], th["thumb_lag"], th["thumb_score"]) == (best[0][0], best[0][1], best[1])
    assert th["thumb_self"] == sum(fr.sim(q, best[0][0] + j, best[0][0] + j) for j in range(M))
    for u in range(40):
        row = [(F[u, l], -l) for l in range(lag, 40 - M + 1) if (u, l) in F]
        want = [max(row)[0], -max(row)[1]] if row and max(row)[0] > 0 else [0, 0]
        assert rep[u].tolist() == want, u
    for L in (1, 5):
        assert fr.novelty(q, L) == [fr.novelty_slow(q, u, L) for u in range(40)]
    rec, units, rep_b, nov, flags = fr.form_batch(fr.random_frames(2, 40), [40], fr.params(seg=M, min_lag=lag, nov=5))
    assert units.shape == (40, 16) and not units[:, 12:].any() and rep_b.tolist() == rep.tolist()
    assert rec["units"][0] == 40 and rec["boundaries"][0] == int(flags.sum()) and rec["nov_max"][0] == int(nov.max())


def test_unit_switches_change_named_frames():
    X = fr.random_frames(3, 50, fr.X_MAX)                      # T = 3 * 16 + 2
    assert fr.units(X, 3, sw("keep_partial")).shape[0] == 17 and fr.units(X, 3).shape[0] == 16
    for name in ("norm_max", "round_div"):
        assert not np.array_equal(fr.units(X, 1, sw(name)), fr.units(X, 1)), name
    assert fr.units(fr.shift_frame(), 1)[0, :2].tolist() == [126, 0]
    assert fr.units(fr.shift_frame(), 1, sw("shift19"))[0, :2].tolist() == [127, 0]
    one = np.zeros((1, 12), np.int64)
    one[0, 7] = 12345                                          # q = 127 in its class whatever the norm
    assert fr.units(one, 1)[0].tolist() == [0] * 7 + [127] + [0] * 4
    small = fr.random_frames(4, 20, 1 << 19)                   # s = 0 either way
    assert np.array_equal(fr.units(small, 1, sw("shift19")), fr.units(small, 1))


def test_thumbnail_switches_change_named_songs():
    M, lag = 12, 7
    equal = fr.units(np.repeat(fr.random_frames(5, 1), 90, axis=0), 1)
    th, rep = fr.thumb(equal, M, lag)
    assert (th["thumb_lag"], th["thumb_start"]) == (lag, 0) and th["thumb_score"] == th["thumb_self"]
    assert fr.thumb(equal, M, lag, sw("lag_start"))[0]["thumb_lag"] == lag + 1
    assert fr.thumb(equal, M, lag, sw("tie_lag"))[0]["thumb_lag"] == 90 - M
    assert fr.thumb(equal, M, lag, sw("tie_start"))[0]["thumb_start"] == 90 - M - lag
    one = fr.units(fr.random_frames(6, M + lag), 1)            # one candidate: l = minlag = U - M
    assert fr.thumb(one, M, lag)[0]["status"] == 0 and fr.thumb(one, M, lag, sw("lag_end"))[0]["status"] == fr.NO_THUMB
    assert fr.thumb(one[:-1], M, lag)[0]["status"] == fr.NO_THUMB
    assert fr.thumb(np.zeros((60, 12), np.int64), M, lag)[0]["status"] == fr.NO_THUMB
    rnd = fr.units(fr.random_frames(7, 80), 1)
    good, bad = fr.thumb(rnd, M, lag)[1], fr.thumb(rnd, M, lag, sw("window_past"))[1]
    assert not good[80 - M - lag + 1:].any() and bad[80 - M - lag + 1:80 - M + 1].all()
    # a planted repeat at the last lag is found, and with lag_end it is not
    x = fr.random_frames(8, 100, 1 << 34)
    x[100 - M:] = x[:M]
    q = fr.units(x, 1)
    assert fr.thumb(q, M, lag)[0]["thumb_lag"] == 100 - M and fr.thumb(q, M, lag, sw("lag_end"))[0]["thumb_lag"] != 100 - M


def test_a_unit_read_across_a_song_edge_shows():
    p = fr.params(seg=16, min_lag=16, nov=4)
    short = fr.random_frames(84, 40, 1 << 35)
    other = np.concatenate([short[24:], fr.random_frames(83, 284, 1 << 35)])
    X = np.concatenate([other, short, other])
    good, bad = fr.form_batch(X, [300, 40, 300], p)[0], fr.form_batch(X, [300, 40, 300], p, sw("cross_edge"))[0]
    assert bad["thumb_score"][1] > good["thumb_score"][1] and bad["thumb_score"][1] == bad["thumb_self"][1]
    assert (bad["thumb_start"][1], bad["thumb_lag"][1]) == (24, 16)
    alone = fr.form_batch(short, [40], p)[0]
    assert alone[0].tobytes() == good[1].tobytes()


def test_novelty_switches_change_named_songs():
    q = fr.units(fr.random_frames(9, 60), 1)
    for name in ("weights_lm", "both_from_u"):
        assert fr.novelty(q, 6, sw(name)) != fr.novelty(q, 6), name
    assert not any(fr.novelty(q[:11], 6)) and [u for u, n in enumerate(fr.novelty(q[:12], 6)) if n] == [6]
    a, b = fr.random_frames(110, 1, 1 << 33), fr.random_frames(111, 1, 1 << 33)
    plateau = fr.units(np.concatenate([np.repeat(a, 5, axis=0), b, np.repeat(a, 5, axis=0)]), 1)
    N = fr.novelty(plateau, 1)
    assert N[5] == N[6] > 0 and not any(N[:5]) and not any(N[7:])
    assert np.flatnonzero(fr.boundaries(N, 1, 1, 4)[0]).tolist() == [5]
    assert np.flatnonzero(fr.boundaries(N, 1, 1, 4, sw("peak_le"))[0]).tolist() == [5, 6]
    # two songs, the second with the weaker changes: against the batch's maximum it keeps no boundary
    strong = fr.section_song(3, hold=None)
    weak = strong.copy()
    weak[:, :] = np.where(weak >= 1 << 30, (weak >> 12) + (1 << 22), weak + (1 << 22))
    p = fr.params(seg=8, min_lag=8, nov=8, peak_num=1, peak_den=2)
    X = np.concatenate([strong, weak])
    good, bad = fr.form_batch(X, [278, 278], p)[0], fr.form_batch(X, [278, 278], p, sw("batch_max"))[0]
    assert good["nov_max"][1] * 2 < good["nov_max"][0]
    assert good["boundaries"][1] >= 1 and bad["boundaries"][1] == 0 and bad["boundaries"][0] == good["boundaries"][0]


def test_thresholds_at_both_ends():
    N = fr.novelty(fr.units(fr.random_frames(10, 200), 1), 6)
    every = fr.boundaries(N, 6, 0, 1)[0]
    top, nmax, at = fr.boundaries(N, 6, 256, 256)
    assert every.sum() > top.sum() >= 1 and top[at] == 1 and N[at] == nmax and N.index(nmax) == at
    assert all(N[u] == nmax for u in np.flatnonzero(top))


def test_a_song_that_is_too_long_has_a_status_and_zero_fields():
    x = fr.random_frames(11, fr.UNITS_MAX + 1)
    rec, units, rep, nov, flags = fr.form_batch(x, [x.shape[0]], fr.params(seg=1024, min_lag=fr.UNITS_MAX, nov=64))
    assert rec["status"][0] == fr.NO_THUMB | fr.TOO_LONG and rec["units"][0] == fr.UNITS_MAX + 1
    assert all(int(rec[k][0]) == 0 for k in fr.FORM_DTYPE.names if k not in ("units", "status"))
    assert units.any() and not rep.any() and not nov.any() and not flags.any()


@pytest.mark.parametrize("seed", [3, 2])
def test_the_thumbnail_of_an_aba_song(seed):
    """intro 40 / A 64 / B 80 / A 64 / outro 30 frames: at P = 1, 2, 3 with M = minlag = 48 / P the lag is exactly
    144 / P and the start lies in [40 / P, 56 / P]"""
    x = fr.section_song(seed)
    assert x.shape == (278, 12) and x.max() < 1 << 32
    for P in (1, 2, 3):
        th, _ = fr.thumb(fr.units(x, P), 48 // P, 48 // P)
        assert th["thumb_lag"] == 144 // P and 40 / P <= th["thumb_start"] <= 56 / P, (P, th)


@pytest.mark.parametrize("seed", [3, 2])
def test_the_boundaries_of_homogeneous_sections(seed):
    x = fr.section_song(seed, hold=None)
    for P, L, want in ((1, 16, [40, 104, 184, 248]), (1, 8, [40, 104, 184, 248]), (2, 8, [20, 52, 92, 124])):
        q = fr.units(x, P)
        flags, nmax, at = fr.boundaries(fr.novelty(q, L), L, 1, 4)
        assert np.flatnonzero(flags).tolist() == want and at in want, (P, L)
        assert fr.sections(flags, q.shape[0]) == list(zip([0] + want, want + [278 // P]))
