"""tests/tbeats_reference.py against itself, without a device: the hop-by-hop definition equals the run-by-run evaluation,
every mistake the reference can make changes its named input, a constant track is tests/beat_reference.py's tracker, the
worked examples of the README give the figures printed there, and the header's bounds hold where they are tightest."""
import numpy as np
import pytest

from tests import beat_reference as br
from tests import tbeats_reference as tb
from tests import tgram_reference as tr


@pytest.mark.parametrize("name", sorted(tb.corpus()))
def test_the_definition_equals_the_evaluation_by_runs(name):
    o, lags, anchor, p = tb.corpus()[name]
    a, b = tb.track(o, lags, anchor, p), tb.track_runs(o, lags, anchor, p)
    assert tb.same(a, b)
    assert a["rec"]["hops"] == o.size and a["rec"]["frames"] == len(lags) and a["rec"]["reserved"] == 0


def test_the_named_inputs_take_both_evaluations():
    for sw, (o, lags, anchor, p) in tb.named().items():
        assert tb.same(tb.track(o, lags, anchor, p), tb.track_runs(o, lags, anchor, p)), sw


@pytest.mark.parametrize("switch", tb.SWITCHES)
def test_every_switch_changes_its_named_input(switch):
    assert set(tb.named()) == set(tb.SWITCHES)
    o, lags, anchor, p = tb.named()[switch]
    assert not tb.same(tb.song(o, lags, anchor, p), tb.song(o, lags, anchor, p, **{switch: True}))


@pytest.mark.parametrize("L", [2, 7, 64, 255, 510])
def test_a_constant_track_is_the_fixed_tracker(L):
    """every valid frame at L, invalid frames between them, an anchor without `fold` and a fold that does not apply"""
    o = tb.noise(1300, L)
    want = br.track(o, L, 128)
    for lags, anchor, p in (([L] * 9, None, tb.params(64, 10, 128)), ([0, L, 0, 511, L, 0], None, tb.params(128, 300, 128)),
                            ([L], 2 * L, tb.params(16, 0, 128)), ([L, 0, L], L, tb.params(256, 7, 128, 1))):
        for got in (tb.track(o, lags, anchor, p), tb.track_runs(o, lags, anchor, p)):
            for k in ("flags", "links", "scores"):
                assert np.array_equal(got[k], want[k]), (L, k)
            for k in ("score", "pen_scale", "n_beats", "first", "last", "status", "hops"):
                assert got["rec"][k] == want["rec"][k], (L, k)
            assert got["rec"]["n_runs"] == 1 and got["rec"]["n_folded"] == 0
            assert got["rec"]["period_first"] == got["rec"]["period_last"] == (L if want["rec"]["n_beats"] else 0)


def test_a_song_without_a_tempo():
    for lags in ([], [0], [1, 511, -3, 0]):
        got = tb.track(tb.noise(50, 1), lags, 40, tb.params(16, 0, 16, 1))
        assert got["rec"] == dict(dict.fromkeys(tb.FIELDS, 0), hops=50, frames=len(lags), status=tb.BL_UNEXPECTED)
        assert not got["flags"].any() and not got["links"].any() and not got["scores"].any() and not got["track"].any()
        assert got["track"].size == len(lags)


def worked():
    o = tr.worked_curve()
    clicks = np.concatenate([np.arange(0, 2000, 40), 2300 + np.arange(0, 2211, 50)])
    return o, clicks


def test_the_worked_tempo_change():
    """clicks of period 40, 300 silent hops, clicks of period 50, under tgram_reference.WORKED with tight 128: the
    tracker that follows the frames finds 102 beats and all 95 clicks, the fixed ones 62 and 56 of them"""
    o, clicks = worked()
    _, frames, _ = tr.song(o, tr.WORKED)
    lags = frames["lag"].tolist()
    assert lags == [40] * 30 + [50] * 25 and clicks.size == 95
    p = tb.from_tgram(tr.WORKED, 128)
    assert (p["seg"], p["origin"]) == (64, 224)
    got = tb.track_runs(o, lags, None, p)
    assert got["rec"]["n_beats"] == 102 and tb.hits(got["flags"], clicks) == 95
    assert (got["rec"]["period_first"], got["rec"]["period_last"], got["rec"]["n_runs"]) == (40, 50, 2)
    assert np.flatnonzero(np.diff(got["track"][tb.frames_of(o.size, 55, p)]))[0] + 1 == 2144
    for L, beats, hit in ((40, 114, 62), (50, 91, 56)):
        fixed = br.track_blocks(o, L, 128)
        assert (fixed["rec"]["n_beats"], tb.hits(fixed["flags"], clicks)) == (beats, hit)
    assert tb.edge_bpm(got["flags"], 22050, 8, False) == 60.0 * 22050 / (128 * 40)
    assert tb.edge_bpm(got["flags"], 22050, 8, True) == 60.0 * 22050 / (128 * 50)


@pytest.mark.parametrize("stride,blocks", [(64, 8), (128, 4)])
def test_an_accelerating_click_track(stride, blocks):
    """139 clicks whose period shrinks from 60 by 0.5 % per click: the following tracker hits every one, the best
    fixed period among 30, 40, 45 and 60 hits 107"""
    o, clicks = tb.accelerating()
    tp = tr.params(stride, blocks)
    _, frames, _ = tr.song(o, tp)
    got = tb.track_runs(o, frames["lag"].tolist(), None, tb.from_tgram(tp, 128))
    assert clicks.size == 139 and tb.hits(got["flags"], clicks) == 139
    assert max(tb.hits(br.track_blocks(o, L, 128)["flags"], clicks) for L in (30, 40, 45, 60)) == 107


def test_the_fill_on_the_gapped_curve():
    _, frames, _ = tr.song(tr.gapped_curve(), tr.SMALL)
    lags = frames["lag"].tolist()
    assert lags == [0] * 3 + [40] * 24 + [20] + [0] * 9 + [90] * 12
    q, n_filled, n_folded = tb.period_track(lags, None, tb.from_tgram(tr.SMALL))
    assert q.tolist() == [40] * 27 + [20] * 6 + [90] * 16 and (n_filled, n_folded) == (12, 0)


def test_the_fold_on_the_octave_curve():
    rec, frames, _ = tr.song(tr.octave_curve(), tr.SMALL)
    lags = frames["lag"].tolist()
    assert sorted(set(lags)) == [42, 88] and rec["lag_median"] == 42
    q, _, n_folded = tb.period_track(lags, rec["lag_median"], tb.from_tgram(tr.SMALL, fold=1))
    assert sorted(set(q.tolist())) == [42, 44] and n_folded == lags.count(88)
    assert [int(x) for x in q[np.sort(np.unique(q, return_index=True)[1])]] == [42, 44]
    assert tb.period_track(lags, rec["lag_median"], tb.from_tgram(tr.SMALL))[0].tolist() == lags      # fold off
    assert tb.period_track(lags, 511, tb.from_tgram(tr.SMALL, fold=1))[0].tolist() == lags            # no anchor
    assert tb.fold_one(510, 300) == 255 and tb.fold_one(300, 500) == 300 and tb.fold_one(3, 6) == 6
    assert tb.fold_one(2, 6) == 4 and tb.fold_one(3, 2) == 3 and tb.fold_one(56, 42) == 56 and tb.fold_one(57, 42) == 28


def test_the_bounds_at_full_scale():
    """a 510 -> 2 -> 510 track over onsets of 2^18 - 1 at tight 4096: pen < 2^26 and C < 2^42"""
    W = 4096 * tb.OMAX
    assert W < 1 << 30
    for L in (2, 510):
        lo, hi = br.bounds(L)
        assert int(br.penalties(L, W, lo, hi).max()) < 1 << 26 and hi - lo <= 765
    o, lags, anchor, p = tb.corpus()["full_scale"]
    assert p["tight"] == 4096 and int(o.min()) == tb.OMAX
    got = tb.track_runs(o, lags, anchor, p)
    assert got["track"].tolist() == [510, 510, 2, 2, 510, 510] and got["rec"]["n_runs"] == 3
    assert 0 <= int(got["scores"].min()) and int(got["scores"].max()) < 1 << 42 and int(got["links"].max()) <= 1020
    assert got["rec"]["pen_scale"] == W
