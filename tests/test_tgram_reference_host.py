"""tests/tgram_reference.py without a device: every mistake it can make on purpose changes its named input (which
tests/test_gpu_tgram.py runs), a single frame with W = T is the tempo call's stages 7 and 8, and the worked tempo-change
case of the header gives the figures the documents quote."""
import numpy as np
import pytest

from tests import rhythm_reference as rr
from tests import tgram_reference as tr


def _same(a, b):
    return a[0] == b[0] and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("switch", sorted(tr.named()))
def test_every_switch_changes_its_named_input(switch):
    o, p, value = tr.named()[switch]
    right, wrong = tr.song(o, p), tr.song(o, p, **{switch: value})
    assert not _same(right, wrong), switch
    assert _same(right, tr.song(o, p))


def test_there_are_at_least_twelve_switches():
    assert len(tr.named()) >= 12


def test_near_by_hand():
    assert tr.near(40, 40, 0, 0) and not tr.near(41, 40, 0, 0) and tr.near(42, 40, 50, 0) and not tr.near(43, 40, 50, 0)
    assert tr.near(38, 40, 50, 0) and not tr.near(37, 40, 50, 0)
    assert not tr.near(80, 40, 60, 0) and tr.near(80, 40, 60, 1) and tr.near(40, 80, 60, 1)
    assert tr.near(84, 40, 60, 1) and not tr.near(85, 40, 60, 1)        # 1000 |L - 2 M| <= tol 2 M = 4800
    assert not tr.near(84, 40, 60, 1, asym_octave=True) and tr.near(82, 40, 60, 1, asym_octave=True)
    assert tr.near(21, 40, 60, 1) and not tr.near(22, 44, 0, 0) and tr.near(22, 44, 0, 1)
    assert tr.near(60, 40, 60, 0, tol_percent=True) and not tr.near(60, 40, 60, 0)


def test_frames_count_by_hand():
    p = tr.params(stride=16, blocks=1)
    assert [tr.frames_count(h, p) for h in (1, 511, 526, 527, 542, 543)] == [0, 0, 0, 1, 1, 2]
    q = tr.params(stride=1024, blocks=16)
    assert tr.frames_count(511 + 16384 - 1, q) == 0 and tr.frames_count(511 + 16384, q) == 1
    assert tr.hops_for(1, p) == 527 and tr.frames_count(tr.hops_for(7, q, extra=1023), q) == 7


@pytest.mark.parametrize("stride,blocks", [(16, 5), (48, 2), (1024, 1)])
def test_a_single_frame_over_all_terms_is_the_tempo_call(stride, blocks):
    p = tr.params(stride=stride, blocks=blocks, lag_min=1, lag_max=510)
    o = tr.noise(tr.hops_for(1, p), 30 + blocks)        # W = T exactly
    rec, frames, rows = tr.song(o, p, gram=True)
    want, R = rr.record_from_onsets(o, 1, 510)
    assert rec["frames"] == 1 and [int(x) for x in rows[0]] == R
    assert {k: int(frames[0][k]) for k in frames.dtype.names} == {k: want[k] for k in frames.dtype.names}
    assert tr.bpm(frames[0]) == rr.bpm(want)


def test_the_worked_tempo_change():
    o = tr.worked_curve()
    assert o.size == 4511 and int(o[2000:2300].max()) == 0
    rec, frames, _ = tr.song(o, tr.WORKED)
    assert rec["frames"] == 55 and [int(x) for x in frames["lag"]] == [40] * 30 + [50] * 25
    assert rec == dict(hops=4511, frames=55, n_tempo=55, status=0, frame_first=0, frame_last=54, lag_first=40,
                       lag_last=50, lag_low=40, lag_high=50, lag_median=40, n_near=30, n_jumps=1, reserved=0)
    assert tr.steadiness(rec) == 30 / 55
    assert tr.seconds(0, tr.WORKED) == 128 * 256 / 22050 and tr.seconds(54, tr.WORKED) == 128 * (54 * 64 + 256) / 22050


def test_short_and_silent_songs():
    p = tr.TINY
    rec, frames, rows = tr.song(tr.noise(tr.hops_for(1, p) - 1, 3), p, gram=True)
    assert rec == dict(dict.fromkeys(tr.SONG_FIELDS, 0), hops=tr.hops_for(1, p) - 1, status=tr.BL_UNEXPECTED)
    assert frames.size == 0 and rows.shape == (0, 512)
    rec, frames, _ = tr.song(np.zeros(tr.hops_for(4, p), dtype=np.int64), p)
    assert rec == dict(dict.fromkeys(tr.SONG_FIELDS, 0), hops=tr.hops_for(4, p), frames=4, frame_first=-1, frame_last=-1)
    assert not frames.view(np.uint8).any()


def test_song_record_on_given_lags():
    p = tr.params(tol=60, octaves=1)
    rec = tr.song_record(9999, [0, 40, 0, 0, 41, 80, 90, 0, 40, 0], p)
    assert (rec["n_tempo"], rec["frame_first"], rec["frame_last"], rec["lag_first"], rec["lag_last"]) == (5, 1, 8, 40, 40)
    assert (rec["lag_low"], rec["lag_high"], rec["lag_median"]) == (40, 90, 41)
    assert rec["n_near"] == 4          # 40, 41, 80 (twice 41 within 60 per mille), 40; not 90
    assert rec["n_jumps"] == 2         # 80 -> 90 and 90 -> 40; 40 -> 41 and 41 -> 80 are near
    assert tr.song_record(9999, [0, 40, 0, 0, 90], p, silent_breaks=True)["n_jumps"] == 0
    assert tr.song_record(9999, [40, 50], p)["lag_median"] == 40
    assert tr.song_record(9999, [40, 50], p, upper_median=True)["lag_median"] == 50
