"""tests/freq_reference.py is what tests/test_gpu_freq_spectrum.py holds the frequency and statistics kernels to, so it
is proved here, without a device: on the whole song set of the GPU test its spectrum, pushed through its finish, gives
the oracle's `frequency` and `freq_peak` bit for bit, and its integers give the oracle's mean, variance and histogram
integral.  Then the errors a kernel's frame loop can make are made in the reference itself: every one of them changes
at least one bin's bits (or one integer) of EVERY song it applies to — the songs are built so that it does — while
most of them leave `frequency`, `mean`, `variance` and `hist_integral`, the only things the suite compared before,
untouched.  The two counts are printed side by side (pytest -s)."""
import ctypes as C

import numpy as np

from tests import freq_reference as fr
from tests.oracle_py import OrcResult


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def oracle_frequency(oracle, sg):
    r = OrcResult()
    pcm = np.ascontiguousarray(sg["pcm"])
    f = oracle.lib.orc_frequency(pcm.ctypes.data_as(C.POINTER(C.c_int16)), pcm.size, sg["channels"], C.byref(r))
    assert r.n_frames == sg["n_frames"]
    return np.float32(f), np.float32(r.freq_peak)


def test_song_set_reaches_every_edge(oracle):
    songs = fr.song_set(oracle)
    for ch, first in ((2, 5), (1, 10)):
        mine = [s for s in songs if s["channels"] == ch]
        assert sorted(s["n_frames"] for s in mine) == list(range(first, 137))
        extras = [s["extra"] for s in mine]
        assert len(set(extras)) == len(extras) and {0, 1, 7, 512 * ch - 1} <= set(extras)
        assert all(0 <= e < 512 * ch for e in extras)
        for m in (64, 32):
            assert {s["n_frames"] % m for s in mine} == set(range(m))
    assert min(s["pcm"].size for s in songs) == 5120
    assert [s["pcm"].size for s in songs] != sorted((s["pcm"].size for s in songs), reverse=True)   # the batch gets sorted
    assert 27e6 < sum(s["pcm"].nbytes for s in songs) < 30e6
    for s in songs:   # the planted values: the last whole frame, the one before, and what fits behind it
        step = 512 * s["channels"]
        for at in ((s["n_frames"] - 1) * step, (s["n_frames"] - 2) * step):
            assert tuple(s["pcm"][at:at + 6]) == fr.PLANTED
        k = min(6, s["extra"])
        assert tuple(s["pcm"][s["n_frames"] * step:][:k]) == fr.PLANTED[:k]
        inside = np.count_nonzero((s["pcm"] >= -2048) & (s["pcm"] < 2048))
        assert inside > 0.9 * s["pcm"].size
    assert len({s["pcm"].size for s in fr.equal_length_set(oracle)}) == 1


def test_reference_gives_the_oracles_bits_on_the_whole_set(oracle):
    for which in ("main", "equal"):
        songs = fr.song_set(oracle) if which == "main" else fr.equal_length_set(oracle)
        for i, (sg, (ps, total, sumsq, hist)) in enumerate(zip(songs, fr.reference(oracle, which))):
            tag = (which, i, sg["channels"], sg["n_frames"], sg["extra"])
            freq, peak = fr.finish(ps)
            want_freq, want_peak = oracle_frequency(oracle, sg)
            assert np.isfinite(want_freq) and want_peak > 0, tag
            assert bits(freq) == bits(want_freq), (tag, "frequency", float(freq), float(want_freq))
            assert bits(peak) == bits(want_peak), (tag, "freq_peak", float(peak), float(want_peak))
            mean, variance = fr.mean_variance(total, sumsq, sg["pcm"].size)
            assert mean == oracle.mean(sg["pcm"]) and variance == oracle.variance(sg["pcm"], mean), tag
            assert int(hist.sum()) == np.count_nonzero((sg["pcm"] >= -2048) & (sg["pcm"] < 2048)), tag


def trim(pcm):
    nz = np.flatnonzero(pcm)
    return int(nz[0]), int(nz[-1])


def test_histogram_integral_restated(oracle):
    """a sample of the set through the oracle's amplitude analysis: the 4096 raw counts carry its integral's bits"""
    songs, ref = fr.song_set(oracle), fr.reference(oracle)
    for i in range(0, len(songs), 16):
        pcm = songs[i]["pcm"]
        r = OrcResult()
        oracle.lib.orc_amplitude(np.ascontiguousarray(pcm).ctypes.data_as(C.POINTER(C.c_int16)), pcm.size, C.byref(r))
        start, end = trim(pcm)
        assert (start, end) == (r.start, r.end)
        got = fr.hist_integral(ref[i][3], start, end, pcm.size)
        assert np.isfinite(got) and bits(got) == bits(np.float32(r.hist_integral)), (i, float(got), r.hist_integral)


def test_every_kernel_error_shows_in_the_bits_of_every_song(oracle):
    songs, ref = fr.song_set(oracle), fr.reference(oracle)
    spec = {k: [0, 0, 0] for k in ("last frame twice", "last frame dropped", "two frames swapped", "two 8-frame blocks swapped",
                                   "floor in the stereo average", "contracted re*re + im*im")}   # applies, raw, frequency
    stat = {k: [0, 0, 0, 0] for k in ("statistics: last frame twice", "statistics: last frame dropped")}
    for i, (sg, (ps, total, sumsq, hist)) in enumerate(zip(songs, ref)):
        nf, ch, pcm = sg["n_frames"], sg["channels"], sg["pcm"]
        tag = (i, ch, nf, sg["extra"])
        x = fr.transform(oracle, fr.windowed_frames(pcm, ch))
        power = fr.frame_power(x)
        assert np.array_equal(bits(fr.accumulate(power)), bits(ps))
        freq = bits(fr.finish(ps)[0])
        plain = list(range(nf))
        pair = 2 * (nf // 2 - 1)   # the last two frames that one lane group transforms together
        blk = 8 * (nf // 8 - 2)    # the last two whole 8-frame blocks: two waves' turns with the baton
        wrong = {
            "last frame twice": fr.accumulate(power, plain + [nf - 1]),                      # the clamped frame leaks in
            "last frame dropped": fr.accumulate(power, plain[:-1]),
            "two frames swapped": fr.accumulate(power, plain[:pair] + [pair + 1, pair] + plain[pair + 2:]),
            "contracted re*re + im*im": fr.accumulate(fr.frame_power(x, contracted=True)),
        }
        if nf >= 16:   # the baton out of turn
            wrong["two 8-frame blocks swapped"] = fr.accumulate(power, plain[:blk] + plain[blk + 8:blk + 16] + plain[blk:blk + 8] + plain[blk + 16:])
        if ch == 2:
            wrong["floor in the stereo average"] = fr.accumulate(fr.frame_power(
                fr.transform(oracle, fr.windowed_frames(pcm, ch, floor_average=True))))
        for name, bad in wrong.items():
            changed = np.flatnonzero(bits(bad)[1:] != bits(ps)[1:])
            assert changed.size, (tag, name, "no bin of the summed spectrum changes: change the song's material")
            spec[name][0] += 1
            spec[name][1] += 1
            spec[name][2] += int(bits(fr.finish(bad)[0]) != freq)
        # the same add and drop for the integers
        step = 512 * ch
        l_sum, l_sq, l_hist = fr.statistics(pcm[(nf - 1) * step:nf * step])
        mean, variance = fr.mean_variance(total, sumsq, pcm.size)
        start, end = trim(pcm)
        for name, sign in (("statistics: last frame twice", 1), ("statistics: last frame dropped", -1)):
            t2, q2, h2 = total + sign * l_sum, sumsq + sign * l_sq, hist + sign * l_hist
            assert t2 != total or q2 != sumsq or not np.array_equal(h2, hist), (tag, name)
            c = stat[name]
            c[0] += 1
            c[1] += int(fr.mean_variance(t2, q2, pcm.size) != (mean, variance))
            if i % 16 == 0:   # 301 smoothing passes per song: a sample
                c[2] += 1
                c[3] += int(bits(fr.hist_integral(h2, start, end, pcm.size)) != bits(fr.hist_integral(hist, start, end, pcm.size)))
    assert spec["floor in the stereo average"][0] == 132 and spec["two 8-frame blocks swapped"][0] == 121 + 121
    print("\nerror made in the reference: songs it applies to | songs whose spectrum bits change | songs whose "
          "`frequency` bits change")
    for name, (n, raw, seen) in spec.items():
        print(f"  {name:32s} {n:4d} | {raw:4d} | {seen:4d}")
    print("error made in the statistics: songs | songs whose integers change | songs whose mean or variance changes | "
          "hist_integral bits changed, of a sample")
    for name, (n, seen, sample, seen_h) in stat.items():
        print(f"  {name:32s} {n:4d} | {n:4d} | {seen:4d} | {seen_h} of {sample}")
