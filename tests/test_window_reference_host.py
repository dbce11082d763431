"""tests/window_reference.py against the oracle, on the CPU: the exact window energies (no DFT: the integer filter sums
and Parseval) bound the oracle's on every song tests/test_gpu_windows.py analyses, the reference cannot pass with a wrong
head, a lost term or a wrong scale, the four sweep batches reach every geometry class of k_env_windows3 on a 256-CU
device, and the song builders give what they were asked for."""
import numpy as np
import pytest

from tests import window_reference as wr


@pytest.fixture(scope="module")
def host_songs(oracle):
    """name -> song: the sweep, the designed songs, the two companions and 16 songs of the split corpus"""
    out = {f"sweep{i}": s for i, s in enumerate(wr.sweep(oracle))}
    out.update(wr.designed())
    out["companion10"], out["companion45"] = wr.companion(oracle, 10), wr.companion(oracle, 45)
    split = wr.split_corpus(oracle)
    for i in list(range(0, wr.SPLIT_HEAD, 32)) + list(range(wr.SPLIT_HEAD, len(split), 128)):
        out[f"split{i}"] = split[i]
    assert sum(k.startswith("split") for k in out) == 16
    return out


@pytest.fixture(scope="module")
def oracle_energies(oracle, host_songs):
    """name -> (mean, variance, the oracle's energies): computed once"""
    out = {}
    for name, (pcm, ch) in host_songs.items():
        mean, var = wr.mean_variance(oracle, pcm)
        rec, en = oracle.envelope(pcm, wr.secs(pcm, ch))
        assert (rec["mean"], rec["variance"], rec["n_windows"]) == (mean, var, wr.n_windows_of(len(pcm))), name
        out[name] = (mean, var, en[:rec["n_windows"]].astype(np.float64))
    return out


def test_the_oracles_energies_lie_within_the_derived_bound_of_the_exact_ones(host_songs, oracle_energies):
    worst = 0.0
    for name, (pcm, _) in host_songs.items():
        mean, var, en = oracle_energies[name]
        exact = wr.exact_energies(pcm, mean, var)
        assert exact.min() > 0, name
        dev = float((np.abs(en - exact) / exact).max())
        worst = max(worst, dev)
        assert wr.within_bound(en, exact).all(), (name, dev, wr.BOUND)
    print(f"largest deviation of the oracle from the exact energy: {worst:.3e} (bound {wr.BOUND:.3e})")


@pytest.mark.parametrize("mutation", ["steady_head", "no_nyquist_term", "variance_plus_one"])
def test_a_wrong_reference_leaves_the_bound(host_songs, oracle_energies, mutation):
    """the head treated as steady state, the (sum (-1)^j Y_j)^2 term dropped, the variance off by one: each leaves the
    bound on at least one window (of the songs named: the first reads real samples in front of every window but a
    song's first; the second has all its energy in that term; the third has a small variance)"""
    name = {"steady_head": "sweep0", "no_nyquist_term": "alternating", "variance_plus_one": "mean+128"}[mutation]
    pcm, _ = host_songs[name]
    mean, var, en = oracle_energies[name]
    assert wr.within_bound(en, wr.exact_energies(pcm, mean, var)).all()
    wrong = {"steady_head": lambda: wr.exact_energies(pcm, mean, var, steady_head=True),
             "no_nyquist_term": lambda: wr.exact_energies(pcm, mean, var, nyquist_term=False),
             "variance_plus_one": lambda: wr.exact_energies(pcm, mean, var + 1)}[mutation]()
    outside = ~wr.within_bound(en, wrong)
    print(f"{mutation} on {name}: {int(outside.sum())} of {len(en)} windows leave the bound")
    assert outside.any()


def _batches(oracle):
    sweep = [len(p) for p, _ in wr.sweep(oracle)]
    alone = [n for n in sweep if n < wr.A_LIMIT]
    return {"A": alone, "B": sweep, "C": sweep + [wr.RATE * 10], "D": sorted(sweep)[:8] + [wr.RATE * 45]}


def test_the_four_batches_reach_every_geometry_class_on_256_cus(oracle):
    gx, reached = {}, {}
    for name, lengths in _batches(oracle).items():
        gx[name] = wr.grid_x(max(lengths), len(lengths), 256)
        reached[name] = wr.geometry_classes([wr.n_windows_of(n) for n in lengths], gx[name])
    assert gx == {"A": 1, "B": 2, "C": 5, "D": 57}
    assert set().union(*reached.values()) == wr.ALL_CLASSES
    # one workgroup per song: the floor split gives the last wave the longest run, and every workgroup has a round
    assert wr.ALL_CLASSES - reached["A"] >= {("wave", 6, "empty"), ("wave", 6, "short"), ("steps0",)}
    for name in "ABCD":
        print(name, "gx", gx[name], "misses", sorted(wr.ALL_CLASSES - reached[name]))
    assert [n for n in "ABCD" if ("steps0",) in reached[n]] == ["D"]


def test_the_geometry_mirror_on_small_cases():
    # 5 rounds on 7 waves: run_begin = 0 0 1 2 2 3 4 5
    assert [wr.run_begin(18, 1, u) for u in range(8)] == [0, 0, 1, 2, 2, 3, 4, 5]
    assert wr.steps(18, 1, 0) == 1 and wr.run_starts(18, 1) == {0, 1, 2, 3, 4, 5}
    assert wr.geometry_classes([18], 1) == {("last", 2), ("run", "first"), ("run", "later"), ("wave", 0, "empty"),
                                            ("wave", 3, "empty"), ("wave", 1, "full"), ("wave", 2, "full"),
                                            ("wave", 4, "full"), ("wave", 5, "full"), ("wave", 6, "full"),
                                            ("base5", 0), ("base5", 4), ("base5", 3), ("base5", 2), ("base5", 1)}
    assert wr.grid_x(5120, 1, 256) == 1 and wr.grid_x(57344, 1, 256) == 2 and wr.grid_x(57343, 1, 256) == 1
    assert wr.grid_x(44100 * 45, 9, 256) == 57 and wr.grid_x(44100 * 45, 9, 304) == 68
    assert len(wr.ALL_CLASSES) == 31


def test_the_builders_are_deterministic_and_give_what_they_were_built_for(oracle):
    sweep = wr.sweep(oracle)
    assert [wr.n_windows_of(len(p)) for p, _ in sweep] == list(range(18, 260, 2))
    assert [len(p) % wr.W for p, _ in sweep[:7]] == list(wr.SWEEP_EXTRA)
    assert [c for _, c in sweep[:8]] == [1, 1, 1, 2, 1, 1, 1, 2]
    assert np.array_equal(sweep[5][0], oracle.synth(93005, wr.RATE, 1, len(sweep[5][0])))
    d = wr.designed()
    assert wr.n_windows_of(len(d["ladder"][0])) == 32 and wr.n_windows_of(len(d["bytes"][0])) == 22
    assert wr.n_windows_of(len(d["alternating"][0])) == 20
    assert set(np.unique(d["bytes"][0])) == set(wr.BYTE_EDGES)
    for name, build in (("ladder", wr.tone_ladder), ("bytes", wr.byte_planes), ("alternating", wr.alternating)):
        assert np.array_equal(build()[0], d[name][0]), name
    targets = wr.mean_targets()
    assert len(targets) == 13 and len(set(targets)) == 13
    k0lo, k0hi, k2lo, k2hi = (wr._const_parts(m) for m in wr.searched_means())
    assert k0lo[0] < 64 and k0hi[0] > 65535 - 64 and k2lo[1] < 64 and k2hi[1] > 65535 - 64
    assert wr._const_parts(128) == (0, 0)
    for i, m in enumerate(targets):
        pcm, _ = d[f"mean{m:+d}"]
        assert np.array_equal(pcm, wr.mean_song(i, m)[0])
        assert len(pcm) == wr.MEAN_N and int(pcm.astype(np.int64).sum()) == m * wr.MEAN_N
        mean, var = wr.mean_variance(oracle, pcm)
        assert mean == m == oracle.mean(pcm) and var > 0, (m, mean, var)
    for name, (pcm, _) in d.items():
        assert wr.mean_variance(oracle, pcm)[1] > 0, name
    split = wr.split_corpus(oracle)
    lengths = [len(p) for p, _ in split]
    assert len(split) == 1280 and all(26000 <= n <= 33000 for n in lengths[:256]) and all(5120 <= n <= 6200 for n in lengths[256:])
    # the rule of blr_analyze_device on the batch sorted longest first
    srt = sorted(lengths, reverse=True)
    k = sum(n > srt[0] // 4 for n in srt)
    assert (k + 63) // 64 * 64 == 256 == wr.SPLIT_HEAD and 12e6 < sum(lengths) < 15e6
    assert np.array_equal(split[300][0], oracle.synth(94300, wr.RATE, 1, lengths[300]))
