"""tests/tail_reference.py (the array-form numpy restatement of the envelope tail the GPU tests compare k_env_tail
with) against the oracle, on the CPU: for every m = floor(n / 512) from 10 to 124 — two periods of (N mod 38,
n_blocks mod 6) — a bursty song whose window energies come from the oracle.  Same C library, so beat, atk_sum, tempo
and attack are equal bit for bit.  Two properties of the inputs are asserted on the reference alone: the peaks fall on
every residue mod 38 (every step of a 38-step block decides a beat somewhere) and no peak decision is closer than 1e-9
to flipping, seven orders above what a last-place difference in a logarithm can move — which is what lets
tests/test_gpu_tail.py demand `beat` exactly from the whole GPU path on the same songs."""
import numpy as np
import pytest

from tests import tail_reference as tr


@pytest.fixture(scope="module")
def sweep(oracle):
    lengths = tr.sweep_lengths()
    durations = [tr.sweep_duration(n) for n in lengths]
    full, energies = [], []
    for n, du in zip(lengths, durations):
        r, en = oracle.envelope(tr.bursty_song(n, 7), du)
        full.append(r)
        energies.append(en)
    return lengths, durations, full, energies, tr.tail_reference(lengths, durations, energies=energies)


def test_the_reference_equals_the_oracle_bit_for_bit(sweep):
    lengths, _, full, _, ref = sweep
    assert [n // 512 for n in lengths] == list(range(10, 125)) and len({n % 512 for n in lengths}) > 50
    for i, (n, o) in enumerate(zip(lengths, full)):
        tag = (n // 512, n)
        assert int(ref["nb_frames"][i]) == o["nb_frames"] and int(ref["n_windows"][i]) == o["n_windows"], tag
        assert int(ref["beat"][i]) == o["beat"], (tag, int(ref["beat"][i]), o["beat"])
        assert np.float64(ref["atk_sum"][i]).view(np.int64) == np.float64(o["atk_sum"]).view(np.int64), \
            (tag, float(ref["atk_sum"][i]), o["atk_sum"])
        assert ref["tempo"][i].view(np.int32) == np.float32(o["tempo"]).view(np.int32), tag
        assert ref["attack"][i].view(np.int32) == np.float32(o["attack"]).view(np.int32), tag
        assert ref["margin"][i] == o["min_peak_margin"], tag


def test_one_song_alone_equals_its_row_in_the_batch(sweep):
    """rows are padded to the longest song: the padding must not reach a shorter song's result"""
    lengths, durations, _, energies, ref = sweep
    for i in (0, 9, 57, 114):
        one = tr.tail_reference([lengths[i]], [durations[i]], energies=[energies[i]])
        for k in ("beat", "atk_sum", "tempo", "attack", "margin"):
            assert one[k][0] == ref[k][i], (i, k)
        assert np.array_equal(one["peaks"][0], ref["peaks"][i])


def test_the_sweep_is_varied_enough_to_stand_on(sweep):
    _, _, _, _, ref = sweep
    residues = set()
    for p in ref["peaks"]:
        residues |= {int(j) % 38 for j in p}
    print("beats", int(ref["beat"].min()), "..", int(ref["beat"].max()), "smallest margin", float(ref["margin"].min()))
    assert residues == set(range(38)), sorted(set(range(38)) - residues)
    assert ref["margin"].min() >= 1e-9, float(ref["margin"].min())
    assert ref["beat"].max() >= 8 and ref["beat"].min() >= 1
