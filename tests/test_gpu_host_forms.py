"""The host forms that had never run more than one upload wave (bl_amd_rhythm_batch_host with onsets and lag products,
bl_amd_loud_batch_host with hop energies, bl_amd_tpeak_batch_host with the block profile), over three waves: what each
wave fetches must land behind the wave before it, the onset curve, the hop energies and the profile by a running
cursor, the records and the rows of lag products by the wave's first song.

Every array is compared byte for byte with the same feature's device form in one call on one corpus, which is never
split; those device forms are what tests/test_gpu_rhythm.py, test_gpu_loud.py and test_gpu_tpeak.py check against their
Python references.  There is no tolerance anywhere."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import bliss_amd
import bliss_amd.loudness as ld
import bliss_amd.rhythm as rh
import bliss_amd.truepeak as tp

pytestmark = pytest.mark.gpu

LENGTHS = (12000, 16000, 40000, 9000, 11000, 10000)   # interleaved samples
CHANNELS = (1, 2, 2, 1, 2, 1)
WAVE_BYTES = 65536                                     # BL_AMD_HOST_WAVE_BYTES of the child: 32 768 samples per wave
LAGS = (4, 40)                                         # below the 42 hops of the shortest song
CEILING, BLOCK = 9000, 1000
ARRAYS = ("rhythm", "onsets", "acf", "loud", "hops", "tpeak", "blocks")


@functools.lru_cache(maxsize=None)
def songs():
    rng = np.random.default_rng(97)
    return tuple(rng.integers(-20000, 20001, n).astype(np.int16) for n in LENGTHS)


def waves_of(lengths, budget):
    """the rule of bl_wave_plan (bliss_amd/csrc/bl_waves.h) written out: songs in order, each padded to 8 samples; a
    song joins while the padded total stays within the budget, and the first song of a wave always joins"""
    waves, total = [], 0
    for i, n in enumerate(lengths):
        padded = (n + 7) & ~7
        if waves and total + padded <= budget:
            waves[-1].append(i)
            total += padded
        else:
            waves.append([i])
            total = padded
    return waves


def host_forms():
    """what the three host forms give, as bytes by name (runs in the child too)"""
    pcm, chans = list(songs()), list(CHANNELS)
    rec, onsets, acf = rh.rhythm_batch_host(pcm, chans, *LAGS, onsets=True, acf=True)
    loud, hops = ld.loud_host(pcm, chans, ld.kweight(22050), hops=True)
    peak, blocks = tp.tpeak_host(pcm, chans, ceiling=CEILING, block=BLOCK)
    return dict(zip(ARRAYS, (a.tobytes() for a in (rec, onsets, acf, loud, hops, peak, blocks))))


def device_forms():
    """the same from the device forms, one call each on one corpus"""
    import torch
    corpus = bliss_amd.DeviceCorpus(LENGTHS, CHANNELS, 1)
    corpus.pcm.fill_(32767)
    for i, p in enumerate(songs()):
        corpus.upload(i, p)
    rh.rhythm_device(corpus, *LAGS, onsets=True, acf=True)
    rec, onsets, acf = rh.fetch_rhythm(corpus)
    loud, hops = ld.loud_device(corpus, ld.kweight(22050), hops=True)
    peak, blocks = tp.tpeak_device(corpus, ceiling=CEILING, block=BLOCK)
    torch.cuda.synchronize()
    got = (rec, onsets, acf) + tuple(t.cpu().numpy() for t in (loud, hops, peak, blocks))
    return dict(zip(ARRAYS, (a.tobytes() for a in got)))


def test_rhythm_loud_and_tpeak_host_forms_over_three_upload_waves(gpu_lib, tmp_path):
    """BL_AMD_HOST_WAVE_BYTES is read when the default context is created, so the waves need a process of their own"""
    budget = WAVE_BYTES // 2
    assert waves_of(LENGTHS, budget) == [[0, 1], [2], [3, 4, 5]]
    assert 12000 + 16000 <= budget < 12000 + 16000 + 40000 and 40000 > budget and 9000 + 11000 + 10000 <= budget
    want = device_forms()
    hops = [n // c // rh.HOP for n, c in zip(LENGTHS, CHANNELS)]
    assert min(hops) > LAGS[1] and len(want["onsets"]) == 4 * sum(hops) and len(want["acf"]) == 8 * rh.LAGS * len(hops)
    assert len(want["hops"]) == 16 * sum(n // c // 2205 for n, c in zip(LENGTHS, CHANNELS))
    assert len(want["blocks"]) == 8 * sum(-(-(n // c) // BLOCK) for n, c in zip(LENGTHS, CHANNELS))
    # one wave, in this process: the default context has the default budget
    one = host_forms()
    for name in ARRAYS:
        assert one[name] == want[name], f"one wave: {name}"
    code = ("import sys, numpy as np\n"
            "from tests import test_gpu_host_forms as t\n"
            "np.savez(sys.argv[1], **{k: np.frombuffer(v, np.uint8) for k, v in t.host_forms().items()})\n")
    out = str(tmp_path / "waves.npz")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code, out], cwd=root, text=True, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300,
                       env=dict(os.environ, BL_AMD_HOST_WAVE_BYTES=str(WAVE_BYTES), PYTHONPATH=root))
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    for name in ARRAYS:
        assert got[name].tobytes() == want[name], f"three waves: {name}"
