"""A reference for the window energies of the envelope analysis that shares nothing with the code under test and nothing
with the oracle's DFT — TEST INFRASTRUCTURE, shared by tests/test_window_reference_host.py (which proves it against the
oracle and shows that it cannot pass with a wrong head, a lost term or a wrong scale), tests/test_fir_int_host.py (the
CPU emulation of FIR mode 2 on the songs built here) and tests/test_gpu_windows.py (which holds k_env_windows3 to it).

The exact energy.  The taps of the 17-tap FIR are literals with seven decimals, c_m = C_m * 1e-7 (the digits of
bliss_amd/csrc/bl_fir_int.h, restated below); with k = s - mean the zero-state filter output of a window is the integer
Y_j = sum_m C_m k[j - m] (samples before the window's first count 0; |Y| < 2^45), and by Parseval for a real 512-point
input

    sum_{k = 0 .. 256} |X_k|^2 = (512 * sum Y_j^2 + (sum Y_j)^2 + (sum (-1)^j Y_j)^2) / 2,

an integer formed here without any rounding and without any transform.  The energy is that integer times
(32768 / (1e7 * variance))^2 — the reference's x = (s / 2^15 - mean / 2^15) / (variance / 2^30) — as one correctly
rounded division of Python integers: the reference's own error is 2^-53 relative.

The launch geometry.  k_env_windows3 (bliss_amd/csrc/bl_env_kernels.hip) splits a song's rounds of four windows over the
7 compute waves of gridDim.x workgroups; grid_x, run_begin and steps mirror that arithmetic, and geometry_classes names
what a batch makes the kernel do: a GEOMETRY CLASS is one of
    ("wave", c, "empty" | "short" | "full")  the run of compute wave c of some workgroup has no round, fewer rounds than
                                             the workgroup's steps, or all of them;
    ("base5", v)                             a run's first round starts at ring position v = (4 r0) % 5;
    ("run", "first" | "later")               a run begins the song (zero padding in front) or lies inside it;
    ("last", 2 | 4)                          the song's last round holds two windows or four;
    ("steps0",)                              a workgroup none of whose waves has a round.
"""
import ctypes as C
import functools

import numpy as np

from tests import freq_reference, stats_reference

RATE = 44100
W = 512
EV_CWAVES = 7   # compute waves per workgroup of k_env_windows3
TAPS = (-23470, 44613, -114627, 226382, -405147, 580037, -779167, 882711, 9065095,
        882711, -779167, 580037, -405147, 226382, -114627, 44613, -23470)
TAPSUM = 9887759
assert sum(TAPS) == TAPSUM
BOUND = 257 * 2.0 ** -24 + 2.0 ** -40   # see within_bound


# ---- the exact energy ---------------------------------------------------------------------------------------------

def mean_variance(oracle, pcm):
    """(mean, variance) by the reference's int32-wrapping definitions: tests/freq_reference.py's exact integers where
    they hold (|mean| <= 13 571: no (sample - mean)^2 leaves an int32), tests/stats_reference.py's wrapping squares
    beyond; the mean is the oracle's and tests/stats_reference.py's, which must agree"""
    pcm = np.asarray(pcm, dtype=np.int16)
    mean = int(oracle.mean(pcm))
    assert mean == stats_reference.mean_wrapped(pcm)
    if abs(mean) > 13571:
        return mean, stats_reference.variance_wrapped(pcm, mean)
    total, sumsq, _ = freq_reference.statistics(pcm)
    m, v = freq_reference.mean_variance(total, sumsq, pcm.size)
    assert m == mean
    return m, v


def n_windows_of(n):
    return 2 * (n // W) - 2


def filter_sums(pcm, mean, steady_head=False):
    """(n_windows, 512) int64: Y_j of every window, exact.  steady_head: the WRONG head, which reads the samples in
    front of the window (zero only in front of the song) — a mutation of the host test."""
    k = np.asarray(pcm, dtype=np.int16).astype(np.int64) - int(mean)
    nw = n_windows_of(k.size)
    kp = np.concatenate([np.zeros(16, dtype=np.int64), k[:256 * (nw + 1)]])
    full = np.zeros(256 * (nw + 1), dtype=np.int64)
    for m, c in enumerate(TAPS):   # full[i] = sum_m C_m k[i - m]
        full += c * kp[16 - m:16 - m + full.size]
    idx = 256 * np.arange(nw)[:, None] + np.arange(W)[None, :]
    y = full[idx]
    if not steady_head:
        for j in range(16):        # take back the taps that reach in front of the window
            for m in range(j + 1, 17):
                y[:, j] -= TAPS[m] * kp[16 + 256 * np.arange(nw) + j - m]
    assert np.abs(y).max(initial=0) < 2 ** 45
    return y


def energy_integers(y, nyquist_term=True):
    """per window the Python int (512 sum Y^2 + (sum Y)^2 + (sum (-1)^j Y)^2) / 2.  Y^2 does not fit an int64: Y is split
    into limbs of 23 bits, whose products summed over 512 samples stay below 2^55.  nyquist_term=False: the WRONG sum
    without the last square (a mutation of the host test)."""
    hi, lo = y >> 23, y & (2 ** 23 - 1)
    hh, hl, ll = (hi * hi).sum(axis=1), (hi * lo).sum(axis=1), (lo * lo).sum(axis=1)
    a = y.sum(axis=1)
    b = (y[:, 0::2] - y[:, 1::2]).sum(axis=1)
    out = []
    for w in range(y.shape[0]):
        s2 = (int(hh[w]) << 46) + (int(hl[w]) << 24) + int(ll[w])
        twice = 512 * s2 + int(a[w]) ** 2 + (int(b[w]) ** 2 if nyquist_term else 0)
        assert twice % 2 == 0 or not nyquist_term
        out.append(twice // 2)
    return out


def exact_energies(pcm, mean, variance, steady_head=False, nyquist_term=True):
    """float64 per window: the exact energy rounded once"""
    den = (10 ** 7 * int(variance)) ** 2
    return np.array([(e << 30) / den for e in energy_integers(filter_sums(pcm, mean, steady_head), nyquist_term)],
                    dtype=np.float64)


def within_bound(energies, exact):
    """bool per window: |energy - exact| <= (257 * 2^-24 + 2^-40) * exact.  Derived, not measured: the reference
    arithmetic differs from the exact value by f64 noise and by the 257 f32 roundings of the ordered sum of non-negative
    terms, each at most 2^-24 of a partial sum that never exceeds the total; 2^-40 covers the f64 noise and this file's
    one rounding."""
    e = np.asarray(energies, dtype=np.float64)
    return np.abs(e - exact) <= BOUND * exact


# ---- the launch geometry ------------------------------------------------------------------------------------------

def grid_x(maxn, count, n_cu):
    """blk_env_windows' grid_x_for(max(1, (2 * (maxn / 512)) / (4 * 4 * 7)), count, 2, n_cu): blocks per song"""
    units_max = max(1, (2 * (maxn // W)) // (4 * 4 * EV_CWAVES))
    return max(1, min((2 * n_cu + count - 1) // count, units_max, 65535))


def run_begin(n_windows, gx, u):
    return (n_windows + 3) // 4 * u // (EV_CWAVES * gx)


def run_starts(n_windows, gx):
    return {run_begin(n_windows, gx, u) for u in range(EV_CWAVES * gx + 1)}


def steps(n_windows, gx, bx):
    return max(run_begin(n_windows, gx, EV_CWAVES * bx + c + 1) - run_begin(n_windows, gx, EV_CWAVES * bx + c)
               for c in range(EV_CWAVES))


ALL_CLASSES = frozenset([("wave", c, k) for c in range(EV_CWAVES) for k in ("empty", "short", "full")]
                        + [("base5", v) for v in range(5)] + [("run", "first"), ("run", "later")]
                        + [("last", 2), ("last", 4), ("steps0",)])


def geometry_classes(n_windows_list, gx):
    """the set of geometry classes (see the head of this file) a launch of gx workgroups per song reaches on songs of
    these window counts"""
    out = set()
    for nw in n_windows_list:
        out.add(("last", nw - 4 * ((nw + 3) // 4 - 1)))
        for bx in range(gx):
            st = steps(nw, gx, bx)
            if st == 0:
                out.add(("steps0",))
            for c in range(EV_CWAVES):
                r0, r1 = (run_begin(nw, gx, EV_CWAVES * bx + c + d) for d in (0, 1))
                out.add(("wave", c, "empty" if r1 == r0 else "short" if r1 - r0 < st else "full"))
                if r1 > r0:
                    out.add(("base5", 4 * r0 % 5))
                    out.add(("run", "first" if r0 == 0 else "later"))
    return out


# ---- the songs ----------------------------------------------------------------------------------------------------
# a song is (pcm int16 read-only, channels)

def secs(pcm, channels):
    return max(1, len(pcm) // (RATE * channels))


def _ro(a):
    a = np.ascontiguousarray(a, dtype=np.int16)
    a.setflags(write=False)
    return a


SWEEP_EXTRA = (0, 1, 7, 8, 255, 256, 511)
A_LIMIT = 57344   # below it a launch of these songs alone has one workgroup per song


@functools.lru_cache(maxsize=None)
def sweep(oracle):
    """one synthetic song for every even n_windows from 18 to 258 (5..65 rounds): 121 songs, every fourth stereo"""
    out = []
    for i, nw in enumerate(range(18, 260, 2)):
        ch = 2 if i % 4 == 3 else 1
        out.append((_ro(oracle.synth(93000 + i, RATE, ch, W * (nw // 2 + 1) + SWEEP_EXTRA[i % 7])), ch))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def companion(oracle, seconds):
    """the longer song a batch is analysed beside, which sets the grid"""
    return (_ro(oracle.synth(93900 + seconds, RATE, 1, RATE * seconds)), 1)


LADDER_BINS = (0, 1, 127, 128, 129, 130, 255, 256)


def tone_ladder():
    """32 windows: consecutive 1 024-sample segments, each a pure tone at one bin of the 512-point window (bin 0: a DC
    step), amplitude about 12 000, then 512 noisy samples.  Almost all of a window's energy sits in one term of the
    ordered sum — around the place where its two halves meet (terms 127..130) and at both ends"""
    rng = np.random.default_rng(93201)
    t = np.arange(1024)
    segs = [np.rint(12000 * np.cos(2 * np.pi * b * t / W + 0.3 * (0 < b < 256))) for b in LADDER_BINS]
    tail = rng.integers(-3000, 3001, W)
    return (_ro(np.concatenate(segs + [tail])), 1)


BYTE_EDGES = (-32768, -32513, -32512, -257, -256, -129, -128, -1, 0, 1, 127, 128, 255, 256, 32512, 32639, 32767)


def byte_planes():
    """22 windows of samples at both ends of the signed low and high bytes FIR mode 2 splits a sample into"""
    rng = np.random.default_rng(93202)
    return (_ro(np.array(BYTE_EDGES)[rng.integers(0, len(BYTE_EDGES), W * 12)]), 1)


def alternating():
    """20 windows of alternating full scale, a zero every 1 001 samples: all energy in term 256"""
    t = np.arange(W * 11)
    s = np.where(t % 2 == 0, 32767, -32768)
    s[::1001] = 0
    return (_ro(s), 1)


def _const_parts(mean):
    k = (128 - mean) * TAPSUM   # bl_firi_const
    return k & 0xFFFF, (k >> 16) & 0xFFFF


@functools.lru_cache(maxsize=None)
def searched_means():
    """four means, the smallest in magnitude for which the low (k0) or the middle (k2) 16 bits of the constant
    K = (128 - mean) * 9 887 759 of the matrix products lie within 64 of 0 and of 65 535"""
    found = {}
    for a in range(1, 32700):
        for mean in (a, -a):
            if mean == 128:
                continue
            k0, k2 = _const_parts(mean)
            for name, v in (("k0", k0), ("k2", k2)):
                for end, hit in (("low", v < 64), ("high", v > 65535 - 64)):
                    if hit:
                        found.setdefault((name, end), mean)
        if len(found) == 4:
            break
    return tuple(found[k] for k in (("k0", "low"), ("k0", "high"), ("k2", "low"), ("k2", "high")))


MEAN_TARGETS = (128, 127, 129, 0, -1, 13571, -13571, 13572, -13572)
MEAN_N = 60000   # the reference's int32 sum of the samples cannot wrap


def mean_targets():
    return MEAN_TARGETS + searched_means()


def mean_song(i, mean):
    """60 000 samples whose exact mean is `mean`, a few LSB of noise around it"""
    rng = np.random.default_rng(93300 + i)
    noise = rng.integers(-20, 21, MEAN_N)
    d = int(noise.sum())
    noise[:abs(d)] -= 1 if d > 0 else -1   # the sum of the noise becomes 0
    assert noise.sum() == 0
    return (_ro(mean + noise), 1)


@functools.lru_cache(maxsize=None)
def designed(oracle=None):
    """dict name -> song: the tone ladder, the byte planes, alternating full scale and the mean classes"""
    out = {"ladder": tone_ladder(), "bytes": byte_planes(), "alternating": alternating()}
    for i, m in enumerate(mean_targets()):
        out[f"mean{m:+d}"] = mean_song(i, m)
    return out


SPLIT_HEAD, SPLIT_REST = 256, 1024


@functools.lru_cache(maxsize=None)
def split_corpus(oracle):
    """256 songs of 26 000..33 000 samples, then 1 024 of 5 120..6 200: one batch of them is split by the rule of
    blr_analyze_device (at least 1 024 songs of mixed lengths; the head, in whole 64s, is every song longer than a
    quarter of the longest; both parts at least 256), with n_head == 256"""
    rng = np.random.default_rng(93400)
    lengths = [int(v) for v in rng.integers(26000, 33001, SPLIT_HEAD)] + [int(v) for v in rng.integers(5120, 6201, SPLIT_REST)]
    assert min(lengths[:SPLIT_HEAD]) > max(lengths) // 4 >= max(lengths[SPLIT_HEAD:])
    return tuple((_ro(oracle.synth(94000 + i, RATE, 1, n)), 1) for i, n in enumerate(lengths))


# ---- helpers of the GPU tests -------------------------------------------------------------------------------------

def analyze(lib, songs, mode):
    """Records and window energies (one array per song) of `songs` analysed as one batch in FIR mode `mode`."""
    import bliss_amd
    corpus = bliss_amd.DeviceCorpus([len(p) for p, _ in songs], [c for _, c in songs], [secs(p, c) for p, c in songs])
    arena = np.zeros(corpus.total_samples, dtype=np.int16)
    for i, (p, _) in enumerate(songs):
        o = int(corpus.desc[i].pcm_offset)
        arena[o:o + len(p)] = p
    corpus.pcm[:arena.size].copy_(corpus.torch.from_numpy(arena))
    try:
        assert lib.bl_amd_set_fir_mode(mode) == 0
        corpus.analyze()
        got = corpus.fetch()
        total = int(sum(int(g["nb_frames"]) for g in got))
        en = np.zeros(total, dtype=np.float32)
        assert lib.bl_amd_last_energies(en.ctypes.data_as(C.POINTER(C.c_float)), total) == total
    finally:
        lib.bl_amd_set_fir_mode(-1)
    offs = np.concatenate([[0], np.cumsum(got["nb_frames"].astype(np.int64))])
    return got, [en[offs[i]:offs[i] + int(got[i]["n_windows"])].copy() for i in range(len(songs))]
