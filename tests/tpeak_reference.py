"""Reference for the true peak (include/bliss_amd.h: bl_amd_song_tpeak, bl_amd_tpeak_*): the oversampled signal, the
record and the block profile in numpy int64, a slow one in Python integers for short songs, the table from its formula,
and switches that make a kernel's plausible mistakes on purpose, so that the tests can show that their songs would
catch each of them."""
import math

import numpy as np

# the table as the header and bliss_amd/csrc/bl_tpeak_table.h print it
TABLE = np.array([
    [0, 0, 0, 0, 0, 16384, 0, 0, 0, 0, 0, 0],
    [-27, 170, -493, 1133, -2645, 14688, 4730, -1695, 758, -304, 80, -3],
    [-16, 170, -552, 1313, -2968, 10253, 10253, -2968, 1313, -552, 170, -16],
    [-3, 80, -304, 758, -1695, 4730, 14688, -2645, 1133, -493, 170, -27]], dtype=np.int64)
FRONT, BACK = 5, 6          # frames in front of t and behind it that y[4t + p] reads
FULL_SCALE = 1 << 29        # a full-scale sample through a unit-gain phase
INDEX_BITS = 33

RECORD_DTYPE = np.dtype([("at", "<i8", (2,)), ("overs", "<i8", (2,)), ("tpeak", "<u4", (2,)), ("peak", "<i4", (2,)),
                         ("frames", "<i4"), ("status", "<i4")])

# the mistakes a kernel could plausibly make
SWITCHES = (
    "halo_swapped",          # a lane's halo 6 in front and 5 behind: the sixth frame behind a run reads as zero
    "phases_exchanged",      # the rows of phase 1 and phase 3 exchanged
    "last_frame_dropped",    # phases 1 to 3 of the last frame not computed
    "front_from_memory",     # frames in front of the song taken from what lies there instead of zero
    "last_index",            # the last index of a maximum instead of the first
    "overs_ge",              # >= for overs
    "pair_across_channels",  # a stereo pair built from the two channels of one frame: odd taps read the other channel
    "signed_max",            # the maximum of y instead of |y|
    "block_at_tile",         # a block cut at the lanes' run edges instead of at `block`
    "odd_tail_frame",        # the last sample of a stereo song with an odd n_samples counted as a frame
    "pair_saturated",        # the two-product sum of a tap pair saturated at +-2^29, as a too narrow accumulator would
    "seam_twice",            # the first frame of every run but the song's first counted twice in overs
)


def generate_table():
    """G[p][j + 5] = floor(2^14 w(m) sinc(m / 4) + 1/2), m = 4 j - p, w the Hann window over |m| < 24"""
    g = np.zeros((4, 12), dtype=np.int64)
    for p in range(4):
        for j in range(-5, 7):
            m = 4 * j - p
            if abs(m) >= 24:
                continue
            w = (1.0 + math.cos(math.pi * m / 24.0)) / 2.0
            s = 1.0 if m == 0 else math.sin(math.pi * m / 4.0) / (math.pi * m / 4.0)
            g[p, j + 5] = math.floor(16384.0 * w * s + 0.5)
    return g


def _channels(pcm, channels, sw):
    pcm = np.asarray(pcm, dtype=np.int64).reshape(-1)
    if "odd_tail_frame" in sw and channels == 2 and pcm.size % 2:
        pcm = np.append(pcm, 0)
    frames = pcm.size // channels
    return [pcm[c:frames * channels:channels] for c in range(channels)], frames


def oversample(xs, c, sw=frozenset(), lane=16, fill=32767):
    """y_c[0 .. 4F) of channel c of the channel list xs, int64"""
    g = TABLE[[0, 3, 2, 1]] if "phases_exchanged" in sw else TABLE
    frames = xs[c].size
    front = np.full(FRONT, fill if "front_from_memory" in sw else 0, dtype=np.int64)
    pad = [np.concatenate([front, x, np.zeros(BACK, dtype=np.int64)]) for x in xs]
    y = np.zeros(4 * frames, dtype=np.int64)
    t = np.arange(frames)
    for p in range(4):
        acc = np.zeros(frames, dtype=np.int64)
        for k in range(0, 12, 2):
            part = np.zeros(frames, dtype=np.int64)
            for kk in (k, k + 1):
                src = pad[c ^ (kk & 1)] if "pair_across_channels" in sw and len(xs) == 2 else pad[c]
                tap = src[kk:kk + frames].copy()
                if "halo_swapped" in sw and kk == 11:
                    tap[t % lane == lane - 1] = 0  # frame t + 6 lies beyond the run's 5 frames of halo
                part += g[p, kk] * tap
            if "pair_saturated" in sw:
                part = np.clip(part, -(1 << 29), (1 << 29) - 1)
            acc += part
        y[p::4] = acc
    if "last_frame_dropped" in sw and frames:
        y[4 * frames - 3:] = 0
    return y


def song(pcm, channels, ceiling=32767, block=None, sw=frozenset(), lane=16, fill=32767):
    """(record as a RECORD_DTYPE scalar array of shape (1,), blocks as uint32 (ceil(F / block), 2) or None)"""
    sw = frozenset(sw)
    assert sw <= set(SWITCHES), sw
    xs, frames = _channels(pcm, channels, sw)
    rec = np.zeros(1, dtype=RECORD_DTYPE)
    rec["at"] = -1
    rec["frames"] = frames
    blocks = None if block is None else np.zeros(((frames + block - 1) // block, 2), dtype=np.uint32)
    for c in range(channels):
        if not frames:
            break
        y = oversample(xs, c, sw, lane, fill)
        a = np.maximum(y, 0) if "signed_max" in sw else np.abs(y)
        top = a.max()
        hits = np.flatnonzero(a == top)
        rec["tpeak"][0, c] = top
        rec["at"][0, c] = hits[-1] if "last_index" in sw else hits[0]
        over = a >= (ceiling << 14) if "overs_ge" in sw else a > (ceiling << 14)
        rec["overs"][0, c] = over.sum()
        if "seam_twice" in sw:
            per_frame = over.reshape(frames, 4).sum(axis=1)
            rec["overs"][0, c] += per_frame[lane::lane].sum()
        rec["peak"][0, c] = np.abs(xs[c]).max()
        if blocks is not None:
            per_frame = a.reshape(frames, 4).max(axis=1)
            if "block_at_tile" not in sw:
                blocks[:, c] = np.maximum.reduceat(per_frame, np.arange(0, frames, block))
                continue
            for b in range(blocks.shape[0]):
                lo, hi = b * block, min(frames, (b + 1) * block)
                lo, hi = lo // lane * lane, frames if hi == frames else hi // lane * lane
                blocks[b, c] = per_frame[lo:hi].max() if hi > lo else 0
    return rec, blocks


def song_slow(pcm, channels, ceiling=32767, block=None):
    """the same in Python integers, straight from the definition; for short songs"""
    pcm = [int(v) for v in np.asarray(pcm).reshape(-1)]
    frames = len(pcm) // channels
    g = [[int(v) for v in row] for row in TABLE]
    rec = np.zeros(1, dtype=RECORD_DTYPE)
    rec["at"] = -1
    rec["frames"] = frames
    blocks = None if block is None else np.zeros(((frames + block - 1) // block, 2), dtype=np.uint32)
    for c in range(channels):
        if not frames:
            break

        def x(t):
            return pcm[t * channels + c] if 0 <= t < frames else 0
        best, at, overs, peak = -1, -1, 0, 0
        for t in range(frames):
            peak = max(peak, abs(x(t)))
            for p in range(4):
                y = abs(sum(g[p][j + 5] * x(t + j) for j in range(-5, 7)))
                if y > best:
                    best, at = y, 4 * t + p
                overs += y > ceiling * 16384
                if blocks is not None:
                    blocks[t // block, c] = max(int(blocks[t // block, c]), y)
        rec["tpeak"][0, c], rec["at"][0, c], rec["overs"][0, c], rec["peak"][0, c] = best, at, overs, peak
    return rec, blocks


def batch(songs, channels, ceiling=32767, block=None):
    """records (n,) and the concatenated profile of a list of songs"""
    out = [song(p, ch, ceiling, block) for p, ch in zip(songs, channels)]
    recs = np.concatenate([r for r, _ in out])
    return recs, None if block is None else np.concatenate([b for _, b in out], axis=0)


def dbtp(tpeak):
    return -math.inf if tpeak == 0 else 20.0 * math.log10(tpeak / FULL_SCALE)


def faded_sine(frames, period, phase_deg, amplitude, fade=480):
    """amplitude * 32767 * sin(2 pi t / period + phase) with a linear fade of `fade` frames at both ends, rounded to
    int16: the metering signals of the accuracy test"""
    t = np.arange(frames, dtype=np.float64)
    env = np.minimum(1.0, np.minimum(t, frames - 1 - t) / fade)
    x = amplitude * 32767.0 * env * np.sin(2.0 * math.pi * t / period + math.radians(phase_deg))
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)
