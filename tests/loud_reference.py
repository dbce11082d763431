"""Reference of the K-weighted gated loudness (include/bliss_amd.h, the numbered block of bl_amd_loud_*): numpy for the
filter, vectorised over all chunks of all songs and looping over the warm + 16 hop frames of a chunk, with every f64
operation written in the header's order; Python ints for everything behind the hop energies Z.  The GPU is compared
with == against it, never with a tolerance.

`mistakes` switches on plausible errors of an implementation, one name each (MISTAKES); the host test proves that each
one changes a named input, so a GPU result equal to the reference has made none of them."""
import math
from types import SimpleNamespace

import numpy as np

CHUNK = 16
FIELDS = ("gated_sum", "gated_count", "abs_sum", "abs_count", "momentary_max", "st_max", "lra_lo", "lra_hi", "st_gated",
          "hops", "blocks", "status")
MISTAKES = (
    "warm_wraps",        # the warm-up not clipped at the song's start: negative frame indices wrap to the song's end
    "state_carried",     # a chunk starts from the state the chunk before it left, not from zero
    "count_from_warm",   # the hops of a chunk counted from the warm-up's first frame
    "a_swapped",         # a1 and a2 of stage 1 exchanged
    "sum_order",         # the five terms of a stage summed in another order
    "z_rounded",         # Z rounded to nearest instead of floored
    "partial_hop",       # the partial last hop included
    "mono_dual",         # a mono song counted as two channels
    "abs_ge",            # >= at the absolute gate
    "rel_ge",            # >= at the relative gate
    "rel_over_all",      # the relative threshold from all blocks instead of those above the absolute gate
    "block_stride4",     # blocks at a stride of four hops (no overlap)
    "st_gate_unscaled",  # the short-term absolute gate not scaled from 4 to 30 hops
    "pct_truncated",     # the percentile index truncated instead of rounded
    "carry_dropped",     # the sums kept in 64 bits
)


def kweight(rate):
    """bl_amd_loud_kweight in Python floats: the same expressions in the same order"""
    if rate < 8000 or rate > 48000 or rate % 10:
        raise ValueError(rate)
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / rate)
    Vh = math.pow(10.0, G / 20.0)
    Vb = math.pow(Vh, 0.4996667741545416)
    a0 = 1.0 + K / Q + K * K
    s1_b = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0]
    s1_a = [2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / rate)
    a0 = 1.0 + K / Q + K * K
    s2_a = [2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    hop = rate // 10
    return SimpleNamespace(s1_b=s1_b, s1_a=s1_a, s2_a=s2_a, hop=hop, warm=4096,
                           abs_gate=int(math.floor(4.0 * hop * 1073741824.0 * math.pow(10.0, -6.9309))))


def plain(p, **kw):
    """a parameter record (SimpleNamespace or the ctypes record) as a SimpleNamespace, with fields replaced"""
    d = dict(s1_b=[float(x) for x in p.s1_b], s1_a=[float(x) for x in p.s1_a], s2_a=[float(x) for x in p.s2_a],
             hop=int(p.hop), warm=int(p.warm), abs_gate=int(p.abs_gate))
    d.update(kw)
    return SimpleNamespace(**d)


# ---- stages 1 to 3 ---------------------------------------------------------------------------------------------------

def _u64(v):
    """a floored energy as an int; a mistake that makes the filter unstable saturates instead of raising"""
    return int(v) if v < 18446744073709551615.0 else (1 << 64) - 1


def hop_energies(pcm_list, channels, p, mistakes=()):
    """Z of every song: a list of uint64 arrays of shape (H, 2), channel 1 of a mono song 0"""
    p = plain(p)
    hop, warm = p.hop, p.warm
    b0, b1, b2 = (np.float64(x) for x in p.s1_b)
    a1, a2 = (np.float64(x) for x in p.s1_a)
    A1, A2 = (np.float64(x) for x in p.s2_a)
    if "a_swapped" in mistakes:
        a1, a2 = a2, a1
    songs = []
    for pcm, ch in zip(pcm_list, channels):
        x = np.asarray(pcm, dtype=np.int16)
        F = x.size // ch
        fr = np.zeros((F, 2), dtype=np.float64)
        fr[:, :ch] = x[:F * ch].reshape(F, ch)
        songs.append(fr)
    Hs = [(-(-fr.shape[0] // hop) if "partial_hop" in mistakes else fr.shape[0] // hop) for fr in songs]
    chunk = max(Hs + [1]) if "state_carried" in mistakes else CHUNK
    if "state_carried" in mistakes:
        warm = 0
    # one lane per chunk; frame f_first of a lane sits at index `warm` of its row
    lanes = [(i, h0, min(h0 + chunk, H)) for i, H in enumerate(Hs) for h0 in range(0, H, chunk)]
    T = warm + chunk * hop
    X = np.zeros((len(lanes), T, 2), dtype=np.float64)
    count_at = np.full(len(lanes), warm, dtype=np.int64)   # the row index at which a lane's hops begin
    for k, (i, h0, h1) in enumerate(lanes):
        fr, f_first = songs[i], h0 * hop
        f_end = min(h1 * hop, fr.shape[0])
        f_start = f_first - warm
        if f_start < 0 and "warm_wraps" not in mistakes:
            f_start = 0
        idx = np.arange(f_start, f_end) % max(fr.shape[0], 1)   # negative indices wrap, which is the mistake
        X[k, warm - (f_first - f_start):warm + (f_end - f_first)] = fr[idx]
        if "count_from_warm" in mistakes:
            count_at[k] = warm - (f_first - max(f_first - warm, 0))
    Z = [np.zeros((H, 2), dtype=np.uint64) for H in Hs]
    n = len(lanes)
    z = np.zeros((n, 2))
    x1, x2, v1, v2, y1, y2, e = z.copy(), z.copy(), z.copy(), z.copy(), z.copy(), z.copy(), z.copy()
    in_hop = np.zeros(n, dtype=np.int64)
    done = np.zeros(n, dtype=np.int64)
    want = np.array([h1 - h0 for _, h0, h1 in lanes], dtype=np.int64)
    with np.errstate(under="ignore", over="ignore", invalid="ignore"):
        for t in range(T):
            x = X[:, t, :]
            if "sum_order" in mistakes:
                v = (b0 * x + (b1 * x1 + b2 * x2)) - (a2 * v2 + a1 * v1)
                y = ((v + v2) - (v1 + v1)) - (A2 * y2 + A1 * y1)
            else:
                v = ((((b0 * x + b1 * x1) + b2 * x2) - a2 * v2) - a1 * v1)
                y = ((((v - (v1 + v1)) + v2) - A2 * y2) - A1 * y1)
            x2, x1, v2, v1, y2, y1 = x1, x, v1, v, y1, y
            on = (t >= count_at) & (done < want)
            if not on.any():
                continue
            e[on] = e[on] + (y * y)[on]
            in_hop[on] += 1
            for k in np.flatnonzero(on & (in_hop == hop)):
                i, h0, _ = lanes[k]
                zz = np.rint(e[k]) if "z_rounded" in mistakes else np.floor(e[k])
                Z[i][h0 + done[k]] = [_u64(zz[0]), _u64(zz[1])]
                e[k] = 0.0
                in_hop[k] = 0
                done[k] += 1
    if "partial_hop" in mistakes:   # the last hop of a song that ends inside it never fills: what it has is its energy
        for k in np.flatnonzero(done < want):
            i, h0, _ = lanes[k]
            Z[i][h0 + done[k]] = [_u64(np.floor(e[k][0])), _u64(np.floor(e[k][1]))]
    return Z


# ---- stages 4 to 6 ---------------------------------------------------------------------------------------------------

def gates(Z, abs_gate, mistakes=(), mono=False):
    """the record of one song from its hop energies (anything of shape (H, 2) or (H,)), as a dict of Python ints"""
    Z = np.asarray(Z)
    if Z.ndim == 1:
        Z = np.stack([Z, np.zeros_like(Z)], axis=1) if Z.size else Z.reshape(0, 2)
    q = [int(a) + int(b) for a, b in Z.tolist()]
    if mono and "mono_dual" in mistakes:
        q = [2 * v for v in q]
    H = len(q)
    pre = [0]
    for v in q:
        pre.append(pre[-1] + v)
    wrap = (lambda s: s % (1 << 64)) if "carry_dropped" in mistakes else (lambda s: s)
    P = [pre[j + 4] - pre[j] for j in range(0, H - 3, 4 if "block_stride4" in mistakes else 1)]
    A = [v for v in P if (v >= abs_gate if "abs_ge" in mistakes else v > abs_gate)]
    base = P if "rel_over_all" in mistakes else A
    N1, S1 = len(base), wrap(sum(base))
    G = [v for v in A if (v * 10 * N1 >= S1 if "rel_ge" in mistakes else v * 10 * N1 > S1)]
    ST = [pre[j + 30] - pre[j] for j in range(H - 29)]
    starts = ST[::10]
    if "st_gate_unscaled" in mistakes:
        B = [v for v in starts if v > abs_gate]
    else:
        B = [v for v in starts if 2 * v > 15 * abs_gate]
    N, S = len(B), wrap(sum(B))
    surv = sorted(v for v in B if v * 100 * N > S)
    M = len(surv)
    if "pct_truncated" in mistakes:
        i_lo, i_hi = (10 * (M - 1)) // 100, (95 * (M - 1)) // 100
    else:
        i_lo, i_hi = (10 * (M - 1) + 50) // 100, (95 * (M - 1) + 50) // 100
    return dict(gated_sum=wrap(sum(G)), gated_count=len(G), abs_sum=S1, abs_count=N1, momentary_max=max(P, default=0),
                st_max=max(ST, default=0), lra_lo=surv[i_lo] if M else 0, lra_hi=surv[i_hi] if M else 0, st_gated=M,
                hops=H, blocks=max(0, H - 3), status=0)


def loud(pcm_list, channels, p, mistakes=()):
    """(records, Z) of songs from their PCM: records a list of dicts, Z a list of (H, 2) uint64 arrays"""
    Z = hop_energies(pcm_list, channels, p, mistakes)
    return [gates(z, int(p.abs_gate), mistakes, mono=ch == 1) for z, ch in zip(Z, channels)], Z


# ---- the record's figures, as bl_api.c computes them -------------------------------------------------------------------

def lufs(rec, hop):
    if not rec["gated_count"] or not rec["gated_sum"]:
        return -math.inf
    return -0.691 + 10.0 * math.log10(rec["gated_sum"] / (rec["gated_count"] * 4.0 * hop * 1073741824.0))


def range_lu(rec):
    if not rec["st_gated"] or not rec["lra_lo"]:
        return 0.0
    return 10.0 * math.log10(rec["lra_hi"] / rec["lra_lo"])


def rec_ints(rec, i):
    """record i of a structured array (bliss_amd.loudness.loud_to_numpy) as the dict gates() returns"""
    d = {f: int(rec[f][i]) for f in FIELDS if f not in ("gated_sum", "abs_sum")}
    for f in ("gated_sum", "abs_sum"):
        d[f] = int(rec[f][i][0]) + (int(rec[f][i][1]) << 64)
    return d


# ---- material the host and the GPU tests share ---------------------------------------------------------------------------

def sine(rate, parts, f=1000.0, ch=2):
    """parts = [(seconds, dBFS)] of a sine, phase continuous, interleaved on ch channels"""
    out, n0 = [], 0
    for secs, db in parts:
        n = int(round(secs * rate))
        t = np.arange(n0, n0 + n)
        out.append(np.rint(32768.0 * 10 ** (db / 20.0) * np.sin(2 * np.pi * f * t / rate)).clip(-32768, 32767))
        n0 += n
    return np.repeat(np.concatenate(out).astype(np.int16), ch)


EBU_3341 = {   # Tech 3341 table 1, cases 1 to 5: the programme loudness, +- 0.1 LU
    1: ([(20, -23)], -23.0), 2: ([(20, -33)], -33.0), 3: ([(10, -36), (60, -23), (10, -36)], -23.0),
    4: ([(10, -72), (10, -36), (60, -23), (10, -36), (10, -72)], -23.0), 5: ([(20, -26), (20.1, -20), (20, -26)], -23.0)}
EBU_3342 = {   # Tech 3342 table 1, cases 1 to 4: the loudness range, +- 1 LU
    1: ([(20, -20), (20, -30)], 10.0), 2: ([(20, -20), (20, -15)], 5.0), 3: ([(20, -40), (20, -20)], 20.0),
    4: ([(20, -50), (20, -35), (20, -20), (20, -35), (20, -50)], 15.0)}

# y = v (stage 2 inverted by its own poles) and v = x + B (x1 - x2): a constant input makes (x + B x1) - B x2 round
# where x + (B x1 - B x2) is exact; B and the constant were found by search
ORDER = SimpleNamespace(s1_b=[1.0, 4095.3333333333335, -4095.3333333333335], s1_a=[0.0, 0.0], s2_a=[-2.0, 1.0], hop=1,
                        warm=0, abs_gate=0)
