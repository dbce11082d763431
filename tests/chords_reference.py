"""CPU reference of the chord sequences (include/bliss_amd.h, the chords block): the definition in numpy int64 and Python
ints, slow and plain.  The GPU tests compare every byte with == against it.

`sw` is a set of SWITCHES: each makes one mistake a kernel could plausibly make, and switch_inputs() names an input on
which that mistake changes the result (tests/test_chords_reference_host.py shows that it does; tests/test_gpu_chords.py
runs the same inputs on the device)."""
import functools
import itertools

import numpy as np

LABELS, NONE, EMPTY = 25, 24, 1
COST_MAX, EMISSION_MAX = 1024, 381
NAMES = ("C", "C#", "D", "D#", "E", "F", "F#", "G", "G#", "A", "A#", "B")

CHORDS_DTYPE = np.dtype([("units", "<i4"), ("status", "<i4"), ("score", "<i4"), ("changes", "<i4"), ("top", "<i4"),
                         ("top_units", "<i4"), ("none_units", "<i4"), ("reserved", "<i4")])

SWITCHES = (
    "minor_as_major",    # 1  a minor third taken as a major third
    "no_fifth",          # 2  the fifth left out
    "rotate_back",       # 3  (r - third) for (r + third)
    "cost_transposed",   # 4  cost[b][a] for cost[a][b]
    "diag_zero",         # 5  the diagonal of cost taken as 0
    "pred_tie_last",     # 6  the predecessor tie goes to the larger a
    "end_tie_last",      # 7  the end tie goes to the larger label
    "v0_transition",     # 8  V_0 charged a transition
    "trace_prev_b",      # 9  the trace reads B_{t-1} for B_t
    "none_silent_only",  # 10 none applied to silent units only
    "changes_count_t0",  # 11 changes counts t = 0
    "top_tie_last",      # 12 the top tie goes to the larger label
    "seed_prev_song",    # 13 a song's V_0 seeded from the previous song's last scores
    "wrap_int16",        # 14 scores wrapped to int16
)


def name(label):
    if label == NONE:
        return "N"
    return NAMES[label % 12] + ("m" if label >= 12 else "") if 0 <= label < 24 else ""


def classes(label):
    r = label % 12
    return {r, (r + (4 if label < 12 else 3)) % 12, (r + 7) % 12}


def costs(change=60, related=15):
    assert 0 <= 2 * related <= change <= COST_MAX
    c = np.zeros((LABELS, LABELS), dtype=np.int64)
    for a in range(LABELS):
        for b in range(LABELS):
            if a != b:
                c[a, b] = change if NONE in (a, b) else change - related * len(classes(a) & classes(b))
    return c


def emissions(q, none, sw=frozenset()):
    """(U, 25) int64 E of units q (U, 12)"""
    q = np.asarray(q, dtype=np.int64).reshape(-1, 12)
    E = np.zeros((q.shape[0], LABELS), dtype=np.int64)
    sign = -1 if "rotate_back" in sw else 1
    for r in range(12):
        for minor in (0, 1):
            third = 4 if (not minor or "minor_as_major" in sw) else 3
            e = q[:, r] + q[:, (r + sign * third) % 12]
            if "no_fifth" not in sw:
                e = e + q[:, (r + 7) % 12]
            E[:, 12 * minor + r] = e
    E[:, NONE] = none
    if "none_silent_only" in sw:
        E[:, NONE] = np.where(q.sum(axis=1) == 0, none, 0)
    return E


def _wrap16(v):
    return ((v + 32768) % 65536) - 32768


def viterbi(E, cost, sw=frozenset(), seed=None):
    """(labels int64 (U,), score, V_{U-1}) of emissions E (U, 25), U >= 1; seed: the scores V_0 is (wrongly) seeded from"""
    E = np.asarray(E, dtype=np.int64)
    C = np.array(cost, dtype=np.int64).reshape(LABELS, LABELS)
    if "cost_transposed" in sw:
        C = C.T.copy()
    if "diag_zero" in sw:
        C[np.arange(LABELS), np.arange(LABELS)] = 0
    U = E.shape[0]
    last_arg = (lambda s: LABELS - 1 - s[::-1].argmax(axis=0)) if "pred_tie_last" in sw else (lambda s: s.argmax(axis=0))
    V = E[0].copy()
    if seed is not None:
        V = V + (np.asarray(seed, dtype=np.int64)[:, None] - C).max(axis=0)
    elif "v0_transition" in sw:
        V = V + (-C).max(axis=0)
    if "wrap_int16" in sw:
        V = _wrap16(V)
    B = np.zeros((U, LABELS), dtype=np.int64)
    for t in range(1, U):
        S = V[:, None] - C                         # S[a][c] = V_{t-1}[a] - cost[a][c]
        B[t] = last_arg(S)
        V = E[t] + S.max(axis=0)
        if "wrap_int16" in sw:
            V = _wrap16(V)
    L = np.zeros(U, dtype=np.int64)
    L[U - 1] = LABELS - 1 - int(V[::-1].argmax()) if "end_tie_last" in sw else int(V.argmax())
    for t in range(U - 1, 0, -1):
        L[t - 1] = B[t - 1][L[t]] if "trace_prev_b" in sw else B[t][L[t]]
    return L, int(V[L[U - 1]]), V


def chords_batch(songs, none, cost, sw=frozenset()):
    """(records CHORDS_DTYPE, labels uint8 concatenated, hist uint32 (n, 25)) of songs: a list of (U, 12) unit arrays"""
    rec = np.zeros(len(songs), dtype=CHORDS_DTYPE)
    hist = np.zeros((len(songs), LABELS), dtype=np.uint32)
    labels, prev_v = [], None
    for i, q in enumerate(songs):
        q = np.asarray(q, dtype=np.int64).reshape(-1, 12)
        U = q.shape[0]
        if U == 0:
            rec[i]["status"], rec[i]["top"] = EMPTY, -1
            continue
        L, score, v = viterbi(emissions(q, none, sw), cost, sw, prev_v if "seed_prev_song" in sw else None)
        prev_v = v
        h = np.bincount(L, minlength=LABELS)
        top = LABELS - 1 - int(h[::-1].argmax()) if "top_tie_last" in sw else int(h.argmax())
        changes = int((L[1:] != L[:-1]).sum()) + (1 if "changes_count_t0" in sw else 0)
        rec[i] = (U, 0, score, changes, top, int(h[top]), int(h[NONE]), 0)
        hist[i] = h
        labels.append(L.astype(np.uint8))
    return rec, (np.concatenate(labels) if labels else np.zeros(0, np.uint8)), hist


def brute_force(E, cost):
    """(labels, score) by trying every label path: the largest score, and among equals the path whose reversed label
    sequence (L_{U-1}, L_{U-2}, .., L_0) is the lexicographically smallest.  That is what the tie rules amount to:
    L_{U-1} is the smallest end of any best path, and B_t[L_t] is the smallest a through which a best path with the
    suffix L_t .. L_{U-1} passes."""
    E = [[int(v) for v in row] for row in np.asarray(E)]
    C = [[int(v) for v in row] for row in np.asarray(cost).reshape(LABELS, LABELS)]
    U = len(E)
    best = None
    for rev in itertools.product(range(LABELS), repeat=U):     # in lexicographic order of the reversed sequence
        path = rev[::-1]
        s = E[0][path[0]] + sum(E[t][path[t]] - C[path[t - 1]][path[t]] for t in range(1, U))
        if best is None or s > best[0]:
            best = (s, path)
    return list(best[1]), best[0]


def segments(labels):
    """(first units, labels) of the runs of equal labels"""
    lab = [int(v) for v in labels]
    starts = [t for t in range(len(lab)) if t == 0 or lab[t] != lab[t - 1]]
    return starts, [lab[t] for t in starts]


def unit_bytes(q):
    """(U, 12) units -> (U, 16) uint8: the twelve values and four zero bytes"""
    q = np.asarray(q, dtype=np.int64).reshape(-1, 12)
    out = np.zeros((q.shape[0], 16), dtype=np.uint8)
    out[:, :12] = q
    return out


def cat(songs):
    return np.concatenate([unit_bytes(q) for q in songs]) if songs else np.zeros((0, 16), np.uint8)


# ---- inputs ------------------------------------------------------------------------------------------------------------

def triad_unit(label, loud=100, rest=0):
    q = np.full(12, rest, dtype=np.int64)
    for k in classes(label):
        q[k] = loud
    return q


def alphabet(seed, n=3):
    """n units that many labels tie on: each has the same value in six classes and zeros elsewhere"""
    rng = np.random.default_rng(seed)
    abc = np.zeros((n, 12), dtype=np.int64)
    for row in abc:
        row[rng.choice(12, size=6, replace=False)] = int(rng.integers(20, 128))
    return abc


def letters_song(seed, n, abc):
    rng = np.random.default_rng(seed)
    return abc[rng.integers(0, len(abc), size=n)] if n else np.zeros((0, 12), np.int64)


def asymmetric_cost(seed):
    """a table that is far from its transpose, with a non-zero diagonal and both ends of the range"""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 200, size=(LABELS, LABELS)).astype(np.int64)
    c[np.triu_indices(LABELS, 1)] += 700
    c[0, 1], c[1, 0], c[3, 3] = COST_MAX, 0, 17
    return c


def switch_inputs():
    """switch -> (songs, none, cost): an input on which the mistake shows in the records or the labels"""
    flat = np.full(12, 50, dtype=np.int64)                         # every label scores 150, N included
    zero = np.zeros((LABELS, LABELS), dtype=np.int64)
    full = np.full((LABELS, LABELS), COST_MAX, dtype=np.int64)
    dflt = costs()
    C, F, G, Cm = triad_unit(0), triad_unit(5), triad_unit(7), triad_unit(12)
    am_c = np.zeros(12, dtype=np.int64)
    am_c[[0, 4, 7, 9]] = (100, 100, 50, 60)                        # Am 260 over C 250; without the fifth C 200 over Am 160
    loud = triad_unit(0, loud=127)
    return {
        "minor_as_major": ([np.stack([Cm] * 3)], 150, dflt),
        "no_fifth": ([np.stack([am_c] * 3)], 150, dflt),
        "rotate_back": ([np.stack([C] * 3)], 150, dflt),
        "cost_transposed": ([np.stack([C, C, G, G, C, F, F, C])], 150, asymmetric_cost(1)),
        "diag_zero": ([np.stack([C] * 4)], 150, full),
        "pred_tie_last": ([np.stack([flat, C])], 150, zero),
        "end_tie_last": ([np.stack([flat])], 150, zero),
        "v0_transition": ([np.stack([C, C])], 150, full),
        "trace_prev_b": ([np.stack([C, C, F, F, G, G])], 150, dflt),
        "none_silent_only": ([np.stack([np.full(12, 40, dtype=np.int64)] * 3)], 150, dflt),
        "changes_count_t0": ([np.stack([C, C, G])], 150, dflt),
        "top_tie_last": ([np.stack([C, C, G, G])], 150, zero),
        "seed_prev_song": ([np.stack([C] * 5), np.stack([G] * 3)], 150, dflt),
        "wrap_int16": ([np.stack([loud] * 100)], 150, dflt),
    }


# ---- the three progressions -------------------------------------------------------------------------------------------

CHORD_FRAMES, SILENCE, NOISE = 32768, 16384, 24576
PROGRESSIONS = ((0, False), (9, True), (6, False))


@functools.lru_cache(maxsize=None)
def progression_pcm(tonic, minor):
    """I-IV-V-I (i-iv-v-i) of 32 768 samples a chord, then 16 384 zero samples, then 24 576 samples of noise"""
    from tests import chroma_reference as ch
    pcm = ch.progression(tonic, minor, chord_frames=CHORD_FRAMES)
    return np.concatenate([pcm, np.zeros(SILENCE, np.int16), ch.noise(5, NOISE, amp=3000)])


@functools.lru_cache(maxsize=None)
def progression_frames(tonic, minor):
    from tests import chroma_reference as ch
    return ch.chromagram(progression_pcm(tonic, minor), 1)


def progression_units(tonic, minor, pool):
    from tests import form_reference as fr
    return np.asarray(fr.units(progression_frames(tonic, minor), pool)).astype(np.int64)


def progression_want(tonic, minor, pool, n_units):
    """per unit: the label it must get, or -1 where its frames straddle two stretches.  Frame t covers samples
    [2048 t, 2048 t + 4096); unit u covers the frames [u pool, u pool + pool)."""
    off = 12 if minor else 0
    played = [off + (tonic + d) % 12 for d in (0, 5, 7, 0)]
    edges = [k * CHORD_FRAMES for k in range(5)] + [4 * CHORD_FRAMES + SILENCE, 4 * CHORD_FRAMES + SILENCE + NOISE]
    stretch = played + [NONE, NONE]
    want = []
    for u in range(n_units):
        lo, hi = 2048 * u * pool, 2048 * (u * pool + pool - 1) + 4096
        inside = [s for s in range(6) if edges[s] <= lo and hi <= edges[s + 1]]
        want.append(stretch[inside[0]] if inside else -1)
    return want
