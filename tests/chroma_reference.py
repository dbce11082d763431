"""Chroma and key of include/bliss_amd.h (bl_amd_song_chroma, bl_amd_frame_chroma) restated in numpy and Python ints:
the table generator op for op in float64 (the same + - * / and floor in the same order as bl_chroma_table.h, the same
literal polynomial coefficients: numpy's elementwise float64 arithmetic is IEEE and fuses nothing), stages 1 to 6 in
int64 and Python ints.  The pitch sums are formed by a float64 matrix product: every product is an integer below
2^23 and every partial sum one below 2^34, so no operation rounds whatever order the BLAS adds in; the result is
converted to int64 and everything after it is integer arithmetic.

The switches make, on purpose, the mistakes a kernel is likely to make: tests/test_chroma_reference_host.py shows that
each of them changes a named song of the corpus tests/test_gpu_chroma.py runs.

    trunc_shift   Re >> 15 rounding towards zero instead of down
    class_p       k(p) = p % 12
    hop4096       frames 4 096 samples apart
    no_128        the constant 128 sum c of the byte split dropped (every sample 128 too low)
    swap_rows     the coefficient rows of pitches p and p + 12 (p < 12) swapped
    tie_last      the key of a tie is the largest index
    s_off         the shift s one too large
"""
import numpy as np

FRAME, HOP, PITCHES, RATE = 4096, 2048, 48, 22050.0
BL_OK, BL_UNEXPECTED = 0, -2
ARENA_FILL = 32767
B = (220.0, 233.081881, 246.941651, 261.625565, 277.182631, 293.664768, 311.126984, 329.627557, 349.228231, 369.994423,
     391.995436, 415.304698)
QM = (10737, -4690, -9, -4315, 3361, 2275, -3604, 6394, -4091, 665, -4465, -2256)
Qm = (10733, -4215, -775, 6842, -4542, -734, -4788, 4262, 1109, -4174, -1512, -2208)
NAMES = ("C", "C#", "D", "D#", "E", "F", "F#", "G", "G#", "A", "A#", "B")
MISTAKES = ("trunc_shift", "class_p", "hop4096", "no_128", "swap_rows", "tie_last", "s_off")


# ---- stage 0: the table ------------------------------------------------------------------------------------------

def cossin(t):
    """(cos, sin) of 2 pi t for float64 t in [0, 1]: bl_chroma_cossin op for op"""
    t = np.asarray(t, dtype=np.float64)
    k = np.floor(4.0 * t + 0.5)
    x = 6.283185307179586 * (t - 0.25 * k)
    z = x * x
    ps = np.full_like(x, 1.6059043836821613e-10)
    ps = ps * z - 2.505210838544172e-08
    ps = ps * z + 2.7557319223985893e-06
    ps = ps * z - 0.0001984126984126984
    ps = ps * z + 0.008333333333333333
    ps = ps * z - 0.16666666666666666
    ps = ps * z + 1.0
    ps = ps * x
    pc = np.full_like(x, 2.08767569878681e-09)
    pc = pc * z - 2.755731922398589e-07
    pc = pc * z + 2.48015873015873e-05
    pc = pc * z - 0.001388888888888889
    pc = pc * z + 0.041666666666666664
    pc = pc * z - 0.5
    pc = pc * z + 1.0
    q = k.astype(np.int64) & 3
    c = np.choose(q, [pc, -ps, -pc, ps])
    s = np.choose(q, [ps, pc, -ps, -pc])
    return c, s


def freq(p):
    return B[p % 12] * float(1 << (p // 12))


def length(p):
    return 2 * int(np.floor(374850.0 / freq(p)))


def gain(p):
    return (65536 * length(PITCHES - 1) ** 2) // (length(p) ** 2)


def pitch_class(p, class_p=False):
    return p % 12 if class_p else (p + 9) % 12


def entries(p):
    """the unquantised row p over its window: (127 w cos, 127 w sin, t) as float64 arrays of L_p values"""
    L = length(p)
    n = np.arange(L, dtype=np.float64)
    c, _ = cossin((n + 0.5) / float(L))
    w = 0.5 - 0.5 * c
    t = freq(p) * ((n - float(L // 2)) + 0.5) / RATE
    t = t - np.floor(t)
    c, s = cossin(t)
    return 127.0 * w * c, 127.0 * w * s, t


_TABLE = None


def table():
    """(re, im, gain, len): int8 (48, 4096) twice, uint32 (48,), int32 (48,); built once"""
    global _TABLE
    if _TABLE is None:
        re, im = np.zeros((PITCHES, FRAME), np.int8), np.zeros((PITCHES, FRAME), np.int8)
        for p in range(PITCHES):
            L = length(p)
            n0 = (FRAME - L) // 2
            a, b, _ = entries(p)
            re[p, n0:n0 + L] = np.floor(a + 0.5).astype(np.int8)
            im[p, n0:n0 + L] = np.floor(b + 0.5).astype(np.int8)
        _TABLE = (re, im, np.array([gain(p) for p in range(PITCHES)], np.uint32),
                  np.array([length(p) for p in range(PITCHES)], np.int32))
    return _TABLE


# ---- stages 1 to 6 -----------------------------------------------------------------------------------------------

def frames_of(n_samples, channels):
    fr = n_samples // channels
    return 0 if fr < FRAME else (fr - FRAME) // HOP + 1


def mix(pcm, channels):
    """m over the song's whole frames of the PCM, int64"""
    fr = pcm.size // channels
    x = np.asarray(pcm[:fr * channels], dtype=np.int64)
    return x[0::2] + x[1::2] if channels == 2 else 2 * x


def pitch_sums(pcm, channels, hop4096=False, no_128=False, swap_rows=False):
    """(Re, Im) int64 arrays of shape (T, 48)"""
    m = mix(pcm, channels)
    if no_128:
        m = m - 256
    hop = FRAME if hop4096 else HOP
    T = 0 if m.size < FRAME else (m.size - FRAME) // hop + 1
    if T == 0:
        return np.zeros((0, PITCHES), np.int64), np.zeros((0, PITCHES), np.int64)
    fr = np.lib.stride_tricks.sliding_window_view(m, FRAME)[::hop][:T].astype(np.float64)
    re, im, _, _ = table()
    if swap_rows:
        order = list(range(12, 24)) + list(range(0, 12)) + list(range(24, PITCHES))
        re, im = re[order], im[order]
    Re, Im = fr @ re.T.astype(np.float64), fr @ im.T.astype(np.float64)
    assert np.abs(Re).max() < 2.0 ** 34 and np.abs(Im).max() < 2.0 ** 34
    return Re.astype(np.int64), Im.astype(np.int64)


def chromagram(pcm, channels, trunc_shift=False, class_p=False, **kw):
    """X: int64 (T, 12), stages 1 to 4"""
    Re, Im = pitch_sums(pcm, channels, **kw)
    if trunc_shift:
        a, b = np.sign(Re) * (np.abs(Re) >> 15), np.sign(Im) * (np.abs(Im) >> 15)
    else:
        a, b = Re >> 15, Im >> 15
    e = a * a + b * b                                   # < 2^37.2
    G = table()[2].astype(np.int64)
    E = (e * G[None, :]) >> 16                          # e G < 2^53.2
    X = np.zeros((Re.shape[0], 12), np.int64)
    for p in range(PITCHES):
        X[:, pitch_class(p, class_p)] += E[:, p]
    return X


def key_of(chroma, tie_last=False, s_off=False):
    """(key, score, score_next) of twelve Python ints, stage 6"""
    mx = max(chroma)
    if mx == 0:
        return -1, 0, 0
    s = max(0, mx.bit_length() - 12) + (1 if s_off else 0)
    c = [v >> s for v in chroma]
    score = [sum(QM[j] * c[(j + k) % 12] for j in range(12)) for k in range(12)]
    score += [sum(Qm[j] * c[(j + k) % 12] for j in range(12)) for k in range(12)]
    best = max(score)
    at = [k for k in range(24) if score[k] == best]
    key = at[-1] if tie_last else at[0]
    return key, best, max(score[k] for k in range(24) if k != key)


def song(pcm, channels, **kw):
    """(record as a dict of Python ints with `chroma` a list, X) of one song"""
    kk = {k: kw.pop(k) for k in ("tie_last", "s_off") if k in kw}
    X = chromagram(pcm, channels, **kw)
    T = X.shape[0]
    if T == 0:
        return dict(chroma=[0] * 12, score=0, score_next=0, frames=0, key=-1, status=BL_UNEXPECTED, reserved=0), X
    chroma = [int(v) for v in X.sum(axis=0)]
    key, score, nxt = key_of(chroma, **kk)
    return dict(chroma=chroma, score=score, score_next=nxt, frames=T, key=key, status=BL_OK, reserved=0), X


def key_name(key):
    return NAMES[key % 12] + ("m" if key >= 12 else "") if 0 <= key <= 23 else ""


# ---- songs -------------------------------------------------------------------------------------------------------

def dual_mono(pcm):
    return np.repeat(np.asarray(pcm, np.int16), 2)


def noise(seed, n, amp=32767):
    rng = np.random.default_rng(seed)
    return rng.integers(-amp - (1 if amp == 32767 else 0), amp + 1, size=n, dtype=np.int64).astype(np.int16)


def tone(freqs, frames, amp=8000.0, harmonics=1, phase=0.0):
    """mono int16 song of `frames` frames: the sum of the given frequencies, each with `harmonics` partials of falling
    weight 1, 1/2, 1/3 ..; the whole scaled so that the largest partial sum of weights has amplitude `amp`"""
    t = np.arange(frames, dtype=np.float64) / RATE
    x = np.zeros(frames)
    for f in freqs:
        for h in range(1, harmonics + 1):
            x += np.sin(2.0 * np.pi * f * h * t + phase) / h
    return np.round(amp * x / max(1, len(freqs))).astype(np.int16)


def triad(root_pitch, minor):
    """frequencies of the triad on pitch index `root_pitch` (0 = A3; may exceed 47: equal temperament from 220 Hz)"""
    return [220.0 * 2.0 ** ((root_pitch + d) / 12.0) for d in (0, 3 if minor else 4, 7)]


def progression(tonic_class, minor, chord_frames=8192):
    """I-IV-V-I (or i-iv-v-i) in the key with tonic pitch class `tonic_class` (C = 0), four harmonics per note, mono"""
    root = (tonic_class - 9) % 12 + 12          # pitch index of the tonic in the octave from A4
    parts = [tone(triad(root + d, minor), chord_frames, harmonics=4) for d in (0, 5, 7, 0)]
    return np.concatenate(parts)


SHAPES_T = (1, 2, 3, 15, 16, 17, 31, 32, 33)
TONES = (0, 13, 30, 47)
TIE = dict(seed=None, amp=None)   # filled by tie_song()


def frames_len(T, extra=0):
    """mono samples of a song of T frames plus `extra` samples that belong to no frame"""
    return FRAME + HOP * (T - 1) + extra


def tie_song():
    """A mono song of one frame whose chroma scores an exact tie between two keys, found by a search over seeded
    low-level noise through this reference (the first hit of a fixed sequence, so it is the same song every time)."""
    for amp in (3, 4, 5, 6, 8, 10, 12):
        for seed in range(400):
            pcm = noise(7000 + seed, FRAME, amp)
            rec, _ = song(pcm, 1)
            if rec["key"] >= 0 and rec["score"] == rec["score_next"]:
                TIE.update(seed=7000 + seed, amp=amp)
                return pcm
    raise AssertionError("no tie found")


_CORPUS = None


def corpus():
    """name -> (int16 PCM, channels): every shape and content tests/test_gpu_chroma.py runs; built once"""
    global _CORPUS
    if _CORPUS is not None:
        return _CORPUS
    c = {}
    c["short_Fr1_1ch"] = (noise(1, 1), 1)
    c["short_Fr1_2ch"] = (noise(2, 3), 2)                       # odd n_samples: one frame of PCM and a stray sample
    c["short_Fr4095_1ch"] = (noise(3, 4095), 1)
    c["short_Fr4095_2ch"] = (noise(4, 2 * 4095 + 1), 2)
    for i, T in enumerate(SHAPES_T):
        c[f"noise_T{T}_1ch"] = (noise(10 + i, frames_len(T, extra=(0, 1, 2047, 700)[i % 4])), 1)
        c[f"noise_T{T}_2ch"] = (noise(30 + i, 2 * frames_len(T, extra=(2047, 0, 1, 333)[i % 4]) + (i & 1)), 2)
    c["noise_T70_1ch"] = (noise(50, frames_len(70, extra=1000)), 1)
    c["noise_T71_2ch"] = (noise(51, 2 * frames_len(71, extra=5) + 1), 2)
    c["all_min_stereo"] = (np.full(2 * frames_len(3), -32768, np.int16), 2)
    c["all_max_stereo"] = (np.full(2 * frames_len(2), 32767, np.int16), 2)
    c["all_max_mono"] = (np.full(frames_len(2), 32767, np.int16), 1)
    c["silence"] = (np.zeros(frames_len(3), np.int16), 1)
    alt = np.ones(frames_len(2), np.int16)
    alt[1::2] = -1
    c["alternating"] = (alt, 1)
    for p in TONES:
        c[f"tone_{p}"] = (tone([freq(p)], frames_len(3), amp=12000.0), 1)
    c["tone_13_dual"] = (dual_mono(c["tone_13"][0]), 2)
    c["noise_T3_dual"] = (dual_mono(c["noise_T3_1ch"][0]), 2)
    c["c_major"] = (progression(0, False, 6144), 1)
    c["a_minor"] = (progression(9, True, 6144), 1)
    c["tie"] = (tie_song(), 1)
    _CORPUS = c
    return c
