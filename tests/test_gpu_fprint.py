"""Fingerprints on the GPU (bl_amd_fprint_words_device, bl_amd_fprint_match_device, their context and host forms,
bliss_amd.fingerprint): every word, every byte of bl_amd_fprint_match and every value of the profile is compared with ==
against tests/fprint_reference.py.  There is no tolerance anywhere.

The outputs are filled with 0xA5 before the call and carry 16 guard bytes, so a byte the kernels do not write, or one
they write too far, shows.  The words kernel gets crafted frame records, not PCM: frame counts around the 16-frame
window and the 256 words of a workgroup, values at the chroma bound, silence, exact ties, songs too short for a word
between others.  The match gets word counts 0, 1, 2 and w - 1, w, w + 1, 2 w + 1 for the lengths w at which its kernel
changes path (bl_amd_fprint_shape: a lane's strip and a tile), at every max_shift that gives another tiling, and sets
whose songs lie against exact copies of the query, so that a word read from a neighbour wins and shows."""
import ctypes as C

import numpy as np
import pytest

import bliss_amd
import bliss_amd.fingerprint as fp
from bliss_amd import _lib
from bliss_amd.records import FPRINT_MATCH_DTYPE
from tests import fprint_reference as fr

pytestmark = pytest.mark.gpu

U = _lib.BL_UNEXPECTED
SENTINEL, GUARD = 0xA5, 16


def filled(nbytes):
    import torch
    return torch.full((nbytes + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")


def fetch(t, nbytes):
    import torch
    torch.cuda.synchronize()
    raw = t.cpu().numpy()
    assert (raw[nbytes:] == SENTINEL).all(), "written past the end"
    return raw[:nbytes].tobytes()


def untouched(*tensors):
    import torch
    torch.cuda.synchronize()
    return all(t is None or bool((t == SENTINEL).all()) for t in tensors)


def to_device(a):
    import torch
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.uint8).reshape(-1).copy() if a.size else np.zeros(8, np.uint8)).cuda()
    return t


# ---- words -------------------------------------------------------------------------------------------------------

class Words:
    """one device call on the chromagrams `songs`; the words were filled with 0xA5.  `stream`: a torch stream instead of
    the default one; `defer`: the call is made by go() (tests/test_gpu_side_ws.py)"""

    def __init__(self, lib, songs, ctx=None, n=None, n_words=None, counts=None, frames=True, out=True, shift=(0, 0),
                 stream=None, defer=False):
        self.counts = [int(x.shape[0]) for x in songs] if counts is None else counts
        self.total = sum(max(0, t - 15) for t in self.counts if 0 <= t)
        X = np.concatenate([np.asarray(x, np.uint64).reshape(-1, 12) for x in songs] + [np.zeros((1, 12), np.uint64)])
        self.frames = to_device(X)
        self.out = filled(4 * self.total)
        arr = (C.c_int32 * len(self.counts))(*self.counts)
        args = (C.c_void_p(self.frames.data_ptr() + shift[0]) if frames else None, arr,
                len(songs) if n is None else n, C.c_void_p(self.out.data_ptr() + shift[1]) if out else None,
                self.total if n_words is None else n_words)
        self._call = ((lib.bl_amd_fprint_words_device, args) if ctx is None
                      else (lib.bl_amd_ctx_fprint_words_device, (ctx.handle,) + args))
        self.rc = None if defer else self.go(stream)

    def go(self, stream=None):
        fn, args = self._call
        self.rc = fn(*args, None if stream is None else C.c_void_p(stream.cuda_stream))
        return self.rc

    def read(self):
        assert self.rc == 0
        return np.frombuffer(fetch(self.out, 4 * self.total), dtype=np.uint32)


def assert_words(got, songs, what=""):
    want = fr.words_batch(np.concatenate(songs) if songs else np.zeros((0, 12)), [x.shape[0] for x in songs])
    assert got.size == want.size, what
    if not np.array_equal(got, want):
        t = int(np.flatnonzero(got != want)[0])
        raise AssertionError(f"{what}: word {t} is {int(got[t]):#010x}, want {int(want[t]):#010x}; "
                             f"{int((got != want).sum())} of {want.size} differ")


def test_words_at_every_frame_count(gpu_lib):
    block = fp.shape(0)[0]
    counts = [0, 1, 15, 16, 17, 31, 32, 33, block + 14, block + 15, block + 16, 2 * block + 16]
    songs = [fr.random_frames(40 + i, t) for i, t in enumerate(counts)]
    assert_words(Words(gpu_lib, songs).read(), songs, "all lengths in one call")
    for x in songs[3:9]:
        assert_words(Words(gpu_lib, [x]).read(), [x], f"T {x.shape[0]} alone")
    w = Words(gpu_lib, songs[:3])          # no song has a word
    assert w.total == 0 and w.read().size == 0


def test_words_at_the_bound_silence_and_ties(gpu_lib):
    top = np.full((40, 12), fr.X_MAX - 1, dtype=np.int64)
    top[::3, ::2] -= 1
    top[5:, 7] -= 2
    few = fr.random_frames(50, 300, 3)      # values 0 .. 2: ties in every group, and windows of silence
    w = fr.words(few)
    s1 = np.lib.stride_tricks.sliding_window_view(few, 8, axis=0).sum(axis=2)
    assert (s1[:-8] == s1[8:]).any() and ((s1[:-8] + s1[8:])[:, :-1] == (s1[:-8] + s1[8:])[:, 1:]).any()
    assert ((s1[:-8, :8] + s1[8:, 1:9]) == (s1[8:, :8] + s1[:-8, 1:9])).any()
    assert len(set(w.tolist())) > 100
    flat = np.full((20, 12), 9, dtype=np.int64)
    silent = np.zeros((48, 12), dtype=np.int64)
    songs = [top, few, flat, silent, fr.random_frames(51, 64, fr.X_MAX)]
    got = Words(gpu_lib, songs).read()
    assert_words(got, songs, "bound, ties, silence")
    assert not got[25 + 285:25 + 285 + 5 + 33].any()          # the flat and the silent song: every word 0


def test_short_songs_between_others_and_a_loud_neighbour(gpu_lib):
    quiet = np.full((20, 12), 7, dtype=np.int64)
    loud = np.zeros((30, 12), dtype=np.int64)
    loud[:, 0] = fr.X_MAX - 1
    # one frame of the neighbour inside the window would set bits of the quiet song's last word
    assert fr.words(np.concatenate([quiet, loud[:1]])[1:])[-1] != fr.words(quiet)[-1]
    songs = [fr.random_frames(60, 40), fr.random_frames(61, 3), np.zeros((0, 12), np.int64), fr.random_frames(62, 15),
             quiet, loud, fr.random_frames(63, 7), fr.random_frames(64, 300), quiet, fr.random_frames(65, 1)]
    assert_words(Words(gpu_lib, songs).read(), songs, "mixed")
    assert_words(Words(gpu_lib, songs[::-1]).read(), songs[::-1], "mixed, reversed")


def test_words_context_and_host_forms_give_the_same_bytes(gpu_lib):
    songs = [fr.random_frames(70 + i, t) for i, t in enumerate((33, 0, 16, 600, 15, 271))]
    want = Words(gpu_lib, songs).read()
    with bliss_amd.Context(0) as ctx:
        assert Words(gpu_lib, songs, ctx=ctx).read().tobytes() == want.tobytes()
        assert Words(gpu_lib, songs, ctx=ctx).read().tobytes() == want.tobytes()
    words, counts = fp.words_host(np.concatenate(songs), [x.shape[0] for x in songs])
    assert words.tobytes() == want.tobytes() and counts == [18, 0, 1, 585, 0, 256]
    t, counts_d = fp.words_from_frames_device(to_device(np.concatenate(songs).astype(np.uint64)),
                                              [x.shape[0] for x in songs])
    assert counts_d == counts
    assert t.cpu().numpy().view(np.uint32).tobytes() == want.tobytes()


def test_words_rejected_arguments_write_nothing(gpu_lib):
    songs = [fr.random_frames(80, 40), fr.random_frames(81, 20)]
    for kw in (dict(frames=False), dict(out=False), dict(n=0), dict(n=-1), dict(n_words=29), dict(n_words=31),
               dict(counts=[40, -1]), dict(counts=[40, 1 << 20]), dict(shift=(4, 0)), dict(shift=(0, 2))):
        w = Words(gpu_lib, songs, **kw)
        assert w.rc == U and untouched(w.out), kw
    assert_words(Words(gpu_lib, songs).read(), songs, "after the rejections")


# ---- match -------------------------------------------------------------------------------------------------------

class Match:
    """one device call; the records and the profile were filled with 0xA5.  `stream` and `defer` as for Words"""

    def __init__(self, lib, set_a, set_b, pairs, D, mo=1, profile=True, ctx=None, self_form=False, bad=None,
                 stream=None, defer=False):
        self.a, self.b = set_a, set_a if self_form else set_b
        self.pairs, self.D, self.mo = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2), D, mo
        self.n = self.pairs.shape[0]
        self.nd = 2 * min(max(D, 0), 1024) + 1
        self.ca, self.cb = [int(w.size) for w in self.a], [int(w.size) for w in self.b]
        self.wa = to_device(np.concatenate(list(self.a) + [np.zeros(1, np.uint32)]))
        self.wb = self.wa if self_form else to_device(np.concatenate(list(self.b) + [np.zeros(1, np.uint32)]))
        self.dp = to_device(self.pairs)
        self.rec = filled(24 * self.n)
        self.prof = filled(8 * self.n * self.nd) if profile else None
        arg = dict(wa=C.c_void_p(self.wa.data_ptr()), ca=(C.c_int32 * len(self.ca))(*self.ca), na=len(self.ca),
                   wb=C.c_void_p(self.wb.data_ptr()), cb=(C.c_int32 * len(self.cb))(*self.cb), nb=len(self.cb),
                   pairs=C.c_void_p(self.dp.data_ptr()), n=self.n, D=D, mo=mo, rec=C.c_void_p(self.rec.data_ptr()),
                   prof=C.c_void_p(self.prof.data_ptr()) if profile else None)
        for k, v in (bad or {}).items():
            arg[k] = v(self) if callable(v) else v
        args = tuple(arg[k] for k in ("wa", "ca", "na", "wb", "cb", "nb", "pairs", "n", "D", "mo", "rec", "prof"))
        self._call = ((lib.bl_amd_fprint_match_device, args) if ctx is None
                      else (lib.bl_amd_ctx_fprint_match_device, (ctx.handle,) + args))
        self.rc = None if defer else self.go(stream)

    def go(self, stream=None):
        fn, args = self._call
        self.rc = fn(*args, None if stream is None else C.c_void_p(stream.cuda_stream))
        return self.rc

    def read(self):
        assert self.rc == 0
        rec = np.frombuffer(fetch(self.rec, 24 * self.n), dtype=FPRINT_MATCH_DTYPE)
        prof = None if self.prof is None else np.frombuffer(fetch(self.prof, 8 * self.n * self.nd),
                                                            dtype=np.uint32).reshape(self.n, self.nd, 2)
        return rec, prof

    def reference(self):
        cat = [np.concatenate(list(s) + [np.zeros(0, np.uint32)]) for s in (self.a, self.b)]
        return fr.match_batch(cat[0], self.ca, cat[1], self.cb, self.pairs, self.D, self.mo)


def assert_match(m, what=""):
    rec, prof = m.read()
    want, want_prof = m.reference()
    for p in range(m.n):
        where = f"{what} pair {p} {m.pairs[p].tolist()} (D {m.D}, min_overlap {m.mo})"
        if prof is not None and not np.array_equal(prof[p], want_prof[p]):
            j = int(np.flatnonzero((prof[p] != want_prof[p]).any(axis=1))[0])
            raise AssertionError(f"{where}: profile at d = {j - m.D} is {prof[p, j].tolist()}, want "
                                 f"{want_prof[p, j].tolist()}; {int((prof[p] != want_prof[p]).any(axis=1).sum())} differ")
        for f in FPRINT_MATCH_DTYPE.names:
            assert int(rec[f][p]) == int(want[f][p]), f"{where}: {f} {int(rec[f][p])}, want {int(want[f][p])}"
    assert rec.tobytes() == want.tobytes(), what
    return rec


def lengths_for(D):
    _, strip, tile, _ = fp.shape(D)
    out = {0, 1, 2}
    for w in (strip, tile):
        out |= {w - 1, w, w + 1, 2 * w + 1}
    return sorted(out)


def sets_for(D, seed):
    """set a: a random song of every length; set b: for every length a copy of that song with a lead-in of its own,
    a few bits flipped, cut or padded to the same length"""
    a, b = [], []
    for k, n in enumerate(lengths_for(D)):
        w = fr.random_words(seed + k, n)
        lead = (3 * k + 1) % 7
        a.append(w)
        b.append(fr.noisy_copy(np.concatenate([fr.random_words(seed + 100 + k, lead), w])[:n], seed + 200 + k, 1))
    return a, b


@pytest.mark.parametrize("D", [0, 1, 64, 130, 1024])
def test_match_at_every_length_and_shift(gpu_lib, D):
    """max_shift 0 and 1 (one group of offsets, 32 strips), 64 (one chunk, 7 strips), 130 (3 strips; at least Wb for
    the shorter songs) and 1024 (three chunks, one strip), every pair of lengths around a strip and a tile"""
    a, b = sets_for(D, 1000 + D)
    n = len(a)
    assert fp.shape(D)[2] in lengths_for(D) and (D < 130 or any(0 < w.size <= D for w in b))
    pairs = [(i, j) for i in range(n) for j in range(n)] if D >= 64 else \
        [(i, j) for i in range(n) for j in range(n) if abs(i - j) <= 2 or i < 3 or j < 3]
    rec = assert_match(Match(gpu_lib, a, b, pairs, D), f"D {D}")
    same = [p for p, (i, j) in enumerate(pairs) if i == j and a[i].size > 40 and D >= 6]
    assert all(rec["offset"][p] == (3 * pairs[p][0] + 1) % 7 for p in same)   # the lead-in is found


def test_min_overlap_at_and_above_the_largest_overlap(gpu_lib):
    a, b = [fr.random_words(1, 100), fr.random_words(2, 3)], [fr.random_words(3, 80), fr.random_words(4, 100)]
    pairs = [(0, 0), (0, 1), (1, 0), (1, 1)]
    for mo, ok in ((1, [0, 0, 0, 0]), (3, [0, 0, 0, 0]), (4, [0, 0, U, U]), (80, [0, 0, U, U]), (81, [U, 0, U, U]),
                   (100, [U, 0, U, U]), (101, [U, U, U, U]), (2 ** 31 - 1, [U, U, U, U])):
        rec = assert_match(Match(gpu_lib, a, b, pairs, 16, mo), f"min_overlap {mo}")
        assert rec["status"].tolist() == ok, mo


def test_self_form_pairs_in_any_order_and_number(gpu_lib):
    base = fr.random_words(5, 700)
    songs = [base, fr.noisy_copy(base[9:], 6), fr.random_words(7, 449), base[:65].copy(), np.zeros(0, np.uint32),
             fr.random_words(8, 1), fr.noisy_copy(np.concatenate([fr.random_words(9, 30), base]), 10)]
    n = len(songs)
    rng = np.random.default_rng(11)
    pairs = [(i, i) for i in range(n)] + [(0, 1), (1, 0), (0, 6), (6, 0), (0, 1), (0, 1), (-1, 0), (0, -1), (n, 0),
                                          (0, n), (-2 ** 31, 2 ** 31 - 1)]
    pairs += [tuple(int(v) for v in rng.integers(0, n, 2)) for _ in range(300)]
    m = Match(gpu_lib, songs, None, pairs, 64, 8, self_form=True)
    rec = assert_match(m, "self form")
    assert rec["offset"][n] == -9 and rec["offset"][n + 1] == 9 and rec["offset"][n + 2] == 30
    assert rec["status"][n + 6:n + 11].tolist() == [U] * 5 and (rec["score"][n + 6:n + 11] == fr.NO_SCORE).all()
    assert all(rec["errors"][i] == 0 and rec["offset"][i] == 0 for i in range(n) if songs[i].size >= 8)
    want = rec.tobytes()
    # a pair's record does not depend on the other pairs, their order, their number or the profile
    order = rng.permutation(len(pairs))
    got = Match(gpu_lib, songs, None, [pairs[i] for i in order], 64, 8, self_form=True, profile=False).read()[0]
    assert got.tobytes() == rec[order].tobytes()
    for p in (0, n, n + 6, len(pairs) - 1):
        one = Match(gpu_lib, songs, None, [pairs[p]], 64, 8, self_form=True).read()[0]
        assert one.tobytes() == rec[p:p + 1].tobytes(), p
    # the cross form with the set given twice, the context form and the host form: the same bytes
    assert Match(gpu_lib, songs, songs, pairs, 64, 8).read()[0].tobytes() == want
    with bliss_amd.Context(0) as ctx:
        assert Match(gpu_lib, songs, None, pairs, 64, 8, ctx=ctx, self_form=True).read()[0].tobytes() == want
        assert Match(gpu_lib, songs, songs, pairs, 64, 8, ctx=ctx).read()[0].tobytes() == want
    cat, counts = np.concatenate(songs), [w.size for w in songs]
    hrec, hprof = fp.match_host(cat, counts, pairs, 64, 8, profile=True)
    assert hrec.tobytes() == want and hprof.tobytes() == m.read()[1].tobytes()
    hrec, hprof = fp.match_host(cat, counts, pairs, 64, 8, words_b=cat.copy(), counts_b=counts)
    assert hrec.tobytes() == want and hprof is None
    import torch
    wt = torch.from_numpy(cat.view(np.int32)).cuda()
    drec, dprof = fp.match_device(wt, counts, np.array(pairs, dtype=np.int64).astype(np.int32), 64, 8, profile=True)
    torch.cuda.synchronize()
    assert fp.match_to_numpy(drec.cpu().numpy()).tobytes() == want
    assert dprof.cpu().numpy().view(np.uint32).tobytes() == m.read()[1].tobytes()


def test_a_neighbour_that_copies_the_query_does_not_win(gpu_lib):
    """set b holds short songs between exact copies of the query: a word of b read before a song's first or past its
    last is a word of the copy, lines up with the query and brings errors down or the overlap up"""
    q = fr.random_words(21, 300)
    short = [fr.random_words(22, 50), fr.random_words(23, 64), fr.random_words(24, 1), fr.random_words(25, 447)]
    b = [q.copy()]
    for s in short:
        b += [s, q.copy()]
    pairs = [(0, j) for j in range(len(b))]
    for D in (0, 3, 64, 1024):
        m = Match(gpu_lib, [q], b, pairs, D)
        rec = assert_match(m, f"copies around, D {D}")
        assert all(rec["errors"][j] == 0 and rec["offset"][j] == 0 for j in range(0, len(b), 2))
    # one word past the end of a song shorter than the query, read on purpose, changes its profile
    cat, at = np.concatenate(b), np.cumsum([0] + [w.size for w in b])
    for j in (1, 3, 5):
        assert fr.profile(q, cat[at[j]:at[j + 1] + 1], 64) != fr.profile(q, b[j], 64)
    # and on the a side: the query between copies of b's song
    a = [short[1], q.copy(), short[1], q.copy()]
    assert_match(Match(gpu_lib, a, [short[1], q], [(1, 0), (1, 1), (3, 0), (0, 1), (2, 1)], 64), "a side")


def test_match_rejected_arguments_write_nothing(gpu_lib):
    a, b = [fr.random_words(31, 40), fr.random_words(32, 50)], [fr.random_words(33, 60)]
    pairs = [(0, 0), (1, 0)]
    bad = [dict(wa=None), dict(wb=None), dict(ca=None), dict(cb=None), dict(pairs=None), dict(rec=None), dict(na=0),
           dict(nb=0), dict(nb=-1), dict(n=0), dict(n=-3), dict(D=-1), dict(D=1025), dict(mo=0), dict(mo=-1),
           dict(ca=(C.c_int32 * 2)(40, -1)), dict(cb=(C.c_int32 * 1)(1 << 20)),
           dict(wa=lambda m: C.c_void_p(m.wa.data_ptr() + 2)), dict(pairs=lambda m: C.c_void_p(m.dp.data_ptr() + 1)),
           dict(rec=lambda m: C.c_void_p(m.rec.data_ptr() + 2)), dict(prof=lambda m: C.c_void_p(m.prof.data_ptr() + 3))]
    for kw in bad:
        m = Match(gpu_lib, a, b, pairs, 1024 if kw.get("D") == 1025 else 8, bad=kw)
        assert m.rc == U and untouched(m.rec, m.prof), list(kw)
    assert_match(Match(gpu_lib, a, b, pairs, 8), "after the rejections")


def test_profile_ms_names_the_two_kernels(gpu_lib):
    n = C.c_int(-1)
    assert gpu_lib.bl_amd_fprint_profile_ms(b"nothing", C.byref(n)) == -1.0 and n.value == 0
    gpu_lib.bl_amd_profile(1)
    try:
        for name in (b"fprint_words", b"fprint_match"):
            gpu_lib.bl_amd_fprint_profile_ms(name, C.byref(n))
        songs = [fr.random_frames(90, 100)]
        Words(gpu_lib, songs).read()
        Match(gpu_lib, [fr.random_words(91, 100)], None, [(0, 0)], 4, self_form=True).read()
        for name in (b"fprint_words", b"fprint_match"):
            ms = gpu_lib.bl_amd_fprint_profile_ms(name, C.byref(n))
            assert n.value == 1 and 0.0 < ms < 1000.0, name
            assert gpu_lib.bl_amd_fprint_profile_ms(name, C.byref(n)) == 0.0 and n.value == 0
    finally:
        gpu_lib.bl_amd_profile(0)


# ---- end to end ------------------------------------------------------------------------------------------------------

def test_from_pcm_to_same_recording_starts_later(gpu_lib):
    """two melodies and a copy of the first, trimmed by 5 hops and at 0.7 of its level: DeviceCorpus -> words_device ->
    match_device, equal to the reference over the chroma host call's frames, and the copy is found 5 hops early"""
    import torch

    import bliss_amd.chroma as ch
    x, y = fr.melody(1, seconds=12.0), fr.melody(2, seconds=12.0)
    copy = np.round(0.7 * x[5 * fr.HOP:].astype(np.int64)).astype(np.int16)
    pcm = [x, y, copy]
    dc = bliss_amd.DeviceCorpus([p.size for p in pcm], [1, 1, 1], 1)
    for i, p in enumerate(pcm):
        dc.upload(i, p)
    words, counts = fp.words_device(dc)
    pairs = fp.pairs_from_knn(np.array([[1, 2], [0, 2], [0, 1]]))
    rec_t, prof_t = fp.match_device(words, counts, pairs, 32, 50, profile=True)
    torch.cuda.synchronize()
    songs, frames = ch.chroma_batch_host(pcm, 1, frames=True)
    T = [int(t) for t in songs["frames"]]
    want_words = fr.words_batch(frames["x"].astype(np.int64), T)
    assert counts == [t - 15 for t in T] and counts[0] == counts[1] == counts[2] + 5
    assert words.cpu().numpy().view(np.uint32).tobytes() == want_words.tobytes()
    want, want_prof = fr.match_batch(want_words, counts, want_words, counts, pairs, 32, 50)
    rec = fp.match_to_numpy(rec_t.cpu().numpy())
    assert rec.tobytes() == want.tobytes()
    assert prof_t.cpu().numpy().view(np.uint32).tobytes() == want_prof.tobytes()
    hw, hc = fp.from_pcm(pcm, 1)
    assert hw.tobytes() == want_words.tobytes() and hc == counts
    ber, sec = fp.ber(rec), fp.offset_seconds(rec)
    assert rec["offset"][1] == -5 and rec["offset"][4] == 5 and ber[1] < 0.05 and ber[4] < 0.05
    assert abs(sec[4] - 5 * 2048 / 22050) < 1e-12 and ber[0] > 0.4 and ber[3] > 0.4
