"""Song structure on the GPU (bl_amd_form_device, its context and host forms, bliss_amd.form): every byte of
bl_amd_song_form and every element of the four optional outputs (units, rep, novelty, flags) is compared with ==
against tests/form_reference.py.  There is no tolerance anywhere.

The outputs are filled with 0xA5 before the call and carry 16 guard bytes, so a byte the kernels do not write, or one
they write too far, shows.  The kernels get crafted frame records, not PCM: frame counts around a unit, a workgroup of
the units kernel, the thumbnail's smallest song and a chunk of its lags (bl_amd_form_shape), values at the chroma bound,
silence, all-equal songs whose every diagonal ties, and a short song between two exact copies of another, so that a
unit read across a song edge would raise its best diagonal and show."""
import ctypes as C

import numpy as np
import pytest

import bliss_amd
import bliss_amd.form as form
from bliss_amd import _lib
from bliss_amd.records import FORM_DTYPE
from tests import form_reference as fr

pytestmark = pytest.mark.gpu

UNEXPECTED = _lib.BL_UNEXPECTED
SENTINEL, GUARD = 0xA5, 16
OUTS = (("units", 16, np.uint8), ("rep", 8, np.uint32), ("nov", 8, np.uint64), ("flags", 1, np.uint8))
ALL = tuple(name for name, _, _ in OUTS)


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
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


class Form:
    """one device call on the chromagrams `songs`; the records and the outputs were filled with 0xA5.  `stream`: a torch
    stream instead of the default one; `defer`: the call is made by go() (tests/test_gpu_side_ws.py)"""

    def __init__(self, lib, songs, p, outs=ALL, ctx=None, bad=None, stream=None, defer=False):
        self.songs, self.p, self.outs = songs, dict(p), outs
        self.counts = [int(x.shape[0]) for x in songs]
        self.n = sum(t // p["pool"] for t in self.counts) if 1 <= p["pool"] <= 16 else sum(self.counts)
        X = np.concatenate([np.asarray(x, np.uint64).reshape(-1, 12) for x in songs] + [np.zeros((1, 12), np.uint64)])
        self.frames = to_device(X)
        self.rec = filled(48 * len(songs))
        self.out = {name: filled(size * self.n) if name in outs else None for name, size, _ in OUTS}
        self.params = _lib.FormParams(*[p[k] for k in ("pool", "seg", "min_lag", "nov", "peak_num", "peak_den",
                                                       "reserved")])
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        arg = dict(frames=ptr(self.frames), counts=(C.c_int32 * len(self.counts))(*self.counts), n=len(songs),
                   params=C.byref(self.params), rec=ptr(self.rec), n_units=self.n,
                   **{name: ptr(self.out[name]) for name in ALL})
        for k, v in (bad or {}).items():
            arg[k] = v(self) if callable(v) else v
        args = tuple(arg[k] for k in ("frames", "counts", "n", "params", "rec") + ALL + ("n_units",))
        self._call = ((lib.bl_amd_form_device, args) if ctx is None
                      else (lib.bl_amd_ctx_form_device, (ctx.handle,) + args))
        self.rc = None if defer else self.go(stream)

    def go(self, stream=None):
        fn, args = self._call
        self.rc = fn(*args, None if stream is None else C.c_void_p(stream.cuda_stream))
        return self.rc

    def read(self):
        assert self.rc == 0
        rec = np.frombuffer(fetch(self.rec, 48 * len(self.songs)), dtype=FORM_DTYPE)
        out = {}
        for name, size, dt in OUTS:
            if self.out[name] is not None:
                out[name] = np.frombuffer(fetch(self.out[name], size * self.n), dtype=dt)
        return rec, out

    def reference(self):
        X = np.concatenate(list(self.songs) + [np.zeros((0, 12), np.int64)])
        rec, units, rep, nov, flags = fr.form_batch(X, self.counts, self.p)
        return rec, dict(units=units.reshape(-1), rep=rep.reshape(-1), nov=nov, flags=flags)


def assert_form(f, what=""):
    rec, out = f.read()
    want, want_out = f.reference()
    at = np.cumsum([0] + [int(u) for u in want["units"]])
    for name, size, dt in OUTS:
        if name not in out:
            continue
        per = size // np.dtype(dt).itemsize
        g, w = out[name].reshape(-1, per), want_out[name].reshape(-1, per)
        assert g.shape == w.shape, f"{what}: {name}"
        if not np.array_equal(g, w):
            j = int(np.flatnonzero((g != w).any(axis=1))[0])
            i = int(np.searchsorted(at, j, side="right") - 1)
            raise AssertionError(f"{what}: {name} of song {i} (U {int(want['units'][i])}) at unit {j - at[i]} is "
                                 f"{g[j].tolist()}, want {w[j].tolist()}; {int((g != w).any(axis=1).sum())} differ")
    for i in range(len(f.songs)):
        for k in FORM_DTYPE.names:
            assert int(rec[k][i]) == int(want[k][i]), f"{what}: song {i} {k} {int(rec[k][i])}, want {int(want[k][i])}"
    assert rec.tobytes() == want.tobytes(), what
    return rec, out


def equal_song(U, seed=0):
    """U frames, all the same: every unit is the same, every diagonal ties"""
    return np.repeat(fr.random_frames(900 + seed, 1), U, axis=0)


# ---- units -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", [1, 3, 16])
def test_units_at_every_count_and_value(gpu_lib, P):
    """T = 0, T < P, T = P U + remainder around a workgroup of the units kernel; a silent frame, a frame with one
    non-zero class, values near 2^39 (s > 0) and below 2^20 (s = 0)"""
    block = form.shape()[1]
    counts = [0, P - 1, P, 2 * P + P // 2, (block - 1) * P, block * P + P - 1, (block + 1) * P, (2 * block + 1) * P + 1]
    songs = [fr.random_frames(10 + i, t, fr.X_MAX if i % 2 else 1 << 19) for i, t in enumerate(counts)]
    songs[3][:P] = 0                               # a silent unit
    songs[4][2 * P:3 * P] = 0
    songs[4][2 * P:3 * P, 7] = 12345               # one class: q = 127 there
    songs[5][:, :] = fr.X_MAX - 1                  # every class at the bound
    songs[6][P:2 * P] = 0
    songs[6][2 * P - 1, 3] = 1                     # the smallest non-silent unit
    songs[7][:P] = 0
    songs[7][0] = fr.shift_frame()                 # tells a shift by bitlength - 19 from one by bitlength - 20
    p = fr.params(pool=P, seg=8, min_lag=4, nov=4)
    rec, out = assert_form(Form(gpu_lib, songs, p), f"P {P}")
    units = out["units"].reshape(-1, 16)
    at = np.cumsum([0] + rec["units"].tolist())
    assert rec["units"].tolist() == [t // P for t in counts]
    assert not units[at[3]].any() and units[at[4] + 2].tolist() == [0] * 7 + [127] + [0] * 8
    assert units[at[6] + 1].tolist() == [0, 0, 0, 127] + [0] * 12 and not units[:, 12:].any()
    for i in (1, 4, 6):
        assert_form(Form(gpu_lib, [songs[i]], p), f"P {P}, song {i} alone")


def test_unit_count_crosses_a_workgroup_by_one_over_many_songs(gpu_lib):
    """many short songs whose units add up to one more than a workgroup of the units kernel holds, then one more song"""
    block = form.shape()[1]
    songs = [fr.random_frames(40 + i, 2 * 5 + 1) for i in range(block // 5)] + [fr.random_frames(39, 2 * (block % 5 + 1))]
    p = fr.params(pool=2, seg=2, min_lag=1, nov=2)
    assert sum(x.shape[0] // 2 for x in songs) == block + 1
    assert_form(Form(gpu_lib, songs, p), "block + 1 units")
    assert_form(Form(gpu_lib, songs + [fr.random_frames(38, 9)], p), "and one more song")


# ---- thumbnail ---------------------------------------------------------------------------------------------------------

def test_thumbnail_smallest_songs_ties_and_silence(gpu_lib):
    M, lag = 12, 7
    p = fr.params(seg=M, min_lag=lag, nov=3)
    songs = [fr.random_frames(50, M + lag - 1), fr.random_frames(51, M + lag), fr.random_frames(52, M + lag + 1),
             equal_song(90), np.zeros((60, 12), np.int64), fr.random_frames(53, 1), np.zeros((0, 12), np.int64)]
    rec, out = assert_form(Form(gpu_lib, songs, p), "small songs")
    assert rec["status"].tolist() == [fr.NO_THUMB, 0, 0, 0, fr.NO_THUMB, fr.NO_THUMB, fr.NO_THUMB]
    assert (rec["thumb_lag"][1], rec["thumb_start"][1]) == (lag, 0)                    # the one candidate
    assert (rec["thumb_lag"][3], rec["thumb_start"][3]) == (lag, 0)                    # every F ties
    assert rec["thumb_score"][3] == rec["thumb_self"][3] > 0
    assert not rec["thumb_score"][4] and not rec["thumb_self"][4]
    rep = out["rep"].reshape(-1, 2)
    at = np.cumsum([0] + rec["units"].tolist())
    assert not rep[at[0]:at[1]].any() and rep[at[1]].tolist() == [int(rec["thumb_score"][1]), lag]
    assert not rep[at[1] + 1:at[2]].any() and not rep[at[4]:at[5]].any()
    assert (rep[at[3]:at[3] + 90 - M - lag + 1, 1] == lag).all() and not rep[at[3] + 90 - M - lag + 1:at[4]].any()


@pytest.mark.parametrize("extra", [-1, 0, 1])
def test_lag_range_around_a_chunk(gpu_lib, extra):
    """the number of lags, U - M - minlag + 1, one short of, equal to and one past what a workgroup takes at a time"""
    chunk = form.shape()[0]
    M, lag = 5, 3
    U = M + lag + chunk + extra - 1
    p = fr.params(seg=M, min_lag=lag, nov=8)
    songs = [fr.random_frames(60 + extra, U, 1 << 34), equal_song(U, 1)]
    rec, _ = assert_form(Form(gpu_lib, songs, p), f"{chunk + extra} lags")
    assert (rec["thumb_lag"][1], rec["thumb_start"][1]) == (lag, 0)
    # the best pair planted in the last lag, which is the second chunk's only one when extra = 1
    x = fr.random_frames(70, U, 1 << 34)
    x[U - M:] = x[:M]
    rec, _ = assert_form(Form(gpu_lib, [x], p, outs=()), "best at the last lag")
    assert (rec["thumb_lag"][0], rec["thumb_start"][0]) == (U - M, 0) and rec["thumb_score"][0] == rec["thumb_self"][0]


@pytest.mark.parametrize("M", [2, 1024])
def test_shortest_and_longest_segment(gpu_lib, M):
    x = fr.random_frames(80, 2100, 1 << 36)
    x[1500:1500 + 400] = x[100:500]                 # a stretch that comes back 1 400 units later
    rec, _ = assert_form(Form(gpu_lib, [x], fr.params(seg=M, min_lag=M, nov=64)), f"M {M}")
    assert rec["status"][0] == 0 and (M == 1024 or rec["thumb_lag"][0] == 1400)


def test_the_longest_song_and_one_unit_more(gpu_lib):
    """U = 8 192 fills the workgroup's LDS; U = 8 193 is too long: a status bit, zero fields, zero outputs but its units.
    M, minlag and L are the defaults of bliss_amd.form.params."""
    d = form.params()
    p = fr.params(seg=d.seg, min_lag=d.min_lag, nov=d.nov, peak_num=d.peak_num, peak_den=d.peak_den)
    assert (d.pool, d.seg, d.min_lag, d.nov) == (1, 161, 161, 43)
    x = fr.random_frames(81, fr.UNITS_MAX + 1, 1 << 38)
    rec, _ = assert_form(Form(gpu_lib, [x[:fr.UNITS_MAX]], p, outs=("rep", "flags")), "U 8192")
    assert rec["status"][0] == 0 and rec["units"][0] == fr.UNITS_MAX
    rec, out = assert_form(Form(gpu_lib, [x], p), "U 8193")
    assert rec["status"][0] == fr.NO_THUMB | fr.TOO_LONG and rec["units"][0] == fr.UNITS_MAX + 1
    assert out["units"].any() and not out["rep"].any() and not out["nov"].any() and not out["flags"].any()
    short = fr.random_frames(82, 500)
    rec, _ = assert_form(Form(gpu_lib, [short, x, short], p, outs=("nov",)), "too long between others")
    assert rec["status"].tolist() == [0, fr.NO_THUMB | fr.TOO_LONG, 0] and rec[0].tobytes() == rec[2].tobytes()


def test_a_short_song_between_copies_of_another(gpu_lib):
    """the short song's own best diagonal is weak; its last 16 units come back as the first of the next song, so the
    window at start 24 and lag 16, which lies wholly over the song's edge, would meet itself and raise the best F"""
    M, lag = 16, 16
    p = fr.params(seg=M, min_lag=lag, nov=4)
    short = fr.random_frames(84, 40, 1 << 35)
    other = np.concatenate([short[24:], fr.random_frames(83, 284, 1 << 35)])
    songs = [other, short, other]
    X = np.concatenate(songs)
    good, bad = (fr.form_batch(X, [300, 40, 300], p, sw)[0] for sw in (frozenset(), frozenset(["cross_edge"])))
    assert bad["thumb_score"][1] > good["thumb_score"][1] and bad["thumb_score"][1] == bad["thumb_self"][1]
    rec, _ = assert_form(Form(gpu_lib, songs, p), "copies around")
    assert rec[0].tobytes() == rec[2].tobytes()
    assert_form(Form(gpu_lib, songs[1:], p), "copy behind")


def test_aba_song_from_frames(gpu_lib):
    """intro 40 / A 64 / B 80 / A 64 / outro 30: the thumbnail's lag is exactly 144 / P, its start in [40 / P, 56 / P]"""
    x = fr.section_song(3)
    for P in (1, 2, 3):
        p = fr.params(pool=P, seg=48 // P, min_lag=48 // P, nov=16 // P)
        rec, out = assert_form(Form(gpu_lib, [x], p), f"A-B-A, P {P}")
        assert rec["thumb_lag"][0] == 144 // P and 40 / P <= rec["thumb_start"][0] <= 56 / P
        assert form.score(rec)[0] > 0.9


# ---- novelty ---------------------------------------------------------------------------------------------------------

def test_novelty_smallest_songs_and_thresholds(gpu_lib):
    L = 6
    songs = [fr.random_frames(100, 2 * L - 1), fr.random_frames(101, 2 * L), fr.random_frames(102, 2 * L + 1),
             fr.random_frames(103, 200)]
    for num, den in ((1, 4), (0, 1), (256, 256), (255, 256)):
        p = fr.params(seg=4, min_lag=2, nov=L, peak_num=num, peak_den=den)
        rec, out = assert_form(Form(gpu_lib, songs, p), f"threshold {num} / {den}")
        assert rec["boundaries"][0] == 0 and rec["nov_max"][0] == 0 and not out["nov"][:2 * L - 1].any()
        assert rec["boundaries"][1] == 1 and rec["nov_max_unit"][1] == L
        assert np.flatnonzero(out["nov"][2 * L - 1:4 * L - 1]).tolist() == [L]
        if num == den:                             # only units that reach the maximum
            at = 6 * L
            assert (out["nov"][at:][out["flags"][at:] == 1] == rec["nov_max"][3]).all() and rec["boundaries"][3] >= 1
    assert rec["boundaries"][3] < assert_form(Form(gpu_lib, songs, fr.params(seg=4, min_lag=2, nov=L, peak_num=0)),
                                              "every peak")[0]["boundaries"][3]


def test_the_first_unit_of_a_plateau_wins(gpu_lib):
    a, b = fr.random_frames(110, 1, 1 << 33), fr.random_frames(111, 1, 1 << 33)
    x = np.concatenate([np.repeat(a, 5, axis=0), b, np.repeat(a, 5, axis=0)])       # N(5) = N(6) at L = 1
    rec, out = assert_form(Form(gpu_lib, [x], fr.params(seg=2, min_lag=1, nov=1)), "plateau")
    assert out["nov"][5] == out["nov"][6] > 0 and np.flatnonzero(out["flags"]).tolist() == [5]
    assert rec["nov_max_unit"][0] == 5 and rec["boundaries"][0] == 1


def test_homogeneous_sections_give_their_boundaries(gpu_lib):
    x = fr.section_song(3, hold=None)
    for P, L, want in ((1, 16, [40, 104, 184, 248]), (1, 8, [40, 104, 184, 248]), (2, 8, [20, 52, 92, 124])):
        rec, out = assert_form(Form(gpu_lib, [x], fr.params(pool=P, seg=8, min_lag=8, nov=L)), f"P {P}, L {L}")
        assert np.flatnonzero(out["flags"]).tolist() == want and rec["boundaries"][0] == 4
        assert form.sections(out["flags"], int(rec["units"][0])) == list(zip([0] + want, want + [278 // P]))


# ---- independence, forms, rejection ------------------------------------------------------------------------------------

def test_a_song_does_not_depend_on_its_batch_outputs_or_form(gpu_lib):
    p = fr.params(pool=2, seg=10, min_lag=6, nov=5)
    lens = [0, 1, 3, 31, 32, 33, 64, 90, 150, 278, 400, 613, 1100]
    songs = [fr.random_frames(200 + i, lens[i % len(lens)] + i, 1 << 37) for i in range(36)]
    songs.insert(17, fr.section_song(3))
    f = Form(gpu_lib, songs, p)
    rec, out = assert_form(f, "37 songs")
    at = np.cumsum([0] + rec["units"].tolist())
    cut = lambda o, i, name, size: o[name].view(np.uint8)[size * at[i]:size * at[i + 1]].tobytes()
    order = np.random.default_rng(5).permutation(len(songs))
    rec2, out2 = assert_form(Form(gpu_lib, [songs[i] for i in order], p), "37 songs, shuffled")
    at2 = np.cumsum([0] + rec2["units"].tolist())
    for j, i in enumerate(order):
        assert rec2[j].tobytes() == rec[i].tobytes()
        for name, size, _ in OUTS:
            assert out2[name].view(np.uint8)[size * at2[j]:size * at2[j + 1]].tobytes() == cut(out, i, name, size), name
    for i in (17, 35, 0, 9):
        r1, o1 = Form(gpu_lib, [songs[i]], p).read()
        assert r1[0].tobytes() == rec[i].tobytes()
        assert all(o1[name].tobytes() == cut(out, i, name, size) for name, size, _ in OUTS), i
    for outs in ((), ("units",), ("rep",), ("nov",), ("flags",), ("units", "flags"), ("rep", "nov")):
        r, o = Form(gpu_lib, songs, p, outs=outs).read()
        assert r.tobytes() == rec.tobytes(), outs
        assert all(o[name].tobytes() == out[name].tobytes() for name in outs), outs
    with bliss_amd.Context(0) as ctx:
        for outs in (ALL, ()):
            r, o = Form(gpu_lib, songs, p, outs=outs, ctx=ctx).read()
            assert r.tobytes() == rec.tobytes() and all(o[name].tobytes() == out[name].tobytes() for name in outs)
    fp = form.params(pool=2, seg=10, min_lag=6, nov=5)
    X, counts = np.concatenate(songs), [x.shape[0] for x in songs]
    h = form.form_host(X, counts, fp, units=True, rep=True, novelty=True, flags=True)
    assert h["records"].tobytes() == rec.tobytes() and h["units"] == rec["units"].tolist()
    for key, name in (("unit_bytes", "units"), ("rep", "rep"), ("novelty", "nov"), ("flags", "flags")):
        assert h[key].tobytes() == out[name].tobytes(), key
    assert form.form_host(X, counts, fp)["records"].tobytes() == rec.tobytes()
    import torch
    d = form.form_device(to_device(X.astype(np.uint64)), counts, fp, rep=True, flags=True)
    torch.cuda.synchronize()
    assert form.form_to_numpy(d["records"].cpu().numpy()).tobytes() == rec.tobytes()
    assert d["rep"].cpu().numpy().tobytes() == out["rep"].tobytes() and "novelty" not in d
    assert d["flags"].cpu().numpy().tobytes() == out["flags"].tobytes()


def test_rejected_arguments_write_nothing(gpu_lib):
    songs = [fr.random_frames(300, 80), fr.random_frames(301, 41)]
    good = fr.params(pool=2, seg=8, min_lag=4, nov=4)
    shifted = lambda name, by: (lambda f: C.c_void_p((f.frames if name == "frames" else f.rec if name == "rec"
                                                      else f.out[name]).data_ptr() + by))
    bad = [dict(frames=None), dict(counts=None), dict(params=None), dict(rec=None), dict(n=0), dict(n=-1),
           dict(n_units=59), dict(n_units=61), dict(counts=(C.c_int32 * 2)(80, -1)),
           dict(counts=(C.c_int32 * 2)(1 << 20, 41)), dict(frames=shifted("frames", 4)), dict(rec=shifted("rec", 4)),
           dict(units=shifted("units", 8)), dict(rep=shifted("rep", 2)), dict(nov=shifted("nov", 4))]
    for kw in bad:
        f = Form(gpu_lib, songs, good, bad=kw)
        assert f.rc == UNEXPECTED and untouched(f.rec, *f.out.values()), list(kw)
    for kw in (dict(pool=0), dict(pool=17), dict(seg=1), dict(seg=1025), dict(min_lag=0),
               dict(min_lag=fr.UNITS_MAX + 1), dict(nov=0), dict(nov=65), dict(peak_den=0), dict(peak_den=257),
               dict(peak_num=-1), dict(peak_num=5), dict(reserved=1), dict(reserved=-1)):
        f = Form(gpu_lib, songs, dict(good, **kw))
        assert f.rc == UNEXPECTED and untouched(f.rec, *f.out.values()), kw
    assert_form(Form(gpu_lib, songs, good), "after the rejections")
    assert_form(Form(gpu_lib, songs, dict(good, seg=1024, min_lag=fr.UNITS_MAX, nov=64, peak_den=256, peak_num=256)),
                "every parameter at its upper end")


def test_profile_ms_names_the_three_kernels(gpu_lib):
    n = C.c_int(-1)
    names = (b"form_units", b"form_thumb", b"form_novelty")
    assert gpu_lib.bl_amd_form_profile_ms(b"nothing", C.byref(n)) == -1.0 and n.value == 0
    gpu_lib.bl_amd_profile(1)
    try:
        for name in names:
            gpu_lib.bl_amd_form_profile_ms(name, C.byref(n))
        Form(gpu_lib, [fr.random_frames(90, 100)], fr.params(seg=8, min_lag=8, nov=4)).read()
        for name in names:
            ms = gpu_lib.bl_amd_form_profile_ms(name, C.byref(n))
            assert n.value == 1 and 0.0 < ms < 1000.0, name
            assert gpu_lib.bl_amd_form_profile_ms(name, C.byref(n)) == 0.0 and n.value == 0
    finally:
        gpu_lib.bl_amd_profile(0)


# ---- end to end ------------------------------------------------------------------------------------------------------

def test_from_pcm_through_the_chroma_call(gpu_lib):
    """a melody whose first four seconds come back: DeviceCorpus -> chroma frames -> structure, equal to the reference
    over the chroma host call's frames, from the device corpus and from host memory"""
    import torch

    import bliss_amd.chroma as ch
    from tests import fprint_reference as fpr
    a, b = fpr.melody(1, seconds=4.1)[:43 * form.HOP], fpr.melody(2, seconds=5.1)[:54 * form.HOP]
    pcm = [np.concatenate([a, b, a]), fpr.melody(3, seconds=6.0)]      # A comes back 97 hops later, to the sample
    dc = bliss_amd.DeviceCorpus([x.size for x in pcm], [1, 1], 1)
    for i, x in enumerate(pcm):
        dc.upload(i, x)
    fp = form.params(pool=1, seg=30, min_lag=30, nov=10)
    d = form.from_device_corpus(dc, fp, units=True, rep=True, novelty=True, flags=True)
    torch.cuda.synchronize()
    songs, frames = ch.chroma_batch_host(pcm, 1, frames=True)
    T = [int(t) for t in songs["frames"]]
    want = fr.form_batch(frames["x"].astype(np.int64), T, fr.params(seg=30, min_lag=30, nov=10))
    rec = form.form_to_numpy(d["records"].cpu().numpy())
    assert rec.tobytes() == want[0].tobytes() and d["units"] == T
    for key, w in zip(("unit_bytes", "rep", "novelty", "flags"), want[1:]):
        assert d[key].cpu().numpy().tobytes() == w.tobytes(), key
    h = form.from_pcm(pcm, 1, fp, flags=True)
    assert h["records"].tobytes() == rec.tobytes() and h["flags"].tobytes() == want[4].tobytes()
    # the frames inside the second A are those inside the first, so a window of 30 units there scores what it scores
    # against itself, which no other pair of stretches of a melody of random notes comes near
    assert rec["status"][0] == 0 and rec["thumb_lag"][0] == 97 and form.score(rec)[0] > 0.9
    assert abs(form.seconds(97) - 97 * 2048 / 22050) < 1e-12
