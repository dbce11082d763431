"""Chord sequences on the GPU (bl_amd_chords_device, its context and host forms, bliss_amd.chords): every byte of
bl_amd_song_chords, of the labels and of the counts is compared with == against tests/chords_reference.py.  There is no
tolerance anywhere.

The outputs are filled with 0xA5 before the call and carry 16 guard bytes, so a byte the kernels do not write, or one
they write too far, shows; a unit of 0x7F bytes follows the input, so a read past the last song's end would show.  The
songs are crafted: lengths around the forward kernel's round and the back-trace's block (bl_amd_chords_shape), odd and
even song counts because the forward kernel has a form in which two songs share a wavefront, a three-letter alphabet so
that ties are the rule, the named input of
every mistake the reference can make, cost tables at both ends of their range, and one song long enough to take the
scores past 2^24."""
import ctypes as C
import functools

import numpy as np
import pytest

import bliss_amd
import bliss_amd.chords as chords
from bliss_amd import _lib
from bliss_amd.records import CHORDS_DTYPE
from tests import chords_reference as cr

pytestmark = pytest.mark.gpu

UNEXPECTED = _lib.BL_UNEXPECTED
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


def to_device(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


def make_params(none, cost, reserved=0, pad=(0, 0, 0)):
    p = _lib.ChordsParams()
    p.none, p.reserved = none, reserved
    p.cost[:] = [int(v) for v in np.asarray(cost).reshape(-1)]
    p.pad[:] = pad
    return p


class Call:
    """one device call over songs (a list of (U, 12) unit arrays); every output was filled with 0xA5"""

    def __init__(self, lib, songs, none, cost, labels=True, hist=True, ctx=None, bad=None, p=None):
        self.songs, self.none, self.cost = songs, none, np.asarray(cost)
        self.n, self.total = len(songs), sum(len(q) for q in songs)
        self.units = to_device(np.concatenate([cr.cat(songs), np.full((1, 16), 0x7F, np.uint8)]))
        self.rec, self.lab, self.hist = filled(32 * self.n), filled(self.total), filled(100 * self.n)
        self.params = make_params(none, cost) if p is None else p
        counts = [len(q) for q in songs]
        ptr = lambda t: C.c_void_p(t.data_ptr())
        arg = dict(u=ptr(self.units), c=(C.c_int32 * max(self.n, 1))(*counts), n=self.n, total=self.total,
                   p=C.byref(self.params), rec=ptr(self.rec), lab=ptr(self.lab) if labels else None,
                   hist=ptr(self.hist) if hist else None)
        for k, v in (bad or {}).items():
            arg[k] = v(self) if callable(v) else v
        args = tuple(arg[k] for k in ("u", "c", "n", "total", "p", "rec", "lab", "hist"))
        if ctx is None:
            self.rc = lib.bl_amd_chords_device(*args, None)
        else:
            self.rc = lib.bl_amd_ctx_chords_device(ctx.handle, *args, None)
        self.with_labels, self.with_hist = labels, hist

    def read(self):
        assert self.rc == 0
        rec = np.frombuffer(fetch(self.rec, 32 * self.n), dtype=CHORDS_DTYPE)
        lab = np.frombuffer(fetch(self.lab, self.total), dtype=np.uint8)
        hist = np.frombuffer(fetch(self.hist, 100 * self.n), dtype=np.uint32).reshape(self.n, 25)
        return rec, lab, hist

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return all(bool((t == SENTINEL).all()) for t in (self.rec, self.lab, self.hist))


def assert_chords(call, want=None, what=""):
    rec, lab, hist = call.read()
    wrec, wlab, whist = want if want is not None else cr.chords_batch(call.songs, call.none, call.cost)
    for i in range(call.n):
        for k in CHORDS_DTYPE.names:
            assert int(rec[k][i]) == int(wrec[k][i]), (f"{what}: song {i} of {len(call.songs[i])} units: {k} "
                                                       f"{int(rec[k][i])}, want {int(wrec[k][i])}; {rec[i]}, want {wrec[i]}")
    assert rec.tobytes() == wrec.tobytes(), what
    if call.with_labels:
        diff = np.nonzero(lab != wlab)[0]
        assert diff.size == 0, f"{what}: {diff.size} labels differ, the first at unit {diff[0]}: {lab[diff[0]]}, want {wlab[diff[0]]}"
    else:
        assert (lab == SENTINEL).all()
    if call.with_hist:
        assert hist.tobytes() == whist.astype(np.uint32).tobytes(), what
    else:
        assert (hist.view(np.uint8) == SENTINEL).all()
    return rec, lab, hist


def shape_lengths():
    step, trace, _ = chords.shape()
    out = {0, 1, 2, 3}
    for edge in (step, 2 * step, trace, 2 * trace):
        out |= {edge - 1, edge, edge + 1}
    return sorted(out)


TABLES = {
    "default": lambda: (150, cr.costs(60, 15)),
    "all_zero": lambda: (150, np.zeros((25, 25), np.int64)),
    "all_1024": lambda: (150, np.full((25, 25), 1024, np.int64)),
    "asymmetric": lambda: (90, cr.asymmetric_cost(7)),
    "none_0": lambda: (0, cr.costs(60, 15)),
    "none_381": lambda: (381, cr.costs(1024, 512)),
}


@functools.lru_cache(maxsize=None)
def length_songs():
    abc = cr.alphabet(11, 3)
    return tuple(cr.letters_song(100 + i, n, abc) for i, n in enumerate(shape_lengths()))


# ---- lengths, tables, ties -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("table", sorted(TABLES))
def test_every_length_around_a_round_and_a_trace_block(gpu_lib, table):
    """one call holds every length (an odd number of songs: where two share a wavefront, the last has one), from a
    three-letter alphabet whose units score the same on many labels"""
    assert chords.shape()[:2] == (4, 256)
    none, cost = TABLES[table]()
    songs = list(length_songs())
    assert len(songs) % 2 == 1 and [len(q) for q in songs] == shape_lengths()
    rec, lab, _ = assert_chords(Call(gpu_lib, songs, none, cost), what=table)
    assert rec["status"].tolist() == [1] + [0] * (len(songs) - 1) and rec["top"][0] == -1
    if table == "none_381":
        assert (lab == 24).all()


@pytest.mark.parametrize("n_songs", [1, 2, 3, 4])
def test_song_counts_that_fill_and_half_fill_a_wavefront(gpu_lib, n_songs):
    abc = cr.alphabet(13, 3)
    lengths = (37, 5, 300, 0)[:n_songs]
    songs = [cr.letters_song(20 + i, n, abc) for i, n in enumerate(lengths)]
    assert_chords(Call(gpu_lib, songs, 150, cr.costs(60, 15)), what=f"{n_songs} songs")
    assert_chords(Call(gpu_lib, songs[::-1], 120, cr.asymmetric_cost(2)), what=f"{n_songs} songs, reversed")


@pytest.mark.parametrize("sw", cr.SWITCHES)
def test_the_input_that_would_show_each_mistake(gpu_lib, sw):
    """the named input of each switch (tests/test_chords_reference_host.py shows that the switch changes its result)"""
    songs, none, cost = cr.switch_inputs()[sw]
    rec, _, _ = assert_chords(Call(gpu_lib, songs, none, cost), what=sw)
    assert (rec["status"] == 0).all()


def test_a_short_song_between_two_copies_of_a_longer_one(gpu_lib):
    """the units behind the short song are a louder chord: a recurrence or a trace that ran over the song's end, or
    started from the song before, would change its score and its last labels"""
    C_, G_ = cr.triad_unit(0, loud=60), cr.triad_unit(7, loud=127)
    long_ = np.stack([G_] * 9 + [C_] * 4)
    short = np.stack([C_] * 5)
    songs = [long_, short, long_]
    rec, lab, _ = assert_chords(Call(gpu_lib, songs, 150, cr.costs(60, 15)), what="between")
    assert rec["score"][1] == 5 * 180 and lab[13:18].tolist() == [0] * 5 and rec[0].tobytes() == rec[2].tobytes()
    bad = cr.chords_batch(songs, 150, cr.costs(60, 15), frozenset(["seed_prev_song"]))
    assert bad[0]["score"][1] != rec["score"][1]


@functools.lru_cache(maxsize=None)
def long_song():
    """70 000 loud units in runs of one to six: the score passes 2^24"""
    rng = np.random.default_rng(17)
    letters = np.stack([cr.triad_unit(k, loud=127, rest=int(r)) for k, r in ((0, 0), (5, 3), (7, 0), (21, 9))])
    runs = rng.integers(1, 7, size=70000)
    which = rng.integers(0, 4, size=70000)
    q = np.repeat(letters[which], runs, axis=0)[:70000]
    return q, cr.chords_batch([q], 150, cr.costs(60, 15))


def test_a_song_whose_scores_pass_two_to_the_24(gpu_lib):
    q, want = long_song()
    assert len(q) == 70000 and want[0]["score"][0] > 1 << 24 and want[0]["changes"][0] > 1000
    assert cr.chords_batch([q[:200]], 150, cr.costs(60, 15))[0]["score"][0] > 1 << 16
    assert_chords(Call(gpu_lib, [q], 150, cr.costs(60, 15)), want, "70 000 units")


# ---- independence, forms, rejection ----------------------------------------------------------------------------------

def test_a_songs_record_does_not_depend_on_its_call(gpu_lib):
    import torch
    abc = cr.alphabet(15, 3)
    songs = [cr.letters_song(40 + i, n, abc) for i, n in enumerate((90, 0, 257, 4, 17, 513, 1))]
    none, cost = 140, cr.costs(80, 30)
    want = cr.chords_batch(songs, none, cost)
    rec, lab, hist = assert_chords(Call(gpu_lib, songs, none, cost), want, "all")
    for labels, hist_ in ((False, False), (True, False), (False, True)):
        assert_chords(Call(gpu_lib, songs, none, cost, labels=labels, hist=hist_), want, f"labels {labels} hist {hist_}")
    back = Call(gpu_lib, songs[::-1], none, cost).read()
    assert back[0][::-1].tobytes() == rec.tobytes() and back[2][::-1].tobytes() == hist.tobytes()
    at = np.cumsum([0] + [len(q) for q in songs])
    for i in (0, 2, 5, 6):
        alone = Call(gpu_lib, [songs[i]], none, cost).read()
        assert alone[0][0].tobytes() == rec[i].tobytes() and alone[1].tobytes() == lab[at[i]:at[i + 1]].tobytes(), i
    with bliss_amd.Context(0) as ctx:
        assert_chords(Call(gpu_lib, songs, none, cost, ctx=ctx), want, "explicit context")
    p = chords.params(none=none, change=80, related=30)
    h = chords.chords_host(cr.cat(songs), [len(q) for q in songs], p, labels=True, hist=True)
    assert h[0].tobytes() == rec.tobytes() and h[1].tobytes() == lab.tobytes() and h[2].tobytes() == hist.tobytes()
    assert chords.chords_host(cr.cat(songs), [len(q) for q in songs], p).tobytes() == rec.tobytes()
    d = chords.chords_device(to_device(cr.cat(songs)), [len(q) for q in songs], p, labels=True, hist=True)
    torch.cuda.synchronize()
    assert chords.chords_to_numpy(d["records"].cpu().numpy()).tobytes() == rec.tobytes()
    assert d["labels"].cpu().numpy().tobytes() == lab.tobytes() and d["hist"].cpu().numpy().tobytes() == hist.tobytes()
    e = chords.chords_host(np.zeros((0, 16), np.uint8), [0, 0], labels=True, hist=True)
    assert e[0]["status"].tolist() == [1, 1] and e[0]["top"].tolist() == [-1, -1] and e[1].size == 0 and not e[2].any()


def test_rejected_arguments_write_nothing(gpu_lib):
    abc = cr.alphabet(19, 3)
    songs = [cr.letters_song(1, 40, abc), cr.letters_song(2, 30, abc)]
    none, cost = 150, cr.costs(60, 15)
    shifted = lambda name, by: (lambda m: C.c_void_p(getattr(m, name).data_ptr() + by))
    bad = [dict(u=None), dict(c=None), dict(p=None), dict(rec=None), dict(n=0), dict(n=-1), dict(total=69), dict(total=71),
           dict(c=(C.c_int32 * 2)(71, -1)), dict(c=(C.c_int32 * 2)(1 << 20, 30)), dict(u=shifted("units", 8)),
           dict(rec=shifted("rec", 2)), dict(hist=shifted("hist", 2))]
    for kw in bad:
        m = Call(gpu_lib, songs, none, cost, bad=kw)
        assert m.rc == UNEXPECTED and m.untouched(), list(kw)
    high = np.array(cost)
    high[24, 24] = 1025
    for p in (make_params(-1, cost), make_params(382, cost), make_params(150, cost, reserved=1),
              make_params(150, cost, pad=(0, 0, 1)), make_params(150, high)):
        m = Call(gpu_lib, songs, none, cost, p=p)
        assert m.rc == UNEXPECTED and m.untouched()
    assert_chords(Call(gpu_lib, songs, none, cost), what="after the rejections")


def test_profile_ms_names_both_kernels(gpu_lib):
    n = C.c_int(-1)
    names = (b"chords_forward", b"chords_trace")
    assert gpu_lib.bl_amd_chords_profile_ms(b"nothing", C.byref(n)) == -1.0 and n.value == 0
    gpu_lib.bl_amd_profile(1)
    try:
        for name in names:
            gpu_lib.bl_amd_chords_profile_ms(name, C.byref(n))
        Call(gpu_lib, [cr.letters_song(1, 100, cr.alphabet(23, 3))], 150, cr.costs()).read()
        for name in names:
            ms = gpu_lib.bl_amd_chords_profile_ms(name, C.byref(n))
            assert n.value == 1 and 0.0 < ms < 1000.0, name
            assert gpu_lib.bl_amd_chords_profile_ms(name, C.byref(n)) == 0.0 and n.value == 0
    finally:
        gpu_lib.bl_amd_profile(0)


# ---- end to end ------------------------------------------------------------------------------------------------------

def test_from_pcm_gives_the_chords_played(gpu_lib):
    """A minor, i-iv-v-i, then silence, then noise (tests/test_chords_reference_host.py has the same on the chroma
    reference's frames): every unit wholly inside a chord gets it, every unit wholly inside silence or noise gets N, and
    the device's labels are the reference's over the device's units"""
    import bliss_amd.cover as cover
    tonic, minor = 9, True
    pcm = cr.progression_pcm(tonic, minor)
    for pool in (1, 2):
        rec, labels, counts = chords.from_pcm([pcm], 1, pool=pool)
        want = cr.progression_want(tonic, minor, pool, counts[0])
        assert all(w < 0 or int(l) == w for l, w in zip(labels, want)), [chords.name(int(l)) for l in labels]
        units, ucounts = cover.from_pcm([pcm], 1, pool)
        assert ucounts == counts and rec["units"][0] == counts[0]
        ref = cr.chords_batch([units[:, :12]], 150, cr.costs(60, 15))
        assert rec.tobytes() == ref[0].tobytes() and labels.tobytes() == ref[1].tobytes()
        played = [chords.name(int(c)) for c in chords.segments([l for l, w in zip(labels, want) if 0 <= w < 24])[1]]
        assert played == ["Am", "Dm", "Em", "Am"]
