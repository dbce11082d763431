"""The call path that the loudness, the true peak, the fingerprints and the song structure share (side_call and the side
workspaces, bliss_amd/csrc/bl_side_ws.h): the pinned ring wrapping with calls in flight on two streams, the record
block growing, workspaces coming and going with their contexts, and bl_amd_loud_profile_ms.  Each test runs once per
feature, on that feature's own helpers and smallest songs (tests/test_gpu_loud.py, test_gpu_tpeak.py, test_gpu_fprint.py,
test_gpu_form.py), and every result is compared with == against that feature's Python reference, as there."""
import ctypes as C

import numpy as np
import pytest

import bliss_amd
import bliss_amd.loudness as ld
from tests import form_reference as form_ref
from tests import fprint_reference as fprint_ref
from tests import loud_reference as lr
from tests import test_gpu_form as t_form
from tests import test_gpu_fprint as t_fprint
from tests import test_gpu_loud as t_loud
from tests import test_gpu_tpeak as t_tpeak

pytestmark = pytest.mark.gpu

PIN_SLOTS = 4   # BL_PIN_SLOTS (bl_runtime.h): the calls that may be in flight before one waits for a pinned block


class Loud:
    """hop 7: the hop counts of test_gpu_loud.HS, mono and stereo"""
    p = lr.plain(t_loud.KW, hop=7, warm=5, abs_gate=7 * 4 * t_loud.GATE)

    def songs(self):
        return t_loud.batch(7)

    def call(self, lib, songs, **kw):
        return t_loud.Call(lib, songs, self.p, **kw)

    def check(self, c, songs, what):
        assert c.rc == 0, what
        t_loud.assert_equal(c.read(), songs, self.p, what)


class TruePeak:
    def songs(self):
        return t_tpeak.small_songs()

    def call(self, lib, songs, **kw):
        return t_tpeak.Call(lib, songs, ceiling=9000, block=7, **kw)

    def check(self, c, songs, what):
        assert c.rc == 0, what
        t_tpeak.assert_equal(c.read(), songs, 9000, 7, what)


class Fingerprint:
    """the words call, at the frame counts around its 16-frame window"""

    def songs(self):
        counts = (33, 0, 16, 17, 15, 40, 32, 1, 31, 64, 20, 48)
        return [fprint_ref.random_frames(40 + i, t) for i, t in enumerate(counts)]

    def call(self, lib, songs, **kw):
        return t_fprint.Words(lib, songs, **kw)

    def check(self, c, songs, what):
        t_fprint.assert_words(c.read(), songs, what)


class Form:
    p = form_ref.params(pool=2, seg=10, min_lag=6, nov=5)

    def songs(self):
        counts = (64, 0, 31, 32, 33, 90, 3, 1, 150, 41, 80, 57)
        return [form_ref.random_frames(200 + i, t, 1 << 37) for i, t in enumerate(counts)]

    def call(self, lib, songs, **kw):
        return t_form.Form(lib, songs, self.p, **kw)

    def check(self, c, songs, what):
        t_form.assert_form(c, what)


FEATURES = [Loud(), TruePeak(), Fingerprint(), Form()]
per_feature = pytest.mark.parametrize("feat", FEATURES, ids=["loud", "tpeak", "fprint", "form"])


@per_feature
def test_ring_wraps_and_hands_over_between_two_streams(gpu_lib, feat):
    """2 * BL_PIN_SLOTS + 1 calls on one context with no host synchronisation between them, on two streams in turn, each
    with another song count and outputs of its own: the pinned ring wraps twice, a block is reused only behind its copy,
    and each call waits on the device for the one before it, which ran on the other stream"""
    import torch
    base = feat.songs()
    sets = [base[k % 3:k % 3 + 2 + k] for k in range(2 * PIN_SLOTS + 1)]
    assert len({len(s) for s in sets}) == len(sets) and len(sets[-1]) == 2 * PIN_SLOTS + 2
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    with bliss_amd.Context(0) as ctx:
        calls = [feat.call(gpu_lib, s, ctx=ctx, defer=True) for s in sets]
        torch.cuda.synchronize()   # the inputs and the 0xA5 of the outputs are in place
        for k, c in enumerate(calls):
            assert c.go(streams[k & 1]) == 0, k
        torch.cuda.synchronize()
        for k, (c, s) in enumerate(zip(calls, sets)):
            feat.check(c, s, f"call {k} of {len(calls)}")


@per_feature
def test_record_blocks_grow_and_are_kept(gpu_lib, feat):
    """one song, then 300: more records than the first pinned block (bytes + bytes / 4 + 4096) and the first device block
    (bytes + bytes / 8 + 4096) hold, whatever the record type; then the one song again, in the blocks that grew"""
    base = feat.songs()
    one = base[5:6]
    many = [base[i % len(base)] for i in range(300)]
    with bliss_amd.Context(0) as ctx:
        for what, songs in (("one song", one), ("300 songs", many), ("one song again", one)):
            feat.check(feat.call(gpu_lib, songs, ctx=ctx), songs, what)


@pytest.mark.parametrize("feat", FEATURES[2:], ids=["fprint", "form"])
def test_the_workspace_goes_with_its_context(gpu_lib, feat):
    """three contexts one after the other, each created, called and destroyed: the workspace of a context is freed with
    it, and a new context (at the same address or not) starts from none"""
    songs = feat.songs()
    for k in range(3):
        with bliss_amd.Context(0) as ctx:
            feat.check(feat.call(gpu_lib, songs, ctx=ctx), songs, f"context {k}")
            feat.check(feat.call(gpu_lib, songs[:5], ctx=ctx), songs[:5], f"context {k} again")
    feat.check(feat.call(gpu_lib, songs), songs, "default context afterwards")


@per_feature
def test_two_contexts_alive_at_once(gpu_lib, feat):
    """calls on two contexts in turn, each with songs of its own, then one context destroyed: the other's workspace is
    its own and still works"""
    base = feat.songs()
    mine = {0: base[:7], 1: base[4:]}
    a, b = bliss_amd.Context(0), bliss_amd.Context(0)
    try:
        for k in range(4):
            ctx, songs = ((a, mine[0]), (b, mine[1]))[k & 1]
            feat.check(feat.call(gpu_lib, songs[k // 2:], ctx=ctx), songs[k // 2:], f"call {k}")
        a.close()
        feat.check(feat.call(gpu_lib, mine[1], ctx=b), mine[1], "the second context after the first was destroyed")
        feat.check(feat.call(gpu_lib, mine[0]), mine[0], "default context")
    finally:
        a.close()
        b.close()


def test_loud_profile_ms(gpu_lib):
    """names, launch counts per kernel, collection on asking, and from_hops running the gate alone"""
    feat, n = FEATURES[0], C.c_int(-1)
    songs = feat.songs()[:6]
    names = (b"loud_filter", b"loud_gate")
    assert gpu_lib.bl_amd_loud_profile_ms(b"nothing", C.byref(n)) == -1.0 and n.value == 0
    n.value = -1
    assert gpu_lib.bl_amd_loud_profile_ms(None, C.byref(n)) == -1.0 and n.value == 0
    gpu_lib.bl_amd_profile(1)
    try:
        for name in names:   # forget what was collected before
            gpu_lib.bl_amd_loud_profile_ms(name, C.byref(n))
        for k in range(2):
            feat.check(feat.call(gpu_lib, songs, hops=bool(k)), songs, f"profiled call {k}")
        for name in names:
            ms = gpu_lib.bl_amd_loud_profile_ms(name, C.byref(n))
            assert n.value == 2 and 0.0 < ms < 1000.0, name
            assert gpu_lib.bl_amd_loud_profile_ms(name, C.byref(n)) == 0.0 and n.value == 0, name
        z = t_loud.reference(songs, feat.p)[1]
        got = ld.from_hops([a.astype(np.int64) for a in z], t_loud.params_of(feat.p))
        assert [lr.rec_ints(got, i) for i in range(len(songs))] == t_loud.reference(songs, feat.p)[0]
        ms = gpu_lib.bl_amd_loud_profile_ms(b"loud_gate", C.byref(n))
        assert n.value == 1 and 0.0 < ms < 1000.0
        assert gpu_lib.bl_amd_loud_profile_ms(b"loud_filter", C.byref(n)) == 0.0 and n.value == 0
    finally:
        gpu_lib.bl_amd_profile(0)
