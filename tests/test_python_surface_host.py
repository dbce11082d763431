"""The Python layer as a caller sees it, without a device: the public names and their signatures, the record dtypes
against the ctypes structures, what the wrappers accept as an integer argument, which C entry point each host wrapper
reaches, and the readers that work on records alone.

SURFACE was printed by these lines and pasted in; a change of the public surface shows as a difference from it:

    import ctypes, inspect, pprint
    import bliss_amd
    table = {}
    for name in sorted(bliss_amd.__all__):
        obj = getattr(bliss_amd, name)
        if inspect.isclass(obj) and not issubclass(obj, ctypes.Structure):
            table[name] = str(inspect.signature(obj))
            for m, f in sorted(vars(obj).items()):
                if not m.startswith("_"):
                    table[f"{name}.{m}"] = "property" if isinstance(f, property) else str(inspect.signature(f))
        else:
            table[name] = str(inspect.signature(obj)) if inspect.isfunction(obj) else None
    pprint.pprint(table, width=120)
"""
import ctypes as C
import inspect
import math
import re

import numpy as np
import pytest

import bliss_amd
from bliss_amd import _lib
from bliss_amd.batch import LEVELS_DTYPE, RESULT_DTYPE, TIMBRE_FRAME_DTYPE, TIMBRE_SONG_DTYPE

SURFACE = {
    'BL_CALM': None,
    'BL_LOUD': None,
    'BL_OK': None,
    'BL_UNEXPECTED': None,
    'BL_UNKNOWN': None,
    'BlSong': None,
    'Context': '(device=0)',
    'Context.analyze_batch_host': '(self, pcm_list, channels, durations)',
    'Context.close': '(self)',
    'DeviceCorpus': "(lengths, channels, durations, device='cuda:0')",
    'DeviceCorpus.analyze': '(self, ctx=None)',
    'DeviceCorpus.fetch': '(self)',
    'DeviceCorpus.fetch_levels': '(self)',
    'DeviceCorpus.fetch_timbre': '(self)',
    'DeviceCorpus.force_vectors': '(self)',
    'DeviceCorpus.levels': '(self, silence=0, ctx=None)',
    'DeviceCorpus.pcm_bytes': 'property',
    'DeviceCorpus.synth': '(self, seed_base, sample_rate)',
    'DeviceCorpus.timbre': '(self, pct=85, min_energy=0, frames=True, ctx=None)',
    'DeviceCorpus.upload': '(self, index, pcm_int16)',
    'DeviceCorpus.upload_s32': '(self, index, pcm_int32)',
    'EnvelopeResult': None,
    'ForceVector': None,
    'FrameTimbre': None,
    'SongDesc': None,
    'SongLevels': None,
    'SongResult': None,
    'SongTimbre': None,
    '_lib': None,
    'analyze_batch_host': '(pcm_list, channels, durations)',
    'analyze_batch_host_rate': '(pcm_list, channels, durations, sample_rate)',
    'analyze_batch_host_s32': '(pcm_list, channels, durations)',
    'analyze_corpus_multi': "(pcm_list, channels, durations, devices, gather='rccl', matrix=True)",
    'analyze_corpus_multi_device': "(corpora, gather='rccl', matrix=True, keep_rows=False)",
    'analyze_files': '(filenames, n_threads=0, keep_pcm=False)',
    'bl_song': '(filename=None, initializer=None, c_struct=None)',
    'bl_song.amplitude_analysis': '(self)',
    'bl_song.analyze': '(self, filename)',
    'bl_song.decode': '(self, filename)',
    'bl_song.envelope_analysis': '(self)',
    'bl_song.free': '(self)',
    'bl_song.frequency_analysis': '(self)',
    'bl_song.get': '(self, key)',
    'bl_song.set': '(self, key, value)',
    'chain': "(vecs, seeds, length, metric='distance')",
    'chain_device': "(d_vecs, d_seeds, length, metric='distance', stream=None)",
    'cosine_matrix': '(vecs)',
    'distance': None,
    'distance_matrix': '(vecs)',
    'duplicate_groups': "(vecs, r, metric='distance')",
    'duplicate_groups_device': "(d_vecs, r, metric='distance', stream=None)",
    'gapless_links': '(levels)',
    'knn': "(vecs, k, metric='distance')",
    'knn_cross': "(queries, vecs, k, metric='distance')",
    'knn_cross_device': "(d_queries, d_vecs, k, metric='distance', stream=None)",
    'knn_device': "(d_vecs, k, metric='distance', row_begin=0, n_rows=None, stream=None)",
    'last_freq_stats': '()',
    'levels_batch_host': '(pcm_list, channels, silence=0)',
    'levels_db': '(levels)',
    'levels_to_numpy': '(raw)',
    'load': '()',
    'mix': "(vecs, seeds, length, metric='distance', tags=None, gap=0, exclude=None, seed_vecs=None)",
    'mix_device': "(d_vecs, d_seeds, length, metric='distance', tags=None, gap=0, exclude=None, seed_vecs=None, "
                  'stream=None)',
    'playlist': '(vecs, seed_index)',
    'playlist_vec': '(vecs, seed_vec)',
    'radius': "(vecs, r, metric='distance')",
    'radius_cross': "(queries, vecs, r, metric='distance')",
    'radius_cross_device': "(d_queries, d_vecs, r, metric='distance', values=True, stream=None)",
    'radius_device': "(d_vecs, r, metric='distance', row_begin=0, n_rows=None, values=True, stream=None)",
    'resample_batch_device': '(d_in, frames, channels, in_rate, stream=None)',
    'resample_host': '(pcm, channels, in_rate)',
    'results_to_numpy': '(raw_bytes)',
    'tail_from_envelope': '(n_samples, durations, envelopes)',
    'timbre_batch_host': '(pcm_list, channels, pct=85, min_energy=0, frames=True)',
    'timbre_hz': '(songs, rate=22050)',
    'timbre_to_numpy': '(raw_songs, raw_frames=None)',
    'version': None,
}


# ---- 1. surface

def test_all_holds_the_same_names_once():
    assert len(bliss_amd.__all__) == len(set(bliss_amd.__all__))
    assert set(bliss_amd.__all__) == {name for name in SURFACE if "." not in name}


def test_signatures():
    got = {}
    for name in bliss_amd.__all__:
        obj = getattr(bliss_amd, name)
        if inspect.isclass(obj) and not issubclass(obj, C.Structure):
            got[name] = str(inspect.signature(obj))
            for m, f in vars(obj).items():
                if not m.startswith("_"):
                    got[f"{name}.{m}"] = "property" if isinstance(f, property) else str(inspect.signature(f))
        else:
            got[name] = str(inspect.signature(obj)) if inspect.isfunction(obj) else None
    assert got == SURFACE


# ---- 2. records

def struct_layout(struct, flatten=()):
    """[(name, offset, numpy dtype)] of a ctypes structure's fields; a member named in `flatten` is replaced by its own
    fields at its offset"""
    out = []
    for name, ctype in struct._fields_:
        off = getattr(struct, name).offset
        if name in flatten:
            out += [(sub, off + o, dt) for sub, o, dt in struct_layout(ctype)]
        else:
            out.append((name, off, np.dtype(ctype)))
    return out


def dtype_layout(dtype):
    return [(name, dtype.fields[name][1], dtype.fields[name][0]) for name in dtype.names]


RECORDS = [(RESULT_DTYPE, _lib.SongResult, ("v",)), (LEVELS_DTYPE, _lib.SongLevels, ()),
           (TIMBRE_SONG_DTYPE, _lib.SongTimbre, ()), (TIMBRE_FRAME_DTYPE, _lib.FrameTimbre, ())]


@pytest.mark.parametrize("dtype, struct, flatten", RECORDS, ids=[s.__name__ for _, s, _ in RECORDS])
def test_record_dtypes_have_the_fields_of_their_structures(dtype, struct, flatten):
    assert dtype_layout(dtype) == struct_layout(struct, flatten)
    assert dtype.itemsize == C.sizeof(struct)


def test_the_force_vector_leads_the_result_record():
    """DeviceCorpus.force_vectors() reads the first 16 bytes of a record as four floats"""
    assert struct_layout(_lib.SongResult, ("v",))[:4] == [(k, 4 * i, np.dtype("<f4")) for i, k in enumerate(
        ("tempo", "amplitude", "frequency", "attack"))]


# ---- 3. integer arguments

V = np.zeros((10, 4), dtype=np.float32)
PCM = [np.zeros(1024, dtype=np.int16)]   # one frame of 512 per channel, also as stereo
TAGS = np.arange(10, dtype=np.int32)


def _t(a):
    return pytest.importorskip("torch").from_numpy(a)   # a CPU tensor: the checks come before anything touches a device


# (function, argument) -> (lo, hi or None for no upper bound, the call with the argument's value).  `length` has no
# upper bound in Python: what does not fit the C int is the library's to refuse.
INT_ARGS = {
    ("knn", "k"): (1, _lib.BL_AMD_KNN_MAX_K, lambda x: bliss_amd.knn(V, x)),
    ("knn_cross", "k"): (1, _lib.BL_AMD_KNN_MAX_K, lambda x: bliss_amd.knn_cross(V[:2], V, x)),
    ("chain", "length"): (1, None, lambda x: bliss_amd.chain(V, 0, x)),
    ("mix", "length"): (1, None, lambda x: bliss_amd.mix(V, 0, x)),
    ("mix", "gap"): (0, _lib.BL_AMD_MIX_MAX_GAP, lambda x: bliss_amd.mix(V, 0, 3, tags=TAGS, gap=x)),
    ("timbre_batch_host", "pct"): (1, 100, lambda x: bliss_amd.timbre_batch_host(PCM, 1, pct=x)),
    ("timbre_batch_host", "min_energy"): (0, 2 ** 64 - 1, lambda x: bliss_amd.timbre_batch_host(PCM, 1, min_energy=x)),
    ("levels_batch_host", "silence"): (0, 32767, lambda x: bliss_amd.levels_batch_host(PCM, 1, silence=x)),
    ("levels_batch_host", "channels"): (1, 2, lambda x: bliss_amd.levels_batch_host(PCM, [x])),
    ("timbre_batch_host", "channels"): (1, 2, lambda x: bliss_amd.timbre_batch_host(PCM, [x])),
}
# the device forms of the same arguments: a CPU tensor gets as far as the integer checks and no further
DEVICE_INT_ARGS = {
    ("knn_device", "k"): (1, _lib.BL_AMD_KNN_MAX_K, lambda x: bliss_amd.knn_device(_t(V), x)),
    ("knn_cross_device", "k"): (1, _lib.BL_AMD_KNN_MAX_K, lambda x: bliss_amd.knn_cross_device(_t(V[:2]), _t(V), x)),
    ("chain_device", "length"): (1, None, lambda x: bliss_amd.chain_device(_t(V), 0, x)),
    ("mix_device", "length"): (1, None, lambda x: bliss_amd.mix_device(_t(V), 0, x)),
    ("mix_device", "gap"): (0, _lib.BL_AMD_MIX_MAX_GAP, lambda x: bliss_amd.mix_device(_t(V), 0, 3, tags=_t(TAGS), gap=x)),
}
ALL_INT_ARGS = {**INT_ARGS, **DEVICE_INT_ARGS}
NOT_AN_INTEGER = [True, 2.0, np.float32(2), "2", None]


def _refused(key, value):
    with pytest.raises(ValueError) as e:
        ALL_INT_ARGS[key][2](value)
    assert str(e.value).startswith(f"{key[1]} must be") and repr(value) in str(e.value), str(e.value)


@pytest.mark.parametrize("key", list(ALL_INT_ARGS), ids=".".join)
@pytest.mark.parametrize("value", NOT_AN_INTEGER, ids=repr)
def test_what_is_not_an_integer_is_refused(key, value):
    _refused(key, value)


@pytest.mark.parametrize("key", list(ALL_INT_ARGS), ids=".".join)
def test_integers_outside_the_range_are_refused(key):
    lo, hi, _ = ALL_INT_ARGS[key]
    _refused(key, lo - 1)
    _refused(key, np.int64(lo - 1))
    if hi is not None:
        _refused(key, hi + 1)


def test_one_channel_count_for_all_songs_that_is_none_is_a_type_error():
    """As found: None is no numpy scalar, so the broadcast takes it for the per-song sequence and list(None) raises
    before the check of each song's count sees it.  [None] is refused like every other non-integer (above)."""
    for fn in (bliss_amd.levels_batch_host, bliss_amd.timbre_batch_host):
        with pytest.raises(TypeError):
            fn(PCM, None)


@pytest.mark.parametrize("key", list(INT_ARGS), ids=".".join)
@pytest.mark.parametrize("kind", [np.int32, np.int64])
def test_numpy_integers_inside_the_range_pass_the_python_checks(key, kind):
    """No ValueError.  Without a device the library then refuses, which shows as a RuntimeError; with one the call
    returns."""
    lo, hi, call = INT_ARGS[key]
    for x in {lo, lo + 1, min(hi, 2 ** 31 - 1) if hi is not None else lo + 2}:
        try:
            call(kind(x))
        except RuntimeError as e:
            assert "bl_amd_" in str(e)


# ---- 4. the entry point each host wrapper reaches

def _songs(dtype=np.int16):
    return [np.zeros(n, dtype=dtype) for n in (6000, 7000, 8000)]


ENTRY_POINTS = [
    ("bl_amd_knn_host", lambda: bliss_amd.knn(V, 3)),
    ("bl_amd_cross_knn_host", lambda: bliss_amd.knn_cross(V[:2], V, 3)),
    ("bl_amd_chain_host", lambda: bliss_amd.chain(V, [0, 4], 3)),
    ("bl_amd_mix_host", lambda: bliss_amd.mix(V, [0, 4], 3, tags=TAGS, gap=1)),
    ("bl_amd_mix_host", lambda: bliss_amd.mix(V, None, 3, seed_vecs=V[:2])),
    ("bl_amd_radius_host", lambda: bliss_amd.radius(V, 1.0)),
    ("bl_amd_cross_radius_host", lambda: bliss_amd.radius_cross(V[:2], V, 1.0)),
    ("bl_amd_groups_host", lambda: bliss_amd.duplicate_groups(V, 1.0)),
    ("bl_amd_playlist_host", lambda: bliss_amd.playlist(V, 2)),
    ("bl_amd_playlist_vec_host", lambda: bliss_amd.playlist_vec(V, [1, 2, 3, 4])),
    ("bl_amd_distance_matrix_host", lambda: bliss_amd.distance_matrix(V)),
    ("bl_amd_cosine_matrix_host", lambda: bliss_amd.cosine_matrix(V)),
    ("bl_amd_levels_batch_host", lambda: bliss_amd.levels_batch_host(_songs(), [1, 2, 1])),
    ("bl_amd_timbre_batch_host", lambda: bliss_amd.timbre_batch_host(_songs(), [1, 2, 1])),
    ("bl_amd_analyze_batch_host", lambda: bliss_amd.analyze_batch_host(_songs(), [1, 2, 1], 1)),
    ("bl_amd_analyze_batch_host_s32", lambda: bliss_amd.analyze_batch_host_s32(_songs(np.int32), [1, 2, 1], 1)),
    ("bl_amd_analyze_batch_host_rate", lambda: bliss_amd.analyze_batch_host_rate(_songs(), [1, 2, 1], 1, 44100)),
]


@pytest.mark.parametrize("name, call", ENTRY_POINTS, ids=[f"{i}-{n}" for i, (n, _) in enumerate(ENTRY_POINTS)])
def test_a_well_formed_call_reaches_its_entry_point(name, call):
    torch = pytest.importorskip("torch")
    if torch.cuda.is_available():
        pytest.skip("a device is present: the call succeeds")
    with pytest.raises(RuntimeError) as e:
        call()
    assert re.findall(r"bl_amd_\w+", str(e.value)) == [name]


# ---- 5. the readers that work on records alone

def _levels(tails, heads):
    lv = np.zeros(3, dtype=LEVELS_DTYPE)
    lv["frames"] = [1000, 777, 2]
    lv["sum"] = [[-5000, 12345], [31, 0], [2, -2]]
    lv["sum_sq"] = [[10 ** 9, 3 * 10 ** 11], [777 * 2 ** 30, 0], [0, 8]]   # song 1: mono, full scale
    lv["peak"] = [[1200, 32768], [32768, 0], [0, 2]]
    lv["zero_cross"] = [[10, 999], [0, 0], [1, 0]]
    lv["tail"], lv["head"] = tails, heads
    return lv


def test_levels_db_is_the_documented_arithmetic():
    lv = _levels(0, 0)
    got = bliss_amd.levels_db(lv)
    assert got.shape == (3,)
    for i in range(3):
        f = float(lv["frames"][i])
        for c in range(2):
            peak, ssq = int(lv["peak"][i, c]), int(lv["sum_sq"][i, c])
            want = dict(peak_db=20.0 * math.log10(peak / 32768.0) if peak else -math.inf,
                        rms_db=10.0 * math.log10(ssq / (f * 2.0 ** 30)) if ssq else -math.inf,
                        dc=int(lv["sum"][i, c]) / f, zcr=int(lv["zero_cross"][i, c]) / max(f - 1.0, 1.0))
            for k, w in want.items():   # a handful of double operations on exact integers
                assert got[k][i, c] == w or abs(got[k][i, c] - w) <= 1e-14 * abs(w), (i, c, k, got[k][i, c], w)
    assert got["rms_db"][1, 0] == 0.0 and got["peak_db"][0, 1] == 0.0


def _linked(tail, head):
    """the rule of the header, in the float arithmetic it is written in"""
    return any(abs(int(t)) >= 5 and abs(int(h)) >= 5 and
               abs((np.float32(t) - np.float32(h)) / np.float32(32767)) < np.float32(0.01) for t, h in zip(tail, head))


@pytest.mark.parametrize("tails, heads, want", [
    # 0 -> 1 by slot 0; 1 -> 2 by slot 1 at the largest difference that still links, 327
    ([[100, -200], [3, 1000], [0, 0]], [[0, 0], [120, 5000], [3, 1327]], [True, True]),
    # 0 -> 1: close, but one side is quieter than 5; 1 -> 2: one step too far, 328
    ([[4, -200], [3, -1000], [9, 9]], [[9, 9], [4, 5000], [3, -1328]], [False, False]),
])
def test_gapless_links_is_the_documented_rule(tails, heads, want):
    lv = _levels(tails, heads)
    got = bliss_amd.gapless_links(lv)
    assert got.dtype == bool and got.tolist() == want
    assert got.tolist() == [_linked(lv["tail"][i], lv["head"][i + 1]) for i in range(2)]


def test_timbre_hz_is_the_documented_arithmetic():
    st = np.zeros(3, dtype=TIMBRE_SONG_DTYPE)
    per_frame = [([40.5, 60.25, 100.0, 20.0], [50, 70, 120, 30], [10, 12, 90, 7]), ([17.0], [33], [5]), ([], [], [])]
    for i, (cen, rol, pk) in enumerate(per_frame):
        cen = [int(c * 4096) for c in cen]   # the centroid is kept in 1 / 4096 bin
        st["used"][i], st["frames"][i] = len(cen), len(cen) + 2
        for name, xs in (("centroid", cen), ("rolloff", rol), ("peak", pk)):
            st[name + "_sum"][i], st[name + "_sumsq"][i] = sum(xs), sum(x * x for x in xs)
    for rate in (22050, 44100):
        got = bliss_amd.timbre_hz(st, rate)
        assert got.shape == (3,)
        for i, (cen, rol, pk) in enumerate(per_frame):
            for name, xs in (("centroid", cen), ("rolloff", rol), ("peak", pk)):
                mean, std = got[name + "_hz"][i], got[name + "_std_hz"][i]
                if not xs:
                    assert math.isnan(mean) and math.isnan(std)
                    continue
                hz = np.asarray(xs, dtype=np.float64) * (rate / 512.0)   # bins of a 512-point frame
                assert abs(mean - hz.mean()) <= 1e-12 * hz.mean(), (i, name, mean, hz.mean())
                # the variance comes from a difference of two sums: absolute to the mean's scale, not to its own
                assert abs(std - hz.std()) <= 1e-9 * hz.mean(), (i, name, std, hz.std())
    assert bliss_amd.timbre_hz(st)["rolloff_hz"].tolist()[:2] == bliss_amd.timbre_hz(st, 22050)["rolloff_hz"].tolist()[:2]


def test_the_readers_refuse_what_is_not_their_record():
    for bad in (np.zeros(3, dtype=TIMBRE_SONG_DTYPE), np.zeros(0, dtype=LEVELS_DTYPE), np.zeros((2, 2), dtype=LEVELS_DTYPE)):
        with pytest.raises(ValueError):
            bliss_amd.levels_db(bad)
        with pytest.raises(ValueError):
            bliss_amd.gapless_links(bad)
    for bad in (np.zeros(3, dtype=LEVELS_DTYPE), np.zeros(0, dtype=TIMBRE_SONG_DTYPE)):
        with pytest.raises(ValueError):
            bliss_amd.timbre_hz(bad)
