"""Device rate converter (bl_rs_kernels.hip) in the launch shapes and placements that the host batch path produces
at scale, against the host form (bl_amd_resample_host, pinned on the reference's digests by tests/test_ingest.py),
bit for bit.  tests/test_gpu_resample.py places five short songs on 8-element boundaries, which keeps every run of
tiles one tile long and takes one alignment branch per kernel; here the descriptors are written by hand.

Covered:
  - runs of tiles in k_resample (tiles_per_wg 1, 2, 5, 16; bank in LDS and in global memory; down- and up-sampling)
    and in k_resample_pm (tiles_per_wg 1, 2, 3, 8; both kinds): songs whose output ends on, one before, one after a
    run boundary, with a last run of one tile, and with fewer than 4 frames in the last tile; at 48 kHz on every
    input alignment, so that the prefetch-ahead and the frame-by-frame staging both walk runs of several tiles;
  - every staging branch of k_resample_1p (44.1 and 88.2 kHz, both kinds, stereo and mono, every in_offset residue
    mod 8 that the descriptor check admits) and both store branches (out_offset residues 0, 2, 4, 6 mod 8);
  - guards: the input arena is full-scale garbage between the songs (gaps of 1..24 elements), the output arena a
    sentinel that must survive everywhere outside the songs' regions.
Which path each song takes is computed by a mirror of the launch plan and of the kernels' branch conditions, and
test_case_table_reaches_every_path (no GPU) fails when the case table stops reaching one of them.

Not covered: more than one launch group (BL_GROUP_SONGS_MAX songs), float sources, arenas past 2^31 elements, and
the fall-back of a 48 kHz-like plan to k_resample (no rate of the table takes it)."""
import functools

import numpy as np
import pytest

import bliss_amd
from bliss_amd import _lib

OUT_RATE = 22050          # bl_runtime.h BL_RS_OUT_RATE
RS_TILE = 1024            # bl_rs_kernels.hip:37
RS_LDS_LIMIT = 160 * 1024  # bl_rs_kernels.hip:40
SENTINEL = -21555         # 0xABCD
PAD = 4096                # elements of the torch allocation in front of and behind either arena


# ---------------------------------------------------------------- the plan, mirrored ----------------------------

def _geometry(rate):
    """bl_resample.c:72-104 bl_rs_plan_geometry: (phase_count, taps, src_incr, dst_incr)."""
    factor = min(1.0, OUT_RATE * 0.97 / rate)
    pc = 1 << 10
    g0 = np.gcd(OUT_RATE, rate)
    if OUT_RATE // g0 <= pc:
        pc = int(OUT_RATE // g0)
    taps = int(np.ceil(32 / factor))
    if taps > 1:
        taps = (taps + 1) & ~1
    num, den = OUT_RATE, rate * pc
    g = int(np.gcd(num, den))
    num, den = num // g, den // g
    while den < (1 << 20) and num < (1 << 20):
        den, num = den * 2, num * 2
    return pc, taps, num, den


def _plan(rate, kind, out_frames, n_songs):
    """blk_resample (bl_rs_kernels.hip:845-883), blk_resample_geom (:824-843), rs_launch (:812-815), rs_launch_pm
    (:790-792), rs_launch_1p (:452): the kernel, its tile, tiles_per_wg and the workgroups per song."""
    pc, taps, src, dst = _geometry(rate)
    max_out = max(out_frames)
    p = dict(rate=rate, kind=kind, pc=pc, taps=taps, src=src, dst=dst, w0=taps - (taps - 1) // 2)
    if pc == 1 and dst % src == 0 and (dst // src, taps) in ((2, 66), (4, 132)):          # :849-856
        p.update(kernel="1p", D=dst // src, T=RS_TILE, tiles_per_wg=1, groups=(max_out + RS_TILE - 1) // RS_TILE)
        return p
    if pc > 1 and dst % src == 0 and taps == 72:                                          # :858-876
        adv = dst // src
        rfr = adv + taps + 4
        rstride = ((rfr + 2) | 1) if kind == "s32" else ((rfr // 2 + 1) | 1)
        lds = (pc * 64 + (1 if kind == "s32" else 2) * 64 * rstride + (0 if kind == "s32" else pc * (taps // 2 + 1))) * 4
        T = pc * 64
        tiles = (max_out + T - 1) // T
        t = min(8, max(1, n_songs * tiles // 1024))
        if adv % 2 == 0 and adv <= 4096 and lds <= RS_LDS_LIMIT:
            p.update(kernel="pm", adv=adv, T=T, tiles_per_wg=t, groups=(tiles + t - 1) // t)
            return p
    taps8 = (taps + 7) & ~7                                                               # :824-842
    adv = (RS_TILE - 1) * dst // (src * pc)
    span = (adv + 2 + taps8 + 1) & ~1
    in_lds = span * 8 + pc * (taps8 + 4) * 4 <= RS_LDS_LIMIT
    assert span * 8 <= RS_LDS_LIMIT
    tiles = (max_out + RS_TILE - 1) // RS_TILE                                            # :812-815
    t = min(16, max(1, tiles * n_songs // 2048))
    p.update(kernel="generic_lds" if in_lds else "generic_global", T=RS_TILE, tiles_per_wg=t,
             groups=(tiles + t - 1) // t)
    return p


def _runs(p, s):
    """The runs of tiles one song is converted in: a list (one entry per workgroup that does not return at once) of
    lists of tiles; a tile is a dict with its number, the staging branch and the store branches its lanes take."""
    T, t, of = p["T"], p["tiles_per_wg"], s["out_frames"]
    tiles_total = (of + T - 1) // T
    runs = []
    for b in range(p["groups"]):
        first = b * t
        if first >= tiles_total:       # n_begin >= out_frames (:99), tile_begin >= tiles_total (:494), n0 >= out_frames (:216)
            continue
        run = []
        for tile in range(first, min(first + t, tiles_total)):
            cnt = min(T, of - tile * T)
            if p["kernel"] == "1p":
                stage, store = _stage_1p(p, s, tile), _store_1p(s, cnt)
            elif p["kernel"] == "pm":
                prev = run[-1]["stage"] if run else None
                stage, store = _stage_pm(p, s, tile), {"dword"}
                if stage == "vector":   # :622-629: fetched ahead while `prev` was computed, or before the loop
                    stage = "commit_after_prefetch_ahead" if prev is not None else "commit_first"
            else:
                stage, store = "span", {"dword"}
            run.append(dict(tile=tile, cnt=cnt, stage=stage, store=store))
        runs.append(run)
    return runs


def _stage_1p(p, s, tile):
    """k_resample_1p's staging branch of a tile (bl_rs_kernels.hip:221, :234-362); the arenas' bases are 16-byte
    aligned (asserted where they are made)."""
    D, L, N = p["D"], p["taps"], s["frames"]
    F = L + 3 * D
    span = (255 * 4 * D + F + 7) & ~7                                                     # :200-201
    x_first = p["w0"] + tile * RS_TILE * D - L
    interior = x_first >= 0 and x_first + span <= N
    stereo = s["channels"] == 2
    if not interior:
        return "edge"
    if p["kind"] == "s32":
        if stereo:
            return "16-byte" if (4 * (s["in_off"] + 2 * x_first)) % 16 == 0 else "8-byte"  # :238, :256
        return "generic"
    if stereo and (2 * (s["in_off"] + 2 * x_first)) % 16 == 0:                            # :289
        return "16-byte"
    if not stereo and (2 * (s["in_off"] + x_first)) % 16 == 0:                            # :308
        return "mono vector"
    return "4-byte" if stereo else "generic"                                              # :331, :349


def _store_1p(s, cnt):
    """:438-446: a lane holds 4 output frames; whole lanes store a uint4 when the address is 16-byte aligned."""
    out = set()
    if cnt >= 4:
        out.add("uint4" if (2 * s["out_off"]) % 16 == 0 else "scalar, whole lane")
    if cnt % 4:
        out.add("scalar, part of a lane")
    return out


def _stage_pm(p, s, tile):
    """k_resample_pm's staging of a tile: s16 :526-533 and :622-629, s32 :678-683."""
    L, adv, N = p["taps"], p["adv"], s["frames"]
    delta = (p["w0"] - L) % 4                       # Python's % is already the non-negative one of :502
    rfr = adv + L + delta
    xf = p["w0"] + tile * 64 * adv - L - delta
    stereo = s["channels"] == 2
    if p["kind"] == "s16":
        nq = (rfr + 2 + 3) // 4
        if not ((2 * s["in_off"]) % 16 == 0 and adv % 4 == 0 and nq <= 128):
            return "slow, unaligned"
        return "vector" if xf >= 0 and xf + 63 * adv + 4 * nq <= N else "slow, edge"
    nu = (rfr + 1) // 2
    if not stereo:
        return "slow, mono"
    if (4 * s["in_off"]) % 16 or nu > 256:
        return "slow, unaligned"
    return "fast" if xf >= 0 and xf + 63 * adv + 2 * nu <= N else "slow, edge"


# ---------------------------------------------------------------- the case table --------------------------------

# tile runs: name -> rate, kind, tiles of the longest song, songs, long songs, tiles_per_wg the plan must give
RUN_CASES = {
    "generic-32000-s32-t2": dict(rate=32000, kind="s32", tiles=32, n_songs=128, n_long=6, tpw=2, kernel="generic_lds"),
    # up-sampling skips output lengths: 2 048 k + 1 frames is first reached at k = 17, hence 36 tiles
    "generic-8000-s16-t2": dict(rate=8000, kind="s16", tiles=36, n_songs=128, n_long=6, tpw=2, kernel="generic_lds"),
    "generic-192000-s32-t5": dict(rate=192000, kind="s32", tiles=40, n_songs=256, n_long=6, tpw=5, kernel="generic_global"),
    "generic-96000-s16-t16": dict(rate=96000, kind="s16", tiles=64, n_songs=512, n_long=6, tpw=16, kernel="generic_lds"),
    "generic-44099-s16-t16": dict(rate=44099, kind="s16", tiles=64, n_songs=512, n_long=6, tpw=16, kernel="generic_global"),
    "generic-96000-s16-t1": dict(rate=96000, kind="s16", tiles=3, n_songs=6, n_long=6, tpw=1, kernel="generic_lds"),
    "pm-48000-s16-t2": dict(rate=48000, kind="s16", tiles=8, n_songs=256, n_long=9, tpw=2, kernel="pm"),
    "pm-48000-s32-t3": dict(rate=48000, kind="s32", tiles=12, n_songs=256, n_long=7, tpw=3, kernel="pm"),
    "pm-48000-s16-t8": dict(rate=48000, kind="s16", tiles=32, n_songs=256, n_long=9, tpw=8, kernel="pm"),
    "pm-48000-s32-t8": dict(rate=48000, kind="s32", tiles=32, n_songs=256, n_long=7, tpw=8, kernel="pm"),
    "pm-48000-s32-t2": dict(rate=48000, kind="s32", tiles=8, n_songs=256, n_long=7, tpw=2, kernel="pm"),
    "pm-48000-s16-t1": dict(rate=48000, kind="s16", tiles=3, n_songs=9, n_long=9, tpw=1, kernel="pm"),
}
# (channels, in_offset mod 8) of the long songs at 48 kHz: s16 stereo on 0, 2, 4, 6, mono on those and an odd one;
# s32 stereo on 0 and 2 mod 4, mono on anything
PM_LONG = {"s16": [(2, 0), (1, 0), (2, 2), (2, 4), (2, 6), (1, 2), (1, 4), (1, 6), (1, 3)],
           "s32": [(2, 0), (2, 2), (2, 4), (2, 6), (1, 0), (1, 5), (1, 2)]}
GENERIC_LONG = [(2, 0), (1, 3), (2, 6), (1, 0), (2, 2), (1, 7)]
ALIGN_CASES = [(44100, "s16"), (44100, "s32"), (88200, "s16"), (88200, "s32")]
# k_resample_1p: every in_offset residue the descriptor check admits (blr_resample_device, bl_runtime.hip), out_offset residues
# 0, 2, 4, 6 three times each and in another pairing for stereo and mono; output frames beyond four whole tiles
ALIGN_SONGS = [(2, 0, 0, 0), (2, 2, 2, 1), (2, 4, 4, 1023), (2, 6, 6, 517), (1, 0, 2, 3), (1, 1, 4, 0), (1, 2, 6, 1024),
               (1, 3, 0, 2), (1, 4, 4, 5), (1, 5, 6, 515), (1, 6, 0, 7), (1, 7, 2, 9)]
CLASSES = ("whole runs", "one frame short of a run", "one frame into a run", "last run of one tile",
           "fewer than 4 frames in the last tile", "one run")


def _frames_for(lib, rate, target):
    """Input frames whose conversion has exactly `target` output frames, or None (up-sampling skips counts)."""
    lo, hi = 1, int(target * rate / OUT_RATE) + 4096
    while lo < hi:
        mid = (lo + hi) // 2
        if lib.bl_amd_resample_out_frames(mid, rate) >= target:
            hi = mid
        else:
            lo = mid + 1
    return lo if lib.bl_amd_resample_out_frames(lo, rate) == target else None


def _class_of(of, t, T):
    """Where a song's output ends relative to its runs of t tiles of T frames."""
    r, out = of % (t * T), set()
    if r == 0:
        out.add(CLASSES[0])
        if of == t * T:
            out.add(CLASSES[5])
    if r == t * T - 1:
        out.add(CLASSES[1])
    if r == 1:
        out.add(CLASSES[2])
    if r == T and of > t * T:
        out.add(CLASSES[3])
    if 1 <= of % T <= 3:
        out.add(CLASSES[4])
    return out


def _long_frames(lib, rate, t, T, tiles, j):
    """Long song j of a batch: input frames such that the output lands on the j-th kind of run boundary."""
    K = tiles // t
    cls = j % len(CLASSES)
    ks = [K] if j == 0 else [(j * 5 + i) % K + 1 for i in range(K)]
    for k in ks:
        target = (k * t * T, k * t * T - 1, k * t * T + 1, (k * t + 1) * T, k * t * T + 3, t * T)[cls]
        if target > tiles * T or (cls == 3 and k == K):
            continue
        fr = _frames_for(lib, rate, target)
        if fr is not None:
            return fr
    if j == 0:   # up-sampling: the longest song ends as close below the last run's end as a length gets
        return max(f for f in range(int(tiles * T * rate / OUT_RATE) - 8, int(tiles * T * rate / OUT_RATE) + 8)
                   if lib.bl_amd_resample_out_frames(f, rate) <= tiles * T)
    raise AssertionError((rate, t, T, tiles, j, "no input length gives this output length"))


def _place(lib, rate, songs):
    """in_offset / out_offset of every song: the wanted residue mod 8, garbage gaps of 1..24 elements in front of
    each input, sentinel gaps of 2..24 in front of each output (out_offset is even)."""
    in_end, out_end = 8, 8
    for i, s in enumerate(songs):
        assert s["channels"] == 1 or s["in_res"] % 2 == 0
        start = in_end + 1
        start += (s["in_res"] - start) % 8 + 8 * (i % 3)
        assert 1 <= start - in_end <= 24 and start % 8 == s["in_res"]
        s["in_off"], in_end = start, start + s["frames"] * s["channels"]
        s["out_frames"] = int(lib.bl_amd_resample_out_frames(s["frames"], rate))
        assert s["out_frames"] > 0
        start = out_end + 2
        start += (s["out_res"] - start) % 8 + 8 * ((i + 1) % 3)
        assert 2 <= start - out_end <= 24 and start % 8 == s["out_res"]
        s["out_off"], out_end = start, start + 2 * s["out_frames"]
    return in_end + 32, out_end + 64


@functools.lru_cache(maxsize=None)
def _layout(name):
    """(songs, input elements, output elements, plan) of a case; songs carry frames, channels, offsets, out_frames
    and whether they are fillers."""
    lib = bliss_amd.load()
    if name in RUN_CASES:
        c = RUN_CASES[name]
        rate, kind = c["rate"], c["kind"]
        pc, taps, _, _ = _geometry(rate)
        T = pc * 64 if c["kernel"] == "pm" else RS_TILE
        long_spec = PM_LONG[kind] if c["kernel"] == "pm" else GENERIC_LONG
        songs = []
        for j in range(c["n_long"]):
            ch, res = long_spec[j]
            songs.append(dict(frames=_long_frames(lib, rate, c["tpw"], T, c["tiles"], j), channels=ch, in_res=res,
                              out_res=2 * (j % 4), filler=None))
        for i in range(c["n_songs"] - c["n_long"]):   # just above the filter length: most of their workgroups return at once
            ch = 1 + i % 2
            songs.append(dict(frames=taps + 1 + 7 * i % 211, channels=ch, in_res=(5 * i + 3) % 8 & (~1 if ch == 2 else 7),
                              out_res=2 * ((3 * i + 1) % 4), filler=i))
        order = np.random.default_rng(len(name)).permutation(len(songs))   # the long songs anywhere in the batch
        songs = [songs[k] for k in order]
    else:
        rate, kind = name
        songs = []
        for ch, in_res, out_res, extra in ALIGN_SONGS:
            fr = _frames_for(lib, rate, 4 * RS_TILE + extra)
            assert fr is not None
            songs.append(dict(frames=fr, channels=ch, in_res=in_res, out_res=out_res, filler=None))
    n_in, n_out = _place(lib, rate, songs)
    plan = _plan(rate, kind, [s["out_frames"] for s in songs], len(songs))
    return songs, n_in, n_out, plan


def _all_runs(name):
    songs, _, _, plan = _layout(name)
    return plan, [(s, _runs(plan, s)) for s in songs]


def _reached():
    """path -> the first (case, song) of the table that takes it, for the listing the CPU test prints."""
    out = {}
    for name in list(RUN_CASES) + ALIGN_CASES:
        plan, per_song = _all_runs(name)
        k, t, T = plan["kernel"], plan["tiles_per_wg"], plan["T"]
        for i, (s, runs) in enumerate(per_song):
            who = f"{plan['kind']} {'stereo' if s['channels'] == 2 else 'mono'}"
            paths = []
            for r in runs:
                if k == "1p":
                    paths += [f"1p {plan['rate']} {who}: staging {r[0]['stage']}"]
                    paths += [f"1p {plan['rate']} {plan['kind']}: store {x}" for x in r[0]["store"]]
                    continue
                paths.append(f"{k}: tiles_per_wg {t}, run of {len(r)} tile(s)" + (", ends inside a tile" if r[-1]["cnt"] < T else ""))
                if k == "pm":
                    paths += [f"pm {who}: {a['stage']} -> {b['stage']}" for a, b in zip(r, r[1:])]
                    paths.append(f"pm {who}: run starts {r[0]['stage']}")
            for path in paths:
                out.setdefault(path, (name, i, s["in_off"] % 8, s["out_off"] % 8))
    return out


def test_case_table_reaches_every_path(lib):
    """No GPU: the plan mirror over the whole case table.  Every path that tests/test_gpu_resample.py leaves out is
    taken by a song of some case."""
    tpw = {"generic": set(), "pm": set()}
    for name, c in RUN_CASES.items():
        plan, per_song = _all_runs(name)
        assert plan["kernel"] == c["kernel"] and plan["tiles_per_wg"] == c["tpw"], (name, plan)
        t, T = plan["tiles_per_wg"], plan["T"]
        assert plan["groups"] * t == c["tiles"] or t == 1, (name, plan)
        tpw[c["kernel"][:7] if c["kernel"] != "pm" else "pm"].add(t)
        longs = [(s, r) for s, r in per_song if s["filler"] is None]
        assert len(longs) >= 6 and {s["channels"] for s, _ in longs} == {1, 2}
        assert len(per_song) == c["n_songs"] and max(s["out_frames"] for s, _ in longs) > (c["tiles"] - 1) * T
        for s, runs in per_song:
            assert sum(len(r) for r in runs) == (s["out_frames"] + T - 1) // T
            if s["filler"] is not None:
                assert s["out_frames"] < T and s["frames"] < 600   # one tile; the other workgroups return at once
        if t == 1:
            continue
        ends = set().union(*(_class_of(s["out_frames"], t, T) for s, _ in longs))
        assert ends == set(CLASSES), (name, set(CLASSES) - ends)
        all_runs = [r for _, runs in longs for r in runs]
        assert any(len(r) == t and r[-1]["cnt"] == T for r in all_runs)          # the loop past its first pass
        assert any(len(r) == t and r[-1]["cnt"] == T - 1 for r in all_runs)      # a run clipped by n_end inside a tile
        assert any(len(r) == 1 and r[0]["cnt"] == T and r[0]["tile"] >= t for r in all_runs)   # last run of one tile
        assert any(len(r) == 1 and r[0]["cnt"] < 4 and r[0]["tile"] >= t for r in all_runs)
        if c["kernel"] != "pm":
            continue
        for ch in (1, 2):
            mine = [(s, r) for s, runs in longs if s["channels"] == ch for r in runs]
            res = {s["in_off"] % 8 for s, _ in mine}
            if c["kind"] == "s16":
                assert res >= ({0, 2, 4, 6} if ch == 2 else {0, 2, 4, 6, 3}), (name, ch, res)
                stages = [[x["stage"] for x in r] for _, r in mine]
                # a tile staged by commit() has a predecessor in its run: prefetch(tile + 1) ran under that one
                assert any("commit_after_prefetch_ahead" in st[1:] for st in stages), (name, ch)
                assert any(st[:2] == ["slow, edge", "commit_after_prefetch_ahead"] for st in stages), (name, ch)
                assert any(len(st) > 1 and st[-2].startswith("commit") and st[-1] == "slow, edge" for st in stages), (name, ch)
                assert any(st[0] == "commit_first" and len(st) > 1 for st in stages), (name, ch)
                for r8 in res - {0}:   # another base: frame by frame for every tile, interior ones in long runs too
                    assert any(len(r) == t and all(x["stage"] == "slow, unaligned" for x in r)
                               for s, r in mine if s["in_off"] % 8 == r8), (name, ch, r8)
            elif ch == 2:
                assert {s["in_off"] % 4 for s, _ in mine} == {0, 2}
                stages = [[x["stage"] for x in r] for _, r in mine]
                assert any(st[:2] == ["slow, edge", "fast"] for st in stages) and any(st[-2:] == ["fast", "slow, edge"] for st in stages)
                assert any(st == ["fast"] * t for st in stages) and any(st == ["slow, unaligned"] * t for st in stages)
            else:
                assert any(len(r) == t and all(x["stage"] == "slow, mono" for x in r) for _, r in mine)
    assert tpw["generic"] == {1, 2, 5, 16} and tpw["pm"] == {1, 2, 3, 8}, tpw
    kernels = {(c["rate"], c["kind"]): c["kernel"] for c in RUN_CASES.values()}
    assert kernels[(32000, "s32")] == kernels[(96000, "s16")] == kernels[(8000, "s16")] == "generic_lds"
    assert kernels[(192000, "s32")] == kernels[(44099, "s16")] == "generic_global"

    # k_resample_1p: the branch a table row takes with 8-element offsets, and the one it never took
    want = {(44100, "s16", 2): ("16-byte", "4-byte"), (44100, "s32", 2): ("16-byte", "8-byte"),
            (44100, "s16", 1): ("mono vector", "generic"), (88200, "s16", 2): ("4-byte", "16-byte"),
            (88200, "s32", 2): ("8-byte", "16-byte"), (88200, "s16", 1): ("generic", "mono vector")}
    seen = {}
    for name in ALIGN_CASES:
        plan, per_song = _all_runs(name)
        assert plan["kernel"] == "1p" and plan["D"] == name[0] // 22050
        stores, res_in, res_out = set(), {1: set(), 2: set()}, set()
        for s, runs in per_song:
            tiles = [r[0] for r in runs]
            assert len(tiles) >= 4 and all(len(r) == 1 for r in runs)
            inner = [x["stage"] for x in tiles if x["stage"] != "edge"]
            assert len(inner) >= 2 and len(set(inner)) == 1, (name, s, inner)   # interior tiles exist
            assert tiles[0]["stage"] == "edge"
            seen.setdefault((name[0], name[1], s["channels"]), {}).setdefault(inner[0], set()).add(s["in_off"] % 8)
            stores |= set().union(*(x["store"] for x in tiles))
            res_in[s["channels"]].add(s["in_off"] % 8)
            res_out.add(s["out_off"] % 8)
            if s["out_off"] % 8:
                assert "scalar, whole lane" in tiles[1]["store"]
        assert res_in == {1: set(range(8)), 2: {0, 2, 4, 6}} and res_out == {0, 2, 4, 6}
        assert stores == {"uint4", "scalar, whole lane", "scalar, part of a lane"}, (name, stores)
    for row, (today, never) in want.items():
        assert set(seen[row]) == {today, never}, (row, seen[row])
        assert 0 in seen[row][today] and 0 not in seen[row][never]     # what offsets of 8 elements reach, and do not
    assert seen[(88200, "s16", 2)]["16-byte"] == {2} and seen[(88200, "s16", 1)]["mono vector"] == {1}
    assert seen[(88200, "s32", 2)]["16-byte"] == {2, 6}
    print()
    for path, (name, i, rin, rout) in sorted(_reached().items()):
        print(f"reached  {path:70s} first by {name} song {i} (in_offset = {rin}, out_offset = {rout} mod 8)")


# ---------------------------------------------------------------- on the GPU ------------------------------------

def _pcm(rng, kind, n):
    if kind == "s16":
        return rng.integers(-32768, 32768, n).astype(np.int16)
    return rng.integers(-(1 << 31), 1 << 31, n).astype(np.int32)


def _run_case(gpu_lib, name, rate, kind):
    """One call of bl_amd_resample_batch_device over the case's batch; every song against the host form, every
    output element outside the songs against the sentinel."""
    import torch
    songs, n_in, n_out, plan = _layout(name)
    rng = np.random.default_rng(rate + 7 * len(songs) + (kind == "s32"))
    dtype = np.int16 if kind == "s16" else np.int32
    info = np.iinfo(dtype)
    host_in = np.where(rng.integers(0, 2, n_in + 2 * PAD) == 1, info.max, info.min).astype(dtype)   # full-scale garbage
    want = []
    for s in songs:
        n = s["frames"] * s["channels"]
        pcm = _pcm(rng, kind, n)
        ref = bliss_amd.resample_host(pcm, s["channels"], rate)
        assert ref.size == 2 * s["out_frames"]
        host_in[PAD + s["in_off"]:PAD + s["in_off"] + n] = pcm
        want.append(ref)
    desc = (_lib.ResampleDesc * len(songs))()
    for d, s in zip(desc, songs):
        d.in_offset, d.out_offset, d.frames, d.channels = s["in_off"], s["out_off"], s["frames"], s["channels"]
    d_in = torch.from_numpy(host_in).cuda()
    d_out = torch.full((n_out + 2 * PAD,), SENTINEL, dtype=torch.int16, device="cuda")
    base_in, base_out = d_in.data_ptr() + PAD * host_in.itemsize, d_out.data_ptr() + PAD * 2
    assert base_in % 16 == 0 and base_out % 16 == 0   # the plan mirror's alignment arithmetic starts here
    rc = gpu_lib.bl_amd_resample_batch_device(base_in, int(kind == "s32"), desc, len(songs), rate, base_out, None)
    torch.cuda.synchronize()
    assert rc == _lib.BL_OK
    got = d_out.cpu().numpy()
    outside = np.ones(got.size, dtype=bool)
    for i, (s, ref) in enumerate(zip(songs, want)):
        lo = PAD + s["out_off"]
        mine = got[lo:lo + ref.size]
        outside[lo:lo + ref.size] = False
        if not np.array_equal(mine, ref):
            first = int(np.argmax(mine != ref))
            runs = _runs(plan, s)
            tile = next(x for r in runs for x in r if x["tile"] == first // 2 // plan["T"])
            raise AssertionError((rate, kind, f"song {i}", {k: s[k] for k in ("frames", "channels", "in_off", "out_off", "out_frames")},
                                  f"first differing index {first}", f"tile {tile['tile']}: {tile['stage']}",
                                  f"tiles_per_wg {plan['tiles_per_wg']}", int(mine[first]), int(ref[first])))
        if s["channels"] == 1:
            assert np.array_equal(mine[0::2], mine[1::2])
    stray = outside & (got != SENTINEL)
    assert not stray.any(), (rate, kind, "written outside the songs: first at output element",
                             int(np.argmax(stray)) - PAD, "of", n_out)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(RUN_CASES))
def test_runs_of_tiles_equal_host_bit_for_bit(gpu_lib, name):
    _run_case(gpu_lib, name, RUN_CASES[name]["rate"], RUN_CASES[name]["kind"])


@pytest.mark.gpu
@pytest.mark.parametrize("rate,kind", ALIGN_CASES)
def test_one_phase_alignments_equal_host_bit_for_bit(gpu_lib, rate, kind):
    _run_case(gpu_lib, (rate, kind), rate, kind)
