#!/usr/bin/env python3
"""Throughput of the cover and version matching (bl_amd_cover_match_device), written down, not asserted.

    python tools/cover_bench.py [--songs 8192] [--seconds 180] [--k 32] [--pool 4] [--pool1-songs 256] [--shift 64]
                                [--asm bl_cover_kernels.s] [--out profiles/cover_align.json]

The alignment is measured on units resident in HBM, drawn from a seeded alphabet of chord-like units: --songs songs of
--seconds at --pool (484 units for 180 s at pool 4) with --k seeded random partners each; --pool1-songs songs at pool 1
(1 936 units) with --k partners; and one query against all --songs.  Beside the first, in alternating windows of the same
run, bl_amd_fprint_match_device runs over the same pairs at +-shift on random words of the same songs' length: the
yardstick, since there is no earlier alignment to compare with.

The floor is an issue floor: the vector instructions of one step of k_cover_align's inner loop (--valu-per-step, counted
in the kernel's own disassembly: `hipcc -S --offload-device-only bl_cover_kernels.hip`, the loop that holds the five
v_mov_b32_dpp wave_shr:1; --asm recounts it from such a file) times the steps of the call (per pair and strip: Ua + columns
of the strip - 1) times 64 lanes, over 256 CUs x 4 SIMDs x 32 lanes per clock (a wave's vector instruction takes a SIMD two cycles
when several waves issue; the first run of this tool, with 16, measured 0.92 of that floor), at --clock-ghz and at the mean shader clock
sampled over the run.  k_cover_profile is set against the bytes it reads (16 per unit) at HBM peak (--hbm-tbs).

A window is about --window-ms of back-to-back calls (--reps at least) between device events, and the windows take turns
--rounds times.  The kernels are timed in a run of their own through bl_amd_profile and bl_amd_cover_profile_ms.  Needs a
GPU: there is no other way to get a time."""
import argparse
import ctypes as C
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LANES_PER_CLOCK = 256 * 4 * 32   # a SIMD of gfx950 takes a wave's vector instruction in two cycles when several waves issue
STRIP = 64
VALU_PER_STEP = 53   # the inner loop of k_cover_align as compiled for gfx950 when this was written


def valu_per_step(path):
    """the vector instructions of the loop that holds the wave shifts, from the kernel's disassembly"""
    lines = open(path).read().split("\n")
    at = [i for i, ln in enumerate(lines) if "wave_shr:1" in ln]
    if not at:
        raise SystemExit(f"{path}: no wave_shr:1 in it")
    head = max(i for i in range(at[0]) if re.match(r"^\.LBB\d+_\d+:", lines[i]))
    label = lines[head].split(":")[0]
    end = next(i for i in range(at[-1], len(lines)) if re.search(r"s_c?branch\S*\s+" + re.escape(label) + r"\b", lines[i]))
    return sum(1 for ln in lines[head:end + 1] if re.match(r"^\s+v_", ln))


def window(torch, reps, call):
    """ms per call over `reps` back-to-back calls between two events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        call()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def summary(ms):
    s = sorted(ms)
    return {"ms_per_call": sum(s) / len(s), "ms_per_call_min": s[0], "ms_per_call_max": s[-1], "windows": ms}


def alternate(torch, a, calls):
    for c in calls.values():
        for _ in range(a.warmup):
            c()
    torch.cuda.synchronize()
    reps = {k: min(4000, max(a.reps, int(a.window_ms / max(window(torch, a.reps, c), 1e-3)) + 1))
            for k, c in calls.items()}
    ms = {k: [] for k in calls}
    for _ in range(a.rounds):
        for k, c in calls.items():
            ms[k].append(window(torch, reps[k], c))
    return {k: dict(summary(v), calls_per_window=reps[k]) for k, v in ms.items()}


def kernel_ms(torch, lib, a, names, call):
    for name in names:
        lib.bl_amd_cover_profile_ms(name.encode(), None)   # forget what was collected before
    lib.bl_amd_profile(1)
    for _ in range(a.reps):
        call()
    torch.cuda.synchronize()
    lib.bl_amd_profile(0)
    out = {}
    for name in names:
        k = C.c_int(0)
        out[name] = {"ms_per_call": lib.bl_amd_cover_profile_ms(name.encode(), C.byref(k)) / a.reps, "launches": k.value}
    return out


def steps_of(ua, ub):
    """steps of one pair: per strip, Ua + its columns - 1"""
    full, rest = divmod(ub, STRIP)
    return full * (ua + STRIP - 1) + ((ua + rest - 1) if rest else 0)


def units_of(torch, np, n, u, seed):
    """n songs of u units from an alphabet of 24 chord-like units (three loud classes), as a CUDA uint8 (n u, 16)"""
    rng = np.random.default_rng(seed)
    abc = np.zeros((24, 16), dtype=np.uint8)
    for row in abc:
        row[:12] = rng.integers(0, 12, size=12)
        row[rng.choice(12, size=3, replace=False)] = (73, 70, 68)
    return torch.from_numpy(abc[rng.integers(0, 24, size=n * u)]).cuda()


def align_case(torch, np, lib, a, cover, name, n, u, pairs, valu, beside=None):
    units = units_of(torch, np, n, u, 1)
    counts = (C.c_int32 * n)(*([u] * n))
    dp = torch.from_numpy(np.ascontiguousarray(pairs, dtype=np.int32)).cuda()
    rec = torch.empty(pairs.shape[0] * 40, dtype=torch.uint8, device="cuda")
    p = cover.params()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call():
        rc = lib.bl_amd_cover_match_device(C.c_void_p(units.data_ptr()), counts, n, C.c_void_p(units.data_ptr()), counts,
                                           n, C.c_void_p(dp.data_ptr()), pairs.shape[0], C.byref(p),
                                           C.c_void_p(rec.data_ptr()), stream)
        assert rc == 0
    calls = {"cover_match": call}
    if beside:
        calls["fprint_match"] = beside(dp, pairs.shape[0])
    res = alternate(torch, a, calls)
    r = res["cover_match"]
    cells = float(pairs.shape[0]) * u * u
    steps = float(pairs.shape[0]) * steps_of(u, u)
    floor_ms = steps * valu * 64 / (LANES_PER_CLOCK * a.clock_ghz * 1e9) * 1e3
    r.update(songs=n, units_per_song=u, pairs=int(pairs.shape[0]), cells=cells, steps=steps,
             cells_per_second=cells / (r["ms_per_call"] * 1e-3), issue_floor_ms=floor_ms,
             ratio_to_issue_floor=r["ms_per_call"] / floor_ms,
             kernels=kernel_ms(torch, lib, a, ("cover_profile", "cover_align"), call))
    prof = r["kernels"]["cover_profile"]
    nbytes = 2.0 * n * u * 16                                    # both sets of the self form are profiled
    prof.update(bytes=nbytes, hbm_floor_ms=nbytes / (a.hbm_tbs * 1e12) * 1e3)
    prof["ratio_to_hbm_floor"] = prof["ms_per_call"] / prof["hbm_floor_ms"] if prof["ms_per_call"] > 0 else None
    got = cover.match_to_numpy(rec.cpu().numpy())
    same = pairs[:, 0] == pairs[:, 1]
    r["check"] = {"ok": int((got["status"] == 0).sum()), "no_match": int((got["status"] == 1).sum()),
                  "self_pairs": int(same.sum()), "self_pairs_aligned_end_to_end":
                      int((same & (got["a_start"] == 0) & (got["a_end"] == u - 1) & (got["b_end"] == u - 1)).sum())}
    print(f"{name}: {r['ms_per_call']:.3f} ms", file=sys.stderr, flush=True)
    if beside:
        f = res["fprint_match"]
        f["ratio_cover_to_fprint"] = r["ms_per_call"] / f["ms_per_call"]
        r["beside_fprint_match"] = f
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--songs", type=int, default=8192)
    ap.add_argument("--seconds", type=int, default=180)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--pool", type=int, default=4)
    ap.add_argument("--pool1-songs", type=int, default=256)
    ap.add_argument("--shift", type=int, default=64)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    ap.add_argument("--valu-per-step", type=int, default=VALU_PER_STEP)
    ap.add_argument("--asm", default=None, help="disassembly of bl_cover_kernels.hip to count --valu-per-step from")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cover_align.json"))
    a = ap.parse_args()
    valu = valu_per_step(a.asm) if a.asm else a.valu_per_step

    import numpy as np
    import torch

    from bench import DeviceState
    if not torch.cuda.is_available():
        sys.exit("cover_bench.py needs a GPU: a time taken anywhere else says nothing")
    import bliss_amd
    import bliss_amd.cover as cover
    import bliss_amd.fingerprint as fp
    lib = bliss_amd.load()
    assert lib.bl_amd_init(0) == 0
    frames = max(0, (a.seconds * 22050 - 4096) // 2048 + 1)
    n, rng = a.songs, np.random.default_rng(2)

    # the yardstick: the fingerprint match over the same pairs, random words of the songs' length
    w = fp.words_count(frames)
    gen = torch.Generator(device="cuda").manual_seed(1)
    words = torch.randint(-2 ** 31, 2 ** 31, (n * w,), dtype=torch.int32, device="cuda", generator=gen)
    wcounts = (C.c_int32 * n)(*([w] * n))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fprint_beside(dp, n_pairs):
        frec = torch.empty(n_pairs * 24, dtype=torch.uint8, device="cuda")

        def call():
            rc = lib.bl_amd_fprint_match_device(C.c_void_p(words.data_ptr()), wcounts, n, C.c_void_p(words.data_ptr()),
                                                wcounts, n, C.c_void_p(dp.data_ptr()), n_pairs, a.shift, 1,
                                                C.c_void_p(frec.data_ptr()), None, stream)
            assert rc == 0
        return call

    state = DeviceState(DeviceState.pci_address(0))
    state.start()
    t0 = time.perf_counter()
    out = {"what": "bl_amd_cover_match_device on seeded units resident in HBM, beside bl_amd_fprint_match_device over "
                   "the same pairs: alternating windows of about `window_ms` of back-to-back calls (`reps` at least) "
                   "between device events, `rounds` windows each, after `warmup` calls; the kernels through "
                   "bl_amd_cover_profile_ms in a run of their own",
           "reps": a.reps, "window_ms": a.window_ms, "rounds": a.rounds, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "valu_per_step": valu, "lanes_per_clock": LANES_PER_CLOCK,
           "clock_ghz": a.clock_ghz, "seconds": a.seconds, "k": a.k, "max_shift": a.shift, "words_per_song": w,
           "shape": dict(zip(("strip_columns", "row_block"), cover.shape()))}
    u4, u1 = frames // a.pool, frames
    cases = {}
    cases["knn_pool%d" % a.pool] = align_case(torch, np, lib, a, cover, "knn", n, u4,
                                              cover.pairs_from_knn(rng.integers(0, n, size=(n, a.k))), valu, fprint_beside)
    m = a.pool1_songs
    cases["knn_pool1"] = align_case(torch, np, lib, a, cover, "pool1", m, u1,
                                    cover.pairs_from_knn(rng.integers(0, m, size=(m, a.k))), valu)
    cases["one_query_pool%d" % a.pool] = align_case(
        torch, np, lib, a, cover, "one_query", n, u4,
        np.stack([np.zeros(n, np.int32), np.arange(n, dtype=np.int32)], axis=1), valu)
    out["calls"] = cases
    state.stop_flag = True
    state.join()
    out["device_state"] = state.summary(t0, time.perf_counter())
    mhz = (out["device_state"].get("sclk_mhz") or {}).get("mean")
    if mhz:   # the floor assumes --clock-ghz; the same ratio at the mean shader clock sampled over the whole run
        for r in cases.values():
            r["issue_floor_ms_at_mean_clock"] = r["issue_floor_ms"] * a.clock_ghz * 1e3 / mhz
            r["ratio_to_issue_floor_at_mean_clock"] = r["ms_per_call"] / r["issue_floor_ms_at_mean_clock"]
        out["mean_clock_mhz"] = mhz
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {"ms": round(v["ms_per_call"], 3), "gcells_per_s": round(v["cells_per_second"] / 1e9, 2),
                          "x_floor": round(v["ratio_to_issue_floor"], 2)} for k, v in cases.items()}), flush=True)


if __name__ == "__main__":
    main()
