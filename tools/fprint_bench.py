#!/usr/bin/env python3
"""Throughput of the fingerprints (bl_amd_fprint_words_device, bl_amd_fprint_match_device), written down, not asserted.

    python tools/fprint_bench.py [--songs 8192] [--seconds 180] [--k 32] [--shift 64] [--words-songs 2048]
                                 [--out profiles/fprint_match.json]

The match is measured on random words resident in HBM: --songs songs of --seconds (at 22 050 Hz: 1 922 words for 180 s),
--k pairs per song with seeded random partners, max_shift --shift; and one query against all songs.  There is no earlier
implementation to compare with, so the yardstick is a floor: two vector instructions (exclusive or, population count
with accumulate) per word pair, the word pairs counted exactly from the overlaps, over 256 CUs x 4 SIMDs x 16 lanes per
clock, at --clock-ghz and at the mean shader clock sampled over the run.

The words pass is measured beside the chroma call that feeds it (bl_amd_chroma_batch_device with frames) over one arena
of --words-songs synthetic songs, in alternating windows of one run.  Its floor is the bytes it must move (96 per frame
read, 4 per word written) at HBM peak (--hbm-tbs, the specification's 8 TB/s).

A window is about --window-ms of back-to-back calls (--reps at least) between device events, and the windows take turns
--rounds times.  The kernels are timed in a run of their own through bl_amd_profile and bl_amd_fprint_profile_ms.  Needs
a GPU: there is no other way to get a time."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LANES_PER_CLOCK = 256 * 4 * 16
OPS_PER_WORD_PAIR = 2


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


def kernel_ms(torch, lib, a, name, call):
    lib.bl_amd_fprint_profile_ms(name.encode(), None)   # forget what was collected before
    lib.bl_amd_profile(1)
    for _ in range(a.reps):
        call()
    torch.cuda.synchronize()
    lib.bl_amd_profile(0)
    k = C.c_int(0)
    return {"ms_per_call": lib.bl_amd_fprint_profile_ms(name.encode(), C.byref(k)) / a.reps, "launches": k.value}


def word_pairs(w, shift):
    """sum over d = -shift .. shift of the overlap of two songs of w words"""
    return sum(max(0, w - abs(d)) for d in range(-shift, shift + 1))


def match_part(torch, lib, a):
    import numpy as np

    import bliss_amd.fingerprint as fp
    frames = max(0, (a.seconds * 22050 - 4096) // 2048 + 1)
    w = fp.words_count(frames)
    n = a.songs
    gen = torch.Generator(device="cuda").manual_seed(1)
    words = torch.randint(-2 ** 31, 2 ** 31, (n * w,), dtype=torch.int32, device="cuda", generator=gen)
    counts = (C.c_int32 * n)(*([w] * n))
    rng = np.random.default_rng(2)
    sets = {"knn": fp.pairs_from_knn(rng.integers(0, n, size=(n, a.k))),
            "one_query": np.stack([np.zeros(n, np.int32), np.arange(n, dtype=np.int32)], axis=1)}
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {}
    for name, pairs in sets.items():
        dp = torch.from_numpy(np.ascontiguousarray(pairs, dtype=np.int32)).cuda()
        rec = torch.empty(pairs.shape[0] * 24, dtype=torch.uint8, device="cuda")

        def call():
            rc = lib.bl_amd_fprint_match_device(C.c_void_p(words.data_ptr()), counts, n, C.c_void_p(words.data_ptr()),
                                                counts, n, C.c_void_p(dp.data_ptr()), pairs.shape[0], a.shift, 1,
                                                C.c_void_p(rec.data_ptr()), None, stream)
            assert rc == 0
        r = alternate(torch, a, {"match": call})["match"]
        ops = float(pairs.shape[0]) * word_pairs(w, a.shift) * OPS_PER_WORD_PAIR
        floor_ms = ops / (LANES_PER_CLOCK * a.clock_ghz * 1e9) * 1e3
        r.update(pairs=int(pairs.shape[0]), word_pairs=ops / OPS_PER_WORD_PAIR, issue_floor_ms=floor_ms,
                 ratio_to_issue_floor=r["ms_per_call"] / floor_ms,
                 kernel=kernel_ms(torch, lib, a, "fprint_match", call))
        got = fp.match_to_numpy(rec.cpu().numpy())
        r["check"] = {"ok": int((got["status"] == 0).sum()), "ber_min": float(fp.ber(got[got["status"] == 0]).min()),
                      "self_pairs_with_zero_errors": int(((pairs[:, 0] == pairs[:, 1]) & (got["errors"] == 0)).sum()),
                      "self_pairs": int((pairs[:, 0] == pairs[:, 1]).sum())}
        res[name] = r
    return {"songs": n, "seconds": a.seconds, "words_per_song": w, "max_shift": a.shift, "k": a.k,
            "geometry": dict(zip(("words_block", "strip_words", "tile_words", "chunk_offsets"), fp.shape(a.shift))),
            "ops_per_word_pair": OPS_PER_WORD_PAIR, "lanes_per_clock": LANES_PER_CLOCK, "clock_ghz": a.clock_ghz,
            "calls": res}


def words_part(torch, lib, a):
    import bliss_amd
    import bliss_amd.chroma as ch
    import bliss_amd.fingerprint as fp
    n, samples = a.words_songs, a.seconds * 22050
    corpus = bliss_amd.DeviceCorpus([samples] * n, 1, a.seconds)
    corpus.synth(seed_base=1, sample_rate=22050)
    rec, frames = ch.chroma_device(corpus, frames=True)
    t = max(0, (samples - 4096) // 2048 + 1)
    w = fp.words_count(t)
    counts = (C.c_int32 * n)(*([t] * n))
    out = torch.empty(max(n * w, 1), dtype=torch.int32, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def chroma():
        rc = lib.bl_amd_chroma_batch_device(C.c_void_p(corpus.pcm.data_ptr()), corpus.desc, n,
                                            C.c_void_p(rec.data_ptr()), C.c_void_p(frames.data_ptr()), n * t, stream)
        assert rc == 0

    def words():
        rc = lib.bl_amd_fprint_words_device(C.c_void_p(frames.data_ptr()), counts, n, C.c_void_p(out.data_ptr()), n * w,
                                            stream)
        assert rc == 0
    res = alternate(torch, a, {"chroma_with_frames": chroma, "words": words})
    nbytes = float(n) * (t * 96 + w * 4)
    floor_ms = nbytes / (a.hbm_tbs * 1e12) * 1e3
    res["words"].update(bytes=nbytes, hbm_floor_ms=floor_ms, hbm_tbs=a.hbm_tbs,
                        ratio_to_hbm_floor=res["words"]["ms_per_call"] / floor_ms,
                        ratio_to_chroma=res["words"]["ms_per_call"] / res["chroma_with_frames"]["ms_per_call"],
                        kernel=kernel_ms(torch, lib, a, "fprint_words", words))
    return {"songs": n, "seconds": a.seconds, "frames_per_song": t, "words_per_song": w, "pcm_bytes": corpus.pcm_bytes,
            "calls": res}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--songs", type=int, default=8192)
    ap.add_argument("--seconds", type=int, default=180)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--shift", type=int, default=64)
    ap.add_argument("--words-songs", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fprint_match.json"))
    a = ap.parse_args()

    import torch

    from bench import DeviceState
    if not torch.cuda.is_available():
        sys.exit("fprint_bench.py needs a GPU: a time taken anywhere else says nothing")
    import bliss_amd
    lib = bliss_amd.load()
    assert lib.bl_amd_init(0) == 0
    state = DeviceState(DeviceState.pci_address(0))
    state.start()
    t0 = time.perf_counter()
    out = {"what": "bl_amd_fprint_match_device on random words and bl_amd_fprint_words_device beside "
                   "bl_amd_chroma_batch_device over one arena: alternating windows of about `window_ms` of back-to-back "
                   "calls (`reps` at least) between device events, `rounds` windows each, after `warmup` calls; the "
                   "kernels through bl_amd_fprint_profile_ms in a run of their own",
           "reps": a.reps, "window_ms": a.window_ms, "rounds": a.rounds, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0)}
    out["match"] = match_part(torch, lib, a)
    torch.cuda.empty_cache()
    out["words"] = words_part(torch, lib, a)
    state.stop_flag = True
    state.join()
    out["device_state"] = state.summary(t0, time.perf_counter())
    mhz = (out["device_state"].get("sclk_mhz") or {}).get("mean")
    if mhz:   # the floor assumes --clock-ghz; the same ratio at the mean shader clock sampled over the whole run
        for r in out["match"]["calls"].values():
            r["issue_floor_ms_at_mean_clock"] = r["issue_floor_ms"] * a.clock_ghz * 1e3 / mhz
            r["ratio_to_issue_floor_at_mean_clock"] = r["ms_per_call"] / r["issue_floor_ms_at_mean_clock"]
        out["match"]["mean_clock_mhz"] = mhz
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"match_ms": {k: round(v["ms_per_call"], 3) for k, v in out["match"]["calls"].items()},
                      "match_floor_ms": {k: round(v["issue_floor_ms"], 3) for k, v in out["match"]["calls"].items()},
                      "words_ms": {k: round(v["ms_per_call"], 3) for k, v in out["words"]["calls"].items()},
                      "words_floor_ms": round(out["words"]["calls"]["words"]["hbm_floor_ms"], 3)}), flush=True)


if __name__ == "__main__":
    main()
