#!/usr/bin/env python3
"""Throughput of the beat grid (bl_amd_beats_device), written down, not asserted: 8 192 synthetic songs of 180 s and
1 024 songs of 30 s at 22 050 Hz stereo, resident in HBM, at the periods the tempo call found for them.

    python tools/beats_throughput.py [--reps 10] [--rounds 3] [--out profiles/beats_throughput.json]

The yardstick is the whole bl_amd_rhythm_batch_device call that produced the curves (with its onset output), over the
same arena, in alternating windows of the same run: a window is about --window-ms of back-to-back calls (--reps at
least) between device events, and the windows of the calls take turns --rounds times, so that a drift of the clock
shows in all of them.  The beat call is
timed reading the lags in place from the tempo records (stride 72), without and with the links and scores outputs.  Its
kernel is also timed in a run of its own through bl_amd_profile ("beats").

The share of the back-trace is measured without another build: the kernel's loops over the scores do not depend on the
data, and a curve of zeros has no beats, so the same call on a zero curve of the same lengths and periods is the call
without its back-trace.  Needs a GPU: there is no other way to get a time."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def shape(torch, a, songs, seconds, lag_min, lag_max):
    import numpy as np

    import bliss_amd
    import bliss_amd.rhythm as rh
    rate, ch = 22050, 2
    n = rate * ch * seconds
    corpus = bliss_amd.DeviceCorpus([n] * songs, ch, seconds)
    corpus.synth(seed_base=1, sample_rate=rate)
    lib = corpus.lib
    hops = [n // ch // rh.HOP] * songs
    rec_t, ons_t, _ = rh.rhythm_device(corpus, lag_min, lag_max)
    torch.cuda.synchronize()
    zero_t = torch.zeros_like(ons_t)

    def rhythm():
        rh.rhythm_device(corpus, lag_min, lag_max)

    # outputs allocated once: the timed calls are the library's call alone
    total = sum(hops)
    out = {k: torch.empty(sz, dtype=dt, device=ons_t.device)
           for k, (sz, dt) in dict(rec=(songs * 40, torch.uint8), flags=(total, torch.uint8),
                                   links=(total, torch.int16), scores=(total, torch.int64)).items()}
    hops_c = (C.c_int32 * songs)(*hops)
    lag_at = rec_t.data_ptr() + rh.RHYTHM_DTYPE.fields["lag"][1]

    def beats(curve, full):
        def call():
            rc = lib.bl_amd_beats_device(
                C.c_void_p(curve.data_ptr()), hops_c, songs, C.c_void_p(lag_at), rh.RHYTHM_DTYPE.itemsize, a.tight,
                C.c_void_p(out["rec"].data_ptr()), C.c_void_p(out["flags"].data_ptr()),
                C.c_void_p(out["links"].data_ptr()) if full else None,
                C.c_void_p(out["scores"].data_ptr()) if full else None,
                C.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0
        return call
    calls = {"rhythm_with_onsets": rhythm, "beats": beats(ons_t, False), "beats_links_scores": beats(ons_t, True),
             "beats_zero_curve": beats(zero_t, False)}
    for c in calls.values():
        for _ in range(a.warmup):
            c()
    torch.cuda.synchronize()
    # a window lasts about --window-ms, and at least --reps calls: a shorter one measures the clock and the scheduler
    reps = {k: min(4000, max(a.reps, int(a.window_ms / max(window(torch, a.reps, c), 1e-3)) + 1)) for k, c in calls.items()}
    ms = {k: [] for k in calls}
    for _ in range(a.rounds):
        for k, c in calls.items():
            ms[k].append(window(torch, reps[k], c))
    res = {k: dict(summary(v), calls_per_window=reps[k]) for k, v in ms.items()}
    yard = res["rhythm_with_onsets"]["ms_per_call"]
    for k in ("beats", "beats_links_scores", "beats_zero_curve"):
        res[k]["ratio_to_rhythm"] = res[k]["ms_per_call"] / yard
    b, z = res["beats"]["ms_per_call"], res["beats_zero_curve"]["ms_per_call"]
    # the kernel in a run of its own
    lib.bl_amd_profile_reset()
    lib.bl_amd_profile(1)
    for _ in range(a.reps):
        calls["beats"]()
    torch.cuda.synchronize()
    lib.bl_amd_profile(0)
    k = C.c_int(0)
    kernel_ms = lib.bl_amd_profile_ms(b"beats", C.byref(k)) / a.reps
    calls["beats"]()
    torch.cuda.synchronize()
    rec = rh.beats_to_numpy(out["rec"].cpu().numpy())
    rhy = rh.rhythm_to_numpy(rec_t.cpu().numpy())
    ok = rec["status"] == 0
    bpm = rh.beats_bpm(rec)
    return {
        "songs": songs, "seconds": seconds, "hops_per_song": hops[0], "lag_min": lag_min, "lag_max": lag_max,
        "calls": res,
        "backtrace": {"ms_per_call": b - z, "share_of_beats_call": (b - z) / b,
                      "what": "beats minus beats_zero_curve: the same call on zeros has no beats to trace"},
        "kernel_beats": {"ms_per_call": kernel_ms, "launches": k.value},
        "score_steps": int(sum(int(h) * (2 * int(L) - ((int(L) + 1) >> 1) + 1)
                               for h, L in zip(hops, rhy["lag"]) if 2 <= L <= 510)),
        "check": {"songs_with_a_tempo": int(ok.sum()), "lag_min_seen": int(rhy["lag"].min()),
                  "lag_max_seen": int(rhy["lag"].max()), "beats_per_song_mean": float(rec["n_beats"][ok].mean()) if ok.any() else 0.0,
                  "grid_bpm_of_song_0": float(bpm[0]), "period_of_song_0": int(rec["period"][0]),
                  "median_beat_spacing_over_period": float(np.median(
                      (rec["last"][ok] - rec["first"][ok]) / np.maximum(rec["n_beats"][ok] - 1, 1) / rec["period"][ok]))
                  if ok.any() else 0.0},
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--tight", type=int, default=128)
    ap.add_argument("--lag-min", type=int, default=58)     # 180 bpm
    ap.add_argument("--lag-max", type=int, default=172)    # 60 bpm
    ap.add_argument("--shapes", default="8192x180,1024x30")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beats_throughput.json"))
    a = ap.parse_args()

    import torch

    from bench import DeviceState
    if not torch.cuda.is_available():
        sys.exit("beats_throughput.py needs a GPU: a time taken anywhere else says nothing")
    state = DeviceState(DeviceState.pci_address(0))
    state.start()
    t0 = time.perf_counter()
    shapes = []
    for s in a.shapes.split(","):
        songs, seconds = (int(x) for x in s.split("x"))
        shapes.append(shape(torch, a, songs, seconds, a.lag_min, a.lag_max))
        torch.cuda.empty_cache()
    t1 = time.perf_counter()
    state.stop_flag = True
    state.join()
    out = {
        "what": "bl_amd_beats_device beside the bl_amd_rhythm_batch_device call that produced its curves, over the same "
                "arena in one run: alternating windows of about `window_ms` of back-to-back calls (`reps` at least) between device "
                "events, `rounds` windows each, after `warmup` calls of every form; periods read in place from the tempo records",
        "tight": a.tight, "reps": a.reps, "window_ms": a.window_ms, "rounds": a.rounds, "warmup": a.warmup, "shapes": shapes,
        "device": torch.cuda.get_device_name(0), "device_state": state.summary(t0, t1),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps([{"songs": s["songs"], "seconds": s["seconds"],
                       "ms": {k: round(v["ms_per_call"], 3) for k, v in s["calls"].items()},
                       "kernel_ms": round(s["kernel_beats"]["ms_per_call"], 3),
                       "backtrace_share": round(s["backtrace"]["share_of_beats_call"], 3)} for s in shapes]))


if __name__ == "__main__":
    main()
