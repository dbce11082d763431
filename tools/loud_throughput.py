#!/usr/bin/env python3
"""Throughput of the K-weighted gated loudness (bl_amd_loud_batch_device), written down, not asserted: synthetic stereo
songs at 44 100 Hz, resident in HBM, with bl_amd_loud_kweight's parameters.

    python tools/loud_throughput.py [--shapes 1024x30,8192x180] [--reps 3] [--rounds 3] [--out profiles/loud_throughput.json]

The yardstick is the whole bl_amd_levels_batch_device call (peak and plain RMS: one streaming pass over the same
bytes) over the same arena, in alternating windows of the same run: a window is about --window-ms of back-to-back
calls (--reps at least) between device events, and the windows of the calls take turns --rounds times, so that a drift
of the clock shows in all of them.  The loudness call is timed without and with its hop-energy output; its two kernels
are timed in a run of their own through bl_amd_profile and bl_amd_loud_profile_ms ("loud_filter", "loud_gate").

The f64 issue floor is the operation count of the filter over the vector f64 rate: 19 unfused operations per sample and
channel (14 of the two sections, the conversion, the square and its sum, rounded up for the hop's bookkeeping), times
1 + warm / (16 hop) for the warm-up, over 256 CUs x 4 SIMDs x 16 lanes per clock at --clock-ghz (the public 78.6 TFLOPS
of the part counts a fused multiply-add as two; an unfused operation is one).  That is the nominal clock; the device runs
below it under load, so the profile also holds the floor and the ratio at the mean shader clock sampled over the run.

8 192 songs of 180 s at 44.1 kHz stereo are 260 GB of PCM; a shape that does not fit the device is recorded as such and
the others stand.  The profile is rewritten after every shape.  Needs a GPU: there is no other way to get a time."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OPS_PER_SAMPLE = 19
LANES_PER_CLOCK = 256 * 4 * 16


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


def shape(torch, a, songs, seconds):
    import bliss_amd
    import bliss_amd.loudness as ld
    rate, ch = a.rate, 2
    n = rate * ch * seconds
    p = ld.kweight(rate)
    corpus = bliss_amd.DeviceCorpus([n] * songs, ch, seconds)
    corpus.synth(seed_base=1, sample_rate=rate)
    lib = corpus.lib
    hops = n // ch // p.hop
    total = hops * songs
    # outputs allocated once: the timed calls are the library's call alone
    rec = torch.empty(songs * ld.LOUD_DTYPE.itemsize, dtype=torch.uint8, device=corpus.device)
    z = torch.empty((total, 2), dtype=torch.int64, device=corpus.device)

    def loud(with_hops):
        def call():
            rc = lib.bl_amd_loud_batch_device(
                C.c_void_p(corpus.pcm.data_ptr()), corpus.desc, songs, C.byref(p), C.c_void_p(rec.data_ptr()),
                C.c_void_p(z.data_ptr()) if with_hops else None, total,
                C.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0
        return call
    calls = {"levels": corpus.levels, "loud": loud(False), "loud_with_hops": loud(True)}
    for c in calls.values():
        for _ in range(a.warmup):
            c()
    torch.cuda.synchronize()
    # a window lasts about --window-ms, and at least --reps calls: a shorter one measures the clock and the scheduler
    reps = {k: min(4000, max(a.reps, int(a.window_ms / max(window(torch, a.reps, c), 1e-3)) + 1))
            for k, c in calls.items()}
    ms = {k: [] for k in calls}
    for _ in range(a.rounds):
        for k, c in calls.items():
            ms[k].append(window(torch, reps[k], c))
    res = {k: dict(summary(v), calls_per_window=reps[k]) for k, v in ms.items()}
    yard = res["levels"]["ms_per_call"]
    ops = float(total) * p.hop * ch * OPS_PER_SAMPLE * (1.0 + p.warm / (16.0 * p.hop))
    floor_ms = ops / (LANES_PER_CLOCK * a.clock_ghz * 1e9) * 1e3
    for k in ("loud", "loud_with_hops"):
        res[k]["ratio_to_levels"] = res[k]["ms_per_call"] / yard
        res[k]["ratio_to_f64_issue_floor"] = res[k]["ms_per_call"] / floor_ms
    # the kernels in a run of their own
    for name in (b"loud_filter", b"loud_gate"):   # forget what was collected before
        lib.bl_amd_loud_profile_ms(name, None)
    lib.bl_amd_profile(1)
    for _ in range(a.reps):
        calls["loud"]()
    torch.cuda.synchronize()
    lib.bl_amd_profile(0)
    kernels = {}
    for name in ("loud_filter", "loud_gate"):
        k = C.c_int(0)
        kernels[name] = {"ms_per_call": lib.bl_amd_loud_profile_ms(name.encode(), C.byref(k)) / a.reps, "launches": k.value}
    kernels["loud_filter"]["ratio_to_f64_issue_floor"] = kernels["loud_filter"]["ms_per_call"] / floor_ms
    calls["loud"]()
    torch.cuda.synchronize()
    got = ld.loud_to_numpy(rec.cpu().numpy())
    integrated = ld.lufs(got, p.hop)[0]
    return {
        "songs": songs, "seconds": seconds, "rate": rate, "channels": ch, "hops_per_song": hops,
        "lanes": songs * ((hops + 15) // 16), "pcm_bytes": corpus.pcm_bytes,
        "calls": res, "kernels": kernels,
        "f64_issue_floor": {"ms": floor_ms, "operations": ops, "ops_per_sample_and_channel": OPS_PER_SAMPLE,
                            "lanes_per_clock": LANES_PER_CLOCK, "clock_ghz": a.clock_ghz},
        "check": {"lufs_of_song_0": float(integrated[0]), "lufs_min": float(integrated.min()),
                  "lufs_max": float(integrated.max()), "range_lu_of_song_0": float(ld.range_lu(got)[0]),
                  "gated_count_of_song_0": int(got["gated_count"][0]), "blocks_of_song_0": int(got["blocks"][0])},
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    ap.add_argument("--shapes", default="1024x30,8192x180")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loud_throughput.json"))
    a = ap.parse_args()

    import torch

    from bench import DeviceState
    if not torch.cuda.is_available():
        sys.exit("loud_throughput.py needs a GPU: a time taken anywhere else says nothing")
    state = DeviceState(DeviceState.pci_address(0))
    state.start()
    t0 = time.perf_counter()
    shapes = []

    def write():
        out = {
            "what": "bl_amd_loud_batch_device beside bl_amd_levels_batch_device over the same arena in one run: "
                    "alternating windows of about `window_ms` of back-to-back calls (`reps` at least) between device "
                    "events, `rounds` windows each, after `warmup` calls of every form; the kernels through "
                    "bl_amd_loud_profile_ms in a run of their own",
            "reps": a.reps, "window_ms": a.window_ms, "rounds": a.rounds, "warmup": a.warmup, "shapes": shapes,
            "device": torch.cuda.get_device_name(0), "device_state": state.summary(t0, time.perf_counter()),
        }
        # the floor assumes --clock-ghz; the same ratio at the mean shader clock sampled over the whole run beside it
        mhz = (out["device_state"].get("sclk_mhz") or {}).get("mean")
        for s in shapes:
            if mhz and "calls" in s:
                at_mean = s["f64_issue_floor"]["ms"] * a.clock_ghz * 1e3 / mhz
                s["f64_issue_floor"]["ms_at_mean_clock"] = at_mean
                s["f64_issue_floor"]["mean_clock_mhz"] = mhz
                s["calls"]["loud"]["ratio_to_f64_issue_floor_at_mean_clock"] = s["calls"]["loud"]["ms_per_call"] / at_mean
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    for s in a.shapes.split(","):
        songs, seconds = (int(x) for x in s.split("x"))
        try:
            shapes.append(shape(torch, a, songs, seconds))
        except torch.cuda.OutOfMemoryError as e:
            shapes.append({"songs": songs, "seconds": seconds, "rate": a.rate, "not_run": "out of device memory",
                           "pcm_bytes": songs * seconds * a.rate * 4, "error": str(e).splitlines()[0]})
        torch.cuda.empty_cache()
        write()
        print(json.dumps({"songs": songs, "seconds": seconds,
                          **({"not_run": shapes[-1]["not_run"]} if "not_run" in shapes[-1] else
                             {"ms": {k: round(v["ms_per_call"], 3) for k, v in shapes[-1]["calls"].items()},
                              "kernel_ms": {k: round(v["ms_per_call"], 3) for k, v in shapes[-1]["kernels"].items()},
                              "floor_ms": round(shapes[-1]["f64_issue_floor"]["ms"], 3)})}), flush=True)
    state.stop_flag = True
    state.join()
    write()


if __name__ == "__main__":
    main()
