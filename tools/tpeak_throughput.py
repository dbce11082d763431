#!/usr/bin/env python3
"""Throughput of the true peak (bl_amd_tpeak_batch_device), written down, not asserted: synthetic stereo songs at
44 100 Hz, resident in HBM.

    python tools/tpeak_throughput.py [--shapes 1024x30,8192x180] [--reps 3] [--rounds 3] [--out profiles/tpeak_throughput.json]

The yardstick is the whole bl_amd_levels_batch_device call (one streaming pass over the same bytes) over the same arena,
in alternating windows of the same run: a window is about --window-ms of back-to-back calls (--reps at least) between
device events, and the windows of the calls take turns --rounds times, so that a drift of the clock shows in all of
them.  The true-peak call is timed without and with its block profile (--block frames per block); its two kernels are
timed in a run of their own through bl_amd_profile and bl_amd_tpeak_profile_ms ("tpeak_scan", "tpeak_finish").

The issue floor is the kernel's own operation count over the vector issue rate: 51.5 vector instructions per sample and
channel, counted in the gfx950 code of one stereo frame of k_tpeak_scan on the path without a profile (103 for its two
samples: 36 packed dot products, 6 moves that clear their accumulators, 2 regroupings of words into pairs, and 59 for
the magnitudes, the count above the ceiling, the largest point and its position and the sample peak; a profile adds 6),
over 256 CUs x 4 SIMDs x 16 lanes per clock at --clock-ghz.  That is the nominal clock; the
device runs below it under load, so the profile also holds the floor and the ratio at the mean shader clock sampled over
the run.

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

OPS_PER_SAMPLE = 51.5
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
    import bliss_amd.truepeak as tp
    rate, ch = a.rate, 2
    n = rate * ch * seconds
    frames = n // ch
    corpus = bliss_amd.DeviceCorpus([n] * songs, ch, seconds)
    corpus.synth(seed_base=1, sample_rate=rate)
    lib = corpus.lib
    n_blocks = (frames + a.block - 1) // a.block * songs
    # outputs allocated once: the timed calls are the library's call alone
    rec = torch.empty(songs * tp.TPEAK_DTYPE.itemsize, dtype=torch.uint8, device=corpus.device)
    prof = torch.empty((n_blocks, 2), dtype=torch.int32, device=corpus.device)

    def tpeak(with_blocks):
        def call():
            rc = lib.bl_amd_tpeak_batch_device(
                C.c_void_p(corpus.pcm.data_ptr()), corpus.desc, songs, a.ceiling, a.block, C.c_void_p(rec.data_ptr()),
                C.c_void_p(prof.data_ptr()) if with_blocks else None, n_blocks,
                C.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0
        return call
    calls = {"levels": corpus.levels, "tpeak": tpeak(False), "tpeak_with_blocks": tpeak(True)}
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
    ops = float(frames) * ch * songs * OPS_PER_SAMPLE
    floor_ms = ops / (LANES_PER_CLOCK * a.clock_ghz * 1e9) * 1e3
    for k in ("tpeak", "tpeak_with_blocks"):
        res[k]["ratio_to_levels"] = res[k]["ms_per_call"] / yard
        res[k]["ratio_to_issue_floor"] = res[k]["ms_per_call"] / floor_ms
    # the kernels in a run of their own
    for name in (b"tpeak_scan", b"tpeak_finish"):   # forget what was collected before
        lib.bl_amd_tpeak_profile_ms(name, None)
    lib.bl_amd_profile(1)
    for _ in range(a.reps):
        calls["tpeak"]()
    torch.cuda.synchronize()
    lib.bl_amd_profile(0)
    kernels = {}
    for name in ("tpeak_scan", "tpeak_finish"):
        k = C.c_int(0)
        kernels[name] = {"ms_per_call": lib.bl_amd_tpeak_profile_ms(name.encode(), C.byref(k)) / a.reps,
                         "launches": k.value}
    kernels["tpeak_scan"]["ratio_to_issue_floor"] = kernels["tpeak_scan"]["ms_per_call"] / floor_ms
    calls["tpeak"]()
    torch.cuda.synchronize()
    got = tp.tpeak_to_numpy(rec.cpu().numpy())
    per, song = tp.dbtp(got)
    return {
        "songs": songs, "seconds": seconds, "rate": rate, "channels": ch, "frames_per_song": frames,
        "block": a.block, "ceiling": a.ceiling, "workgroups": songs * ((frames + 4095) // 4096),
        "pcm_bytes": corpus.pcm_bytes, "calls": res, "kernels": kernels,
        "issue_floor": {"ms": floor_ms, "operations": ops, "ops_per_sample_and_channel": OPS_PER_SAMPLE,
                        "lanes_per_clock": LANES_PER_CLOCK, "clock_ghz": a.clock_ghz},
        "check": {"dbtp_of_song_0": float(song[0]), "dbtp_min": float(song.min()), "dbtp_max": float(song.max()),
                  "tpeak_of_song_0": [int(v) for v in got["tpeak"][0]], "peak_of_song_0": [int(v) for v in got["peak"][0]],
                  "overs_of_song_0": [int(v) for v in got["overs"][0]], "at_of_song_0": [int(v) for v in got["at"][0]]},
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--block", type=int, default=4410, help="frames per block of the profile: 100 ms")
    ap.add_argument("--ceiling", type=int, default=32767)
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    ap.add_argument("--shapes", default="1024x30,8192x180")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tpeak_throughput.json"))
    a = ap.parse_args()

    import torch

    from bench import DeviceState
    if not torch.cuda.is_available():
        sys.exit("tpeak_throughput.py needs a GPU: a time taken anywhere else says nothing")
    state = DeviceState(DeviceState.pci_address(0))
    state.start()
    t0 = time.perf_counter()
    shapes = []

    def write():
        out = {
            "what": "bl_amd_tpeak_batch_device beside bl_amd_levels_batch_device over the same arena in one run: "
                    "alternating windows of about `window_ms` of back-to-back calls (`reps` at least) between device "
                    "events, `rounds` windows each, after `warmup` calls of every form; the kernels through "
                    "bl_amd_tpeak_profile_ms in a run of their own",
            "reps": a.reps, "window_ms": a.window_ms, "rounds": a.rounds, "warmup": a.warmup, "shapes": shapes,
            "device": torch.cuda.get_device_name(0), "device_state": state.summary(t0, time.perf_counter()),
        }
        # the floor assumes --clock-ghz; the same ratio at the mean shader clock sampled over the whole run beside it
        mhz = (out["device_state"].get("sclk_mhz") or {}).get("mean")
        for s in shapes:
            if mhz and "calls" in s:
                at_mean = s["issue_floor"]["ms"] * a.clock_ghz * 1e3 / mhz
                s["issue_floor"]["ms_at_mean_clock"] = at_mean
                s["issue_floor"]["mean_clock_mhz"] = mhz
                s["calls"]["tpeak"]["ratio_to_issue_floor_at_mean_clock"] = s["calls"]["tpeak"]["ms_per_call"] / at_mean
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
                              "floor_ms": round(shapes[-1]["issue_floor"]["ms"], 3)})}), flush=True)
    state.stop_flag = True
    state.join()
    write()


if __name__ == "__main__":
    main()
