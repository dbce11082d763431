#!/usr/bin/env python3
"""Throughput of the signal-level pass (bl_amd_levels_batch_device) on the bench.py corpus shape, written down, not
asserted: 8 192 synthetic songs of 180 s at 22 050 Hz stereo, resident in HBM.

    python tools/levels_throughput.py [--songs 8192] [--seconds 180] [--reps 50] [--out profiles/levels_throughput.json]

levels() is timed with device events over --reps repetitions after a warm-up.  The yardstick, "one streaming pass over
the PCM as this project writes it", is taken in the same process over the same arena: the statistics pass of the
analysis as bl_amd_profile_ms names it — "pcm_scan", or "freq_scan" where the statistics ride along with the frequency
pass (all three analysers, which is what DeviceCorpus.analyze() asks for; that kernel also does the frequency work, so
the ratio flatters the level pass and says so in the file).  The shader clock is read from the amdgpu hwmon files
while the timed loop runs (bench.DeviceState).  Needs a GPU: there is no other way to get a time."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_TBS = 8.0   # the part's specified peak; about 6.3 TB/s is what a plain copy achieves


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--songs", type=int, default=8192)
    ap.add_argument("--seconds", type=int, default=180)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--analyze-steps", type=int, default=3)
    ap.add_argument("--silence", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "levels_throughput.json"))
    a = ap.parse_args()

    import ctypes as C

    import torch

    import bliss_amd
    from bench import DeviceState
    if not torch.cuda.is_available():
        sys.exit("levels_throughput.py needs a GPU: a time taken anywhere else says nothing")
    rate, ch = 22050, 2
    n = rate * ch * a.seconds
    corpus = bliss_amd.DeviceCorpus([n] * a.songs, ch, a.seconds)
    corpus.synth(seed_base=1, sample_rate=rate)
    torch.cuda.synchronize()
    lib = corpus.lib
    pcm_bytes = corpus.pcm_bytes

    # the yardstick: the analysis' own statistics pass over the same arena
    corpus.analyze()
    torch.cuda.synchronize()
    lib.bl_amd_profile_reset()
    lib.bl_amd_profile(1)
    for _ in range(a.analyze_steps):
        corpus.analyze()
    torch.cuda.synchronize()
    lib.bl_amd_profile(0)
    yard = {}
    for name in ("pcm_scan", "freq_scan"):
        k = C.c_int(0)
        ms = lib.bl_amd_profile_ms(name.encode(), C.byref(k))
        if k.value:
            yard[name] = {"ms_avg": ms / k.value, "launches": k.value}
    yard_name = "pcm_scan" if "pcm_scan" in yard else "freq_scan"

    for _ in range(a.warmup):
        corpus.levels(silence=a.silence)
    torch.cuda.synchronize()
    state = DeviceState(DeviceState.pci_address(0))
    state.start()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.reps + 1)]
    t0 = time.perf_counter()
    ev[0].record()
    for i in range(a.reps):
        corpus.levels(silence=a.silence)
        ev[i + 1].record()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    state.stop_flag = True
    state.join()
    per = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(a.reps))
    ms = ev[0].elapsed_time(ev[a.reps]) / a.reps
    lv = corpus.fetch_levels()
    gbs = pcm_bytes / (ms * 1e-3) / 1e9
    out = {
        "what": "bl_amd_levels_batch_device over a resident corpus, device events over `reps` back-to-back calls "
                "after `warmup` calls; one call = memset of the records, k_level_scan, k_level_ends",
        "songs": a.songs, "seconds": a.seconds, "sample_rate": rate, "channels": ch, "silence": a.silence,
        "pcm_bytes": pcm_bytes, "reps": a.reps, "warmup": a.warmup,
        "ms_per_batch": ms, "ms_per_batch_min": per[0], "ms_per_batch_median": per[len(per) // 2],
        "ms_per_batch_max": per[-1],
        "pcm_gb_per_s": gbs,
        "fraction_of_hbm_peak": gbs / (HBM_PEAK_TBS * 1e3), "hbm_peak_tb_per_s": HBM_PEAK_TBS,
        "yardstick": {"name": yard_name, "all": yard, "analyze_steps": a.analyze_steps,
                      "what": "the statistics pass of DeviceCorpus.analyze() over the same arena in the same process "
                              "(bl_amd_profile_ms); freq_scan also carries the frequency pass"},
        "ratio_to_yardstick": ms / yard[yard_name]["ms_avg"] if yard else None,
        "device": torch.cuda.get_device_name(0),
        "device_state": state.summary(t0, t1),
        "check": {"frames": int(lv["frames"][0]), "status_all_ok": bool((lv["status"] == 0).all()),
                  "peak_max": int(lv["peak"].max())},
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("ms_per_batch", "pcm_gb_per_s", "fraction_of_hbm_peak",
                                          "ratio_to_yardstick")}))


if __name__ == "__main__":
    main()
