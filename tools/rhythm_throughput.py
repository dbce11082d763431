#!/usr/bin/env python3
"""Throughput of the tempo call (bl_amd_rhythm_batch_device) on the bench.py corpus shape, written down, not asserted:
8 192 synthetic songs of 180 s at 22 050 Hz stereo, resident in HBM.

    python tools/rhythm_throughput.py [--songs 8192] [--seconds 180] [--reps 20] [--out profiles/rhythm_throughput.json]

The call is timed with device events over --reps back-to-back repetitions after a warm-up, without the optional
outputs, with the onset curve, and with the onset curve and the lag products.  Its three kernels are timed separately in
a run of their own through bl_amd_profile ("rhythm_hops", "rhythm_acf", "rhythm_pick").  The yardstick is
bl_amd_levels_batch_device over the same arena in the same process, the project's leanest pass over the PCM: every
time is also given as a ratio to it.  The shader clock and the power are read while the timed loops run
(bench.DeviceState).  Needs a GPU: there is no other way to get a time."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_TBS = 8.0   # the part's specified peak; about 6.3 TB/s is what a plain copy achieves


def timed(torch, reps, call):
    """ms per call over `reps` back-to-back calls: (mean, min, median, max)"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        call()
        ev[i + 1].record()
    torch.cuda.synchronize()
    per = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(reps))
    return {"ms_per_batch": ev[0].elapsed_time(ev[reps]) / reps, "ms_per_batch_min": per[0],
            "ms_per_batch_median": per[len(per) // 2], "ms_per_batch_max": per[-1]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--songs", type=int, default=8192)
    ap.add_argument("--seconds", type=int, default=180)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--lag-min", type=int, default=58)     # 180 bpm
    ap.add_argument("--lag-max", type=int, default=172)    # 60 bpm
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rhythm_throughput.json"))
    a = ap.parse_args()

    import torch

    import bliss_amd
    import bliss_amd.rhythm as rh
    from bench import DeviceState
    if not torch.cuda.is_available():
        sys.exit("rhythm_throughput.py needs a GPU: a time taken anywhere else says nothing")
    rate, ch = 22050, 2
    n = rate * ch * a.seconds
    corpus = bliss_amd.DeviceCorpus([n] * a.songs, ch, a.seconds)
    corpus.synth(seed_base=1, sample_rate=rate)
    torch.cuda.synchronize()
    lib = corpus.lib
    pcm_bytes = corpus.pcm_bytes
    forms = {"records_only": dict(onsets=False, acf=False), "with_onsets": dict(onsets=True, acf=False),
             "with_onsets_and_acf": dict(onsets=True, acf=True)}

    def rhythm(**kw):
        return lambda: rh.rhythm_device(corpus, a.lag_min, a.lag_max, **kw)
    for _ in range(a.warmup):
        corpus.levels()
        for kw in forms.values():
            rhythm(**kw)()
    torch.cuda.synchronize()
    state = DeviceState(DeviceState.pci_address(0))
    state.start()
    t0 = time.perf_counter()
    yard = timed(torch, a.reps, corpus.levels)
    out_forms = {name: timed(torch, a.reps, rhythm(**kw)) for name, kw in forms.items()}
    yard2 = timed(torch, a.reps, corpus.levels)      # the yardstick again behind the calls: its own spread
    t1 = time.perf_counter()
    state.stop_flag = True
    state.join()
    for f in out_forms.values():
        f["ratio_to_levels"] = f["ms_per_batch"] / yard["ms_per_batch"]
        f["pcm_gb_per_s"] = pcm_bytes / (f["ms_per_batch"] * 1e-3) / 1e9

    # the three kernels, in a run of their own (events around every launch)
    lib.bl_amd_profile_reset()
    lib.bl_amd_profile(1)
    for _ in range(a.reps):
        rhythm(onsets=False, acf=False)()
    torch.cuda.synchronize()
    lib.bl_amd_profile(0)
    kernels = {}
    for name in ("rhythm_hops", "rhythm_acf", "rhythm_pick"):
        k = C.c_int(0)
        ms = lib.bl_amd_profile_ms(name.encode(), C.byref(k))
        kernels[name] = {"ms_per_batch": ms / a.reps, "launches": k.value,
                         "ratio_to_levels": ms / a.reps / yard["ms_per_batch"]}
    hops_ms = kernels["rhythm_hops"]["ms_per_batch"]
    kernels["rhythm_hops"]["pcm_gb_per_s"] = pcm_bytes / (hops_ms * 1e-3) / 1e9
    kernels["rhythm_hops"]["fraction_of_hbm_peak"] = kernels["rhythm_hops"]["pcm_gb_per_s"] / (HBM_PEAK_TBS * 1e3)
    hops = n // ch // rh.HOP
    kernels["rhythm_acf"]["multiply_adds"] = a.songs * (hops - 511) * 512
    kernels["rhythm_acf"]["multiply_adds_per_s"] = kernels["rhythm_acf"]["multiply_adds"] / (
        kernels["rhythm_acf"]["ms_per_batch"] * 1e-3)

    rec, _, _ = rh.fetch_rhythm(corpus)
    bpm, strength = rh.rhythm_bpm(rec)
    out = {
        "what": "bl_amd_rhythm_batch_device over a resident corpus, device events over `reps` back-to-back calls after "
                "`warmup` calls of every form; one call = memsets, k_rhythm_hops, k_rhythm_acf, k_rhythm_pick per "
                "launch group",
        "songs": a.songs, "seconds": a.seconds, "sample_rate": rate, "channels": ch, "hops_per_song": hops,
        "lag_min": a.lag_min, "lag_max": a.lag_max, "pcm_bytes": pcm_bytes, "reps": a.reps, "warmup": a.warmup,
        "forms": out_forms,
        "kernels": kernels,
        "kernels_what": "bl_amd_profile_ms over `reps` calls without the optional outputs, in a run of their own",
        "lag_stage_over_hop_pass": kernels["rhythm_acf"]["ms_per_batch"] / hops_ms,
        "yardstick": {"name": "bl_amd_levels_batch_device", "before": yard, "after": yard2,
                      "pcm_gb_per_s": pcm_bytes / (yard["ms_per_batch"] * 1e-3) / 1e9,
                      "what": "DeviceCorpus.levels() over the same arena in the same process, timed the same way before "
                              "and after the tempo calls; the ratios use the run before"},
        "hbm_peak_tb_per_s": HBM_PEAK_TBS,
        "device": torch.cuda.get_device_name(0),
        "device_state": state.summary(t0, t1),
        "check": {"hops": int(rec["hops"][0]), "status_all_ok": bool((rec["status"] == 0).all()),
                  "lag_min_seen": int(rec["lag"].min()), "lag_max_seen": int(rec["lag"].max()),
                  "bpm_of_song_0": float(bpm[0]), "strength_of_song_0": float(strength[0])},
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"levels_ms": yard["ms_per_batch"],
                      "forms_ms": {k: v["ms_per_batch"] for k, v in out_forms.items()},
                      "kernels_ms": {k: v["ms_per_batch"] for k, v in kernels.items()},
                      "lag_stage_over_hop_pass": out["lag_stage_over_hop_pass"]}))


if __name__ == "__main__":
    main()
