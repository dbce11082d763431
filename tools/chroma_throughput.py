#!/usr/bin/env python3
"""Throughput of the chroma call (bl_amd_chroma_batch_device), written down, not asserted, on two arenas of synthetic
22 050 Hz stereo songs resident in HBM: 1 024 songs of 30 s and 8 192 songs of 180 s.

    python tools/chroma_throughput.py [--reps 10] [--out profiles/chroma_throughput.json]

Every arena is measured by a child process of its own (`--one SONGS SECONDS`) under its own time limit, and the chain
stops at the first child that fails or runs out of time: nothing more is started on a device that has just misbehaved.
The parent never touches the device.

A child times, with device events over --reps back-to-back calls after a warm-up, the whole chroma call without and
with the frame records; then, in runs of their own through bl_amd_profile, the pitch kernel and the key kernel
("chroma_pitch", "chroma_key").  The yardsticks are measured in the same process over the same arena, as they are on
the parent commit: bl_amd_levels_batch_device (the project's leanest pass over the PCM), the tempo's hop pass
("rhythm_hops") and the analysis' window kernel ("env_windows").  Every time is also given as a ratio to them, and the
pitch kernel's distance from its two floors is worked out: the PCM stream at the level pass's rate, and the int8
operations of the live coefficient blocks at the matrix cores' peak.  Needs a GPU: there is no other way to get a
time."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARENAS = ((1024, 30, 240), (8192, 180, 600))   # songs, seconds, the child's time limit in seconds
HBM_PEAK_TBS = 8.0        # the part's specified peak
INT8_PEAK_OPS = 5.0e15    # dense int8 operations per second of the matrix cores: twice the 2.5e15 specified for bf16


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


def profiled(torch, lib, reps, call, names):
    """ms per call of the named kernels over `reps` calls with events around every launch"""
    lib.bl_amd_profile_reset()
    lib.bl_amd_profile(1)
    for _ in range(reps):
        call()
    torch.cuda.synchronize()
    lib.bl_amd_profile(0)
    out = {}
    for name in names:
        k = C.c_int(0)
        ms = lib.bl_amd_profile_ms(name.encode(), C.byref(k))
        out[name] = {"ms_per_batch": ms / reps, "launches": k.value}
    return out


def live_operations(frames, channels):
    """int8 operations (multiply and add counted apart) of `frames` frames: per live block of 128 samples and row tile
    of 16, two byte planes per channel"""
    import numpy as np

    import bliss_amd.chroma as ch
    re, im, _, _ = ch.chroma_table()
    rows = np.stack([re, im], axis=1).reshape(96, 4096)
    live = (rows.reshape(6, 16, 32, 128) != 0).any(axis=(1, 3)).sum()        # (row tile, block) pairs with a coefficient
    return int(live), int(live) * 16 * 128 * 2 * 2 * channels * frames, 96 * 4096 * 2 * 2 * channels * frames


def one(songs, seconds, reps, warmup):
    import torch

    import bliss_amd
    import bliss_amd.chroma as ch
    import bliss_amd.rhythm as rh
    from bench import DeviceState
    if not torch.cuda.is_available():
        sys.exit("chroma_throughput.py needs a GPU: a time taken anywhere else says nothing")
    rate, chn = 22050, 2
    n = rate * chn * seconds

    def stage(what):       # a line per stage on stderr: a long arena is seen to be alive
        print(f"[{songs} x {seconds} s] {what}", file=sys.stderr, flush=True)
    stage("corpus")
    corpus = bliss_amd.DeviceCorpus([n] * songs, chn, seconds)
    corpus.synth(seed_base=1, sample_rate=rate)
    torch.cuda.synchronize()
    lib, pcm_bytes = corpus.lib, corpus.pcm_bytes

    def chroma(frames):
        return lambda: ch.chroma_device(corpus, frames=frames)

    def rhythm():
        rh.rhythm_device(corpus, 58, 172, onsets=False, acf=False)
    stage("warm-up")
    for _ in range(warmup):
        corpus.levels()
        rhythm()
        chroma(False)()
        chroma(True)()
    corpus.analyze()
    torch.cuda.synchronize()
    stage("whole calls")
    state = DeviceState(DeviceState.pci_address(0))
    state.start()
    t0 = time.perf_counter()
    yard = timed(torch, reps, corpus.levels)
    forms = {"records_only": timed(torch, reps, chroma(False)), "with_frames": timed(torch, reps, chroma(True))}
    yard2 = timed(torch, reps, corpus.levels)      # the yardstick again behind the calls: its own spread
    t1 = time.perf_counter()
    state.stop_flag = True
    state.join()
    stage("kernels")
    kernels = profiled(torch, lib, reps, chroma(False), ("chroma_pitch", "chroma_key"))
    hops = profiled(torch, lib, reps, rhythm, ("rhythm_hops",))["rhythm_hops"]
    env = profiled(torch, lib, 1, corpus.analyze, ("env_windows",))["env_windows"]
    rec, _ = ch.fetch_chroma(corpus)
    frames = int(rec["frames"].sum())
    pairs, ops_live, ops_dense = live_operations(frames, chn)
    pitch_ms, level_ms = kernels["chroma_pitch"]["ms_per_batch"], yard["ms_per_batch"]
    for f in list(forms.values()) + list(kernels.values()):
        f["ratio_to_levels"] = f["ms_per_batch"] / level_ms
        f["ratio_to_rhythm_hops"] = f["ms_per_batch"] / hops["ms_per_batch"]
        f["ratio_to_env_windows"] = f["ms_per_batch"] / env["ms_per_batch"]
    return {
        "songs": songs, "seconds": seconds, "sample_rate": rate, "channels": chn, "frames_per_song": int(rec["frames"][0]),
        "pcm_bytes": pcm_bytes, "reps": reps, "warmup": warmup,
        "forms": forms, "kernels": kernels,
        "kernels_what": "bl_amd_profile_ms over `reps` calls without the frame records, in a run of their own",
        "yardsticks": {
            "levels": {"name": "bl_amd_levels_batch_device", "before": yard, "after": yard2,
                       "pcm_gb_per_s": pcm_bytes / (level_ms * 1e-3) / 1e9,
                       "what": "DeviceCorpus.levels() timed the same way before and after the chroma calls; the ratios "
                               "use the run before"},
            "rhythm_hops": dict(hops, what="k_rhythm_hops of bl_amd_rhythm_batch_device, bl_amd_profile_ms over `reps` "
                                           "calls"),
            "env_windows": dict(env, what="the window kernel of one analysis of the arena, bl_amd_profile_ms"),
        },
        "floors": {
            "pcm_stream_ms": level_ms,
            "pitch_kernel_over_pcm_stream": pitch_ms / level_ms,
            "pitch_kernel_pcm_gb_per_s": pcm_bytes / (pitch_ms * 1e-3) / 1e9,
            "live_tile_block_pairs_of_192": pairs,
            "int8_operations_live": ops_live, "int8_operations_dense": ops_dense,
            "int8_peak_operations_per_s": INT8_PEAK_OPS,
            "matrix_cores_ms": ops_live / INT8_PEAK_OPS * 1e3,
            "pitch_kernel_over_matrix_cores": pitch_ms / (ops_live / INT8_PEAK_OPS * 1e3),
            "pitch_kernel_int8_operations_per_s": ops_live / (pitch_ms * 1e-3),
        },
        "whole_call_exceeds_env_windows": forms["records_only"]["ms_per_batch"] > env["ms_per_batch"],
        "hbm_peak_tb_per_s": HBM_PEAK_TBS,
        "device": torch.cuda.get_device_name(0),
        "device_state": state.summary(t0, t1),
        "check": {"status_all_ok": bool((rec["status"] == 0).all()), "keys_seen": sorted({int(k) for k in rec["key"]})[:24],
                  "key_of_song_0": ch.key_names(rec[:1])[0], "score_of_song_0": int(rec["score"][0])},
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--one", nargs=2, type=int, metavar=("SONGS", "SECONDS"), help="measure this arena and print its JSON")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chroma_throughput.json"))
    a = ap.parse_args()
    if a.one:
        print("RESULT " + json.dumps(one(a.one[0], a.one[1], a.reps, a.warmup)))
        return 0
    arenas = []
    for songs, seconds, limit in ARENAS:          # the chain: the next arena only behind a clean end of this one
        cmd = [sys.executable, os.path.abspath(__file__), "--one", str(songs), str(seconds), "--reps", str(a.reps),
               "--warmup", str(a.warmup)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"arena {songs} x {seconds} s ran out of its {limit} s: stopping", file=sys.stderr)
            return 1
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or len(lines) != 1:
            print(f"arena {songs} x {seconds} s failed with status {r.returncode}: stopping", file=sys.stderr)
            return 1
        arenas.append(json.loads(lines[0][len("RESULT "):]))
    out = {
        "what": "bl_amd_chroma_batch_device over a resident corpus, device events over `reps` back-to-back calls after "
                "`warmup` calls of every form; one call = a memset, k_chroma_pitch and k_chroma_key per launch group; "
                "each arena in a process of its own",
        "arenas": arenas,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for r in arenas:
        print(json.dumps({"songs": r["songs"], "seconds": r["seconds"], "levels_ms": r["floors"]["pcm_stream_ms"],
                          "forms_ms": {k: v["ms_per_batch"] for k, v in r["forms"].items()},
                          "kernels_ms": {k: v["ms_per_batch"] for k, v in r["kernels"].items()},
                          "rhythm_hops_ms": r["yardsticks"]["rhythm_hops"]["ms_per_batch"],
                          "env_windows_ms": r["yardsticks"]["env_windows"]["ms_per_batch"],
                          "over_pcm_stream": r["floors"]["pitch_kernel_over_pcm_stream"],
                          "over_matrix_cores": r["floors"]["pitch_kernel_over_matrix_cores"]}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
