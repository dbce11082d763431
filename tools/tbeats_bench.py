#!/usr/bin/env python3
"""Throughput of the beats that follow the tempo over time (bl_amd_tbeats_device), written down, not asserted.

    python tools/tbeats_bench.py [--shapes 8192x180,1024x30] [--windows 128x16,256x4]
                                 [--out profiles/tbeats_throughput.json]

For every shape (songs x seconds of mono PCM at 22 050 Hz, synthesised on the device) the tempo call gives the onset
curves and the tempogram at every S x m of --windows its frames.  The yardstick is bl_amd_beats_device over the same
curves at each song's median lag (the tempogram's lag_median at the first window; the tempo call's lag, and failing
that 43, where a song has none).  The legs of the new call, all without the optional outputs as the yardstick is:

    constant        every frame at the song's median lag: the same arithmetic as the yardstick, so the ratio is the cost
                    of the run machinery (the track kernel, the search for a run's end, one table for one run)
    tgram_SxM       the tempogram's own frames read in place (stride 40), no fold
    churn           a synthetic track that alternates between the median lag and the median lag + 1 from frame to frame:
                    a run change, with a new penalty table, every frame of 128 hops

The yardstick and the legs take turns in alternating windows of one run: a turn is --reps back-to-back calls between
device events, and the turns come round --rounds times.  The kernels (beats; tbeats_track, tbeats) are timed through
bl_amd_profile_ms and bl_amd_tbeats_profile_ms in turns of their own in the same rounds.  The device's clocks are sampled
over the whole run.  Needs a GPU: there is no other way to get a time."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TB_KERNELS = ("tbeats_track", "tbeats")
TIGHT, FALLBACK_LAG = 128, 43


def timed(torch, reps, call):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        call()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def summary(ms):
    s = sorted(ms)
    return {"ms_per_call": sum(s) / len(s), "ms_per_call_min": s[0], "ms_per_call_max": s[-1], "turns": ms}


def shape_part(torch, lib, a, n, seconds):
    import numpy as np

    import bliss_amd
    import bliss_amd.rhythm as rh
    import bliss_amd.tempogram as tg
    from bliss_amd.records import TBEATS_DTYPE
    samples = seconds * 22050
    corpus = bliss_amd.DeviceCorpus([samples] * n, 1, seconds)
    corpus.synth(seed_base=1, sample_rate=22050)
    rec, ons, _ = rh.rhythm_device(corpus, 20, 200, onsets=True)
    torch.cuda.synchronize()
    hops = samples // 128
    hop_list = [hops] * n
    h_hops = (C.c_int32 * n)(*hop_list)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda x: C.c_void_p(x.data_ptr())
    tgrams = {}
    for stride, blocks in a.windows:
        p = tg.params(stride, blocks)
        tgrams[(stride, blocks)] = (p, tg.tgram_device(ons, hop_list, p))
    torch.cuda.synchronize()
    p0, t0 = tgrams[a.windows[0]]
    med = tg.tgram_to_numpy(t0["songs"].cpu().numpy().tobytes())["lag_median"].astype(np.int32)
    tempo = rh.rhythm_to_numpy(rec.cpu().numpy().tobytes())["lag"].astype(np.int32)
    period = np.where(med > 0, med, np.where(tempo > 1, tempo, FALLBACK_LAG)).astype(np.int32)
    d_period = torch.from_numpy(period).cuda()
    f0 = t0["counts"][0]
    frames = max(f0, 1)
    d_const = torch.from_numpy(np.repeat(period, frames)).cuda()
    d_churn = torch.from_numpy((np.repeat(period, frames).reshape(n, frames) +
                                (np.arange(frames) & 1)[None, :]).astype(np.int32).reshape(-1)).cuda()
    flags = torch.empty(n * hops, dtype=torch.uint8, device="cuda")
    fixed_out = torch.empty(n * 40, dtype=torch.uint8, device="cuda")
    out = torch.empty(n * 64, dtype=torch.uint8, device="cuda")

    def yard():
        rc = lib.bl_amd_beats_device(ptr(ons), h_hops, n, ptr(d_period), 4, TIGHT, ptr(fixed_out), ptr(flags), None, None,
                                     stream)
        assert rc == 0

    def leg(lag_ptr, lag_stride, count, bp):
        h_frames = (C.c_int32 * n)(*([count] * n))

        def call():
            rc = lib.bl_amd_tbeats_device(ptr(ons), h_hops, h_frames, n, lag_ptr, lag_stride, None, 4, C.byref(bp),
                                          ptr(out), ptr(flags), None, None, None, stream)
            assert rc == 0
        return call

    bp0 = tg.beats_params(p0, TIGHT)
    calls = {"beats_fixed": yard, "constant": leg(ptr(d_const), 4, frames, bp0)}
    meta = {"constant": dict(frames_per_song=frames, seg=bp0.seg, origin=bp0.origin)}
    for (stride, blocks), (p, t) in tgrams.items():
        f = t["counts"][0]
        if f < 1:
            continue
        name = f"tgram_S{stride}_m{blocks}"
        bp = tg.beats_params(p, TIGHT)
        calls[name] = leg(C.c_void_p(t["frames"].data_ptr() + 32), 40, f, bp)
        meta[name] = dict(frames_per_song=f, seg=bp.seg, origin=bp.origin)
    calls["churn"] = leg(ptr(d_churn), 4, frames, bp0)
    meta["churn"] = dict(frames_per_song=frames, seg=bp0.seg, origin=bp0.origin)
    checks = {}
    for k, c in calls.items():
        for _ in range(a.warmup):
            c()
        torch.cuda.synchronize()
        if k == "beats_fixed":
            got = rh.beats_to_numpy(fixed_out.cpu().numpy().tobytes())
            checks[k] = {"n_beats_mean": float(got["n_beats"].mean()), "with_tempo": int((got["status"] == 0).sum())}
        else:
            got = np.frombuffer(out.cpu().numpy().tobytes(), TBEATS_DTYPE)
            checks[k] = {"n_beats_mean": float(got["n_beats"].mean()), "n_runs_mean": float(got["n_runs"].mean()),
                         "n_filled_mean": float(got["n_filled"].mean()), "with_tempo": int((got["status"] == 0).sum())}
    wall = {k: [] for k in calls}
    kern = {k: {name: [] for name in (("beats",) if k == "beats_fixed" else TB_KERNELS)} for k in calls}
    clock = []
    for _ in range(a.rounds):
        for k, c in calls.items():
            clock.append({"call": k, "t": time.time()})
            wall[k].append(timed(torch, a.reps, c))
        lib.bl_amd_profile(1)          # the kernels in turns of their own: the events would sit between the calls
        for k, c in calls.items():
            torch.cuda.synchronize()
            if k == "beats_fixed":     # forget what was collected before
                lib.bl_amd_profile_reset()
            else:
                for name in TB_KERNELS:
                    lib.bl_amd_tbeats_profile_ms(name.encode(), None)
            for _ in range(a.reps):
                c()
            torch.cuda.synchronize()
            for name in kern[k]:
                fn = lib.bl_amd_profile_ms if k == "beats_fixed" else lib.bl_amd_tbeats_profile_ms
                kern[k][name].append(fn(name.encode(), None) / a.reps)
        lib.bl_amd_profile(0)
    res = {k: dict(summary(v), kernels={name: summary(ms) for name, ms in kern[k].items()}, check=checks[k])
           for k, v in wall.items()}
    yard_ms, yard_kernel = res["beats_fixed"]["ms_per_call"], res["beats_fixed"]["kernels"]["beats"]["ms_per_call"]
    for name, m in meta.items():
        r = res[name]
        track, grid = (r["kernels"][k]["ms_per_call"] for k in TB_KERNELS)
        r.update(m, ratio_to_fixed=r["ms_per_call"] / yard_ms, kernels_ratio_to_fixed=(track + grid) / yard_kernel,
                 grid_kernel_ratio_to_fixed=grid / yard_kernel, track_share=track / (track + grid))
        print(f"{n}x{seconds} {name}: {r['ms_per_call']:.3f} ms ({r['ratio_to_fixed']:.3f} x the fixed tracker's "
              f"{yard_ms:.3f} ms), track kernel {100 * r['track_share']:.2f} %", file=sys.stderr, flush=True)
    return {"songs": n, "seconds": seconds, "hops_per_song": hops, "period_median": float(np.median(period)),
            "calls": res, "clock": clock}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="8192x180,1024x30")
    ap.add_argument("--windows", default="128x16,256x4", help="S x m, comma separated; the first gives the median lag")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tbeats_throughput.json"))
    a = ap.parse_args()
    a.windows = [tuple(int(v) for v in s.split("x")) for s in a.windows.split(",")]
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]

    import torch

    from bench import DeviceState
    if not torch.cuda.is_available():
        sys.exit("tbeats_bench.py needs a GPU: a time taken anywhere else says nothing")
    import bliss_amd
    from bliss_amd import _lib
    lib = bliss_amd.load()
    assert lib.bl_amd_init(0) == 0
    state = DeviceState(DeviceState.pci_address(0))
    state.start()
    t0 = time.perf_counter()
    out = {"what": "bl_amd_tbeats_device beside bl_amd_beats_device (the yardstick, at each song's median lag) over the "
                   "same onset curves, one arena per shape: turns of `reps` back-to-back calls between device events in "
                   "alternating windows of one run, `rounds` rounds, after `warmup` calls; the kernels through "
                   "bl_amd_profile_ms and bl_amd_tbeats_profile_ms in turns of their own in the same rounds; `clock`: "
                   "the wall time at which each timed turn began",
           "reps": a.reps, "rounds": a.rounds, "warmup": a.warmup, "tight": TIGHT,
           "library": os.path.basename(_lib.LIB_PATH), "device": torch.cuda.get_device_name(0), "shapes": []}
    for n, seconds in shapes:
        out["shapes"].append(shape_part(torch, lib, a, n, seconds))
        torch.cuda.empty_cache()
    state.stop_flag = True
    state.join()
    out["device_state"] = state.summary(t0, time.perf_counter())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for s in out["shapes"]:
        print(json.dumps({"songs": s["songs"], "seconds": s["seconds"],
                          "ms": {k: round(v["ms_per_call"], 3) for k, v in s["calls"].items()},
                          "x_fixed": {k: round(v["ratio_to_fixed"], 3) for k, v in s["calls"].items()
                                      if "ratio_to_fixed" in v},
                          "track_share": {k: round(v["track_share"], 4) for k, v in s["calls"].items()
                                          if "track_share" in v}}), flush=True)


if __name__ == "__main__":
    main()
