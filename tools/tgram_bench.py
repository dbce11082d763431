#!/usr/bin/env python3
"""Throughput of the tempo over time (bl_amd_tgram_device), written down, not asserted.

    python tools/tgram_bench.py [--shapes 8192x180,1024x30] [--windows 128x16,256x4] [--asm bl_tgram_kernels.s]
                                [--out profiles/tgram_throughput.json]

For every shape (songs x seconds of mono PCM at 22 050 Hz, synthesised on the device) the tempo call
(bl_amd_rhythm_batch_device with its onset curve) and the tempogram over that curve, at each S x m of --windows without
and with the lag products (d_gram_out), take turns in alternating windows of one run.  The yardstick is the lag stage of
the tempo call, its kernels rhythm_acf + rhythm_pick through bl_amd_profile_ms: it forms the same multiply-adds over the
same curve once, for one frame per song.  The tempogram's kernels are timed through bl_amd_tgram_profile_ms in the same
turns.  A ratio of the block kernel to the yardstick well above 1, without the lag products, would mean that the
sharing of block rows between frames is not working.

The block kernel is also set against an issue floor of its own instruction stream: the vector instructions of one turn
of its product loop (32 products per lane; counted in the kernel's disassembly, `hipcc -S --offload-device-only
bl_tgram_kernels.hip`, the innermost loop of k_tgram_blocks; --asm recounts them from such a file), of which the 64-bit
multiply-adds issue at a quarter of the plain rate, times the turns of the call (S / 16 per block and lane, f + m - 1
blocks for a run of f frames), over 256 CUs x 4 SIMDs x 32 lanes per clock, at --clock-ghz and at the mean shader clock
sampled over the run.

A turn is --reps back-to-back calls between device events, and the turns come round --rounds times.  Needs a GPU:
there is no other way to get a time."""
import argparse
import ctypes as C
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LANES_PER_CLOCK = 256 * 4 * 32
N_CU, RUN_FRAMES = 256, 64          # the launcher's run split: blk_tgram_blocks
# the product loop of k_tgram_blocks as compiled for gfx950 when this was written, per turn of 32 products a lane
LOOP_COUNTS = {"valu": 34, "mad64": 32, "ds": 7}
TG_KERNELS = ("tgram_blocks", "tgram_songs")
RH_KERNELS = ("rhythm_acf", "rhythm_pick")


def loop_counts(path):
    lines = open(path).read().split("\n")
    start = next((i for i, ln in enumerate(lines) if ln.startswith("_Z14k_tgram_blocks")), None)
    if start is None:
        raise SystemExit(f"{path}: no k_tgram_blocks in it")
    end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
    heads = [i for i in range(start, end) if "Inner Loop Header" in lines[i]]
    best = None
    for h in heads:       # the innermost loop that holds the 64-bit multiply-adds
        back = next(i for i in range(h, end) if re.search(r"s_c?branch", lines[i]))
        body = lines[h:back + 1]
        mad = sum(1 for ln in body if re.match(r"^\s+v_mad_u64_u32", ln))
        if mad and (best is None or mad > best["mad64"]):
            best = {"valu": sum(1 for ln in body if re.match(r"^\s+v_", ln)), "mad64": mad,
                    "ds": sum(1 for ln in body if re.match(r"^\s+ds_", ln))}
    if best is None:
        raise SystemExit(f"{path}: no product loop found in k_tgram_blocks")
    return best


def turns_of(n, frames, stride, blocks):
    """turns of the product loop per lane over a call of n songs of `frames` frames each"""
    if frames < 1:
        return 0
    want = (N_CU * 8 + n - 1) // n
    run = max(RUN_FRAMES, (frames + want - 1) // want)
    total_blocks = 0
    for f0 in range(0, frames, run):
        total_blocks += min(run, frames - f0) + blocks - 1
    return n * total_blocks * (stride // 16)


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


def shape_part(torch, lib, a, n, seconds, counts):
    import bliss_amd
    import bliss_amd.rhythm as rh
    import bliss_amd.tempogram as tg
    samples = seconds * 22050
    corpus = bliss_amd.DeviceCorpus([samples] * n, 1, seconds)
    corpus.synth(seed_base=1, sample_rate=22050)
    rec, ons, _ = rh.rhythm_device(corpus, 20, 200, onsets=True)
    torch.cuda.synchronize()
    hops = samples // 128
    h_hops = (C.c_int32 * n)(*([hops] * n))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda x: C.c_void_p(x.data_ptr())

    def tempo():
        rc = lib.bl_amd_rhythm_batch_device(ptr(corpus.pcm), corpus.desc, n, 20, 200, ptr(rec), ptr(ons), n * hops, None,
                                            stream)
        assert rc == 0

    calls, meta, keep = {"tempo_call": tempo}, {}, []
    for stride, blocks in a.windows:
        p = tg.params(stride, blocks)
        f = tg.frames_count(hops, p)
        songs = torch.empty(n * 56, dtype=torch.uint8, device="cuda")
        frames = torch.empty(max(n * f, 1) * 40, dtype=torch.uint8, device="cuda")
        gram = torch.empty((max(n * f, 1), 512), dtype=torch.int64, device="cuda")
        keep.append((p, songs, frames, gram))
        for with_gram in (False, True):
            def call(p=p, f=f, songs=songs, frames=frames, g=gram if with_gram else None):
                rc = lib.bl_amd_tgram_device(ptr(ons), h_hops, n, C.byref(p), ptr(songs), ptr(frames), n * f,
                                             ptr(g) if g is not None else None, stream)
                assert rc == 0
            name = f"tgram_S{stride}_m{blocks}" + ("_gram" if with_gram else "")
            calls[name] = call
            meta[name] = dict(stride=stride, blocks=blocks, frames_per_song=f, gram=with_gram,
                              loop_turns_per_lane=turns_of(n, f, stride, blocks))
    for c in calls.values():
        for _ in range(a.warmup):
            c()
    torch.cuda.synchronize()
    wall = {k: [] for k in calls}
    kern = {k: {name: [] for name in (RH_KERNELS if k == "tempo_call" else TG_KERNELS)} for k in calls}
    for _ in range(a.rounds):
        for k, c in calls.items():
            wall[k].append(timed(torch, a.reps, c))
        lib.bl_amd_profile(1)          # the kernels in turns of their own: the events would sit between the calls
        for k, c in calls.items():
            if k == "tempo_call":      # forget what was collected before
                torch.cuda.synchronize()
                lib.bl_amd_profile_reset()
            for name in kern[k]:
                if k != "tempo_call":
                    lib.bl_amd_tgram_profile_ms(name.encode(), None)
            for _ in range(a.reps):
                c()
            torch.cuda.synchronize()
            for name in kern[k]:
                fn = lib.bl_amd_profile_ms if k == "tempo_call" else lib.bl_amd_tgram_profile_ms
                kern[k][name].append(fn(name.encode(), None) / a.reps)
        lib.bl_amd_profile(0)
    res = {k: dict(summary(v), kernels={name: summary(ms) for name, ms in kern[k].items()}) for k, v in wall.items()}
    yard = sum(res["tempo_call"]["kernels"][name]["ms_per_call"] for name in RH_KERNELS)
    res["tempo_call"]["lag_stage_ms"] = yard
    res["tempo_call"]["multiply_adds"] = float(n) * 512 * max(hops - 511, 0)
    for name, m in meta.items():
        r = res[name]
        blocks_ms = r["kernels"]["tgram_blocks"]["ms_per_call"]
        slots = m["loop_turns_per_lane"] * 256.0 * (counts["valu"] + 3 * counts["mad64"])
        floor_ms = slots / (LANES_PER_CLOCK * a.clock_ghz * 1e9) * 1e3
        r.update(m, ratio_to_lag_stage=(blocks_ms + r["kernels"]["tgram_songs"]["ms_per_call"]) / yard,
                 blocks_ratio_to_lag_stage=blocks_ms / yard,
                 multiply_adds=m["loop_turns_per_lane"] * 256.0 * 32, issue_floor_ms=floor_ms,
                 ratio_to_issue_floor=blocks_ms / floor_ms if floor_ms > 0 else None)
        got = tg.tgram_to_numpy(keep[[w for w in a.windows].index((m["stride"], m["blocks"]))][1].cpu().numpy().tobytes())
        r["check"] = {"frames": int(got["frames"][0]), "n_tempo_mean": float(got["n_tempo"].mean()),
                      "n_jumps_mean": float(got["n_jumps"].mean())}
        print(f"{n}x{seconds} {name}: {r['ms_per_call']:.3f} ms, blocks {blocks_ms:.3f} ms, lag stage {yard:.3f} ms",
              file=sys.stderr, flush=True)
    return {"songs": n, "seconds": seconds, "hops_per_song": hops, "calls": res}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="8192x180,1024x30")
    ap.add_argument("--windows", default="128x16,256x4", help="S x m, comma separated")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    ap.add_argument("--asm", default=None, help="disassembly of bl_tgram_kernels.hip to count the loop from")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tgram_throughput.json"))
    a = ap.parse_args()
    a.windows = [tuple(int(v) for v in s.split("x")) for s in a.windows.split(",")]
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    counts = loop_counts(a.asm) if a.asm else LOOP_COUNTS

    import torch

    from bench import DeviceState
    if not torch.cuda.is_available():
        sys.exit("tgram_bench.py needs a GPU: a time taken anywhere else says nothing")
    import bliss_amd
    from bliss_amd import _lib
    lib = bliss_amd.load()
    assert lib.bl_amd_init(0) == 0
    state = DeviceState(DeviceState.pci_address(0))
    state.start()
    t0 = time.perf_counter()
    out = {"what": "bl_amd_tgram_device beside the bl_amd_rhythm_batch_device call that produces its onset curves, over "
                   "one arena per shape: turns of `reps` back-to-back calls between device events, `rounds` rounds, after "
                   "`warmup` calls; the kernels through bl_amd_profile_ms and bl_amd_tgram_profile_ms in turns of their "
                   "own in the same rounds; the yardstick is rhythm_acf + rhythm_pick; the block kernel against the "
                   "issue floor the tool's docstring defines",
           "reps": a.reps, "rounds": a.rounds, "warmup": a.warmup, "loop_counts": counts,
           "lanes_per_clock": LANES_PER_CLOCK, "clock_ghz": a.clock_ghz, "library": os.path.basename(_lib.LIB_PATH),
           "device": torch.cuda.get_device_name(0), "shapes": []}
    for n, seconds in shapes:
        out["shapes"].append(shape_part(torch, lib, a, n, seconds, counts))
        torch.cuda.empty_cache()
    state.stop_flag = True
    state.join()
    out["device_state"] = state.summary(t0, time.perf_counter())
    mhz = (out["device_state"].get("sclk_mhz") or {}).get("mean")
    if mhz:   # the issue floor assumes --clock-ghz; the same ratio at the mean shader clock of the whole run
        out["mean_clock_mhz"] = mhz
        for s in out["shapes"]:
            for r in s["calls"].values():
                if "issue_floor_ms" in r:
                    r["issue_floor_ms_at_mean_clock"] = r["issue_floor_ms"] * a.clock_ghz * 1e3 / mhz
                    r["ratio_to_issue_floor_at_mean_clock"] = \
                        r["kernels"]["tgram_blocks"]["ms_per_call"] / r["issue_floor_ms_at_mean_clock"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for s in out["shapes"]:
        print(json.dumps({"songs": s["songs"], "seconds": s["seconds"],
                          "lag_stage_ms": round(s["calls"]["tempo_call"]["lag_stage_ms"], 3),
                          "ms": {k: round(v["ms_per_call"], 3) for k, v in s["calls"].items()},
                          "x_lag_stage": {k: round(v["ratio_to_lag_stage"], 2) for k, v in s["calls"].items()
                                          if "ratio_to_lag_stage" in v},
                          "x_floor": {k: round(v["ratio_to_issue_floor"] or 0.0, 2) for k, v in s["calls"].items()
                                      if "ratio_to_issue_floor" in v}, "mean_clock_mhz": mhz}), flush=True)


if __name__ == "__main__":
    main()
