#!/usr/bin/env python3
"""Throughput of the chord sequences (bl_amd_chords_device), written down, not asserted.

    python tools/chords_bench.py [--shapes 8192x180,1024x30] [--pools 1,4] [--asm bl_chords_kernels.s]
                                 [--spw 1,2] [--out profiles/chords_throughput.json]

For every shape (songs x seconds of mono PCM at 22 050 Hz, synthesised on the device) the chroma call that produces the
frames (bl_amd_chroma_batch_device with frames), bl_amd_cover_units_device at each pool of --pools over those frames and
the chords call over those units take turns in alternating windows of one run, the chords call without and with its two
optional outputs (labels and counts).  The ratio to the chroma call is the figure a caller plans with.

There is no earlier implementation to compare with, so the forward kernel is also set against an issue floor of its own
instruction stream: the vector instructions of one round of its loop (four units; counted in the kernel's own
disassembly, `hipcc -S --offload-device-only bl_chords_kernels.hip`, the loop of k_chords_forward<SPW>; --asm recounts
them from such a file) times the rounds of the call (per wavefront the rounds of its longest song) times 64 lanes, over
256 CUs x 4 SIMDs x 32 lanes per clock (a wave's vector instruction takes a SIMD two cycles when several waves issue), at
--clock-ghz and at the mean shader clock sampled over the run.  A round decides 4 x 625 candidates per song, so the
count per candidate is the round's count over 2500 SPW.  The cross-lane reads of the two-song form are LDS-pipe
instructions (ds_bpermute_b32) and are counted beside the vector instructions, not among them.

--spw 1,2 adds the A/B of the songs per wavefront: it needs the measurement build (`make measure`, loaded through
BLISS_AMD_LIB), which reads BL_AMD_CHORDS_SPW at every call; the two forms then take turns in the same alternating
windows.  The product library ignores the variable, and the tool says so in its output.

A window is about --window-ms of back-to-back calls (--reps at least) between device events, and the windows take turns
--rounds times.  The kernels are timed in a run of their own through bl_amd_profile and bl_amd_chords_profile_ms; the
back-trace's share is its kernel's time over the two kernels' sum.  Needs a GPU: there is no other way to get a time."""
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
ROUND_UNITS, CANDIDATES = 4, 625
# the loop of k_chords_forward<SPW> as compiled for gfx950 when this was written: vector and LDS-pipe instructions a round
LOOP_COUNTS = {1: {"valu": 318, "ds": 0}, 2: {"valu": 219, "ds": 101}}
KERNELS = ("chords_forward", "chords_trace")


def loop_counts(path, spw):
    """the vector and the LDS-pipe instructions of the loop of k_chords_forward<spw>, from the kernel's disassembly;
    blocks of the loop the compiler placed behind its back branch count too"""
    lines = open(path).read().split("\n")
    start = next((i for i, ln in enumerate(lines) if ln.startswith(f"_Z16k_chords_forwardILi{spw}E")), None)
    if start is None:
        raise SystemExit(f"{path}: no k_chords_forward<{spw}> in it")
    end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
    head = next(i for i in range(start, end) if "Inner Loop Header" in lines[i])
    label = lines[head].split(":")[0]
    back = max(i for i in range(head, end) if re.search(r"s_c?branch\S*\s+" + re.escape(label) + r"\b", lines[i]))
    body, inside = list(lines[head:back + 1]), False
    for ln in lines[back + 1:end]:
        if re.match(r"^\.LBB", ln):
            inside = "in Loop: Header=" + label[2:] in ln
        elif inside:
            body.append(ln)
    return {"valu": sum(1 for ln in body if re.match(r"^\s+v_", ln)), "ds": sum(1 for ln in body if re.match(r"^\s+ds_", ln))}


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


def kernels_ms(torch, lib, a, call):
    for name in KERNELS:
        lib.bl_amd_chords_profile_ms(name.encode(), None)   # forget what was collected before
    lib.bl_amd_profile(1)
    for _ in range(a.reps):
        call()
    torch.cuda.synchronize()
    lib.bl_amd_profile(0)
    out = {}
    for name in KERNELS:
        k = C.c_int(0)
        out[name] = {"ms_per_call": lib.bl_amd_chords_profile_ms(name.encode(), C.byref(k)) / a.reps, "launches": k.value}
    return out


def shape_part(torch, lib, a, n, seconds, counts_of):
    import bliss_amd
    import bliss_amd.chords as chords
    import bliss_amd.chroma as ch
    samples = seconds * 22050
    corpus = bliss_amd.DeviceCorpus([samples] * n, 1, seconds)
    corpus.synth(seed_base=1, sample_rate=22050)
    rec, frames = ch.chroma_device(corpus, frames=True)
    t = max(0, (samples - 4096) // 2048 + 1)
    fcounts = (C.c_int32 * n)(*([t] * n))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
    hist = torch.empty(n * 25, dtype=torch.int32, device="cuda")
    p = chords.params()
    ptr = lambda x: C.c_void_p(x.data_ptr())

    def chroma():
        rc = lib.bl_amd_chroma_batch_device(ptr(corpus.pcm), corpus.desc, n, ptr(rec), ptr(frames), n * t, stream)
        assert rc == 0

    calls, meta, keep = {"chroma_with_frames": chroma}, {}, []
    for pool in a.pools:
        u = t // pool
        units = torch.empty(max(n * u, 1) * 16, dtype=torch.uint8, device="cuda")
        labels = torch.empty(max(n * u, 1), dtype=torch.uint8, device="cuda")
        ucounts = (C.c_int32 * n)(*([u] * n))
        keep.append((units, labels, ucounts))

        def units_call(pool=pool, u=u, units=units):
            rc = lib.bl_amd_cover_units_device(ptr(frames), fcounts, n, pool, ptr(units), n * u, stream)
            assert rc == 0
        units_call()
        calls[f"units_p{pool}"] = units_call
        for spw in a.spw or [None]:
            for outputs in (False, True):
                def call(u=u, units=units, ucounts=ucounts, lab=labels if outputs else None,
                         hs=hist if outputs else None, spw=spw):
                    if spw is not None:
                        os.environ["BL_AMD_CHORDS_SPW"] = str(spw)
                    rc = lib.bl_amd_chords_device(ptr(units), ucounts, n, n * u, C.byref(p), ptr(out),
                                                  ptr(lab) if lab is not None else None,
                                                  ptr(hs) if hs is not None else None, stream)
                    assert rc == 0
                name = f"chords_p{pool}" + (f"_spw{spw}" if spw is not None else "") + ("_outputs" if outputs else "")
                calls[name] = call
                meta[name] = dict(pool=pool, units_per_song=u, outputs=outputs,
                                  songs_per_wave=spw if spw is not None else chords.shape()[2])
    res = alternate(torch, a, calls)
    base = res["chroma_with_frames"]["ms_per_call"]
    for name, m in meta.items():
        r = res[name]
        spw, u = m["songs_per_wave"], m["units_per_song"]
        cnt = counts_of[spw]
        rounds = ((n + spw - 1) // spw) * ((u + ROUND_UNITS - 1) // ROUND_UNITS)
        floor_ms = rounds * cnt["valu"] * 64 / (LANES_PER_CLOCK * a.clock_ghz * 1e9) * 1e3
        ks = kernels_ms(torch, lib, a, calls[name])
        both = ks["chords_forward"]["ms_per_call"] + ks["chords_trace"]["ms_per_call"]
        fw = ks["chords_forward"]
        fw.update(issue_floor_ms=floor_ms, ratio_to_issue_floor=fw["ms_per_call"] / floor_ms if floor_ms > 0 else None)
        r.update(m, ratio_to_chroma=r["ms_per_call"] / base, ratio_to_units=r["ms_per_call"] / res[f"units_p{m['pool']}"]["ms_per_call"],
                 candidates=float(n) * u * CANDIDATES, rounds=rounds, valu_per_round=cnt["valu"], ds_per_round=cnt["ds"],
                 valu_per_candidate=cnt["valu"] / (ROUND_UNITS * CANDIDATES * spw), kernels=ks,
                 trace_share=ks["chords_trace"]["ms_per_call"] / both if both > 0 else None)
        got = chords.chords_to_numpy(out.cpu().numpy())
        r["check"] = {"changes_mean": float(got["changes"].mean()), "none_units_mean": float(got["none_units"].mean()),
                      "units": int(got["units"][0])}
        print(f"{n}x{seconds} {name}: {r['ms_per_call']:.3f} ms", file=sys.stderr, flush=True)
    os.environ.pop("BL_AMD_CHORDS_SPW", None)
    return {"songs": n, "seconds": seconds, "frames_per_song": t, "pcm_bytes": corpus.pcm_bytes, "calls": res}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="8192x180,1024x30")
    ap.add_argument("--pools", default="1,4")
    ap.add_argument("--spw", default="", help="1,2: the A/B of the songs per wavefront (measurement build only)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    ap.add_argument("--asm", default=None, help="disassembly of bl_chords_kernels.hip to count the loop from")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chords_throughput.json"))
    a = ap.parse_args()
    a.pools = [int(x) for x in a.pools.split(",")]
    a.spw = [int(x) for x in a.spw.split(",")] if a.spw else []
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    counts_of = {s: loop_counts(a.asm, s) for s in (1, 2)} if a.asm else LOOP_COUNTS

    import torch

    from bench import DeviceState
    if not torch.cuda.is_available():
        sys.exit("chords_bench.py needs a GPU: a time taken anywhere else says nothing")
    import bliss_amd
    from bliss_amd import _lib
    lib = bliss_amd.load()
    measure = "measure" in os.path.basename(_lib.LIB_PATH)
    if a.spw and not measure:
        sys.exit("--spw needs the measurement build: make -C bliss_amd/csrc measure, BLISS_AMD_LIB=.../libbliss_amd_measure.so")
    assert lib.bl_amd_init(0) == 0
    state = DeviceState(DeviceState.pci_address(0))
    state.start()
    t0 = time.perf_counter()
    out = {"what": "bl_amd_chords_device beside the bl_amd_chroma_batch_device call that produces the frames and the "
                   "bl_amd_cover_units_device call that produces its units, over one arena per shape: alternating "
                   "windows of about `window_ms` of back-to-back calls (`reps` at least) between device events, `rounds` "
                   "windows each, after `warmup` calls; the kernels through bl_amd_chords_profile_ms in a run of their "
                   "own; the forward kernel against the issue floor the tool's docstring defines",
           "reps": a.reps, "window_ms": a.window_ms, "rounds": a.rounds, "warmup": a.warmup, "loop_counts": counts_of,
           "lanes_per_clock": LANES_PER_CLOCK, "clock_ghz": a.clock_ghz, "library": os.path.basename(_lib.LIB_PATH),
           "songs_per_wave_ab": a.spw, "device": torch.cuda.get_device_name(0), "shapes": []}
    for n, seconds in shapes:
        out["shapes"].append(shape_part(torch, lib, a, n, seconds, counts_of))
        torch.cuda.empty_cache()
    state.stop_flag = True
    state.join()
    out["device_state"] = state.summary(t0, time.perf_counter())
    mhz = (out["device_state"].get("sclk_mhz") or {}).get("mean")
    if mhz:   # the issue floor assumes --clock-ghz; the same ratio at the mean shader clock of the whole run
        out["mean_clock_mhz"] = mhz
        for s in out["shapes"]:
            for r in s["calls"].values():
                if "kernels" in r:
                    fw = r["kernels"]["chords_forward"]
                    fw["issue_floor_ms_at_mean_clock"] = fw["issue_floor_ms"] * a.clock_ghz * 1e3 / mhz
                    fw["ratio_to_issue_floor_at_mean_clock"] = fw["ms_per_call"] / fw["issue_floor_ms_at_mean_clock"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for s in out["shapes"]:
        print(json.dumps({"songs": s["songs"], "seconds": s["seconds"],
                          "ms": {k: round(v["ms_per_call"], 3) for k, v in s["calls"].items()},
                          "x_floor": {k: round(v["kernels"]["chords_forward"]["ratio_to_issue_floor"] or 0.0, 2)
                                      for k, v in s["calls"].items() if "kernels" in v},
                          "trace_share": {k: round(v["trace_share"] or 0.0, 3)
                                          for k, v in s["calls"].items() if "kernels" in v}}), flush=True)


if __name__ == "__main__":
    main()
