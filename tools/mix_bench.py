#!/usr/bin/env python3
"""bl_amd_mix_device beside bl_amd_chain_device, timed with HIP events in one process on one device: 3 warm-up calls,
then --runs runs of --calls calls each; a leg's figure is the median run, with the runs' extremes beside it.  One JSON
object on stdout (and in --out).

Shapes: those of tools/chain_bench.py (N = 65 536 with 1, 256 and 4 096 chains of 100; N = 1 048 576 with 1 and 64
chains of 100; one full-length chain at N = 16 384), both metrics.  Per shape four legs, interleaved run by run:
  chain        bl_amd_chain_device: its kernels are untouched, so this is the baseline
  mix          bl_amd_mix_device with index seeds, no mask, gap 0
  mix_gap4     tags = 1 024 values spread at random, gap 4
  mix_half     half the library excluded at random (the seeds may be among them)
After the warm-up calls and before anything is timed, the mix leg's indices and value bits are checked against the
chain's; every timed call's return code is checked once its run has been timed.
usage: python tools/mix_bench.py [--runs 7] [--calls 10] [--out profiles/mix_bench.json]   (--out "" writes no file)"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="small sizes: a rehearsal of the tool, not a measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mix_bench.json"))
    a = ap.parse_args()
    import torch
    import bliss_amd
    from bliss_amd import _lib
    lib = bliss_amd.load()
    assert torch.cuda.is_available(), "mix_bench needs a GPU"
    assert lib.bl_amd_init(0) == 0
    shape_name = {_lib.BL_AMD_CHAIN_PER_CHAIN: "per_chain", _lib.BL_AMD_CHAIN_SPLIT: "split"}
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def vectors(n, seed):
        g = torch.Generator(device="cpu").manual_seed(seed)
        return (torch.randn((n, 4), generator=g) * 8).cuda()

    def legs_for(v, n_chains, length, metric):
        n = v.shape[0]
        g = torch.Generator(device="cpu").manual_seed(n_chains)
        seeds = torch.randint(0, n, (n_chains,), generator=g, dtype=torch.int32).cuda()
        tags = torch.randint(0, 1024, (n,), generator=g, dtype=torch.int32).cuda()
        half = (torch.rand((n,), generator=g) < 0.5).cuda()
        m = _lib.BL_AMD_KNN_COSINE if metric == "cosine" else _lib.BL_AMD_KNN_DISTANCE
        out = {k: (torch.empty((n_chains, length), dtype=torch.int32, device="cuda"),
                   torch.empty((n_chains, length), dtype=torch.float32, device="cuda"))
               for k in ("chain", "mix", "mix_gap4", "mix_half")}

        def mix(key, t, gap, ex):
            o, x = out[key]
            return lambda: lib.bl_amd_mix_device(P(v), n, P(seeds), None, n_chains, length, m, P(t), gap, P(ex), P(o), P(x),
                                                 None)
        o, x = out["chain"]
        calls = {"chain": lambda: lib.bl_amd_chain_device(P(v), n, P(seeds), n_chains, length, m, P(o), P(x), None),
                 "mix": mix("mix", None, 0, None), "mix_gap4": mix("mix_gap4", tags, 4, None),
                 "mix_half": mix("mix_half", None, 0, half)}
        return calls, out

    def measure(calls, out, n_calls):
        for fn in calls.values():
            for _ in range(3):
                assert fn() == 0
        torch.cuda.synchronize()
        assert torch.equal(out["mix"][0], out["chain"][0]) and torch.equal(
            out["mix"][1].view(torch.int32), out["chain"][1].view(torch.int32)), "mix without rules is not the chain"
        us = {k: [] for k in calls}
        for _ in range(a.runs):          # the legs alternate within a run, so drift lands on all of them
            for k, fn in calls.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                rc = 0
                t0.record()
                for _ in range(n_calls):
                    rc |= fn()
                t1.record()
                t1.synchronize()
                assert rc == 0, f"a timed call of the {k} leg failed"
                us[k].append(1e3 * t0.elapsed_time(t1) / n_calls)
        return us

    q = a.quick
    sizes = {"mid": 4096 if q else 65536, "big": 1 << (14 if q else 20), "full": 512 if q else 16384}
    length = 20 if q else 100
    vecs = {k: vectors(n, i + 1) for i, (k, n) in enumerate(sizes.items())}
    plan = [("mid", 1, length), ("mid", 256, length), ("mid", 4096, length), ("big", 1, length), ("big", 64, length),
            ("full", 1, sizes["full"])]
    res = {"tool": "tools/mix_bench.py", "device": torch.cuda.get_device_name(0), "runs": a.runs, "calls": a.calls,
           "warmup_calls": 3, "quick": q, "legs": []}
    for metric in ("distance", "cosine"):
        for key, n_chains, ln in plan:
            v = vecs[key]
            n = v.shape[0]
            calls, out = legs_for(v, n_chains, ln, metric)
            us = measure(calls, out, max(2, a.calls // 3) if ln > 1000 else a.calls)   # full length: fewer calls
            steps = max(1, min(ln, n) - 1)
            leg = {"n": n, "n_chains": n_chains, "length": ln, "metric": metric,
                   "shape": shape_name[lib.bl_amd_chain_shape(n, n_chains)],
                   "picks_gap4": int((out["mix_gap4"][0][0] >= 0).sum()), "picks_half": int((out["mix_half"][0][0] >= 0).sum())}
            med = {k: statistics.median(x) for k, x in us.items()}
            for k, x in us.items():
                leg[k] = {"us": round(med[k], 1), "min": round(min(x), 1), "max": round(max(x), 1),
                          "us_per_step": round(med[k] / steps, 3), "over_chain": round(med[k] / med["chain"], 4)}
            res["legs"].append(leg)
            print(f"n={n} chains={n_chains} length={ln} {metric} {leg['shape']}: " +
                  " ".join(f"{k}={med[k]:.1f}" for k in us), file=sys.stderr, flush=True)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
