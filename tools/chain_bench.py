#!/usr/bin/env python3
"""bl_amd_chain_device timed with HIP events (warm-up first, then the mean of --reps calls per leg) beside the same
chains built from the older public calls, in one run on one device.  One JSON object on stdout (and in --out).

Legs (both metrics): N = 65 536 with 1, 256 and 4 096 chains of length 100; N = 1 048 576 with 1 and 64 chains of
length 100; one full-length chain at N = 16 384.  Every single-chain leg is also timed with each launch shape forced
(bl_amd_chain_force_shape), and two sweeps with both shapes forced (one chain over N, and the number of chains at
N = 16 384, 65 536 and 1 048 576) back the switch constants of the launch layer.

Baseline: per step one bl_amd_distance_matrix_device / bl_amd_cosine_matrix_device row per chain into a device
buffer, one torch masked argmin (argmax) over all chains, and the picked indices (4 bytes per chain) back to the
host, because the matrix call takes its row as a host argument; the rows themselves never leave the device.  It is
serial in the steps and linear in the chains, so it is measured on at most --base-chains chains and --base-steps
steps, the best of --base-reps runs, and scaled to the leg ("baseline_measured" says on what); its indices are checked against the new call's
before it is timed.
usage: python tools/chain_bench.py [--reps 10] [--out profiles/chain_bench.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--base-chains", type=int, default=16)
    ap.add_argument("--base-steps", type=int, default=100)
    ap.add_argument("--base-reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="small sizes: a rehearsal of the tool, not a measurement")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bliss_amd
    from bliss_amd import _lib
    lib = bliss_amd.load()
    assert torch.cuda.is_available(), "chain_bench needs a GPU"
    assert lib.bl_amd_init(0) == 0
    AUTO, PER_CHAIN, SPLIT = _lib.BL_AMD_CHAIN_AUTO, _lib.BL_AMD_CHAIN_PER_CHAIN, _lib.BL_AMD_CHAIN_SPLIT
    shape_name = {PER_CHAIN: "per_chain", SPLIT: "split"}

    def vectors(n, seed):
        g = torch.Generator(device="cpu").manual_seed(seed)
        return (torch.randn((n, 4), generator=g) * 8).cuda()

    def seeds_for(n, n_chains):
        g = torch.Generator(device="cpu").manual_seed(n_chains)
        return torch.randint(0, n, (n_chains,), generator=g, dtype=torch.int32).cuda()

    def chain_call(v, seeds, length, metric, order, value):
        m = _lib.BL_AMD_KNN_COSINE if metric == "cosine" else _lib.BL_AMD_KNN_DISTANCE
        return lib.bl_amd_chain_device(C.c_void_p(v.data_ptr()), v.shape[0], C.c_void_p(seeds.data_ptr()),
                                       seeds.numel(), length, m, C.c_void_p(order.data_ptr()),
                                       C.c_void_p(value.data_ptr()), None)

    def timed(fn, reps, warm=2):
        for _ in range(warm):
            assert fn() == 0
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        t1.synchronize()
        return 1e3 * t0.elapsed_time(t1) / reps   # microseconds per call

    def new_leg(v, n_chains, length, metric, force, reps):
        n = v.shape[0]
        seeds = seeds_for(n, n_chains)
        order = torch.empty((n_chains, length), dtype=torch.int32, device="cuda")
        value = torch.empty((n_chains, length), dtype=torch.float32, device="cuda")
        prev = lib.bl_amd_chain_force_shape(force)
        try:
            shape = lib.bl_amd_chain_shape(n, n_chains)
            us = timed(lambda: chain_call(v, seeds, length, metric, order, value), reps)
        finally:
            lib.bl_amd_chain_force_shape(prev)
        steps = min(length, n) - 1
        print(f"n={n} chains={n_chains} length={length} {metric} {shape_name[shape]}: {us:.1f} us", file=sys.stderr,
              flush=True)
        return {"n": n, "n_chains": n_chains, "length": length, "metric": metric, "forced": force != AUTO,
                "shape": shape_name[shape], "us": round(us, 1), "us_per_step": round(us / max(1, steps), 3)}, order

    def baseline(v, seeds, steps, metric):
        """the chains of `seeds` for `steps` steps from the matrix-row call; returns (order, seconds)"""
        n, nc = v.shape[0], seeds.numel()
        fn = lib.bl_amd_cosine_matrix_device if metric == "cosine" else lib.bl_amd_distance_matrix_device
        rows = torch.empty((nc, n), dtype=torch.float32, device="cuda")
        played = torch.zeros((nc, n), dtype=torch.bool, device="cuda")
        ar = torch.arange(nc, device="cuda")
        cur = seeds.to(torch.int64)
        played[ar, cur] = True
        host = cur.tolist()
        out = [host]
        fill = float("-inf") if metric == "cosine" else float("inf")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            for c in range(nc):
                fn(C.c_void_p(v.data_ptr()), n, host[c], 1, C.c_void_p(rows[c].data_ptr()), None)
            masked = rows.masked_fill(played, fill)
            cur = masked.argmax(dim=1) if metric == "cosine" else masked.argmin(dim=1)
            played[ar, cur] = True
            host = cur.tolist()   # the synchronisation of the step: the next row index is a host argument
            out.append(host)
        sec = time.perf_counter() - t0
        return torch.tensor(out, dtype=torch.int32).t().contiguous(), sec

    def baseline_leg(v, n_chains, length, metric, order_new):
        n = v.shape[0]
        nc = min(n_chains, a.base_chains)
        steps_all = min(length, n) - 1
        steps = min(steps_all, a.base_steps)
        seeds = seeds_for(n, n_chains)[:nc].contiguous()
        got, _ = baseline(v, seeds, steps, metric)                      # warm-up and check
        assert torch.equal(got, order_new[:nc, :steps + 1].cpu()), "baseline and bl_amd_chain_device disagree"
        sec = min(baseline(v, seeds, steps, metric)[1] for _ in range(a.base_reps))   # the baseline's best run
        us_step_chain = 1e6 * sec / steps / nc
        return {"baseline_us": round(us_step_chain * n_chains * steps_all, 1),
                "baseline_us_per_step": round(us_step_chain * n_chains, 3),
                "baseline_measured": {"chains": nc, "steps": steps, "best_of": a.base_reps, "seconds": round(sec, 4)},
                "baseline_indices_equal": True}

    res = {"tool": "tools/chain_bench.py", "device": torch.cuda.get_device_name(0), "reps": a.reps, "quick": a.quick,
           "legs": [], "forced_single_chain": [], "sweep_n_one_chain": [], "sweep_chains": []}
    q = a.quick
    sizes = {"mid": 4096 if q else 65536, "big": 1 << (14 if q else 20), "full": 512 if q else 16384}
    length = 20 if q else 100
    vecs = {k: vectors(n, i + 1) for i, (k, n) in enumerate(sizes.items())}
    plan = [("mid", 1, length), ("mid", 256, length), ("mid", 4096, length), ("big", 1, length), ("big", 64, length),
            ("full", 1, sizes["full"])]
    for metric in ("distance", "cosine"):
        for key, n_chains, ln in plan:
            v = vecs[key]
            reps = max(2, a.reps // 3) if ln > 1000 else a.reps
            leg, order = new_leg(v, n_chains, ln, metric, AUTO, reps)
            leg.update(baseline_leg(v, n_chains, ln, metric, order))
            leg["speedup"] = round(leg["baseline_us"] / leg["us"], 1)
            res["legs"].append(leg)
            if n_chains == 1:
                for force in (PER_CHAIN, SPLIT):
                    f, o = new_leg(v, 1, ln, metric, force, reps)
                    assert torch.equal(o, order), "the two launch shapes disagree"
                    res["forced_single_chain"].append(f)
    for lg in ((10, 12) if q else (12, 13, 14, 15, 16, 17, 18, 19, 20)):
        v = vectors(1 << lg, 40 + lg)
        for metric in ("distance", "cosine"):
            for force in (PER_CHAIN, SPLIT):
                res["sweep_n_one_chain"].append(new_leg(v, 1, length, metric, force, a.reps)[0])
        del v
    for key in ("full", "mid", "big"):
        for n_chains in ((2, 8) if q else (2, 4, 8, 16, 32, 64, 128, 256, 512)):
            for force in (PER_CHAIN, SPLIT):
                res["sweep_chains"].append(new_leg(vecs[key], n_chains, length, "distance", force, a.reps)[0])
    res["all_legs_faster_than_baseline"] = all(x["us"] < x["baseline_us"] for x in res["legs"])
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
