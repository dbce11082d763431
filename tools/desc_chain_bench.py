#!/usr/bin/env python3
"""bl_amd_desc_chain_device timed with HIP events (a warm-up, then the mean of --reps calls per leg) beside two
yardsticks taken in the same run on the same device.  One JSON object on stdout (and in --out).

Yardstick: bl_amd_mix_device (existing code, force vectors, the f32 distance) at the same (n, n_chains, length), index
seeds and no rules on both sides.

Baseline: the same chains built from the existing public descriptor calls: per step one bl_amd_desc_cross_knn_device
with k = songs played + 1 over the chains' current songs, the lists copied to the host and the first unplayed entry
picked there (numpy).  It is serial in the steps and stops at k = BL_AMD_KNN_MAX_K.  It is measured at the leg's own
number of chains, the best of --base-reps runs; its rows are checked against the new call's before anything is timed.

Legs (length 100): N = 65 536 with 1, 16, 256 and 4 096 chains; N = 1 048 576 with 1 and 64 chains; N = 4 096 and
16 384 with one chain under each forced shape (bl_amd_chain_force_shape).  Two sweeps with both shapes forced back the
constants of the launch layer's shape rule: one chain over N, and the number of 16-chain groups at four N.  The shader
clock is sampled while the loops run (bench.DeviceState).
usage: python tools/desc_chain_bench.py [--reps 5] [--out profiles/desc_chain.json]"""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--base-reps", type=int, default=3)
    ap.add_argument("--sweeps-only", action="store_true", help="skip the legs and the baseline: only the two sweeps")
    ap.add_argument("--quick", action="store_true", help="small sizes: a rehearsal of the tool, not a measurement")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 5 or a.quick, "the mean of at least 5 calls"
    import torch
    import bliss_amd
    from bench import DeviceState
    from bliss_amd import _lib
    lib = bliss_amd.load()
    if not torch.cuda.is_available():
        sys.exit("desc_chain_bench.py needs a GPU: a time taken anywhere else says nothing")
    assert lib.bl_amd_init(0) == 0
    AUTO, PER_CHAIN, SPLIT = _lib.BL_AMD_CHAIN_AUTO, _lib.BL_AMD_CHAIN_PER_CHAIN, _lib.BL_AMD_CHAIN_SPLIT
    shape_name = {PER_CHAIN: "per_chain", SPLIT: "split"}
    P = lambda t: C.c_void_p(t.data_ptr())

    def library(n, seed):
        g = torch.Generator(device="cpu").manual_seed(seed)
        desc = torch.randint(-_lib.BL_AMD_DESC_SCALE_MAX, _lib.BL_AMD_DESC_SCALE_MAX + 1, (n, 32), generator=g,
                             dtype=torch.int16).cuda()
        vecs = (torch.randn((n, 4), generator=g) * 8).cuda()
        return desc, vecs

    def seeds_for(n, n_chains):
        g = torch.Generator(device="cpu").manual_seed(n_chains)
        return torch.randint(0, n, (n_chains,), generator=g, dtype=torch.int32).cuda()

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

    def new_leg(desc, vecs, n_chains, length, force, reps, yardstick=True):
        n = desc.shape[0]
        seeds = seeds_for(n, n_chains)
        order = torch.empty((n_chains, length), dtype=torch.int32, device="cuda")
        dist2 = torch.empty((n_chains, length), dtype=torch.int64, device="cuda")
        value = torch.empty((n_chains, length), dtype=torch.float32, device="cuda")
        morder = torch.empty_like(order)
        call = lambda: lib.bl_amd_desc_chain_device(P(desc), n, P(seeds), None, n_chains, length, None, 0, None,
                                                    P(order), P(dist2), None)
        mix = lambda: lib.bl_amd_mix_device(P(vecs), n, P(seeds), None, n_chains, length, _lib.BL_AMD_KNN_DISTANCE,
                                            None, 0, None, P(morder), P(value), None)
        prev = lib.bl_amd_chain_force_shape(force)
        try:
            shape, mix_shape = lib.bl_amd_desc_chain_shape(n, n_chains), lib.bl_amd_chain_shape(n, n_chains)
            us = timed(call, reps)
            mix_us = timed(mix, reps) if yardstick else None
        finally:
            lib.bl_amd_chain_force_shape(prev)
        steps = max(1, min(length, n) - 1)
        leg = {"n": n, "n_chains": n_chains, "length": length, "forced": force != AUTO, "shape": shape_name[shape],
               "us": round(us, 1), "us_per_step": round(us / steps, 3)}
        if yardstick:
            leg.update(mix_shape=shape_name[mix_shape], mix_us=round(mix_us, 1), mix_us_per_step=round(mix_us / steps, 3),
                       ratio_to_mix=round(us / mix_us, 3))
        print(json.dumps(leg), file=sys.stderr, flush=True)
        return leg, order, dist2

    def baseline(desc, seeds, steps):
        """the chains of `seeds` for `steps` steps from the cross kNN; returns (order, dist2, seconds)"""
        import numpy as np
        n, nc = desc.shape[0], seeds.numel()
        cur = seeds.to(torch.int64)
        order = np.empty((nc, steps + 1), dtype=np.int32)
        dist2 = np.zeros((nc, steps + 1), dtype=np.int64)
        order[:, 0] = cur.cpu().numpy()
        rows = np.arange(nc)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(1, steps + 1):
            k = t + 1   # the list holds the t songs played (the current one at distance 0 among them) and one more
            q = desc.index_select(0, cur)
            index = torch.empty((nc, k), dtype=torch.int32, device="cuda")
            d2 = torch.empty((nc, k), dtype=torch.int64, device="cuda")
            assert lib.bl_amd_desc_cross_knn_device(P(q), nc, P(desc), n, k, P(index), P(d2), None) == 0
            hi, hd = index.cpu().numpy(), d2.cpu().numpy()   # the round trip of the step
            played = (hi[:, :, None] == order[:, None, :t]).any(axis=2)
            j = np.argmin(played, axis=1)                    # the first entry of each list that is not played
            order[:, t], dist2[:, t] = hi[rows, j], hd[rows, j]
            cur = torch.from_numpy(order[:, t].astype(np.int64)).cuda()
        sec = time.perf_counter() - t0
        return torch.from_numpy(order), torch.from_numpy(dist2), sec

    def baseline_leg(desc, n_chains, length, order_new, dist2_new):
        """the baseline at the leg's own chain count; it cannot go past k = BL_AMD_KNN_MAX_K"""
        n = desc.shape[0]
        steps = min(max(1, min(length, n) - 1), _lib.BL_AMD_KNN_MAX_K - 1)
        seeds = seeds_for(n, n_chains)
        got_o, got_d, _ = baseline(desc, seeds, steps)                 # warm-up and check
        assert torch.equal(got_o, order_new[:, :steps + 1].cpu()), "baseline and bl_amd_desc_chain_device disagree"
        assert torch.equal(got_d, dist2_new[:, :steps + 1].cpu()), "baseline and bl_amd_desc_chain_device disagree"
        sec = min(baseline(desc, seeds, steps)[2] for _ in range(a.base_reps))
        return {"baseline_us": round(1e6 * sec, 1), "baseline_us_per_step": round(1e6 * sec / steps, 3),
                "baseline_measured": {"chains": n_chains, "steps": steps, "best_of": a.base_reps,
                                      "seconds": round(sec, 4)},
                "baseline_rows_equal": True}

    state = DeviceState(DeviceState.pci_address(0))
    state.start()
    t_begin = time.perf_counter()
    res = {"tool": "tools/desc_chain_bench.py", "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "quick": a.quick, "legs": [], "forced_single_chain": [], "sweep_n_one_chain": [], "sweep_groups": []}
    q = a.quick
    length = 20 if q else 100
    sizes = {"mid": 4096 if q else 65536, "big": 1 << (14 if q else 20)}
    libs = {k: library(n, i + 1) for i, (k, n) in enumerate(sizes.items())}
    plan = [("mid", 1), ("mid", 16), ("mid", 256), ("mid", 64 if q else 4096), ("big", 1), ("big", 64)]
    for key, n_chains in ([] if a.sweeps_only else plan):
        desc, vecs = libs[key]
        leg, order, dist2 = new_leg(desc, vecs, n_chains, length, AUTO, a.reps)
        leg.update(baseline_leg(desc, n_chains, length, order, dist2))
        leg["ratio_to_baseline"] = round(leg["us"] / leg["baseline_us"], 4)
        res["legs"].append(leg)
    for n in ([] if a.sweeps_only else (512, 1024) if q else (4096, 16384)):
        desc, vecs = library(n, 30 + n)
        rows = []
        for force in (PER_CHAIN, SPLIT):
            leg, order, dist2 = new_leg(desc, vecs, 1, length, force, a.reps)
            rows.append((order.clone(), dist2.clone()))
            res["forced_single_chain"].append(leg)
        assert torch.equal(rows[0][0], rows[1][0]) and torch.equal(rows[0][1], rows[1][1]), "the shapes disagree"
    for lg in ((10, 12) if q else (10, 11, 12, 13, 14, 15, 16, 17, 18, 20)):
        desc, vecs = library(1 << lg, 40 + lg)
        for force in (PER_CHAIN, SPLIT):
            res["sweep_n_one_chain"].append(new_leg(desc, vecs, 1, length, force, a.reps, yardstick=False)[0])
        del desc, vecs
    sweep_n = (1024, 4096) if q else (4096, 16384, 65536, 1 << 20)
    for n in sweep_n:
        desc, vecs = libs["mid"] if n == sizes["mid"] else libs["big"] if n == sizes["big"] else library(n, 60)
        for groups in ((1, 4) if q else (1, 2, 4, 8, 16, 32, 64, 128, 256)):
            for force in (PER_CHAIN, SPLIT):
                res["sweep_groups"].append(new_leg(desc, vecs, 16 * groups, length, force, a.reps, yardstick=False)[0])
    state.stop_flag = True
    state.join()
    res["device_state"] = state.summary(t_begin, time.perf_counter())
    res["legs_slower_than_baseline"] = [(x["n"], x["n_chains"]) for x in res["legs"] if x["us"] >= x["baseline_us"]]
    res["legs_slower_than_mix"] = [(x["n"], x["n_chains"]) for x in res["legs"] if x["us"] >= x["mix_us"]]
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
