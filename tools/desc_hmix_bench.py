#!/usr/bin/env python3
"""bl_amd_desc_hmix_device timed with HIP events beside bl_amd_desc_chain_device in the same run on the same device.
One JSON object on stdout (and in --out).

Yardstick: bl_amd_desc_chain_device with tags (existing code) at the same (n, n_chains, length), seeds, tags and gap.
Three calls are timed per leg: the yardstick, the mix under the rule, and the mix with the rule's flags 0.  They are
timed in alternating windows (yardstick, ruled, flags 0, yardstick, ...), --reps windows each after two warm-up calls
each; a figure is the mean of its windows, and the smallest and largest window are kept beside it.

Inputs: full-scale random descriptors, index seeds, tags uniform over 256 with gap 2, keys uniform over 24, tempos
uniform over 60.00 .. 180.00 BPM, the Camelot table at 60 per mille with half and double time.  A chain that ended
early would make a step look cheaper than it is, so the filled slots are counted and a leg says whether every chain
filled its row.

Legs (length 100): N = 65 536 with 1, 16, 256 and 4 096 chains; N = 1 048 576 with 1 and 64 chains.  The shader clock is
sampled while the loops run (bench.DeviceState).
usage: python tools/desc_hmix_bench.py [--reps 5] [--out profiles/desc_hmix.json]"""
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
    ap.add_argument("--quick", action="store_true", help="small sizes: a rehearsal of the tool, not a measurement")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 5 or a.quick, "the mean of at least 5 windows"
    import numpy as np
    import torch
    import bliss_amd
    import bliss_amd.descriptor as D
    from bench import DeviceState
    from bliss_amd import _lib
    lib = bliss_amd.load()
    if not torch.cuda.is_available():
        sys.exit("desc_hmix_bench.py needs a GPU: a time taken anywhere else says nothing")
    assert lib.bl_amd_init(0) == 0
    shape_name = {_lib.BL_AMD_CHAIN_PER_CHAIN: "per_chain", _lib.BL_AMD_CHAIN_SPLIT: "split"}
    P = lambda t: C.c_void_p(t.data_ptr())
    GAP, TOL = 2, 60
    ruled = np.zeros(1, dtype=D.HMIX_RULE_DTYPE)
    ruled[0] = D.camelot_rule(TOL, half_double=True)
    off = ruled.copy()
    off["flags"] = 0
    RULE = lambda r: r.ctypes.data_as(C.POINTER(_lib.HmixRule))

    def library(n, seed):
        g = torch.Generator(device="cpu").manual_seed(seed)
        desc = torch.randint(-_lib.BL_AMD_DESC_SCALE_MAX, _lib.BL_AMD_DESC_SCALE_MAX + 1, (n, 32), generator=g,
                             dtype=torch.int16).cuda()
        tags = torch.randint(0, 256, (n,), generator=g, dtype=torch.int32).cuda()
        rng = np.random.default_rng(seed)
        attrs = np.zeros(n, dtype=D.HMIX_ATTR_DTYPE)
        attrs["tempo"], attrs["key"] = rng.integers(6000, 18001, size=n), rng.integers(0, 24, size=n)
        return desc, tags, torch.from_numpy(attrs.view(np.uint8).reshape(n, 4)).cuda()

    def seeds_for(n, n_chains):
        g = torch.Generator(device="cpu").manual_seed(n_chains)
        return torch.randint(0, n, (n_chains,), generator=g, dtype=torch.int32).cuda()

    def window(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        return 1e3 * t0.elapsed_time(t1)   # microseconds

    def leg(desc, tags, attrs, n_chains, length):
        n = desc.shape[0]
        seeds = seeds_for(n, n_chains)
        out = {k: (torch.empty((n_chains, length), dtype=torch.int32, device="cuda"),
                   torch.empty((n_chains, length), dtype=torch.int64, device="cuda")) for k in ("chain", "ruled", "off")}
        tail = lambda k: (P(seeds), None, n_chains, length, P(tags), GAP, None, P(out[k][0]), P(out[k][1]), None)
        calls = {"chain": lambda: lib.bl_amd_desc_chain_device(P(desc), n, *tail("chain")),
                 "ruled": lambda: lib.bl_amd_desc_hmix_device(P(desc), P(attrs), n, RULE(ruled), *tail("ruled")),
                 "off": lambda: lib.bl_amd_desc_hmix_device(P(desc), P(attrs), n, RULE(off), *tail("off"))}
        for fn in calls.values():
            for _ in range(2):
                assert fn() == 0
        torch.cuda.synchronize()
        assert torch.equal(out["off"][0], out["chain"][0]) and torch.equal(out["off"][1], out["chain"][1])
        assert not torch.equal(out["ruled"][0], out["chain"][0])
        filled = {k: int((out[k][0] >= 0).sum()) for k in calls}
        complete = filled["ruled"] == filled["chain"] == n_chains * min(length, n)
        us = {k: [] for k in calls}
        for _ in range(a.reps):
            for k, fn in calls.items():
                us[k].append(window(fn))
        steps = max(1, min(length, n) - 1)
        mean = {k: sum(v) / len(v) for k, v in us.items()}
        res = {"n": n, "n_chains": n_chains, "length": length,
               "shape": shape_name[lib.bl_amd_desc_chain_shape(n, n_chains)], "filled_slots": filled, "every_chain_fills_its_row": complete}
        for k in calls:
            res[k + "_us_per_step"] = round(mean[k] / steps, 3)
            res[k + "_us_per_step_min_max"] = [round(min(us[k]) / steps, 3), round(max(us[k]) / steps, 3)]
        res["ratio_ruled_to_chain"] = round(mean["ruled"] / mean["chain"], 3)
        res["ratio_off_to_chain"] = round(mean["off"] / mean["chain"], 3)
        print(json.dumps(res), file=sys.stderr, flush=True)
        return res

    state = DeviceState(DeviceState.pci_address(0))
    state.start()
    t_begin = time.perf_counter()
    res = {"tool": "tools/desc_hmix_bench.py", "device": torch.cuda.get_device_name(0), "windows": a.reps,
           "quick": a.quick, "gap": GAP, "tags": 256, "tempo_tol": TOL, "rule_flags": int(ruled["flags"][0]),
           "yardstick": "bl_amd_desc_chain_device with the same tags and gap", "legs": []}
    q = a.quick
    length = 20 if q else 100
    sizes = {"mid": 4096 if q else 65536, "big": 1 << (14 if q else 20)}
    libs = {k: library(n, i + 1) for i, (k, n) in enumerate(sizes.items())}
    for key, n_chains in [("mid", 1), ("mid", 16), ("mid", 256), ("mid", 64 if q else 4096), ("big", 1), ("big", 64)]:
        res["legs"].append(leg(*libs[key], n_chains, length))
    state.stop_flag = True
    state.join()
    res["device_state"] = state.summary(t_begin, time.perf_counter())
    res["legs_ruled_above_1_5"] = [(x["n"], x["n_chains"]) for x in res["legs"] if x["ratio_ruled_to_chain"] > 1.5]
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
