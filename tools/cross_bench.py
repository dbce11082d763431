#!/usr/bin/env python3
"""The cross queries (bl_amd_cross_knn_device, bl_amd_cross_radius_*_device) timed with HIP events beside the self
forms at the same shapes in one run on one device: warm-up first, then --runs runs of --reps calls per leg; a leg
reports the median of its runs and their spread (min, max).  bench.DeviceState samples the shader clock meanwhile.
One JSON object on stdout (and in --out).

Legs:
  * N = 65 536, k = 32, all rows, both metrics: bl_amd_knn_device beside bl_amd_cross_knn_device with the queries a
    separate copy of the library (the same work but for one compare per pair, a 1 MB query stream and, for the
    cosine, one more prep launch);
  * 1 and 64 queries over N = 1 048 576 (the column-split path), self and cross;
  * radius count + fill with values at N = 65 536, all rows, about 32 neighbours per row (tools/radius_bench.py's
    shape and vectors), self and cross.
--parent-lib PATH: also an A/B of every leg between that build of libbliss_amd.so (the parent commit's, which must
have the cross forms) and this tree's, in the manner of tools/ab_libs.py: each library in a process of its own, taking
turns (this, parent, ... this; --rounds of the parent), each leg with its shader clock.  A leg passes when this
tree's median lies inside the spread of the parent's own runs or below it.  The child loads its library with ctypes
alone, so a build need not have every symbol bliss_amd binds.
usage: python tools/cross_bench.py [--reps 10] [--runs 7] [--parent-lib PATH] [--out profiles/cross_bench.json]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DIST, COS = 0, 1   # BL_AMD_KNN_DISTANCE, BL_AMD_KNN_COSINE


def P(t):
    return C.c_void_p(t.data_ptr())


def timed(torch, fn, reps, runs, smp=None):
    """microseconds per call: the median of `runs` runs of `reps` calls, and the runs' extremes; with a running
    bench.DeviceState `smp` also the mean shader clock while they ran"""
    for _ in range(3):
        assert fn() == 0
    torch.cuda.synchronize()
    us = []
    t_begin = time.perf_counter()
    for _ in range(runs):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        t1.synchronize()
        us.append(1e3 * t0.elapsed_time(t1) / reps)
    res = {"us": round(float(np.median(us)), 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2)}
    if smp is not None:
        res["sclk_mhz"] = (smp.summary(t_begin, time.perf_counter()).get("sclk_mhz") or {}).get("mean")
    return res


def vectors(torch, n, seed, scale):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn((n, 4), generator=g) * scale).cuda()


def radius_for(torch, lib, v, per_row):
    """tools/radius_bench.py's: the radius below which a sampled row holds per_row songs on average"""
    n = v.shape[0]
    rows = torch.empty((256, n), dtype=torch.float32, device="cuda")
    assert lib.bl_amd_distance_matrix_device(P(v), n, n // 3, 256, P(rows), None) == 0
    flat = rows.flatten().sort().values
    return float(flat[256 + int(per_row * 256)].item())


def all_legs(torch, lib, reps, runs, smp=None):
    """every leg of the docstring, self and cross, through the C names alone (any build that has the cross forms)"""
    legs = {}
    n, k = 65536, 32
    v = vectors(torch, n, 1, 8)
    q = v.clone()               # the same shapes from a separate copy of the library as the queries
    idx = torch.empty((n, k), dtype=torch.int32, device="cuda")
    val = torch.empty((n, k), dtype=torch.float32, device="cuda")
    for name, metric in (("distance", DIST), ("cosine", COS)):
        legs[f"knn_self_{name}"] = timed(torch, lambda: lib.bl_amd_knn_device(P(v), n, 0, n, k, metric, P(idx), P(val),
                                                                              None), reps, runs, smp)
        legs[f"knn_cross_{name}"] = timed(torch, lambda: lib.bl_amd_cross_knn_device(P(q), n, P(v), n, k, metric, P(idx),
                                                                                     P(val), None), reps, runs, smp)
    w = vectors(torch, n, 1, 10)
    wq = w.clone()
    r = C.c_float(radius_for(torch, lib, w, 32))
    off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    assert lib.bl_amd_radius_count_device(P(w), n, 0, n, DIST, r, P(off), None) == 0
    total = int(off[-1].item())
    ri = torch.empty(total + n, dtype=torch.int32, device="cuda")
    rv = torch.empty(total + n, dtype=torch.float32, device="cuda")

    def pair():
        return (lib.bl_amd_radius_count_device(P(w), n, 0, n, DIST, r, P(off), None) or
                lib.bl_amd_radius_fill_device(P(w), n, 0, n, DIST, r, P(off), P(ri), P(rv), None))
    legs["radius_self_count_fill"] = dict(timed(torch, pair, reps, runs, smp), radius=r.value, total=total)
    assert lib.bl_amd_cross_radius_count_device(P(wq), n, P(w), n, DIST, r, P(off), None) == 0
    assert int(off[-1].item()) == total + n                         # every query finds its copy besides

    def cross_pair():
        return (lib.bl_amd_cross_radius_count_device(P(wq), n, P(w), n, DIST, r, P(off), None) or
                lib.bl_amd_cross_radius_fill_device(P(wq), n, P(w), n, DIST, r, P(off), P(ri), P(rv), None))
    legs["radius_cross_count_fill"] = dict(timed(torch, cross_pair, reps, runs, smp), radius=r.value, total=total + n)
    del v, q, w, wq, idx, val, ri, rv
    torch.cuda.empty_cache()

    # few queries over a million songs: the column-split path
    n_big = 1 << 20
    big = vectors(torch, n_big, 2, 8)
    for rows in (1, 64):
        bq = big[500000:500000 + rows].clone()
        bi = torch.empty((rows, k), dtype=torch.int32, device="cuda")
        bv = torch.empty((rows, k), dtype=torch.float32, device="cuda")
        legs[f"knn_self_1M_{rows}q"] = timed(torch, lambda: lib.bl_amd_knn_device(P(big), n_big, 500000, rows, k, DIST,
                                                                                  P(bi), P(bv), None), 5 * reps, runs, smp)
        legs[f"knn_cross_1M_{rows}q"] = timed(torch, lambda: lib.bl_amd_cross_knn_device(P(bq), rows, P(big), n_big, k,
                                                                                         DIST, P(bi), P(bv), None),
                                              5 * reps, runs, smp)
    del big
    torch.cuda.empty_cache()
    return legs


def child(a):
    """one library (BLISS_AMD_LIB), ctypes alone"""
    import torch
    from bench import DeviceState
    lib = C.CDLL(os.environ["BLISS_AMD_LIB"], mode=C.RTLD_GLOBAL)
    assert lib.bl_amd_init(0) == 0
    smp = DeviceState(DeviceState.pci_address(0), period=0.01)
    smp.start()
    legs = all_legs(torch, lib, a.reps, a.runs, smp)
    smp.stop_flag = True
    smp.join()
    print(json.dumps(legs))


def ab(a):
    """this, parent, this, ... this: `rounds` turns of the parent between rounds + 1 of this tree's library.  A leg
    passes when this library's median is inside the spread (min to max over every run of every turn) of the parent's
    own runs, or below it: that spread is the only noise floor these legs have."""
    libs = {"parent": os.path.abspath(a.parent_lib), "this": os.path.join(ROOT, "bliss_amd", "libbliss_amd.so")}
    got = {name: [] for name in libs}
    for name in ["this", "parent"] * a.rounds + ["this"]:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--runs",
                              str(a.runs)], env=dict(os.environ, BLISS_AMD_LIB=libs[name]), capture_output=True,
                             text=True, check=True).stdout
        got[name].append(json.loads(out.strip().splitlines()[-1]))
    rep = {"manner": "tools/ab_libs.py: a process per library, taking turns this / parent / ... / this",
           "rounds": a.rounds, "legs": {}}
    for leg in got["this"][0]:
        side = {}
        for name in libs:
            turns = [x[leg] for x in got[name]]
            side[name] = {"us": round(float(np.median([t["us"] for t in turns])), 2),
                          "us_min": min(t["us_min"] for t in turns), "us_max": max(t["us_max"] for t in turns),
                          "us_turns": [t["us"] for t in turns], "sclk_mhz_turns": [t.get("sclk_mhz") for t in turns]}
        rep["legs"][leg] = dict(side, this_over_parent=round(side["this"]["us"] / side["parent"]["us"], 4),
                                within_parent_spread=side["this"]["us"] <= side["parent"]["us_max"])
    rep["all_within_parent_spread"] = all(x["within_parent_spread"] for x in rep["legs"].values())
    return rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    import torch
    import bliss_amd
    from bench import DeviceState
    lib = bliss_amd.load()
    assert torch.cuda.is_available(), "cross_bench needs a GPU"
    assert lib.bl_amd_init(0) == 0
    smp = DeviceState(DeviceState.pci_address(0), period=0.01)
    smp.start()
    t_begin = time.perf_counter()
    res = {"tool": "tools/cross_bench.py", "device": torch.cuda.get_device_name(0), "reps": a.reps, "runs": a.runs,
           "timing": "HIP events around `reps` back-to-back calls; us = median of `runs` such runs, us_min / us_max "
                     "their spread"}
    legs = all_legs(torch, lib, a.reps, a.runs, smp)
    t_end = time.perf_counter()
    smp.stop_flag = True
    smp.join()
    res["legs"] = legs
    res["device_state"] = smp.summary(t_begin, t_end)

    def ratio(x, y):
        return round(legs[x]["us"] / legs[y]["us"], 4)
    res["summary"] = {
        "knn_cross_over_self_distance": ratio("knn_cross_distance", "knn_self_distance"),
        "knn_cross_over_self_cosine": ratio("knn_cross_cosine", "knn_self_cosine"),
        "radius_cross_over_self": ratio("radius_cross_count_fill", "radius_self_count_fill"),
        "knn_cross_over_self_1M_1q": ratio("knn_cross_1M_1q", "knn_self_1M_1q"),
        "knn_cross_over_self_1M_64q": ratio("knn_cross_1M_64q", "knn_self_1M_64q"),
    }
    if a.parent_lib:
        res["parent_vs_this"] = ab(a)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
