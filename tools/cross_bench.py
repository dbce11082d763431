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
--parent-lib PATH: also an A/B of the self calls between that build of libbliss_amd.so (the parent commit's) and this
tree's, in the manner of tools/ab_libs.py: each library in a process of its own, taking turns --rounds times, medians
compared.  The child loads its library with ctypes alone, since an older build lacks the symbols bliss_amd binds.
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


def timed(torch, fn, reps, runs):
    """microseconds per call: the median of `runs` runs of `reps` calls, and the runs' extremes"""
    for _ in range(3):
        assert fn() == 0
    torch.cuda.synchronize()
    us = []
    for _ in range(runs):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        t1.synchronize()
        us.append(1e3 * t0.elapsed_time(t1) / reps)
    return {"us": round(float(np.median(us)), 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2)}


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


def self_legs(torch, lib, reps, runs):
    """the self calls both builds have: kNN N = 65 536 k = 32 all rows (both metrics), radius count + fill"""
    out = {}
    n, k = 65536, 32
    v = vectors(torch, n, 1, 8)
    idx = torch.empty((n, k), dtype=torch.int32, device="cuda")
    val = torch.empty((n, k), dtype=torch.float32, device="cuda")
    for name, metric in (("distance", DIST), ("cosine", COS)):
        out[f"knn_self_{name}"] = timed(torch, lambda: lib.bl_amd_knn_device(P(v), n, 0, n, k, metric, P(idx), P(val),
                                                                             None), reps, runs)
    w = vectors(torch, n, 1, 10)
    r = C.c_float(radius_for(torch, lib, w, 32))
    off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    assert lib.bl_amd_radius_count_device(P(w), n, 0, n, DIST, r, P(off), None) == 0
    total = int(off[-1].item())
    ri = torch.empty(total, dtype=torch.int32, device="cuda")
    rv = torch.empty(total, dtype=torch.float32, device="cuda")

    def pair():
        return (lib.bl_amd_radius_count_device(P(w), n, 0, n, DIST, r, P(off), None) or
                lib.bl_amd_radius_fill_device(P(w), n, 0, n, DIST, r, P(off), P(ri), P(rv), None))
    out["radius_self_count_fill"] = dict(timed(torch, pair, reps, runs), radius=r.value, total=total)
    return out


def child(a):
    """one library (BLISS_AMD_LIB), ctypes alone"""
    import torch
    lib = C.CDLL(os.environ["BLISS_AMD_LIB"], mode=C.RTLD_GLOBAL)
    assert lib.bl_amd_init(0) == 0
    print(json.dumps(self_legs(torch, lib, a.reps, a.runs)))


def ab(a):
    libs = {"parent": os.path.abspath(a.parent_lib), "this": os.path.join(ROOT, "bliss_amd", "libbliss_amd.so")}
    got = {name: [] for name in libs}
    for _ in range(a.rounds):
        for name, path in libs.items():
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--runs",
                                  str(a.runs)], env=dict(os.environ, BLISS_AMD_LIB=path), capture_output=True, text=True,
                                 check=True).stdout
            got[name].append(json.loads(out.strip().splitlines()[-1]))
    rep = {"manner": "tools/ab_libs.py: a process per library, taking turns", "rounds": a.rounds, "legs": {}}
    for leg in got["this"][0]:
        med = {name: [x[leg]["us"] for x in got[name]] for name in libs}
        rep["legs"][leg] = {"parent_us_rounds": med["parent"], "this_us_rounds": med["this"],
                            "parent_us": round(float(np.median(med["parent"])), 2),
                            "this_us": round(float(np.median(med["this"])), 2),
                            "this_over_parent": round(float(np.median(med["this"]) / np.median(med["parent"])), 4)}
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
    legs = self_legs(torch, lib, a.reps, a.runs)

    # the same shapes from a separate copy of the library as the queries
    n, k = 65536, 32
    v = vectors(torch, n, 1, 8)
    q = v.clone()
    idx = torch.empty((n, k), dtype=torch.int32, device="cuda")
    val = torch.empty((n, k), dtype=torch.float32, device="cuda")
    for name, metric in (("distance", DIST), ("cosine", COS)):
        legs[f"knn_cross_{name}"] = timed(torch, lambda: lib.bl_amd_cross_knn_device(P(q), n, P(v), n, k, metric, P(idx),
                                                                                     P(val), None), a.reps, a.runs)
    w = vectors(torch, n, 1, 10)
    wq = w.clone()
    r = C.c_float(legs["radius_self_count_fill"]["radius"])
    off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    assert lib.bl_amd_cross_radius_count_device(P(wq), n, P(w), n, DIST, r, P(off), None) == 0
    total = int(off[-1].item())
    assert total == legs["radius_self_count_fill"]["total"] + n      # every query finds its copy besides
    ri = torch.empty(total, dtype=torch.int32, device="cuda")
    rv = torch.empty(total, dtype=torch.float32, device="cuda")

    def pair():
        return (lib.bl_amd_cross_radius_count_device(P(wq), n, P(w), n, DIST, r, P(off), None) or
                lib.bl_amd_cross_radius_fill_device(P(wq), n, P(w), n, DIST, r, P(off), P(ri), P(rv), None))
    legs["radius_cross_count_fill"] = dict(timed(torch, pair, a.reps, a.runs), radius=r.value, total=total)
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
                                                                                  P(bi), P(bv), None), 5 * a.reps, a.runs)
        legs[f"knn_cross_1M_{rows}q"] = timed(torch, lambda: lib.bl_amd_cross_knn_device(P(bq), rows, P(big), n_big, k,
                                                                                         DIST, P(bi), P(bv), None),
                                              5 * a.reps, a.runs)
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
    del big
    torch.cuda.empty_cache()
    if a.parent_lib:
        res["self_calls_parent_vs_this"] = ab(a)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
