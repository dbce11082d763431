#!/usr/bin/env python3
"""bl_amd_desc_knn_device timed with HIP events beside bl_amd_knn_device (distance) over force vectors at the same
shapes, in the same process and in alternating rounds: each round times --reps calls of the descriptor leg, then --reps
calls of the force-vector leg; a leg's figure is the median of its rounds, with the fastest and slowest round beside it.
Every shape is warmed up first.  Legs (the shapes of DESIGN 4.6): N = 65 536, all rows, k in {10, 32, 128};
N = 1 048 576 with 1 and 64 query rows, k = 32.  Also range and quantise at N = 1 048 576, d = 25.  The descriptors are
25 normally distributed features per song, fitted and quantised on the device; the other 7 dimensions are 0.
One JSON object on stdout and in --out.  Needs a GPU: there is no other way to a time.
usage: python tools/desc_knn_bench.py [--reps 50] [--rounds 5] [--out profiles/desc_knn.json]"""
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
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "desc_knn.json"))
    a = ap.parse_args()
    import torch
    import bliss_amd
    import bliss_amd.descriptor as D
    from bliss_amd import _lib
    lib = bliss_amd.load()
    if not torch.cuda.is_available():
        sys.exit("desc_knn_bench.py needs a GPU: a time taken anywhere else says nothing")
    assert lib.bl_amd_init(0) == 0

    def window(fn, reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        t1.synchronize()
        return 1e3 * t0.elapsed_time(t1) / reps   # microseconds per call

    def alternate(legs, reps):
        """legs: name -> call; returns name -> {us (median of the rounds), us_min, us_max}"""
        for fn in legs.values():
            for _ in range(3):
                assert fn() == 0
        torch.cuda.synchronize()
        seen = {name: [] for name in legs}
        for _ in range(a.rounds):
            for name, fn in legs.items():
                seen[name].append(window(fn, reps))
        return {name: {"us": round(statistics.median(v), 2), "us_min": round(min(v), 2), "us_max": round(max(v), 2)}
                for name, v in seen.items()}

    def library(n, seed):
        g = torch.Generator(device="cpu").manual_seed(seed)
        x = torch.randn((n, 25), generator=g).cuda()
        desc, _ = D.fit_device(x)
        vecs = (torch.randn((n, 4), generator=g) * 8).cuda()
        return x, desc, vecs

    def knn_pair(desc, vecs, row_begin, n_rows, k, reps):
        n = desc.shape[0]
        idx = torch.empty((n_rows, k), dtype=torch.int32, device="cuda")
        d2 = torch.empty((n_rows, k), dtype=torch.int64, device="cuda")
        val = torch.empty((n_rows, k), dtype=torch.float32, device="cuda")
        legs = {
            "desc_knn": lambda: lib.bl_amd_desc_knn_device(C.c_void_p(desc.data_ptr()), n, row_begin, n_rows, k,
                                                           C.c_void_p(idx.data_ptr()), C.c_void_p(d2.data_ptr()), None),
            "force_knn": lambda: lib.bl_amd_knn_device(C.c_void_p(vecs.data_ptr()), n, row_begin, n_rows, k,
                                                       _lib.BL_AMD_KNN_DISTANCE, C.c_void_p(idx.data_ptr()),
                                                       C.c_void_p(val.data_ptr()), None),
        }
        t = alternate(legs, reps)
        pairs = float(n) * n_rows
        return {"n": n, "row_begin": row_begin, "n_rows": n_rows, "k": k, "reps": reps, "rounds": a.rounds,
                "split": lib.bl_amd_desc_knn_scratch_bytes(n, n_rows, k) > 0, **t,
                "desc_over_force": round(t["desc_knn"]["us"] / t["force_knn"]["us"], 3),
                "desc_pairs_per_us": round(pairs / t["desc_knn"]["us"], 1),
                "desc_int8_TOPS": round(pairs * 2 * 128 / t["desc_knn"]["us"] / 1e6, 2)}   # 128 int8 MACs per pair

    res = {"tool": "tools/desc_knn_bench.py", "device": torch.cuda.get_device_name(0), "knn": []}
    x64, d64, v64 = library(65536, 1)
    for k in (10, 32, 128):
        res["knn"].append(knn_pair(d64, v64, 0, 65536, k, a.reps))
    del x64, d64, v64
    torch.cuda.empty_cache()
    x1m, d1m, v1m = library(1 << 20, 2)
    for rows in (1, 64):
        res["knn"].append(knn_pair(d1m, v1m, 500000, rows, 32, 20 * a.reps))
    n, d = x1m.shape
    rng = torch.empty(D.RANGE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    out = torch.empty((n, 32), dtype=torch.int16, device="cuda")
    build = alternate({
        "desc_range": lambda: lib.bl_amd_desc_range_device(C.c_void_p(x1m.data_ptr()), n, d, C.c_void_p(rng.data_ptr()), None),
        "desc_quantize": lambda: lib.bl_amd_desc_quantize_device(C.c_void_p(x1m.data_ptr()), n, d, C.c_void_p(rng.data_ptr()),
                                                                 None, C.c_void_p(out.data_ptr()), None),
    }, 20 * a.reps)
    build["desc_range"]["GBps"] = round(4.0 * n * d / build["desc_range"]["us"] / 1e3, 1)
    build["desc_quantize"]["GBps"] = round((4.0 * n * d + 64.0 * n) / build["desc_quantize"]["us"] / 1e3, 1)
    res["build"] = {"n": n, "d": d, **build}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
