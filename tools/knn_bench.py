#!/usr/bin/env python3
"""bl_amd_knn_device timed with HIP events (warm-up first, then the mean of --reps calls per leg), beside
bl_amd_distance_matrix_device on the same vectors in the same run.  One JSON object on stdout (and in --out).
Legs: N = 65 536, all rows, k in {10, 32, 128}, both metrics; N = 1 048 576 with 1 and 64 query rows, k = 32;
the distance matrix over all 65 536 rows and over one row at N = 1 048 576.
usage: python tools/knn_bench.py [--reps 20] [--out profiles/knn_bench.json]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bliss_amd
    from bliss_amd import _lib
    lib = bliss_amd.load()
    assert torch.cuda.is_available(), "knn_bench needs a GPU"
    assert lib.bl_amd_init(0) == 0

    def timed(fn, reps):
        for _ in range(3):
            assert fn() == 0
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        t1.synchronize()
        return 1e3 * t0.elapsed_time(t1) / reps   # microseconds per call

    def vectors(n, seed):
        g = torch.Generator(device="cpu").manual_seed(seed)
        return (torch.randn((n, 4), generator=g) * 8).cuda()

    def knn_leg(v, row_begin, n_rows, k, metric, reps):
        n = v.shape[0]
        idx = torch.empty((n_rows, k), dtype=torch.int32, device="cuda")
        val = torch.empty((n_rows, k), dtype=torch.float32, device="cuda")
        m = _lib.BL_AMD_KNN_COSINE if metric == "cosine" else _lib.BL_AMD_KNN_DISTANCE
        us = timed(lambda: lib.bl_amd_knn_device(C.c_void_p(v.data_ptr()), n, row_begin, n_rows, k, m,
                                                 C.c_void_p(idx.data_ptr()), C.c_void_p(val.data_ptr()), None), reps)
        return {"n": n, "row_begin": row_begin, "n_rows": n_rows, "k": k, "metric": metric, "us": round(us, 2),
                "output_bytes": 8 * n_rows * k}

    def matrix_leg(v, row_begin, n_rows, reps):
        n = v.shape[0]
        out = torch.empty((n_rows, n), dtype=torch.float32, device="cuda")
        us = timed(lambda: lib.bl_amd_distance_matrix_device(C.c_void_p(v.data_ptr()), n, row_begin, n_rows,
                                                             C.c_void_p(out.data_ptr()), None), reps)
        del out
        return {"n": n, "row_begin": row_begin, "n_rows": n_rows, "us": round(us, 2), "output_bytes": 4 * n_rows * n,
                "TBps": round(4 * n_rows * n / us / 1e6, 3)}

    res = {"tool": "tools/knn_bench.py", "device": torch.cuda.get_device_name(0), "reps": a.reps, "knn": [],
           "distance_matrix": []}
    v64 = vectors(65536, 1)
    for metric in ("distance", "cosine"):
        for k in (10, 32, 128):
            res["knn"].append(knn_leg(v64, 0, 65536, k, metric, a.reps))
    res["distance_matrix"].append(matrix_leg(v64, 0, 65536, max(3, a.reps // 4)))
    torch.cuda.empty_cache()
    v1m = vectors(1 << 20, 2)
    for metric in ("distance", "cosine"):
        for rows in (1, 64):
            res["knn"].append(knn_leg(v1m, 500000, rows, 32, metric, 5 * a.reps))
    res["distance_matrix"].append(matrix_leg(v1m, 500000, 1, 5 * a.reps))
    knn32 = next(x["us"] for x in res["knn"] if x["n"] == 65536 and x["k"] == 32 and x["metric"] == "distance")
    one = next(x["us"] for x in res["knn"] if x["n"] == 1 << 20 and x["n_rows"] == 1 and x["metric"] == "distance")
    res["summary"] = {
        "knn_65536_k32_over_matrix_65536": round(knn32 / res["distance_matrix"][0]["us"], 4),
        "knn_1M_one_row_over_matrix_one_row": round(one / res["distance_matrix"][1]["us"], 3),
    }
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
