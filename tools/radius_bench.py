#!/usr/bin/env python3
"""bl_amd_radius_count_device / bl_amd_radius_fill_device / bl_amd_groups_device timed with HIP events (warm-up first,
then the mean of --reps calls per leg) beside the same answer built from the older public calls, in one run on one
device.  One JSON object on stdout (and in --out).

Legs: N = 65 536, all rows, count alone and count + fill with values at radii that give about 1, 32 and 1 000
neighbours per row (random N(0, 1) * 10 vectors; the radii are quantiles of 256 sampled matrix rows); N = 1 048 576
with 1 and 64 query rows; duplicate groups at N = 65 536 and 1 048 576 with about 1 % planted duplicates at a radius
that finds exactly them.  Beside them: the distance-matrix call alone and bl_amd_knn_device with k = 10 at N = 65 536.

Baseline: bl_amd_distance_matrix_device rows in blocks of at most --block-bytes, then torch on the device: `<=`, the
diagonal cleared, count_nonzero per row and a cumsum (count), nonzero and a gather of the values (fill), and for the
groups the edges of all blocks followed by min-label propagation with pointer jumping.  Where the whole matrix is
more than --base-blocks blocks the baseline is measured on that many blocks and scaled ("baseline_measured" says on
what).  Before anything is timed the new calls' pairs are checked against the baseline's on the measured rows.
usage: python tools/radius_bench.py [--reps 5] [--out profiles/radius_bench.json]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--block-bytes", type=int, default=1 << 30)
    ap.add_argument("--base-blocks", type=int, default=16)
    ap.add_argument("--quick", action="store_true", help="small sizes: a rehearsal of the tool, not a measurement")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bliss_amd
    from bliss_amd import _lib
    lib = bliss_amd.load()
    assert torch.cuda.is_available(), "radius_bench needs a GPU"
    assert lib.bl_amd_init(0) == 0
    DIST = _lib.BL_AMD_KNN_DISTANCE
    P = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731

    def vectors(n, seed):
        g = torch.Generator(device="cpu").manual_seed(seed)
        return (torch.randn((n, 4), generator=g) * 10).cuda()

    def timed(fn, reps, warm=1):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        t1.synchronize()
        return 1e3 * t0.elapsed_time(t1) / reps   # microseconds per call

    def matrix_rows(v, r0, cnt, out):
        assert lib.bl_amd_distance_matrix_device(P(v), v.shape[0], r0, cnt, P(out), None) == 0

    def block_rows(n):
        return max(1, min(n, a.block_bytes // (4 * n)))

    def radius_for(v, per_row):
        """the radius below which a sampled row holds per_row songs on average (the query itself excluded)"""
        n = v.shape[0]
        rows = torch.empty((256, n), dtype=torch.float32, device="cuda")
        matrix_rows(v, n // 3, 256, rows)
        flat = rows.flatten().sort().values
        return float(flat[256 + int(per_row * 256)].item())   # 256 zeros of the diagonal come first

    # ---- the new calls ------------------------------------------------------------------------------------------
    def count_call(v, r0, cnt, r, off):
        assert lib.bl_amd_radius_count_device(P(v), v.shape[0], r0, cnt, DIST, r, P(off), None) == 0

    def fill_call(v, r0, cnt, r, off, idx, val):
        assert lib.bl_amd_radius_fill_device(P(v), v.shape[0], r0, cnt, DIST, r, P(off), P(idx), P(val), None) == 0

    # ---- the baseline -------------------------------------------------------------------------------------------
    def base_block(v, r0, cnt, r, buf, want_lists):
        n = v.shape[0]
        m = buf[:cnt]
        matrix_rows(v, r0, cnt, m)
        w = m <= r
        w[torch.arange(cnt, device="cuda"), torch.arange(r0, r0 + cnt, device="cuda")] = False
        counts = torch.count_nonzero(w, dim=1)
        if not want_lists:
            return counts, None, None, None
        ri, ci = torch.nonzero(w, as_tuple=True)
        return counts, ri + r0, ci.to(torch.int32), m[ri, ci]

    def baseline(v, r0, cnt, r, want_lists, max_blocks=None):
        """(offsets, rows, index, value) of rows [r0, r0 + cnt) limited to max_blocks blocks; rows actually done"""
        n = v.shape[0]
        b = block_rows(n)
        buf = torch.empty((min(b, cnt), n), dtype=torch.float32, device="cuda")
        counts, rows, idx, val, done = [], [], [], [], 0
        for k, s in enumerate(range(r0, r0 + cnt, b)):
            if max_blocks is not None and k >= max_blocks:
                break
            c = min(b, r0 + cnt - s)
            cn, ri, ci, va = base_block(v, s, c, r, buf, want_lists)
            counts.append(cn)
            if want_lists:
                rows.append(ri); idx.append(ci); val.append(va)
            done += c
        off = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(torch.cat(counts), 0)])
        if want_lists:
            return off, torch.cat(rows), torch.cat(idx), torch.cat(val), done
        return off, None, None, None, done

    def propagate(n, src, dst):
        label = torch.arange(n, device="cuda")
        while True:
            new = label.scatter_reduce(0, src, label[dst], "amin")
            new = new.scatter_reduce(0, dst, label[src], "amin")
            new = new[new]
            if torch.equal(new, label):   # the host round trip of the baseline
                return label
            label = new

    res = {"tool": "tools/radius_bench.py", "device": torch.cuda.get_device_name(0), "reps": a.reps, "quick": a.quick,
           "metric": "distance", "legs": [], "beside": {}}
    q = a.quick
    n_mid, n_big = (4096, 1 << 14) if q else (65536, 1 << 20)

    def radius_leg(v, r0, cnt, r, label):
        n = v.shape[0]
        off = torch.empty(cnt + 1, dtype=torch.int64, device="cuda")
        count_call(v, r0, cnt, r, off)
        total = int(off[-1].item())
        idx = torch.empty(max(total, 1), dtype=torch.int32, device="cuda")
        val = torch.empty(max(total, 1), dtype=torch.float32, device="cuda")
        fill_call(v, r0, cnt, r, off, idx, val)
        # check against the baseline's pairs before timing
        nb = (cnt + block_rows(n) - 1) // block_rows(n)
        mb = None if nb <= a.base_blocks else a.base_blocks
        boff, _, bidx, bval, done = baseline(v, r0, cnt, r, True, mb)
        hi = int(off[done].item())
        assert torch.equal(boff, off[:done + 1]), "baseline and bl_amd_radius_count_device disagree"
        assert torch.equal(bidx, idx[:hi]) and torch.equal(bval.view(torch.int32), val[:hi].view(torch.int32)), \
            "baseline and bl_amd_radius_fill_device disagree"
        del boff, bidx, bval
        us_count = timed(lambda: count_call(v, r0, cnt, r, off), a.reps)
        us_both = timed(lambda: (count_call(v, r0, cnt, r, off), fill_call(v, r0, cnt, r, off, idx, val)), a.reps)
        scale = cnt / done
        b_count = timed(lambda: baseline(v, r0, cnt, r, False, mb), max(1, a.reps // 2)) * scale
        b_both = timed(lambda: baseline(v, r0, cnt, r, True, mb), max(1, a.reps // 2)) * scale
        leg = {"leg": label, "n": n, "n_rows": cnt, "radius": r, "per_row": round(total / cnt, 2), "total": total,
               "count_us": round(us_count, 1), "count_fill_us": round(us_both, 1),
               "baseline_count_us": round(b_count, 1), "baseline_count_fill_us": round(b_both, 1),
               "baseline_measured": {"rows": done, "of": cnt, "block_rows": block_rows(n)}, "baseline_pairs_equal": True,
               "speedup_count": round(b_count / us_count, 1), "speedup_count_fill": round(b_both / us_both, 1)}
        print(json.dumps(leg), file=sys.stderr, flush=True)
        res["legs"].append(leg)
        return leg

    v = vectors(n_mid, 1)
    count_mid = None
    for per_row in (1, 32, 1000):
        leg = radius_leg(v, 0, n_mid, radius_for(v, per_row), f"all rows, about {per_row} per row")
        if per_row == 32:
            count_mid = leg["count_us"]
    # beside: the matrix call alone (into one block, every block) and kNN k = 10
    b = block_rows(n_mid)
    buf = torch.empty((b, n_mid), dtype=torch.float32, device="cuda")
    us_matrix = timed(lambda: [matrix_rows(v, s, min(b, n_mid - s), buf) for s in range(0, n_mid, b)], a.reps)
    ki = torch.empty((n_mid, 10), dtype=torch.int32, device="cuda")
    kv = torch.empty((n_mid, 10), dtype=torch.float32, device="cuda")
    us_knn = timed(lambda: lib.bl_amd_knn_device(P(v), n_mid, 0, n_mid, 10, DIST, P(ki), P(kv), None), a.reps)
    res["beside"] = {"n": n_mid, "count_us_at_32_per_row": count_mid, "distance_matrix_us": round(us_matrix, 1),
                     "knn_k10_us": round(us_knn, 1)}
    del buf, v
    v = vectors(n_big, 2)
    r_big = radius_for(v, 32)
    radius_leg(v, n_big // 2, 1, r_big, "1 query row")
    radius_leg(v, n_big // 2, 64, r_big, "64 query rows")
    del v

    # ---- duplicate groups ---------------------------------------------------------------------------------------
    def groups_leg(n, seed):
        v = vectors(n, seed)
        g = torch.Generator(device="cpu").manual_seed(seed + 100)
        pick = torch.randperm(n, generator=g)[:2 * (n // 100)].cuda()
        half = pick.numel() // 2
        v[pick[half:]] = v[pick[:half]]            # 1 % of the songs are exact copies of another 1 %
        r = 1e-4
        out = torch.empty(n, dtype=torch.int32, device="cuda")
        call = lambda: lib.bl_amd_groups_device(P(v), n, DIST, r, P(out), None)   # noqa: E731
        assert call() == 0
        b = block_rows(n)
        nb = (n + b - 1) // b
        mb = None if nb <= a.base_blocks else a.base_blocks

        def base():
            _, rows, idx, _, done = baseline(v, 0, n, r, True, mb)
            return propagate(n, rows, idx.to(torch.int64)), done
        label, done = base()
        if done == n:
            assert torch.equal(label.to(torch.int32), out), "baseline and bl_amd_groups_device disagree"
        else:   # a partial baseline has the edges of its rows only: every edge it found must be inside one group
            _, rows, idx, _, _ = baseline(v, 0, n, r, True, mb)
            assert torch.equal(out[rows], out[idx.to(torch.int64)]), "baseline edges cross bl_amd_groups_device groups"
        want = torch.arange(n, device="cuda", dtype=torch.int32)
        want[pick[half:]] = torch.minimum(pick[half:], pick[:half]).to(torch.int32)
        want[pick[:half]] = torch.minimum(pick[half:], pick[:half]).to(torch.int32)
        assert torch.equal(out, want), "the groups are not the planted duplicates"
        us = timed(call, a.reps)
        b_us = timed(base, 1, warm=0) * (n / done)
        leg = {"leg": "duplicate groups, 1 % planted", "n": n, "radius": r, "groups_us": round(us, 1),
               "baseline_us": round(b_us, 1), "baseline_measured": {"rows": done, "of": n, "block_rows": b},
               "speedup": round(b_us / us, 1)}
        print(json.dumps(leg), file=sys.stderr, flush=True)
        res["legs"].append(leg)

    groups_leg(n_mid, 3)
    groups_leg(n_big, 4)
    res["all_legs_faster_than_baseline"] = all(
        (x["count_us"] < x["baseline_count_us"] and x["count_fill_us"] < x["baseline_count_fill_us"])
        if "count_us" in x else x["groups_us"] < x["baseline_us"] for x in res["legs"])
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
