#!/usr/bin/env python3
"""Throughput of the song structure (bl_amd_form_device), written down, not asserted.

    python tools/form_bench.py [--shapes 8192x180,1024x30] [--pools 1,4] [--seg-seconds 15] [--nov-seconds 4]
                               [--out profiles/form_throughput.json]

For every shape (songs x seconds of mono PCM at 22 050 Hz, synthesised on the device) the chroma call that produces the
frames (bl_amd_chroma_batch_device with frames) and the structure call over those frames take turns in alternating
windows of one run: for every pool P of --pools, with M = minlag of about --seg-seconds and L of about --nov-seconds,
without and with the rep output.  The ratio to the chroma call is the figure a caller plans with.

There is no earlier implementation to compare with, so each kernel is also set against a floor of its own, over 256 CUs
x 4 SIMDs x 16 lanes per clock at --clock-ghz and at the mean shader clock sampled over the run:
  k_form_thumb    every similarity S(v, v + l) of every valid lag once: 3 packed dot products, one addition when it
                  enters a window and one subtraction when it leaves: 5 vector instructions for each of the
                  sum over l of (U - l) similarities;
  k_form_novelty  the direct form: per unit with a value and per a = 1 .. L, 12 x (subtract, multiply-add), then
                  12 x 3 for the squares: 24 L + 36;
  k_form_units    the bytes it must move (96 P read, 16 written per unit) at HBM peak (--hbm-tbs).

A song of 30 s has 321 frames: at P = 1 and M = minlag = 161 it is one unit short of a thumbnail, so that shape times the
units and the novelty, and its thumbnail floor is 0; at P = 4 it has one candidate.  A floor below a microsecond is below
any launch, so its ratio is written as null.

A window is about --window-ms of back-to-back calls (--reps at least) between device events, and the windows take turns
--rounds times.  The kernels are timed in a run of their own through bl_amd_profile and bl_amd_form_profile_ms.  Needs a
GPU: there is no other way to get a time."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LANES_PER_CLOCK = 256 * 4 * 16
OPS_PER_SIMILARITY = 5
KERNELS = ("form_units", "form_thumb", "form_novelty")
FLOOR_MIN_MS = 1e-3


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
        lib.bl_amd_form_profile_ms(name.encode(), None)   # forget what was collected before
    lib.bl_amd_profile(1)
    for _ in range(a.reps):
        call()
    torch.cuda.synchronize()
    lib.bl_amd_profile(0)
    out = {}
    for name in KERNELS:
        k = C.c_int(0)
        out[name] = {"ms_per_call": lib.bl_amd_form_profile_ms(name.encode(), C.byref(k)) / a.reps, "launches": k.value}
    return out


def floors(n, t, p, a):
    """the three floors in ms at --clock-ghz for n songs of t frames under the parameters p"""
    u = t // p.pool
    sims = sum(u - l for l in range(p.min_lag, u - p.seg + 1))
    valued = max(0, u - 2 * p.nov + 1)
    per_ms = LANES_PER_CLOCK * a.clock_ghz * 1e6
    return {"units_per_song": u, "similarities_per_song": sims,
            "form_thumb": n * sims * OPS_PER_SIMILARITY / per_ms,
            "form_novelty": n * valued * (24 * p.nov + 36) / per_ms,
            "form_units": n * u * (96 * p.pool + 16) / (a.hbm_tbs * 1e9)}


def shape_part(torch, lib, a, n, seconds):
    import bliss_amd
    import bliss_amd.chroma as ch
    import bliss_amd.form as form
    samples = seconds * 22050
    corpus = bliss_amd.DeviceCorpus([samples] * n, 1, seconds)
    corpus.synth(seed_base=1, sample_rate=22050)
    rec, frames = ch.chroma_device(corpus, frames=True)
    t = max(0, (samples - 4096) // 2048 + 1)
    counts = (C.c_int32 * n)(*([t] * n))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = torch.empty(n * 48, dtype=torch.uint8, device="cuda")

    def chroma():
        rc = lib.bl_amd_chroma_batch_device(C.c_void_p(corpus.pcm.data_ptr()), corpus.desc, n,
                                            C.c_void_p(rec.data_ptr()), C.c_void_p(frames.data_ptr()), n * t, stream)
        assert rc == 0

    calls, meta, keep = {"chroma_with_frames": chroma}, {}, []
    for pool in a.pools:
        per_s = 22050 / 2048 / pool
        seg = min(1024, max(2, round(a.seg_seconds * per_s)))
        p = form.params(pool=pool, seg=seg, min_lag=seg, nov=min(64, max(1, round(a.nov_seconds * per_s))))
        u = t // pool
        rep = torch.empty(max(n * u, 1) * 2, dtype=torch.int32, device="cuda")
        keep.append((p, rep))
        for with_rep in (False, True):
            def call(p=p, u=u, rp=rep if with_rep else None):
                rc = lib.bl_amd_form_device(C.c_void_p(frames.data_ptr()), counts, n, C.byref(p),
                                            C.c_void_p(out.data_ptr()), None, C.c_void_p(rp.data_ptr()) if rp is not None
                                            else None, None, None, n * u, stream)
                assert rc == 0
            name = f"form_p{pool}" + ("_rep" if with_rep else "")
            calls[name] = call
            meta[name] = dict(pool=pool, seg=p.seg, min_lag=p.min_lag, nov=p.nov, rep=with_rep, params=p)
    res = alternate(torch, a, calls)
    base = res["chroma_with_frames"]["ms_per_call"]
    for name, m in meta.items():
        p = m.pop("params")
        r = res[name]
        fl = floors(n, t, p, a)
        r.update(m, ratio_to_chroma=r["ms_per_call"] / base, units_per_song=fl.pop("units_per_song"),
                 similarities_per_song=fl.pop("similarities_per_song"), kernels=kernels_ms(torch, lib, a, calls[name]))
        for k in KERNELS:
            r["kernels"][k]["floor_ms"] = fl[k]
            # a floor below a microsecond is below any launch: a ratio to it would measure the launch
            r["kernels"][k]["ratio_to_floor"] = r["kernels"][k]["ms_per_call"] / fl[k] if fl[k] >= FLOOR_MIN_MS else None
        got = form.form_to_numpy(out.cpu().numpy())
        r["check"] = {"with_thumbnail": int((got["status"] == 0).sum()), "boundaries_mean": float(got["boundaries"].mean()),
                      "score_mean": float(form.score(got[got["status"] == 0]).mean()) if (got["status"] == 0).any()
                      else None}
    return {"songs": n, "seconds": seconds, "frames_per_song": t, "pcm_bytes": corpus.pcm_bytes, "calls": res}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="8192x180,1024x30")
    ap.add_argument("--pools", default="1,4")
    ap.add_argument("--seg-seconds", type=float, default=15.0)
    ap.add_argument("--nov-seconds", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "form_throughput.json"))
    a = ap.parse_args()
    a.pools = [int(x) for x in a.pools.split(",")]
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]

    import torch

    from bench import DeviceState
    if not torch.cuda.is_available():
        sys.exit("form_bench.py needs a GPU: a time taken anywhere else says nothing")
    import bliss_amd
    lib = bliss_amd.load()
    assert lib.bl_amd_init(0) == 0
    state = DeviceState(DeviceState.pci_address(0))
    state.start()
    t0 = time.perf_counter()
    out = {"what": "bl_amd_form_device beside the bl_amd_chroma_batch_device call that produces its frames, over one "
                   "arena per shape: alternating windows of about `window_ms` of back-to-back calls (`reps` at least) "
                   "between device events, `rounds` windows each, after `warmup` calls; the kernels through "
                   "bl_amd_form_profile_ms in a run of their own, against the floors the tool's docstring defines",
           "reps": a.reps, "window_ms": a.window_ms, "rounds": a.rounds, "warmup": a.warmup,
           "ops_per_similarity": OPS_PER_SIMILARITY, "lanes_per_clock": LANES_PER_CLOCK, "clock_ghz": a.clock_ghz,
           "hbm_tbs": a.hbm_tbs, "device": torch.cuda.get_device_name(0), "shapes": []}
    for n, seconds in shapes:
        out["shapes"].append(shape_part(torch, lib, a, n, seconds))
        torch.cuda.empty_cache()
    state.stop_flag = True
    state.join()
    out["device_state"] = state.summary(t0, time.perf_counter())
    mhz = (out["device_state"].get("sclk_mhz") or {}).get("mean")
    if mhz:   # the instruction floors assume --clock-ghz; the same ratios at the mean shader clock of the whole run
        out["mean_clock_mhz"] = mhz
        for s in out["shapes"]:
            for r in s["calls"].values():
                for k in ("form_thumb", "form_novelty"):
                    if "kernels" in r and r["kernels"][k]["floor_ms"] >= FLOOR_MIN_MS:
                        kk = r["kernels"][k]
                        kk["floor_ms_at_mean_clock"] = kk["floor_ms"] * a.clock_ghz * 1e3 / mhz
                        kk["ratio_to_floor_at_mean_clock"] = kk["ms_per_call"] / kk["floor_ms_at_mean_clock"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for s in out["shapes"]:
        print(json.dumps({"songs": s["songs"], "seconds": s["seconds"],
                          "ms": {k: round(v["ms_per_call"], 3) for k, v in s["calls"].items()},
                          "thumb_ratio_to_floor": {k: round(v["kernels"]["form_thumb"]["ratio_to_floor"] or 0.0, 2)
                                                   for k, v in s["calls"].items() if "kernels" in v}}), flush=True)


if __name__ == "__main__":
    main()
