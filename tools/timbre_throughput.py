#!/usr/bin/env python3
"""Device time of the spectral timbre (bl_amd_timbre_batch_device) beside the frequency pass it shares its transform
with, written down, not asserted: synthetic songs at 22 050 Hz stereo, resident in HBM, in two shapes — 1 024 songs of
30 s and 256 songs of 180 s.

    python tools/timbre_throughput.py [--reps 1000] [--out profiles/timbre_throughput.json]

timbre() is timed with device events over --reps back-to-back calls after a warm-up, with and without the per-frame
records, and with them once more, so that the spread between two windows of the same work is in the file.  One call
takes about a millisecond: the default of 1 000 repetitions makes every window about a second, long enough for the
shader clock to settle.  The yardstick is taken in the same process over the same arena: k_freq_scan as
bl_amd_profile_ms("freq_scan") reports it for DeviceCorpus.analyze() of the same batch.  That kernel runs the same
transform (freq_frames_lavc) with the statistics riding along and eight waves per workgroup; k_timbre runs it with four
waves per workgroup and the per-frame integer stage behind it.  The shader clock is read from the amdgpu hwmon files while the timed loops run
(bench.DeviceState).  Needs a GPU: there is no other way to get a time."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((1024, 30), (256, 180))


def timed(corpus, torch, reps, warmup, **kw):
    for _ in range(warmup):
        corpus.timbre(**kw)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        corpus.timbre(**kw)
        ev[i + 1].record()
    torch.cuda.synchronize()
    per = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(reps))
    return {"ms_per_batch": ev[0].elapsed_time(ev[reps]) / reps, "ms_per_batch_min": per[0],
            "ms_per_batch_median": per[len(per) // 2], "ms_per_batch_max": per[-1]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--analyze-steps", type=int, default=20)
    ap.add_argument("--pct", type=int, default=85)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "timbre_throughput.json"))
    a = ap.parse_args()

    import ctypes as C

    import torch

    import bliss_amd
    from bench import DeviceState
    if not torch.cuda.is_available():
        sys.exit("timbre_throughput.py needs a GPU: a time taken anywhere else says nothing")
    rate, ch = 22050, 2
    state = DeviceState(DeviceState.pci_address(0))
    state.start()
    t0 = time.perf_counter()
    shapes = []
    for songs, seconds in SHAPES:
        n = rate * ch * seconds
        corpus = bliss_amd.DeviceCorpus([n] * songs, ch, seconds)
        corpus.synth(seed_base=1, sample_rate=rate)
        torch.cuda.synchronize()
        lib = corpus.lib
        # the yardstick: k_freq_scan of the analysis over the same arena
        corpus.analyze()
        torch.cuda.synchronize()
        lib.bl_amd_profile_reset()
        lib.bl_amd_profile(1)
        for _ in range(a.analyze_steps):
            corpus.analyze()
        torch.cuda.synchronize()
        lib.bl_amd_profile(0)
        k = C.c_int(0)
        yard_ms = lib.bl_amd_profile_ms(b"freq_scan", C.byref(k))
        assert k.value == a.analyze_steps, "the analysis did not run k_freq_scan once per step"
        yard_ms /= k.value
        with_frames = timed(corpus, torch, a.reps, a.warmup, pct=a.pct, frames=True)
        st, fr = corpus.fetch_timbre()
        without = timed(corpus, torch, a.reps, a.warmup, pct=a.pct, frames=False)
        st2, _ = corpus.fetch_timbre()
        again = timed(corpus, torch, a.reps, a.warmup, pct=a.pct, frames=True)
        frames = int(st["frames"].sum())
        shapes.append({
            "songs": songs, "seconds": seconds, "pcm_bytes": corpus.pcm_bytes, "frames": frames,
            "freq_scan_ms": yard_ms,
            "timbre_with_frames": with_frames, "timbre_without_frames": without, "timbre_with_frames_again": again,
            "ratio_with_frames": with_frames["ms_per_batch"] / yard_ms,
            "ratio_without_frames": without["ms_per_batch"] / yard_ms,
            "ns_per_frame_without_frames": without["ms_per_batch"] * 1e6 / frames,
            "check": {"status_all_ok": bool((st["status"] == 0).all()), "used": int(st["used"].sum()),
                      "frame_records": int(fr.size), "same_song_records": st.tobytes() == st2.tobytes(),
                      "rolloff_mean_bins": float(st["rolloff_sum"].sum()) / max(int(st["used"].sum()), 1)},
        })
        del corpus
        torch.cuda.empty_cache()
    t1 = time.perf_counter()
    state.stop_flag = True
    state.join()
    out = {
        "what": "bl_amd_timbre_batch_device (k_timbre) over a resident corpus, device events over `reps` back-to-back "
                "calls after `warmup` calls, with and without the per-frame records; the yardstick is k_freq_scan of "
                "DeviceCorpus.analyze() over the same arena in the same process (bl_amd_profile_ms), average of "
                "`analyze_steps` launches",
        "sample_rate": rate, "channels": ch, "pct": a.pct, "min_energy": 0, "reps": a.reps, "warmup": a.warmup,
        "analyze_steps": a.analyze_steps,
        "shapes": shapes,
        "device": torch.cuda.get_device_name(0),
        "device_state": state.summary(t0, t1),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps([{k: s[k] for k in ("songs", "seconds", "freq_scan_ms", "ratio_with_frames", "ratio_without_frames")}
                      for s in shapes]))


if __name__ == "__main__":
    main()
