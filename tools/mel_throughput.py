#!/usr/bin/env python3
"""Device time of the mel call (bl_amd_mel_batch_device) beside the spectral timbre and the frequency pass it shares its
transform with, written down, not asserted: synthetic songs at 22 050 Hz stereo, resident in HBM, in the two shapes of
profiles/timbre_throughput.json — 1 024 songs of 30 s and 256 songs of 180 s — so the two files read side by side.

    python tools/mel_throughput.py [--reps 300] [--out profiles/mel_throughput.json]

Three things are timed in one run on one GPU.  The whole mel call, with both per-frame outputs (frame records and band
levels) and with neither, and bl_amd_timbre_batch_device without its frame records over the same arena: device events
over --reps back-to-back calls after a warm-up, into buffers allocated once.  And k_freq_scan as
bl_amd_profile_ms("freq_scan") reports it for DeviceCorpus.analyze() of the same batch.  All three run the same
transform (freq_frames_lavc); k_freq_scan with the statistics riding along and eight waves per workgroup, k_timbre and
k_mel with four and their per-frame integer stages behind it.  The shader clock is read from the amdgpu hwmon files
while the timed loops run (bench.DeviceState).  Needs a GPU: there is no other way to get a time."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((1024, 30), (256, 180))


def timed(enqueue, torch, reps, warmup):
    for _ in range(warmup):
        enqueue()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        enqueue()
        ev[i + 1].record()
    torch.cuda.synchronize()
    per = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(reps))
    return {"ms_per_batch": ev[0].elapsed_time(ev[reps]) / reps, "ms_per_batch_min": per[0],
            "ms_per_batch_median": per[len(per) // 2], "ms_per_batch_max": per[-1]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--analyze-steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mel_throughput.json"))
    a = ap.parse_args()

    import ctypes as C

    import numpy as np
    import torch

    import bliss_amd
    from bench import DeviceState
    from bliss_amd.records import FRAME_MEL_DTYPE, MEL_DTYPE
    if not torch.cuda.is_available():
        sys.exit("mel_throughput.py needs a GPU: a time taken anywhere else says nothing")
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
        scan_ms = lib.bl_amd_profile_ms(b"freq_scan", C.byref(k))
        assert k.value == a.analyze_steps, "the analysis did not run k_freq_scan once per step"
        scan_ms /= k.value
        frames = songs * ((n // ch) // 512)
        rec = torch.zeros(songs * MEL_DTYPE.itemsize, dtype=torch.uint8, device=corpus.device)
        rec2 = torch.zeros_like(rec)
        fr = torch.zeros(frames * FRAME_MEL_DTYPE.itemsize, dtype=torch.uint8, device=corpus.device)
        bd = torch.zeros(frames * 128, dtype=torch.uint8, device=corpus.device)
        pcm, stream = C.c_void_p(corpus.pcm.data_ptr()), corpus._stream()

        def mel(out, with_frames):
            corpus._call("mel_batch_device", None, pcm, corpus.desc, songs, 0, C.c_void_p(out.data_ptr()),
                         C.c_void_p(fr.data_ptr()) if with_frames else C.c_void_p(),
                         C.c_void_p(bd.data_ptr()) if with_frames else C.c_void_p(), frames, stream)
        timbre = timed(lambda: corpus.timbre(frames=False), torch, a.reps, a.warmup)
        with_frames = timed(lambda: mel(rec, True), torch, a.reps, a.warmup)
        without = timed(lambda: mel(rec2, False), torch, a.reps, a.warmup)
        again = timed(lambda: mel(rec, True), torch, a.reps, a.warmup)
        st = np.frombuffer(rec.cpu().numpy().tobytes(), dtype=MEL_DTYPE)
        st2 = np.frombuffer(rec2.cpu().numpy().tobytes(), dtype=MEL_DTYPE)
        shapes.append({
            "songs": songs, "seconds": seconds, "pcm_bytes": corpus.pcm_bytes, "frames": frames,
            "freq_scan_ms": scan_ms, "timbre_without_frames": timbre,
            "mel_with_frames": with_frames, "mel_without_frames": without, "mel_with_frames_again": again,
            "ratio_to_timbre_with_frames": with_frames["ms_per_batch"] / timbre["ms_per_batch"],
            "ratio_to_timbre_without_frames": without["ms_per_batch"] / timbre["ms_per_batch"],
            "ratio_to_freq_scan_with_frames": with_frames["ms_per_batch"] / scan_ms,
            "ratio_to_freq_scan_without_frames": without["ms_per_batch"] / scan_ms,
            "ns_per_frame_without_frames": without["ms_per_batch"] * 1e6 / frames,
            "check": {"status_all_ok": bool((st["status"] == 0).all()), "frames": int(st["frames"].sum()),
                      "used": int(st["used"].sum()), "same_song_records": st.tobytes() == st2.tobytes(),
                      "mfcc0_mean_log2": float(st["mfcc_sum"][:, 0].sum()) / max(int(st["used"].sum()), 1) / 4096.0},
        })
        del corpus, rec, rec2, fr, bd
        torch.cuda.empty_cache()
    t1 = time.perf_counter()
    state.stop_flag = True
    state.join()
    out = {
        "what": "bl_amd_mel_batch_device (k_mel) over a resident corpus, device events over `reps` back-to-back calls "
                "after `warmup` calls, with both per-frame outputs and with neither; beside it, the same way, "
                "bl_amd_timbre_batch_device (k_timbre) without frame records, and k_freq_scan of DeviceCorpus.analyze() "
                "over the same arena in the same process (bl_amd_profile_ms), average of `analyze_steps` launches",
        "sample_rate": rate, "channels": ch, "min_energy": 0, "reps": a.reps, "warmup": a.warmup,
        "analyze_steps": a.analyze_steps,
        "shapes": shapes,
        "device": torch.cuda.get_device_name(0),
        "device_state": state.summary(t0, t1),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps([{k: s[k] for k in ("songs", "seconds", "freq_scan_ms", "ratio_to_timbre_with_frames",
                                         "ratio_to_timbre_without_frames")} for s in shapes]))


if __name__ == "__main__":
    main()
