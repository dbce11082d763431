#!/usr/bin/env python3
"""Two builds of libbliss_amd.so on one synthetic S180 corpus, compared bit for bit: every f32 window energy (how many
moved, by how many ulp) and every field of the song records (how many songs differ per field).  Each library runs in
its own process (BLISS_AMD_LIB) and leaves its energies and records in a temporary directory; prints one JSON object.
Where tools/ab_libs.py says whether the records are identical, this says what differs.
usage: python tools/energy_ab.py --libs bliss_amd/libbliss_amd.so,<other>/libbliss_amd.so [--songs 8192]
       [--seconds 180] [--fir-mode 2] [--seed-base 100000]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(a):
    sys.path.insert(0, ROOT)
    import torch
    import bliss_amd
    lib = bliss_amd.load()
    if a.fir_mode >= 0:
        assert lib.bl_amd_set_fir_mode(a.fir_mode) == 0
    corpus = bliss_amd.DeviceCorpus([44100 * 2 * a.seconds] * a.songs, 2, a.seconds)
    corpus.synth(seed_base=a.seed_base, sample_rate=44100)
    torch.cuda.synchronize()
    corpus.analyze()
    got = corpus.fetch()
    total = int(got["nb_frames"].astype(np.int64).sum())
    en = np.zeros(total, dtype=np.float32)
    assert lib.bl_amd_last_energies(en.ctypes.data_as(C.POINTER(C.c_float)), total) == total
    np.save(a.out + "_rec.npy", got)
    np.save(a.out + "_en.npy", en)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", default="")
    ap.add_argument("--songs", type=int, default=8192)
    ap.add_argument("--seconds", type=int, default=180)
    ap.add_argument("--fir-mode", type=int, default=2)
    ap.add_argument("--seed-base", type=int, default=100000)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.child:
        return child(a)
    libs = [os.path.abspath(p) for p in a.libs.split(",") if p]
    if len(libs) != 2:
        ap.error("--libs: two libraries, comma-separated")
    with tempfile.TemporaryDirectory() as d:
        outs = []
        for i, p in enumerate(libs):
            out = os.path.join(d, str(i))
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--out", out, "--songs", str(a.songs),
                            "--seconds", str(a.seconds), "--fir-mode", str(a.fir_mode), "--seed-base", str(a.seed_base)],
                           env=dict(os.environ, BLISS_AMD_LIB=p), check=True)
            outs.append(out)
        ra, rb = (np.load(o + "_rec.npy") for o in outs)
        ea, eb = (np.load(o + "_en.npy") for o in outs)
    d = np.abs(ea.view(np.int32).astype(np.int64) - eb.view(np.int32).astype(np.int64))
    moved = np.nonzero(d)[0]
    fields = {}
    for k in ra.dtype.names:
        x = np.ascontiguousarray(ra[k]).view(np.uint8).reshape(len(ra), -1)
        y = np.ascontiguousarray(rb[k]).view(np.uint8).reshape(len(rb), -1)
        fields[k] = int(np.count_nonzero(np.any(x != y, axis=1)))
    offs = np.concatenate([[0], np.cumsum(ra["nb_frames"].astype(np.int64))])
    print(json.dumps({
        "libs": [os.path.relpath(p, ROOT) for p in libs], "songs": a.songs, "seconds": a.seconds, "fir_mode": a.fir_mode,
        "seed_base": a.seed_base, "energy_slots": int(len(ea)), "windows": int(ra["n_windows"].astype(np.int64).sum()),
        "energies_moved": int(len(moved)), "energies_moved_per_window": len(moved) / max(int(ra["n_windows"].sum()), 1),
        "max_ulp_moved": int(d.max()) if len(d) else 0,
        "moved_at": [{"song": int(np.searchsorted(offs, i, side="right") - 1), "slot": int(i - offs[np.searchsorted(offs, i, side="right") - 1])}
                     for i in moved[:20]],
        "songs_differing_by_field": fields}, indent=1))


if __name__ == "__main__":
    sys.exit(main())
