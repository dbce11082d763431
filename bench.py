#!/usr/bin/env python3
"""bench.py — throughput of the bliss analysis hot path on MI355X.

One *step* = one pass of the hot path over one resident batch of synthetic decoded
songs: frequency pass with the statistics riding along -> envelope / amplitude kernels -> force vectors
(bl_analyze after decode, ref src/analyze.c:40-80), then — as BASELINE.json's
batch-of-songs mode asks — an all-gather of the 16-byte force vectors over RCCL and this
rank's row block of the bl_distance matrix (ref src/analyze.c:96-100).

Workload: BASELINE.json configs[2] shape — 3-minute 44.1 kHz s16 stereo buffers
(15 876 000 interleaved int16 each), `--songs-per-gpu` of them resident in HBM per rank
(default: the configs[2] shard of 8 192 per GPU when it fits, else the largest count that
does; the count used is printed in config.workload).  Songs are sharded by index across
ranks (weak scaling, no data-path collective other than the vector all-gather).

Launch: `python bench.py --gpus N --steps K --warmup W` — for N > 1 (or with `--launch`) the
script starts its own N ranks, one per GPU, under torch.distributed.run on 127.0.0.1 and passes
their output through — or the launcher form the driver uses,
`python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1
 --master-port P bench.py --gpus N --steps K --warmup W`.
Either way rank 0 prints ONE JSON line.  `--plumbing-only` runs launch, process group (gloo),
sharding and the all-gather on stand-in vectors without a GPU: the CPU test of this plumbing.

A plain run sets up, warms up, times the K steps and prints the line (`value`, `ms_per_step`, the
per-kernel HIP-event times of the timed steps and the roofline arithmetic on them).  `--full` adds
everything measured or checked beside it after the timed region: the oracle check of `--verify`
songs, the FIR mode 0 steps, BASELINE configs[1] / configs[4], the 10 000 x 10 000 matrices, the
PMC traffic passes and the CPU baseline.  `--dump-outputs DIR` writes what the last timed step
computed (rank 0's share) as DIR/<name>.npy, for comparing two builds output for output.
"""
import argparse
import ctypes as C
import glob
import json
import os
import subprocess
import sys
import threading
import time

# dmabuf IPC: RCCL (and any CUDA-tensor sharing across processes) needs it on this driver; it has to be in the
# environment before the HIP runtime starts, whichever launcher started this rank
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

SONG_SAMPLES = 44100 * 2 * 180          # S180 of SURVEY.md §8
SONG_SECONDS = 180
SAMPLE_RATE = 44100
HBM_PEAK_GBS = 8000.0                   # spec, /opt/skills/guides/MI355X_MICROARCH.md
HBM_ACHIEVABLE_GBS = 6290.0             # measured float4 copy, same guide
FP64_VALU_PEAK_TFLOPS = 78.6            # spec (FMA = 2 flop); the faithful path's real ceiling


class DeviceState(threading.Thread):
    """Shader clock, socket power and temperature of one GPU while something runs on it: a thread that reads the
    amdgpu hwmon files of the device with PCI address `bdf` every `period` seconds.  The envelope window kernel does not
    run at the 2.4 GHz the part is specified with (f64 vector load: ~2.2 GHz at ~1.15 kW on the boxes measured), and
    boxes differ by a few per cent; this is what makes a slow lease distinguishable from a regression."""

    FILES = ("freq1_input", "power1_average", "power1_input", "temp2_input", "temp1_input", "power1_cap")

    def __init__(self, bdf, period=0.02):
        super().__init__(daemon=True)
        self.period, self.rows, self.stop_flag, self.files = period, [], False, {}
        self.bdf = bdf
        for card in sorted(glob.glob("/sys/class/drm/card[0-9]*")):
            dev = os.path.join(card, "device")
            try:
                if os.path.basename(os.path.realpath(dev)).lower() != (bdf or "").lower():
                    continue
            except OSError:
                continue
            for hw in glob.glob(os.path.join(dev, "hwmon", "hwmon*")):
                for f in self.FILES:
                    if os.path.exists(os.path.join(hw, f)):
                        self.files[f] = os.path.join(hw, f)
            break

    @staticmethod
    def pci_address(ordinal):
        try:
            buf = C.create_string_buffer(64)
            if C.CDLL("libamdhip64.so").hipDeviceGetPCIBusId(buf, 64, int(ordinal)) == 0:
                return buf.value.decode()
        except OSError:
            pass
        return None

    @staticmethod
    def _rd(path, scale):
        try:
            with open(path) as f:
                return float(f.read().strip()) / scale
        except (OSError, ValueError):
            return None

    def run(self):
        f = self.files
        while not self.stop_flag and "freq1_input" in f:
            t = time.perf_counter()
            self.rows.append((t, self._rd(f["freq1_input"], 1e6),
                              self._rd(f.get("power1_average") or f.get("power1_input", ""), 1e6),
                              self._rd(f.get("temp2_input") or f.get("temp1_input", ""), 1e3)))
            dt = self.period - (time.perf_counter() - t)
            if dt > 0:
                time.sleep(dt)

    def summary(self, t0, t1):
        import numpy as np
        sel = [r for r in self.rows if t0 <= r[0] <= t1]
        out = {"pci": self.bdf, "samples": len(sel), "period_s": self.period,
               "source": "amdgpu hwmon (freq1_input / power1_* / temp*_input) of this rank's device, sampled over the "
                         "timed region" if self.files else "no amdgpu hwmon files found for this device"}
        for j, k in ((1, "sclk_mhz"), (2, "power_w"), (3, "temp_c")):
            v = np.array([r[j] for r in sel if r[j] is not None], dtype=float)
            if len(v):
                out[k] = {"mean": round(float(v.mean()), 1), "min": round(float(v.min()), 1),
                          "p50": round(float(np.median(v)), 1), "max": round(float(v.max()), 1)}
        cap = self._rd(self.files["power1_cap"], 1e6) if "power1_cap" in self.files else None
        out["power_cap_w"] = cap
        return out


def _cpu_limits():
    """What the box lets this process use: affinity mask, cgroup quota."""
    info = {"os_cpu_count": os.cpu_count()}
    try:
        info["sched_affinity"] = len(os.sched_getaffinity(0))
    except Exception:
        info["sched_affinity"] = None
    quota = None
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                quota = None if txt[0] == "max" else float(txt[0]) / float(txt[1])
            else:
                q = float(txt[0])
                per = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                quota = None if q <= 0 else q / per
            break
        except Exception:
            continue
    info["cgroup_cpu_quota"] = quota
    return info


def cpu_baseline(ladder_levels=(1, 8, 32, 64, 128, 256)):
    """Oracle (CPU restatement, kind 'port') timed on this box's host cores on a bounded sample of
    the same workload.  One process per worker (not threads: the reference is not thread
    re-entrant — FFTW planner globals, ref src/tempo_atk_sort.c:94,294-295), each analysing
    synthetic 3-minute songs; like the GPU number, the rate counts analysis time only (orc_cli
    times orc_analyze_pcm, not the integer synthesis).  A ladder of 1 / 8 / 32 / 64 / 128 / 256
    concurrent processes shows where the box stops scaling: `cores` is the smallest process count
    that reaches 90 % of the best throughput — or the cgroup CPU quota when that is smaller (the
    GPU boxes of this pool expose 256 hardware threads under a quota of 16 CPUs) — and `value`
    the best throughput."""
    from tests.oracle_py import build_oracle
    build_oracle()
    cli = os.path.join(ROOT, "oracle", "orc_cli")
    limits = _cpu_limits()
    avail = limits["sched_affinity"] or limits["os_cpu_count"] or 1

    def level(procs, per_proc, seed0):
        t0 = time.time()
        ps = [subprocess.Popen([cli, "time", str(seed0 + 16 * i), str(SAMPLE_RATE), "2", str(SONG_SECONDS),
                                str(per_proc)], stdout=subprocess.PIPE, text=True) for i in range(procs)]
        rate, done = 0.0, 0
        for p in ps:
            o, _ = p.communicate()
            try:
                r = json.loads(o.strip().splitlines()[-1])
                rate += r["songs"] / r["seconds"]
                done += r["songs"]
            except Exception:
                pass
        wall = time.time() - t0
        return {"processes": procs, "songs": done, "songs_per_s": rate, "wall_s": wall}

    ladder = [level(1, 2, 9000)]
    one = ladder[0]["songs_per_s"]
    # rungs beyond four times the cgroup CPU quota only measure oversubscription (round 5: 44 songs/s at 32-64 processes
    # under a quota of 16, 30 at 256, 20 s of the driver's run): the ladder stops there, and as soon as two rungs in a
    # row are slower than the best so far
    quota = limits.get("cgroup_cpu_quota")
    top = min(avail, int(4 * quota)) if quota else avail
    slower = 0
    for procs in [p for p in ladder_levels if p > 1]:
        if procs > max(top, 1) or slower >= 2:
            break
        ladder.append(level(procs, 1, 9100 + procs))
        slower = slower + 1 if ladder[-1]["songs_per_s"] < max(l["songs_per_s"] for l in ladder[:-1]) else 0
    if not quota and ladder[-1]["processes"] != avail and avail > 1 and avail not in ladder_levels and len(ladder_levels) > 2 and slower < 2:
        ladder.append(level(avail, 1, 9700))
    best = max(l["songs_per_s"] for l in ladder)
    eff = next(l["processes"] for l in ladder if l["songs_per_s"] >= 0.9 * best)
    # a cgroup CPU quota below that count is the real amount of CPU the processes shared
    if quota and quota < eff:
        eff = int(round(quota))
    model = ""
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    # second half of the metric: the 10 000 x 10 000 bl_distance matrix as the nested loop of
    # the reference's per-pair function, one core
    dm_cpu = None
    try:
        import numpy as np
        from tests.oracle_py import Oracle
        orc = Oracle()
        v = (np.random.default_rng(4).standard_normal((10000, 4)) * 8).astype(np.float32)
        out = np.empty((10000, 10000), dtype=np.float32)
        t1 = time.time()
        orc.lib.orc_distance_matrix(v.ctypes.data_as(C.POINTER(C.c_float)), 10000,
                                    out.ctypes.data_as(C.POINTER(C.c_float)))
        dm_cpu = time.time() - t1
    except Exception:
        pass
    songs = sum(l["songs"] for l in ladder)
    return {"value": best, "unit": "songs/s", "cores": eff, "kind": "port",
            "distance_matrix_10k_s_one_core": dm_cpu,
            "sample": f"{songs} synthetic 3-min 44.1 kHz s16 stereo songs over a ladder of "
                      f"{[l['processes'] for l in ladder]} concurrent single-threaded processes "
                      "(1 song each, 2 at the first level), analysis time only; cores = min(smallest "
                      "process count within 10 % of the best throughput, cgroup CPU quota)",
            "sample_short": f"{songs} synthetic 3-min songs over {'/'.join(str(l['processes']) for l in ladder)} concurrent "
                            "1-thread oracle processes",
            "ladder": ladder, "limits": limits, "cpu_model": model,
            "one_core_songs_per_s": one, "scaling_vs_one_core": best / one if one else None}


def verify_songs(res, picks, seed_first, seconds):
    """Untimed: re-synthesise `picks` of the resident batch on the host (same integer generator,
    seeds = global song index) and analyse them with the CPU oracle (orc_cli); integers must be
    identical, f32 features within 1e-4 relative (north_star).  Returns (ok, details)."""
    import numpy as np
    from tests.oracle_py import build_oracle
    build_oracle()
    cli = os.path.join(ROOT, "oracle", "orc_cli")
    procs = [subprocess.Popen([cli, "synth", str(seed_first + i), str(SAMPLE_RATE), "2", str(seconds)],
                              stdout=subprocess.PIPE, text=True) for i in picks]
    ok, details = True, []
    for i, p in zip(picks, procs):
        o, _ = p.communicate()
        ref = json.loads(o.strip().splitlines()[-1])
        g = res[i]
        bad = [k for k in ("start", "end", "mean", "variance", "n_frames", "nb_frames", "n_windows", "beat",
                           "calm_or_loud") if int(g[k]) != int(ref[k])]
        worst, by_field = 0.0, {}
        for k in ("tempo", "amplitude", "frequency", "attack", "force"):
            a, b = float(g[k]), float(ref[k])
            rel = abs(a - b) / max(abs(b), 1e-6)
            worst = max(worst, rel)
            by_field[k] = rel
            if not rel <= 1e-4:
                bad.append(k)
        # all five f32 features bit-identical to the oracle's (orc_cli prints %.9g: a float survives the round trip)
        bits = all(np.float32(g[k]).view(np.int32) == np.float32(ref[k]).view(np.int32) for k in by_field)
        details.append({"song": int(i), "beat": int(g["beat"]), "max_rel_err": worst, "rel_err_by_field": by_field,
                        "value_by_field": {k: float(ref[k]) for k in by_field}, "features_bit_identical": bool(bits),
                        "mismatch": bad})
        ok = ok and not bad
    return ok, details


F64_ISSUE_TWAVEINSTR_S = 0.56     # measured f64 VALU issue rate, T wave-instr/s (tools/ubench_rate.hip; = 71.5 TF as FMA):
                                  # the rate at the clock the power cap leaves the kernel (1 024 SIMDs x ~2.19 GHz / 4)
F64_ISSUE_NOMINAL_TWAVEINSTR_S = 256 * 4 * 2.4e9 / 4 / 1e12   # 0.6144: the same pipe at the specified 2.4 GHz (78.6 TF as FMA;
                                  # /opt/skills/guides/MI355X_MICROARCH.md chip table: 256 CU x 4 SIMD, 2 400 MHz)
LINE_BYTES_MAX = 1700             # the printed line: the driver keeps the last 2 000 bytes of stdout + stderr
LINE_BYTES_MAX_LAUNCHED = 1450    # N > 1: torch.distributed.run adds ~420 bytes of its own to stderr (OMP_NUM_THREADS note)
# f64 wave-instructions per window the arithmetic needs, by FIR mode: mode 0 the
# reference's unfused FIR (25 ops/output) and two-op normalisation; 1: 17 ops/output; 2: no normalisation
F64_FLOOR_INSTR_PER_WINDOW = {0: 289, 1: 255, 2: 247}


def _committed_profile(songs, song_samples):
    """Counters of the newest committed PMC profile (profiles/*_hbm_traffic.json): HBM bytes per
    launch scaled to this launch, VALU instructions per window, busy fractions, the whole step's
    traffic ratio.  Never raises: what is missing is None and `error` says why."""
    import glob
    out = {"traffic": None, "error": None, "file": None}
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_hbm_traffic.json")))
    if not files:
        out["error"] = "no profiles/*_hbm_traffic.json committed"
        return out
    out["file"] = os.path.relpath(files[-1], ROOT)
    try:
        tj = json.load(open(files[-1]))
        kernels = tj["kernels"]
        tk = kernels["k_env_windows3"]
        scale = song_samples / 15876000.0
        out["traffic"] = tk["hbm_bytes_per_song"] * songs * scale
        out["git_head"] = tj.get("git_head")
        out["fir_mode"] = tj.get("fir_mode")
        out["valu_busy_frac"], out["lds_busy_frac"] = tk.get("valu_busy_frac"), tk.get("lds_busy_frac")
        psongs = tj.get("songs") or 0
        if tk.get("SQ_INSTS_VALU") and psongs:
            out["valu_instr_per_window"] = tk["SQ_INSTS_VALU"] / (psongs * 62012.0)
        step = [kernels[k]["hbm_bytes"] for k in ("k_pcm_scan", "k_freq_scan", "k_trim", "k_env_windows3", "k_freq_frames",
                                                  "k_amp_finish", "k_env_tail") if k in kernels and "hbm_bytes" in kernels[k]]
        if step and tj.get("algorithmic_bytes_per_launch"):
            out["whole_step_traffic_ratio"] = sum(step) / tj["algorithmic_bytes_per_launch"]
    except (OSError, KeyError, ValueError, TypeError) as e:
        out["error"] = f"{type(e).__name__}: {e}"
    return out


def _oracle_check(res, lengths, channels, durations, picks, seed_first):
    """Untimed: songs `picks` of a batch re-synthesised on the host and analysed by the CPU oracle (orc_cli synthn, one
    process per song); integers identical, f32 features <= 1e-4 relative."""
    from tests.oracle_py import build_oracle
    build_oracle()
    cli = os.path.join(ROOT, "oracle", "orc_cli")
    procs = [subprocess.Popen([cli, "synthn", str(seed_first + i), str(SAMPLE_RATE), str(channels[i]), str(lengths[i]),
                               str(durations[i])], stdout=subprocess.PIPE, text=True) for i in picks]
    ok, worst = True, 0.0
    for i, p in zip(picks, procs):
        o, _ = p.communicate()
        ref = json.loads(o.strip().splitlines()[-1])
        g = res[i]
        ok = ok and all(int(g[k]) == int(ref[k]) for k in ("start", "end", "mean", "variance", "n_frames", "nb_frames",
                                                            "n_windows", "beat", "calm_or_loud"))
        for k in ("tempo", "amplitude", "frequency", "attack", "force"):
            rel = abs(float(g[k]) - float(ref[k])) / max(abs(float(ref[k])), 1e-6)
            worst = max(worst, rel)
            ok = ok and rel <= 1e-4
    return bool(ok), worst


def other_configs(lib, dev, main_songs, steps=3):
    """BASELINE configs[1] and configs[4] through the same library, timed by this process after the main run (its
    resident batch has been freed): not `value`, which the contract quotes on configs[2] — the driver's clock on the
    other two shapes.  configs[1]: 1 024 synthetic 30-s 44.1 kHz s16 stereo buffers.  configs[4]: songs of log-uniform
    length in [10 s, 600 s] at 44.1 kHz, half mono / half stereo (the corpus of tools/mixed_bench.py; s32 sources are
    narrowed to s16 before the analysis and analysed as s16: the parity tests cover that path, this times the analysis)."""
    import numpy as np
    import torch
    import bliss_amd
    out = {}

    def run(name, lengths, channels, durations, seed0, what):
        corpus = bliss_amd.DeviceCorpus(lengths, channels, durations, device=str(dev))
        corpus.synth(seed_base=seed0, sample_rate=SAMPLE_RATE)
        corpus.analyze()
        torch.cuda.synchronize(dev)
        lib.bl_amd_profile_reset()
        lib.bl_amd_profile(1)
        t0 = time.perf_counter()
        for _ in range(steps):
            corpus.analyze()
        torch.cuda.synchronize(dev)
        dt = (time.perf_counter() - t0) / steps
        lib.bl_amd_profile(0)
        kern = {}
        for k in ("freq_scan", "env_windows", "env_tail", "amp_finish"):
            n = C.c_int(0)
            ms = lib.bl_amd_profile_ms(k.encode(), C.byref(n))
            kern[k] = ms / steps      # per batch (a mixed batch launches the window and tail kernels twice)
        res = corpus.fetch()
        n = len(lengths)
        order = np.argsort(np.asarray(lengths))
        picks = sorted(set(int(order[int(q * (n - 1))]) for q in (0.0, 0.3, 0.6, 0.85)))   # by length; not the longest: ~1 s of oracle each
        ok, worst = _oracle_check(res, lengths, channels, durations, picks, seed0)
        ok = ok and bool(np.all(res["status"] == 0))
        gb = corpus.pcm_bytes / 1e9
        out[name] = {"workload": what, "songs": n, "pcm_GB": gb, "ms_per_batch": 1e3 * dt, "songs_per_s": n / dt,
                     "pcm_GB_per_s": gb / dt, "frac_hbm": gb / dt / HBM_PEAK_GBS, "kernels_ms_per_batch": kern,
                     "steps": steps, "results_ok": ok, "verified_songs": len(picks), "worst_rel_err": worst}
        del corpus
        torch.cuda.empty_cache()

    n1 = 1024 if main_songs >= 1024 else max(4, main_songs)
    run("configs1", [SAMPLE_RATE * 2 * 30] * n1, [2] * n1, [30] * n1, 700000,
        f"BASELINE configs[1]: {n1} synthetic 30-s 44.1 kHz s16 stereo buffers, one batch call")
    n4 = min(8192, max(8, main_songs))
    rng = np.random.default_rng(5)
    secs = np.exp(rng.uniform(np.log(10.0), np.log(600.0), n4))
    ch = rng.integers(1, 3, n4)
    lengths = (np.floor(secs * SAMPLE_RATE).astype(np.int64) * ch).tolist()
    durs = np.maximum(1, np.floor(secs)).astype(np.int64).tolist()
    run("configs4_mixed", lengths, ch.tolist(), durs, 0,
        f"BASELINE configs[4] shape: {n4} songs of log-uniform length in [10 s, 600 s] at 44.1 kHz, half mono / half "
        "stereo, s16, one batch call (long songs first, own window launch: DESIGN.md section 4.2)")
    return out


def live_traffic(seconds, songs=1024, timeout=240):
    """HBM traffic of the kernels, collected in THIS run: two `rocprofv3 --pmc` passes (FETCH_SIZE, WRITE_SIZE — separate
    passes, --kernel-trace only, as /opt/skills/guides/MI355X_MICROARCH.md prescribes) around one step of this script
    over `songs` songs of the same shape, started as child processes after the parent has released its resident batch.
    Returns {kernel: bytes per song} with the gfx950 corrections (FETCH_SIZE counts half of a wide coalesced streaming
    read and is in KB; WRITE_SIZE is taken as is) or {"error": ...}: the caller falls back on the committed profile."""
    import csv
    import shutil
    import tempfile
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return {"error": "no rocprofv3 on this box"}
    acc = {}
    tmp = tempfile.mkdtemp(prefix="bl_traffic_", dir="/tmp")
    try:
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            out = os.path.join(tmp, counter)
            cmd = [exe, "--pmc", counter, "--kernel-trace", "--output-format", "csv", "-d", out, "--", sys.executable,
                   os.path.abspath(__file__), "--songs-per-gpu", str(songs), "--seconds", str(seconds), "--steps", "1",
                   "--warmup", "0", "--no-cpu-baseline", "--verify", "0", "--no-mode0-pass", "--no-other-configs",
                   "--no-live-traffic"]
            env = dict(os.environ, TMPDIR="/tmp")
            for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
                env.pop(k, None)
            r = subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
            files = glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True)
            if r.returncode != 0 or not files:
                return {"error": f"rocprofv3 --pmc {counter} failed (rc {r.returncode}): {r.stderr[-200:]}"}
            for f in files:
                for row in csv.DictReader(open(f)):
                    if row["Counter_Name"] != counter:
                        continue
                    k = row["Kernel_Name"].split("(")[0].replace("void ", "").split("<")[0]
                    v = float(row["Counter_Value"]) * 1024.0 * (2.0 if counter == "FETCH_SIZE" else 1.0)
                    acc[k] = acc.get(k, 0.0) + v
        return {k: v / songs for k, v in acc.items()}
    except (OSError, subprocess.TimeoutExpired, KeyError, ValueError) as e:
        return {"error": f"{type(e).__name__}: {e}"}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def _sig(x, sig=5):
    """A float of the printed line, rounded to `sig` significant digits (None for NaN / inf)."""
    if isinstance(x, bool) or x is None or isinstance(x, (int, str)):
        return x
    try:
        x = float(x)
    except (TypeError, ValueError):
        return None
    if x != x or x in (float("inf"), float("-inf")):
        return None
    return float(f"{x:.{sig}g}")


def compact_line(d, details_path=None, limit=LINE_BYTES_MAX):
    """The ONE line on stdout, from the full record `d` (which goes to bench_details.json).  The driver keeps the last
    2 000 bytes of stdout + stderr (BENCH_r05.json: a 21 KB line could not be parsed), so the line stays under `limit`
    bytes: the contract's keys first, then scalars in the order in which they are given up if the line were too long."""
    rf, cb = d.get("roofline") or {}, d.get("cpu_baseline") or {}
    cfg = d.get("config") or {}
    line = {k: d.get(k) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                                  "scaling", "vs_baseline", "dtype", "data")}
    for k in ("value", "ms_per_step"):
        line[k] = _sig(line[k], 7)
    line["config"] = {"workload": cfg.get("workload_short") or cfg.get("workload"), "songs_per_gpu": cfg.get("songs_per_gpu"),
                      "parallelism": cfg.get("parallelism"), "fir_mode": (d.get("fir_modes") or {}).get("timed_mode")}
    line["results_ok"], line["verified_songs"] = d.get("results_ok"), d.get("verified_songs")
    line["roofline"] = None if not rf else {
        "bound": rf.get("bound"), "kernel": rf.get("kernel"), "achieved": _sig(rf.get("achieved")), "peak": rf.get("peak"),
        "unit": rf.get("unit"), "frac": _sig(rf.get("frac")), "traffic": _sig(rf.get("traffic"), 6),
        "traffic_src": ("live_pmc" if str((rf.get("traffic_source") or {}).get("what", "")).startswith("collected in this run")
                        else ((rf.get("traffic_source") or {}).get("file") if rf.get("traffic") else None)),
        "ms_avg_launch": _sig(rf.get("ms_avg_launch")), "algorithmic_bytes_per_launch": rf.get("algorithmic_bytes_per_launch"),
        "frac_of_f64_floor": _sig(rf.get("frac_of_f64_floor"), 4),
        "frac_of_f64_floor_nominal": _sig(rf.get("frac_of_f64_floor_nominal"), 4),
        "whole_step_traffic_ratio": _sig(rf.get("whole_step_traffic_ratio"), 4),
        "frac_fir_mode0": _sig(rf.get("frac_fir_mode0"), 4)}
    line["cpu_baseline"] = {"value": _sig(cb.get("value"), 4), "unit": cb.get("unit"), "cores": cb.get("cores"),
                            "kind": cb.get("kind"), "sample": cb.get("sample_short") or cb.get("sample"),
                            "cpu_model": cb.get("cpu_model"), "one_core_songs_per_s": _sig(cb.get("one_core_songs_per_s"), 4)}
    oc, ds = d.get("other_configs") or {}, d.get("device_state") or {}
    fs = (rf.get("other_pcm_pass") or {}) if rf else {}
    strict = ((d.get("verification") or {}).get("n_failing_strict_1e-4_rel") or {})
    optional = [   # given up from the END of this list if the line were longer than `limit`
        ("value_fir_mode0", _sig(d.get("value_fir_mode0"), 6)),
        ("ms_per_step_fir_mode0", _sig(d.get("ms_per_step_fir_mode0"), 6)),
        ("distance_matrix_10k_s", _sig(d.get("distance_matrix_10k_s"), 4)),
        ("rehearsal", True if d.get("rehearsal") else None),
        ("details", os.path.basename(details_path) if details_path else None),
        ("collective", (d.get("collective") or {}).get("backend")),
        ("per_rank_ms", [_sig(x, 5) for x in (d.get("per_rank") or {}).get("ms_per_step", [])] if (d.get("n_gpus") or 1) > 1 else None),
        ("other_configs", None if not oc else ({"error": str(oc["error"])[:80]} if "error" in oc else {
            "configs1_ms": _sig((oc.get("configs1") or {}).get("ms_per_batch"), 4),
            "configs1_songs_per_s": _sig((oc.get("configs1") or {}).get("songs_per_s"), 4),
            "configs4_ms": _sig((oc.get("configs4_mixed") or {}).get("ms_per_batch"), 4),
            "configs4_songs_per_s": _sig((oc.get("configs4_mixed") or {}).get("songs_per_s"), 4),
            "ok": bool((oc.get("configs1") or {}).get("results_ok") and (oc.get("configs4_mixed") or {}).get("results_ok"))})),
        ("device_state", {"sclk_mhz": (ds.get("sclk_mhz") or {}).get("mean"), "power_w": (ds.get("power_w") or {}).get("mean"),
                          "power_cap_w": ds.get("power_cap_w"), "joules_per_song": _sig(ds.get("joules_per_song"), 3)}),
        ("strict_1e-4_rel_failures", sum(strict.values()) if strict else None),
        ("bit_identical_songs", (d.get("verification") or {}).get("songs_with_all_features_bit_identical")),
        ("freq_scan", None if not fs else {"ms": _sig(fs.get("ms_avg_launch"), 4), "frac_hbm": _sig(fs.get("frac"), 3)}),
        ("distance_matrix_10k_frac_hbm", _sig(d.get("distance_matrix_10k_frac_hbm"), 3)),
        ("cosine_matrix_10k_s", _sig(d.get("cosine_matrix_10k_s"), 4)),
        ("whole_path_frac_hbm", _sig(d.get("whole_path_frac_hbm"), 3)),
    ]
    optional = [(k, v) for k, v in optional if v is not None]
    while True:
        out = dict(line, **dict(optional))
        if len(json.dumps(out, separators=(",", ":"))) <= limit or not optional:
            return out
        optional.pop()


class QuietFds:
    """While a rank runs, its fd 1 and fd 2 go to a log file: RCCL prints a version banner and gloo its connection
    notes on stdout, libdrm a complaint about amdgpu.ids on stderr per process — and the driver keeps only the last
    2 000 bytes of stdout + stderr, which have to hold the JSON line.  `out` is the real stdout (the line goes there and
    nothing else does); when the run fails the log's tail and the error are replayed on the real stderr."""

    def __init__(self, tag):
        import tempfile
        sys.stdout.flush()
        sys.stderr.flush()
        self.path = os.path.join(tempfile.gettempdir(), f"bench_py_{tag}_{os.getpid()}.log")
        self.out = os.fdopen(os.dup(1), "w")
        self.err_fd = os.dup(2)
        log = os.open(self.path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        os.dup2(log, 1)
        os.dup2(log, 2)
        os.close(log)

    def replay(self, keep=6000):
        """Back to the real stderr, with what the log holds."""
        sys.stdout.flush()
        sys.stderr.flush()
        os.dup2(self.err_fd, 2)
        os.dup2(self.err_fd, 1)
        try:
            with open(self.path, errors="replace") as f:
                txt = f.read()
            if txt:
                sys.stderr.write(f"---- {self.path} (last {keep} bytes) ----\n{txt[-keep:]}\n")
        except OSError:
            pass
        sys.stderr.flush()

    def done(self):
        try:
            os.unlink(self.path)
        except OSError:
            pass


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def self_launch(args, argv):
    """`python bench.py --gpus N` without a launcher: start N ranks of this script under
    torch.distributed.run (one process per GPU, rendezvous on 127.0.0.1) and hand their stdout /
    stderr through; rank 0's JSON line is the only stdout line.  Returns the launcher's exit code."""
    if not args.plumbing_only:
        import torch
        have = torch.cuda.device_count() if torch.cuda.is_available() else 0
        if args.share_device and have >= 1:
            have = args.gpus
        if have < args.gpus:
            print(f"bench.py --gpus {args.gpus}: this box exposes {have} HIP device(s); the N-GPU run needs "
                  f"{args.gpus} (one rank per GPU).  Nothing was launched.", file=sys.stderr)
            return 2
    env = dict(os.environ)   # HSA_ENABLE_IPC_MODE_LEGACY=0 is in it (top of this file)
    env["MASTER_ADDR"] = "127.0.0.1"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)]
    cmd += [a for a in argv if a != "--launch"]
    # stdout carries the JSON line and nothing else: whatever a rank or a library prints there
    # besides it (gloo announces its connections on stdout) goes to stderr
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True, bufsize=1)
    for out in proc.stdout:
        dst = sys.stdout if out.lstrip().startswith("{") else sys.stderr
        dst.write(out)
        dst.flush()
    return proc.wait()


def plumbing_only(args):
    """No GPU: the launch / process-group / sharding / all-gather path of an N-rank run with a
    deterministic stand-in vector per global song index instead of the analysis (which exists on
    the GPU only).  gloo backend; rank 0 prints one JSON line shaped like the real one."""
    import numpy as np
    import torch
    import torch.distributed as dist
    from bliss_amd.dist import gather_force_vectors, shard_range

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if "RANK" in os.environ:
        dist.init_process_group("gloo")
    songs = args.songs_per_gpu if args.songs_per_gpu > 0 else 8
    total = songs * world
    first, count = shard_range(total, rank, world)
    assert count == songs

    def vec(i):
        return (np.random.default_rng(1000 + i).standard_normal(4) * 10).astype(np.float32)

    mine = torch.from_numpy(np.stack([vec(i) for i in range(first, first + count)]))
    gathers = 0
    t0 = time.perf_counter()
    for _ in range(args.warmup + args.steps):
        allv = gather_force_vectors(mine, [songs] * world)
        gathers += 1
    if dist.is_initialized():
        dist.barrier()
    elapsed = time.perf_counter() - t0
    ok = bool(np.array_equal(allv.numpy(), np.stack([vec(i) for i in range(total)])))
    per_rank = torch.tensor([[1e3 * elapsed / max(args.steps + args.warmup, 1)]], dtype=torch.float64)
    if dist.is_initialized():
        gathered = torch.empty((world, 1), dtype=torch.float64)
        dist.all_gather_into_tensor(gathered, per_rank)
        per_rank = gathered
    if rank == 0:
        print(json.dumps({"metric": "plumbing-only (no analysis, stand-in vectors)", "value": None,
                          "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": 1e3 * elapsed / max(args.steps + args.warmup, 1),
                          "config": {"workload": f"{songs} stand-in vectors per rank, {total} total",
                                     "parallelism": f"shard{world}"},
                          "collective": {"backend": dist.get_backend() if dist.is_initialized() else None,
                                         "all_gather_calls": gathers if dist.is_initialized() else 0,
                                         "bytes_per_rank": 16 * songs},
                          "per_rank": {"ms_per_step": [float(x) for x in per_rank[:, 0]],
                                       "ms_per_step_min": float(per_rank.min()), "ms_per_step_max": float(per_rank.max())},
                          "results_ok": ok}), flush=True)
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--songs-per-gpu", type=int, default=0,
                    help="0 = configs[2] shard (8192) if it fits in HBM, else the largest count that does")
    ap.add_argument("--seconds", type=int, default=SONG_SECONDS, help="song length (default 180)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: leave out the CPU baseline")
    ap.add_argument("--no-mode0-pass", action="store_true",
                    help="--full: skip the untimed extra pass in FIR mode 0 (profiling runs: one envelope launch per step)")
    ap.add_argument("--cpu-ladder", default="1,8,32,64,128,256",
                    help="concurrent oracle processes per rung of the CPU baseline of --full (tests shorten it)")
    ap.add_argument("--no-live-traffic", action="store_true",
                    help="--full: do not collect roofline.traffic in this run (two rocprofv3 --pmc passes over 1 024 songs, N = 1 "
                         "only, ~20 s): take the committed profile's figure")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="--full: skip the untimed-for-value legs on BASELINE configs[1] and configs[4] (profiling runs)")
    ap.add_argument("--verbose", action="store_true",
                    help="leave stdout / stderr of the rank alone (default: library chatter goes to a log file in the temp "
                         "directory, replayed on failure, so that stdout is the JSON line and stderr stays short)")
    ap.add_argument("--details-out", default="",
                    help="where the full record goes (verification per song, per-kernel times, CPU ladder, traffic by "
                         "kernel ...; default: bench_details.json next to this script); stdout carries the compact line only")
    ap.add_argument("--verify", type=int, default=32,
                    help="--full: songs of the resident batch re-analysed by the CPU oracle after the timed region")
    ap.add_argument("--emulate-world", type=int, default=0,
                    help="diagnostic: size the gather buffer and this rank's row block as for a job of W ranks "
                         "(all_vecs = W x songs vectors, rows = songs x W*songs floats; the other ranks' vectors "
                         "are copies of this rank's) — checks that the configs[2] shard still fits at W = 8")
    ap.add_argument("--share-device", action="store_true",
                    help="rehearsal of the N-rank job on ONE GPU: every rank uses device 0 and the process group is "
                         "gloo (RCCL cannot put two ranks on one device), the vectors travel through host memory; "
                         "everything else — shards, seeds, gather order, row blocks, the reductions — is the N-rank "
                         "code.  Needs a small --songs-per-gpu; not a measurement")
    ap.add_argument("--launch", action="store_true",
                    help="start the ranks through the self-launcher even for --gpus 1 (RCCL group of one)")
    ap.add_argument("--plumbing-only", action="store_true",
                    help="no GPU: launch, gloo process group, sharding and all-gather on stand-in vectors")
    ap.add_argument("--full", action="store_true",
                    help="after the timed region, also run the oracle check (--verify), the FIR mode 0 steps, "
                         "BASELINE configs[1] / configs[4], the 10 000 x 10 000 matrices, the PMC traffic passes and the "
                         "CPU baseline (the --no-* options leave parts of it out); a plain run does none of these")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write what the last timed step computed (rank 0's song records, the gathered force vectors, "
                         "a seeded sample of its distance rows) as DIR/<name>.npy, float32 / float64, under 64 MB")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")

    under_launcher = "RANK" in os.environ and "WORLD_SIZE" in os.environ
    if not under_launcher and (args.gpus > 1 or args.launch):
        raise SystemExit(self_launch(args, sys.argv[1:]))
    if args.plumbing_only:
        raise SystemExit(plumbing_only(args))
    if args.verbose:
        return run_rank(args, under_launcher, sys.stdout)
    quiet = QuietFds(f"rank{os.environ.get('RANK', '0')}")
    try:
        run_rank(args, under_launcher, quiet.out)
    except BaseException as e:
        if not (isinstance(e, SystemExit) and e.code in (0, None)):
            quiet.replay()
        raise
    quiet.done()


DUMP_SONGS_MAX = 1 << 17          # per-song records written whole up to this many songs (116 B each), else a sample
DUMP_VECS_MAX = 1 << 18           # gathered force vectors (16 B each)
DUMP_COLS_MAX = 1 << 20           # columns of one sampled distance row (4 B each)
DUMP_ROWS_BYTES = 16 << 20        # the sampled distance rows together


def _dump_sample(n, cap, seed):
    """Sorted indices of a fixed, seeded sample of `cap` out of range(n); all of them when n <= cap."""
    import numpy as np
    if n <= cap:
        return np.arange(n)
    return np.sort(np.random.default_rng(seed).choice(n, cap, replace=False))


def dump_outputs(path, res, first, all_vecs, rows):
    """--dump-outputs: what a caller of the timed step receives, as DIR/<name>.npy in float32 / float64 (under
    48 MB): every field of this rank's song records (integers as float64, exact), the gathered force vectors and the
    distance row block, each with the global song indices it holds (`*_index`); a seeded sample where the output is
    larger than the DUMP_* caps.  Same arguments, same inputs (seeds = global song index): same files."""
    import numpy as np
    import torch
    os.makedirs(path, exist_ok=True)

    def save(name, a):
        a = np.asarray(a)
        np.save(os.path.join(path, name + ".npy"), a if a.dtype in (np.float32, np.float64) else a.astype(np.float64))

    songs = _dump_sample(len(res), DUMP_SONGS_MAX, 1)
    save("song_index", first + songs)
    for k in res.dtype.names:
        save(k, res[k][songs])
    vi = _dump_sample(all_vecs.shape[0], DUMP_VECS_MAX, 2)
    save("force_vectors_index", vi)
    save("force_vectors", all_vecs[torch.from_numpy(vi).to(all_vecs.device)].cpu().numpy())
    ci = _dump_sample(rows.shape[1], DUMP_COLS_MAX, 3)
    ri = _dump_sample(rows.shape[0], max(1, DUMP_ROWS_BYTES // (4 * len(ci))), 4)
    block = rows.index_select(0, torch.from_numpy(ri).to(rows.device))
    if len(ci) < rows.shape[1]:
        block = block.index_select(1, torch.from_numpy(ci).to(rows.device))
    save("distance_rows_index", first + ri)
    save("distance_cols_index", ci)
    save("distance_rows", block.cpu().numpy())


def matrices_10k(lib, dev, stream):
    """--full: BASELINE config 4, the standalone 10 000 x 10 000 bl_distance matrix on one GPU, and its sibling
    bl_cosine_similarity matrix on the same vectors.  Returns the seconds of each (mean of 10 launches)."""
    import torch
    g = torch.Generator(device="cpu").manual_seed(4)
    v10 = (torch.randn((10000, 4), generator=g) * 8).to(dev)
    m10 = torch.empty((10000, 10000), dtype=torch.float32, device=dev)
    for _ in range(2):
        lib.bl_amd_distance_matrix_device(C.c_void_p(v10.data_ptr()), 10000, 0, 10000,
                                          C.c_void_p(m10.data_ptr()), stream)
    torch.cuda.synchronize(dev)
    reps = 10
    t1 = time.perf_counter()
    for _ in range(reps):
        lib.bl_amd_distance_matrix_device(C.c_void_p(v10.data_ptr()), 10000, 0, 10000,
                                          C.c_void_p(m10.data_ptr()), stream)
    torch.cuda.synchronize(dev)
    dm_s = (time.perf_counter() - t1) / reps
    # its sibling on the same vectors: the 10 000 x 10 000 bl_cosine_similarity matrix
    # (ref src/analyze.c:127-143; f32 dot and norms, double sqrt, product and divide)
    for _ in range(2):
        lib.bl_amd_cosine_matrix_device(C.c_void_p(v10.data_ptr()), 10000, 0, 10000,
                                        C.c_void_p(m10.data_ptr()), stream)
    torch.cuda.synchronize(dev)
    t1 = time.perf_counter()
    for _ in range(reps):
        lib.bl_amd_cosine_matrix_device(C.c_void_p(v10.data_ptr()), 10000, 0, 10000,
                                        C.c_void_p(m10.data_ptr()), stream)
    torch.cuda.synchronize(dev)
    cm_s = (time.perf_counter() - t1) / reps
    return dm_s, cm_s


def run_rank(args, under_launcher, out):
    """One rank of the job (the only one at N = 1): everything it or a library prints goes wherever fd 1 / fd 2 point;
    the JSON line goes to `out`."""

    import numpy as np
    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks: pass "
                         f"--nproc-per-node {args.gpus}, or run plain `python bench.py --gpus {args.gpus}` "
                         "(it launches its own ranks)")
    assert torch.cuda.is_available(), "bench.py needs MI355X GPUs"
    if args.share_device:
        local_rank = 0
    if local_rank >= torch.cuda.device_count():
        raise SystemExit(f"rank {rank}: LOCAL_RANK {local_rank} but this box exposes "
                         f"{torch.cuda.device_count()} HIP device(s) (one rank per GPU)")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # where the tensors of the collectives live: on the GPU for RCCL, in host memory for the gloo rehearsal
    cdev = torch.device("cpu") if args.share_device else dev
    side = None   # a gloo group beside the RCCL one: the ranks park in its barrier (a blocked socket, no spinning
                  # host thread) while rank 0 times the CPU baseline on the host cores they share
    if world > 1 or (under_launcher and "MASTER_ADDR" in os.environ):  # torchrun: RCCL group even at world size 1
        import datetime
        if args.share_device:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)
        side = dist.new_group(backend="gloo", timeout=datetime.timedelta(minutes=30))

    import bliss_amd
    from bliss_amd import _lib
    lib = bliss_amd.load()
    assert lib.bl_amd_init(local_rank) == 0

    song_samples = SAMPLE_RATE * 2 * args.seconds
    song_bytes = 2 * song_samples
    # per-song scratch: 12 B per envelope slot + histogram + small records
    scratch_per_song = 12 * (2 * (song_samples // 512)) + 4 * 4096 + 4096
    free_b, total_b = torch.cuda.mem_get_info(dev)
    want = args.songs_per_gpu if args.songs_per_gpu > 0 else 8192
    margin = 8 << 30
    fit_world = max(world, args.emulate_world)   # ranks the gather buffer and the row block are sized for
    fit = int((free_b - margin) // (song_bytes + scratch_per_song + 16 + 4 * want * fit_world))
    songs = want
    capped = False
    if songs > fit:
        songs = max(1, 1 << (max(fit, 1).bit_length() - 1))
        capped = True
    if dist.is_initialized():  # every rank uses the smallest count any rank can hold
        t = torch.tensor([songs], device=cdev)
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        songs = int(t.item())
    from bliss_amd.dist import gather_force_vectors, shard_range
    total_songs = songs * world
    my_first, my_count = shard_range(total_songs, rank, world)
    assert my_count == songs
    cols = songs * fit_world                      # columns of this rank's row block

    corpus = bliss_amd.DeviceCorpus([song_samples] * songs, 2, args.seconds, device=f"cuda:{local_rank}")
    corpus.synth(seed_base=my_first, sample_rate=SAMPLE_RATE)
    torch.cuda.synchronize(dev)

    all_vecs = torch.empty((cols, 4), dtype=torch.float32, device=dev)
    rows = torch.empty((songs, cols), dtype=torch.float32, device=dev)
    mem_after_alloc = torch.cuda.mem_get_info(dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    n_gathers = [0]

    def step():
        corpus.analyze()
        mine = corpus.force_vectors()
        gathered = gather_force_vectors(mine.to(cdev), [songs] * world).to(dev)   # RCCL all-gather, 16 B/song
        n_gathers[0] += 1
        if cols == total_songs:
            all_vecs.copy_(gathered)
        else:  # --emulate-world: the absent ranks' blocks are copies of the gathered ones
            all_vecs.view(cols // total_songs, total_songs, 4).copy_(gathered.unsqueeze(0).expand(cols // total_songs, -1, -1))
        rc = lib.bl_amd_distance_matrix_device(C.c_void_p(all_vecs.data_ptr()), cols, my_first,
                                               songs, C.c_void_p(rows.data_ptr()), stream)
        assert rc == 0

    def fence():
        torch.cuda.synchronize(dev)
        if dist.is_initialized():
            dist.barrier()
            torch.cuda.synchronize(dev)

    for _ in range(args.warmup):
        step()
    fence()
    devstate = DeviceState(DeviceState.pci_address(local_rank))
    devstate.start()
    lib.bl_amd_profile_reset()
    lib.bl_amd_profile(1)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    fence()
    elapsed = time.perf_counter() - t0
    lib.bl_amd_profile(0)
    devstate.stop_flag = True
    device_state = devstate.summary(t0, t0 + elapsed)
    my_elapsed = elapsed
    if dist.is_initialized():
        t = torch.tensor([elapsed], dtype=torch.float64, device=cdev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    # per-kernel device time of the timed region (HIP events on the launch stream)
    kern = {}
    for name in ("pcm_scan", "freq_scan", "amp_finish", "freq_frames", "freq_finish", "env_windows", "env_tail",
                 "distance"):
        n = C.c_int(0)
        ms = lib.bl_amd_profile_ms(name.encode(), C.byref(n))
        kern[name] = {"ms_total": ms, "launches": n.value,
                      "ms_avg": (ms / n.value) if n.value else None}

    # every rank's own clock and its dominant kernel, so that a scaling loss can be put on a slow rank (a gather of
    # two doubles per rank) rather than on the collective
    mine2 = torch.tensor([1e3 * my_elapsed / args.steps, kern["env_windows"]["ms_avg"] or 0.0,
                          (device_state.get("sclk_mhz") or {}).get("mean", 0.0), (device_state.get("power_w") or {}).get("mean", 0.0)],
                         dtype=torch.float64, device=cdev)
    per_rank = mine2.unsqueeze(0)
    if dist.is_initialized():
        per_rank = torch.empty((world, 4), dtype=torch.float64, device=cdev)
        dist.all_gather_into_tensor(per_rank, mine2.unsqueeze(0))
    per_rank = per_rank.cpu().numpy()

    res = corpus.fetch()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, res, my_first, all_vecs, rows)
    # --full, outside the timed region: the same steps in FIR mode 0 (the reference's operation order, window energies
    # bit-identical to the CPU oracle) — what the timed default (mode 2: fused taps, normalisation folded in; DESIGN.md
    # section 4.1) buys, measured on real steps (one warm-up, then min(K, 3) steps between fences, max over ranks), and
    # whether any integer or feature of this batch depends on the mode.
    fir_active = int(lib.bl_amd_fir_mode())
    fir_report = {"timed_mode": fir_active}
    if args.full and fir_active != 0 and not args.no_mode0_pass:
        lib.bl_amd_set_fir_mode(0)
        n0 = max(1, min(args.steps, 3))
        step()
        fence()
        lib.bl_amd_profile_reset()
        lib.bl_amd_profile(1)
        t1 = time.perf_counter()
        for _ in range(n0):
            step()
        fence()
        el0 = time.perf_counter() - t1
        lib.bl_amd_profile(0)
        if dist.is_initialized():
            t = torch.tensor([el0], dtype=torch.float64, device=cdev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el0 = float(t.item())
        c0 = C.c_int(0)
        ms0 = lib.bl_amd_profile_ms(b"env_windows", C.byref(c0))
        res0 = corpus.fetch()
        lib.bl_amd_set_fir_mode(fir_active)
        step()          # leave the resident results (and the gathered vectors the checks below read) in the timed mode
        fence()
        ints = ("start", "end", "mean", "variance", "n_frames", "nb_frames", "n_windows", "beat", "calm_or_loud", "status")
        flts = ("tempo", "amplitude", "frequency", "attack", "force")
        fir_report.update({
            "mode0_steps": n0, "mode0_ms_per_step": 1e3 * el0 / n0,
            "mode0_env_windows_ms": ms0 / max(c0.value, 1),
            "timed_mode_env_windows_ms": kern["env_windows"]["ms_avg"],
            "songs_with_an_integer_differing_from_mode0": int(sum(np.count_nonzero(res[k] != res0[k]) for k in ints)),
            "songs_with_a_feature_bit_differing_from_mode0": int(sum(np.count_nonzero(res[k].view(np.int32) != res0[k].view(np.int32))
                                                                   for k in flts)),
            "what": "mode 0 = the reference's unfused FIR: real steps over the same resident batch after the timed "
                    "region (measured, not derived); bl_amd_set_fir_mode(0) selects it"})
    ok = bool(np.all(res["status"] == 0) and np.all(np.isfinite(res["force"])))
    # the gathered vectors are the analysed ones, rank-major, and this rank's rows are distances
    ok = ok and bool(torch.equal(all_vecs[my_first:my_first + songs].cpu(),
                                 torch.from_numpy(np.stack([res[k] for k in ("tempo", "amplitude", "frequency",
                                                                             "attack")], axis=1))))
    # every rank's row block holds bl_distance of its own songs against the gathered vectors: spot-check
    # one entry per rank against the host form of the same expression (ref src/analyze.c:96-100)
    if songs > 1 and cols >= 2:
        i, j = songs - 1, (my_first + songs) % cols
        a, b = all_vecs[my_first + i].cpu().numpy(), all_vecs[j].cpu().numpy()
        want_d = lib.bl_distance(_lib.ForceVector(*[float(x) for x in a]), _lib.ForceVector(*[float(x) for x in b]))
        ok = ok and float(rows[i, j].item()) == want_d
    # --full: the oracle check is shared out, every rank re-analyses its part of the --verify songs on the host
    verified, verify_details = 0, []
    n_verify = args.verify if args.full else 0
    if n_verify > 0 and dist.is_initialized():   # one rank (re)builds the oracle, the others wait for it
        if rank == 0:
            from tests.oracle_py import build_oracle
            build_oracle()
        dist.barrier()
    if n_verify > 0:
        k = min(max(1, n_verify // world), songs)
        picks = sorted(set(int(round(j * (songs - 1) / max(k - 1, 1))) for j in range(k)))
        v_ok, verify_details = verify_songs(res, picks, my_first, args.seconds)
        ok = ok and v_ok
        verified = len(picks)
    if dist.is_initialized():  # results_ok and verified_songs describe every rank, not only rank 0
        t = torch.tensor([1 if ok else 0, verified], dtype=torch.int64, device=cdev)
        tmin, tsum = t.clone(), t.clone()
        dist.all_reduce(tmin, op=dist.ReduceOp.MIN)
        dist.all_reduce(tsum, op=dist.ReduceOp.SUM)
        ok, verified = bool(tmin[0].item()), int(tsum[1].item())

    if rank == 0:
        ms_per_step = 1e3 * elapsed / args.steps
        value = total_songs * args.steps / elapsed
        alg_bytes_song = song_bytes + 16          # 2n read + 16 written
        dom = kern["env_windows"]
        launch_bytes = alg_bytes_song * songs     # one env_windows launch covers this rank's batch
        roof = None
        fir_mode = int(lib.bl_amd_fir_mode())
        if dom["ms_avg"]:
            t_launch = dom["ms_avg"] * 1e-3
            ach = launch_bytes / t_launch / 1e9
            windows = songs * max(2 * (song_samples // 512) - 2, 0)   # ref tempo_atk_sort.c:63-67,120
            prof = _committed_profile(songs, song_samples)
            # secondary ceiling, measured: VALU wave-instructions per window from the committed SQ
            # counters of this kernel (SQ_INSTS_VALU / windows) x the windows of this launch / its
            # HIP-event time, against the f64 issue rate the chip sustains (tools/ubench_rate.hip)
            valu = None
            prof_mode = prof.get("fir_mode") if prof.get("fir_mode") is not None else 0   # r02 profiles: mode 0
            if prof.get("valu_instr_per_window") and prof_mode != fir_mode:
                valu = {"frac": None, "error": f"committed profile {prof.get('file')} was taken in FIR mode {prof_mode}, "
                                               f"this run is mode {fir_mode}: its instruction count does not apply"}
            elif prof.get("valu_instr_per_window"):
                rate = prof["valu_instr_per_window"] * windows / t_launch / 1e12
                valu = {"achieved_Twaveinstr_per_s": rate, "peak_Twaveinstr_per_s": F64_ISSUE_TWAVEINSTR_S,
                        "frac": rate / F64_ISSUE_TWAVEINSTR_S,
                        "valu_instr_per_window_profiled": prof["valu_instr_per_window"],
                        "valu_busy_frac_profiled": prof.get("valu_busy_frac"),
                        "lds_busy_frac_profiled": prof.get("lds_busy_frac"),
                        "source": "SQ_INSTS_VALU of the committed profile (not this run)"}
            floor_instr = F64_FLOOR_INSTR_PER_WINDOW[fir_mode]
            floor_s = windows * floor_instr / (F64_ISSUE_TWAVEINSTR_S * 1e12)
            roof = {"bound": "hbm", "kernel": "k_env_windows3", "achieved": ach, "peak": HBM_PEAK_GBS,
                    "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
                    "traffic": prof.get("traffic"), "traffic_error": prof.get("error"),
                    "traffic_source": {"what": "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes, gfx950 "
                                               "corrections of MI355X_MICROARCH.md; per-song figure of the "
                                               "committed profile scaled to this launch (not collected in this run)",
                                       "file": prof.get("file"), "git_head_of_profile": prof.get("git_head"),
                                       "profiled_fir_mode": prof.get("fir_mode")},
                    "frac_of_measured_copy_peak": ach / HBM_ACHIEVABLE_GBS,
                    "ms_avg_launch": dom["ms_avg"], "launches": dom["launches"],
                    "algorithmic_bytes_per_launch": launch_bytes,
                    "fir_mode": fir_mode,
                    "frac_of_f64_floor": floor_s / t_launch,
                    # the same instruction count at the specified clock (2.4 GHz, 0.6144 T wave-instr/s = 78.6 TF): the
                    # figure that does not move with the power cap's clock
                    "frac_of_f64_floor_nominal": windows * floor_instr / (F64_ISSUE_NOMINAL_TWAVEINSTR_S * 1e12) / t_launch,
                    "f64_floor": {"wave_instr_per_window": floor_instr,
                                  "issue_rate_Twaveinstr_per_s": F64_ISSUE_TWAVEINSTR_S,
                                  "issue_rate_nominal_Twaveinstr_per_s": F64_ISSUE_NOMINAL_TWAVEINSTR_S,
                                  "what": "static: the f64 operations the arithmetic of this FIR mode needs per "
                                          "window (DESIGN.md section 4.1) at the measured f64 issue rate"},
                    "secondary_f64_valu": valu,
                    "whole_step_traffic_ratio": prof.get("whole_step_traffic_ratio"),
                    # the other pass over the PCM: the frequency analysis with the statistics riding along
                    "other_pcm_pass": ({"kernel": "k_freq_scan", "ms_avg_launch": kern["freq_scan"]["ms_avg"],
                                        "achieved": launch_bytes / (1e-3 * kern["freq_scan"]["ms_avg"]) / 1e9,
                                        "unit": "GB/s", "frac": launch_bytes / (1e-3 * kern["freq_scan"]["ms_avg"]) / 1e9
                                        / HBM_PEAK_GBS, "bound": "issue (DESIGN.md section 4.4)"}
                                       if kern.get("freq_scan", {}).get("ms_avg") else None)}
            if fir_report.get("mode0_env_windows_ms"):
                roof["frac_fir_mode0"] = launch_bytes / (1e-3 * fir_report["mode0_env_windows_ms"]) / 1e9 / HBM_PEAK_GBS
                roof["frac_of_f64_floor_fir_mode0"] = (windows * F64_FLOOR_INSTR_PER_WINDOW[0] / (F64_ISSUE_TWAVEINSTR_S * 1e12)
                                                       / (1e-3 * fir_report["mode0_env_windows_ms"]))
        whole_path_gbs = value / world * alg_bytes_song / 1e9
        # the reference's operation order (FIR mode 0): real steps timed in that mode after the timed region — the
        # strict-order throughput beside `value`
        value_mode0 = ms_per_step_mode0 = None
        if fir_active == 0:
            value_mode0, ms_per_step_mode0 = value, ms_per_step
        elif fir_report.get("mode0_ms_per_step"):
            ms_per_step_mode0 = fir_report["mode0_ms_per_step"]
            value_mode0 = total_songs / (1e-3 * ms_per_step_mode0)
        # the literal north_star bar, per field: |gpu - oracle| <= 1e-4 |oracle| with no absolute term
        strict = {k: int(sum(1 for d in verify_details if not d["rel_err_by_field"][k] <= 1e-4))
                  for k in ("tempo", "amplitude", "frequency", "attack", "force")}

        # the driver's clock on the other two batch shapes of BASELINE.json (the resident batch is freed first)
        others = None
        if args.full and not args.no_other_configs:
            try:
                del corpus
                del rows, all_vecs
                torch.cuda.empty_cache()
                others = other_configs(lib, dev, songs)
            except Exception as e:   # a diagnostic leg must never sink the line
                others = {"error": f"{type(e).__name__}: {e}"}

        # roofline.traffic collected in this run (N = 1; the resident batch is gone by now, the children fit)
        if args.full and roof is not None and world == 1 and not args.no_live_traffic and not args.share_device:
            try:
                del corpus
            except NameError:
                pass
            torch.cuda.empty_cache()
            lt = live_traffic(args.seconds, songs=min(1024, songs))
            if "error" not in lt and lt.get("k_env_windows3"):
                scale = 1.0   # bytes per song of this shape already
                roof["traffic"] = lt["k_env_windows3"] * songs * scale
                roof["traffic_error"] = None
                roof["traffic_source"] = {"what": "collected in this run: rocprofv3 --pmc FETCH_SIZE and --pmc WRITE_SIZE, one pass "
                                                  "each (--kernel-trace only), around one step of this script over "
                                                  f"{min(1024, songs)} songs of the same shape in a child process; bytes per song x the "
                                                  "songs of the launch; gfx950 corrections of MI355X_MICROARCH.md",
                                          "bytes_per_song_by_kernel": {k: v for k, v in sorted(lt.items())},
                                          "committed_profile_for_comparison": prof.get("file"),
                                          "committed_profile_traffic": prof.get("traffic")}
                # the analysis kernels of a step (not the synthesis of the corpus, not the stand-alone 10 000^2 matrices)
                step_b = sum(v for k, v in lt.items() if k.startswith("k_") and k not in ("k_synth", "k_pairwise"))
                roof["whole_step_traffic_ratio"] = step_b / alg_bytes_song
            else:
                roof["traffic_source"]["live_collection_error"] = lt.get("error", "no k_env_windows3 row")

        dm_s = cm_s = None
        if args.full:
            dm_s, cm_s = matrices_10k(lib, dev, stream)
        dm_bytes = 4 * 10000 * 10000 + 16 * 10000

        line = {
            "metric": "songs/sec bl_analyze (3-min 44.1kHz s16) + 10k x 10k distance-matrix sec",
            "value": value, "unit": "songs/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": ms_per_step, "higher_is_better": True,
            "value_fir_mode0": value_mode0, "ms_per_step_fir_mode0": ms_per_step_mode0,
            "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": f"BASELINE configs[2] shape: {songs} synthetic {args.seconds}-s 44.1 kHz s16 "
                                   f"stereo songs resident per GPU ({songs * song_bytes / 1e9:.1f} GB PCM/GPU"
                                   + (", capped by free HBM" if capped else "")
                                   + f"), {total_songs} songs total, sharded by song; step = analyze + "
                                     "all-gather of force vectors + row-block distance matrix; envelope FIR mode "
                                   + f"{fir_active} (library default; mode 0 = the reference's operation order, timed beside "
                                     "it in fir_modes)",
                       "workload_short": f"configs[2] shard: {songs} synthetic {args.seconds}-s 44.1 kHz s16 stereo songs/GPU resident "
                                         f"({songs * song_bytes / 1e9:.1f} GB), {total_songs} total; step = analyze + all-gather + "
                                         "row-block distance",
                       "songs_per_gpu": songs, "song_samples": song_samples, "parallelism": f"shard{world}",
                       "generator": "integer-only device synth, seeds = global song index"},
            "distance_matrix_10k_s": dm_s,
            "distance_matrix_10k_gbs": dm_bytes / dm_s / 1e9 if dm_s else None,
            "distance_matrix_10k_frac_hbm": dm_bytes / dm_s / 1e9 / HBM_PEAK_GBS if dm_s else None,
            "cosine_matrix_10k_s": cm_s,
            "cosine_matrix_10k_frac_hbm": dm_bytes / cm_s / 1e9 / HBM_PEAK_GBS if cm_s else None,
            "whole_path_algorithmic_gbs_per_gpu": whole_path_gbs,
            "whole_path_frac_hbm": whole_path_gbs / HBM_PEAK_GBS,
            "kernels_ms": kern, "fir_modes": fir_report, "results_ok": ok, "verified_songs": verified,
            "verification": {"against": "CPU oracle (oracle/orc_cli) on the re-synthesised songs, untimed; every rank "
                                        "checks its share of --verify (results_ok / verified_songs are reduced over the "
                                        "ranks, the list below is rank 0's)",
                             "bar": "integers identical, f32 features <= 1e-4 relative (no absolute term)",
                             "n_failing_strict_1e-4_rel": strict,
                             "songs_with_all_features_bit_identical": int(sum(1 for d in verify_details
                                                                              if d.get("features_bit_identical"))),
                             "worst_rel_err_by_field": {k: max((d["rel_err_by_field"][k] for d in verify_details), default=None)
                                                        for k in ("tempo", "amplitude", "frequency", "attack", "force")},
                             "songs": verify_details},
            "memory": {"free_bytes_before_alloc": int(free_b), "total_bytes": int(total_b),
                       "free_bytes_after_alloc": int(mem_after_alloc[0]),
                       "row_block_bytes": 4 * songs * cols, "emulated_world": args.emulate_world or None},
            "rehearsal": ("ranks share device 0, gloo group, vectors staged through host memory: not a measurement"
                          if args.share_device else None),
            "collective": {"backend": dist.get_backend() if dist.is_initialized() else None,
                           "all_gather_calls": n_gathers[0] if dist.is_initialized() else 0,
                           "bytes_per_rank": 16 * songs},
            "per_rank": {"ms_per_step": [float(x) for x in per_rank[:, 0]],
                         "ms_per_step_min": float(per_rank[:, 0].min()), "ms_per_step_max": float(per_rank[:, 0].max()),
                         "env_windows_ms": [float(x) for x in per_rank[:, 1]],
                         "what": "each rank's own wall clock over the timed steps (the line's ms_per_step is the max) "
                                 "and its k_env_windows3 HIP-event average"},
            "device_state": dict(device_state, per_rank_sclk_mhz=[float(x) for x in per_rank[:, 2]],
                                 per_rank_power_w=[float(x) for x in per_rank[:, 3]],
                                 # the analysis runs against the socket power cap: what a song costs
                                 joules_per_song=(float(per_rank[:, 3].sum()) * elapsed / (total_songs * args.steps)
                                                  if float(per_rank[:, 3].min()) > 0 else None),
                                 power_capped=(bool(device_state["power_w"]["p50"] > 0.9 * device_state["power_cap_w"])
                                               if device_state.get("power_w") and device_state.get("power_cap_w") else None)),
            "other_configs": others,
            "roofline": roof,
        }
        # the CPU baseline runs on rank 0 at every N (after the timed region and every reduction; the other
        # ranks wait in a gloo barrier, which blocks on a socket instead of spinning)
        if not args.full or args.no_cpu_baseline:
            why = "--no-cpu-baseline" if args.full else "no --full"
            line["cpu_baseline"] = {"value": None, "unit": "songs/s", "cores": None, "kind": "port",
                                    "sample": f"not measured in this run ({why}): see the N = 1 line of the "
                                              "same box, BENCH_r*.json", "sample_short": f"not measured ({why})"}
        else:
            try:
                line["cpu_baseline"] = cpu_baseline(tuple(int(x) for x in args.cpu_ladder.split(",")))
                if world > 1:
                    line["cpu_baseline"]["sample"] += f"; timed on rank 0 of {world} after the timed region, the other ranks parked"
                    line["cpu_baseline"]["sample_short"] += f"; rank 0 of {world}"
            except Exception as e:  # the baseline must never sink the GPU number
                line["cpu_baseline"] = {"value": None, "unit": "songs/s", "cores": None,
                                        "kind": "port", "sample": f"failed: {e}"}
        # everything above goes to a side file; stdout gets ONE compact line (the driver keeps the last 2 000 bytes)
        details_path = args.details_out or os.path.join(ROOT, "bench_details.json")
        try:
            with open(details_path, "w") as f:
                json.dump(line, f, indent=1)
        except OSError as e:
            print(f"bench.py: could not write {details_path}: {e}", file=sys.stderr)
            details_path = None
        limit = LINE_BYTES_MAX if world == 1 else LINE_BYTES_MAX_LAUNCHED
        print(json.dumps(compact_line(line, details_path, limit), separators=(",", ":")), file=out, flush=True)
    if dist.is_initialized():
        dist.barrier(group=side)
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
