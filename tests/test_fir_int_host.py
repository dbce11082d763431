"""Runs FIR mode 2's exact integer convolution (bliss_amd/csrc/bl_fir_int.h: limb split, the five weighted sums, the
constant split, the combine and the f64 form of the run-in block and the heads) on the CPU against an int64 convolution,
and the window energies it gives — with bl_fft_tan.h's lane code behind it, scaled as the kernel did and unscaled as the
shipped kernel does — against the oracle's: on the songs of tests/test_gpu_fir_int.py, and on the songs
tests/window_reference.py builds for tests/test_gpu_windows.py (tests/host/test_fir_int_host.cpp)."""
import os
import re
import subprocess

from tests import window_reference as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_program(tmp_path):
    exe = str(tmp_path / "test_fir_int_host.bin")
    orc = [os.path.join(ROOT, "oracle", f) for f in ("bliss_oracle.c", "orc_fft.c", "orc_fft_alt.c", "orc_fft_lavc.c", "orc_synth.c")]
    cc = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "host", "test_fir_int_host.cpp"),
                         "-x", "c"] + orc + ["-o", exe, "-lm"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert cc.returncode == 0, "g++ failed:\n" + cc.stdout
    return exe


_LINE = re.compile(r"^\(e\) (\S+)\s+\d channel\(s\),\s*(\d+) windows: shipped route (\d+) differ, largest step (\d+) ulp; "
                   r"scaled route (\d+) differ, largest step (\d+) ulp$", re.M)


def run_files(exe, tmp_path, songs, jobs=4):
    """the program on `songs` (name -> (pcm, channels)) as raw s16 files, `jobs` processes side by side; returns
    name -> (windows, shipped differ, shipped step, scaled differ, scaled step) and prints what the program printed"""
    args = [[] for _ in range(jobs)]
    for i, (name, (pcm, ch)) in enumerate(songs.items()):
        path = str(tmp_path / name)
        pcm.tofile(path)
        args[i % jobs] += [str(ch), path]
    procs = [subprocess.Popen([exe] + a, stdout=subprocess.PIPE, text=True) for a in args if a]
    out = {}
    for p in procs:
        text = p.communicate()[0]
        print(text)
        assert p.returncode == 0, text
        for m in _LINE.finditer(text):
            out[m.group(1)] = tuple(int(v) for v in m.groups()[1:])
    assert set(out) == set(songs), sorted(set(songs) - set(out))
    return out


def test_integer_fir_host(tmp_path):
    exe = build_program(tmp_path)
    out = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout
    assert out.stdout.strip().endswith("OK"), out.stdout
    # the shipped route on the same songs: the allowance of (d)
    m = re.search(r"^\(e\) (\d+) windows, shipped route: (\d+) energies moved against the oracle, (\d+) by more than one ulp$",
                  out.stdout, re.M)
    assert m and int(m.group(1)) == 5344 and int(m.group(2)) <= 2 and int(m.group(3)) == 0, out.stdout


def test_the_emulation_meets_the_allowance_on_the_window_songs(tmp_path, oracle):
    """The sweep, the designed songs and the mean classes of tests/window_reference.py through the CPU emulation of mode
    2, scaled and shipped route: no energy more than one f32 ulp from the oracle's, at most 2 differ over the whole
    set — the project's allowance for modes 1 and 2, met by the arithmetic alone before tests/test_gpu_windows.py
    relies on it."""
    songs = {f"sweep{i}": s for i, s in enumerate(wr.sweep(oracle))}
    songs.update(wr.designed())
    got = run_files(build_program(tmp_path), tmp_path, songs, jobs=8)
    for name, (pcm, _) in songs.items():
        assert got[name][0] == wr.n_windows_of(len(pcm)), name
    for route, (d, s) in (("shipped", (1, 2)), ("scaled", (3, 4))):
        differ = {n: v[d] for n, v in got.items() if v[d]}
        print(f"{route} route: {sum(differ.values())} energies differ from the oracle's over {sum(v[0] for v in got.values())} "
              f"windows {differ}, largest step {max(v[s] for v in got.values())} ulp")
        assert max(v[s] for v in got.values()) <= 1, (route, {n: v[s] for n, v in got.items() if v[s] > 1})
        assert sum(differ.values()) <= 2, (route, differ)
