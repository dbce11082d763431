"""Runs the wave planner of the host-fed entry points (bliss_amd/csrc/bl_waves.h: songs in order, each at a multiple of 8
samples, as many as fit a budget but at least one) on the CPU: on 4 000 seeded length lists every song is in exactly one
wave, the waves are in order and contiguous, offsets are multiples of 8 and songs do not overlap, only a single-song wave
exceeds the budget and every wave is maximal; and the thirteen songs tests/test_gpu_runtime.py feeds the host batch split
as worked out by hand from the rule (tests/host/test_waves_host.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wave_planner_host(tmp_path):
    exe = str(tmp_path / "test_waves_host.bin")
    cc = subprocess.run(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "host", "test_waves_host.cpp"), "-o", exe],
                        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert cc.returncode == 0, "g++ failed:\n" + cc.stdout
    out = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout
    assert out.stdout.strip().endswith("OK"), out.stdout
    assert "rate 22050 budget 150000: 6 waves [3,2,2,2,2,2]" in out.stdout
    assert "rate 44100 budget 150000: 9 waves [2,1,1,1,2,1,2,1,2]" in out.stdout
    assert "rate 44100 budget 75000: 13 waves [1,1,1,1,1,1,1,1,1,1,1,1,1]" in out.stdout
