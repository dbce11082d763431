"""Runs FIR mode 2's exact integer convolution (bliss_amd/csrc/bl_fir_int.h: limb split, the five weighted sums, the
constant split, the combine and the f64 form of the run-in block and the heads) on the CPU against an int64 convolution,
and the window energies it gives — with bl_fft_tan.h's lane code behind it — against the oracle's on the songs of
tests/test_gpu_fir_int.py (tests/host/test_fir_int_host.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_integer_fir_host(tmp_path):
    exe = str(tmp_path / "test_fir_int_host.bin")
    orc = [os.path.join(ROOT, "oracle", f) for f in ("bliss_oracle.c", "orc_fft.c", "orc_fft_alt.c", "orc_fft_lavc.c", "orc_synth.c")]
    cc = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "host", "test_fir_int_host.cpp"),
                         "-x", "c"] + orc + ["-o", exe, "-lm"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert cc.returncode == 0, "g++ failed:\n" + cc.stdout
    out = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout
    assert out.stdout.strip().endswith("OK"), out.stdout
