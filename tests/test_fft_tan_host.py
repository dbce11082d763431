"""Runs the tan-form lane code of k_env_windows3's DFT (bliss_amd/csrc/bl_fft_tan.h) on the CPU: accuracy against a
long-double FFT no worse than bl_fft.h's, and every window energy equal to the oracle's (tests/host/test_fft_tan_host.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tan_form_lane_code(tmp_path):
    exe = str(tmp_path / "test_fft_tan_host.bin")
    orc = [os.path.join(ROOT, "oracle", f) for f in ("bliss_oracle.c", "orc_fft.c", "orc_fft_alt.c", "orc_fft_lavc.c", "orc_synth.c")]
    cc = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "host", "test_fft_tan_host.cpp"),
                         "-x", "c"] + orc + ["-o", exe, "-lm"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert cc.returncode == 0, "g++ failed:\n" + cc.stdout
    out = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    assert out.returncode == 0, out.stdout
    assert out.stdout.strip().endswith("OK"), out.stdout
