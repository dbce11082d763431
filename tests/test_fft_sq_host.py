"""Runs FIR mode 2's unscaled transform (bliss_amd/csrc/bl_fft_tan.h: bl_fft512_power1_sq and its constants; bl_fir_int.h:
bl_firi_power_scale) on the CPU: every power term against a long-double DFT no worse than the scaled tan path within the
stated margins, every f32 ordered sum equal to the long-double one, the pair function's sign and factor, and kappa at
the ends of its range (tests/host/test_fft_sq_host.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_unscaled_lane_code(tmp_path):
    exe = str(tmp_path / "test_fft_sq_host.bin")
    cc = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "host", "test_fft_sq_host.cpp"),
                         "-o", exe, "-lm"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert cc.returncode == 0, "g++ failed:\n" + cc.stdout
    out = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout
    assert out.stdout.strip().endswith("OK"), out.stdout
