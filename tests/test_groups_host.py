"""Runs the launch-group planner of the tempo and the beats call (bliss_amd/csrc/bl_groups.h: longest first, as many songs
as fit group_songs songs and group_hops hops but at least one) on the CPU: on 4 000 seeded lists with limits small
enough that every branch is taken many times the records are a permutation of the input, hops never increase, equal hops
keep the caller's order, hop_off is 0 exactly at group starts and the sum of the group's earlier hops elsewhere, no group
has more than group_songs songs, only a single-song group exceeds group_hops, every group is maximal and the group_end
walk returns the same boundaries and sums; and hops [5, 9, 3, 9, 1, 4] with budget 16 split as worked out by hand from
the rule (tests/host/test_groups_host.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_group_planner_host(tmp_path):
    exe = str(tmp_path / "test_groups_host.bin")
    cc = subprocess.run(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "host", "test_groups_host.cpp"), "-o", exe],
                        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert cc.returncode == 0, "g++ failed:\n" + cc.stdout
    out = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout
    assert out.stdout.strip().endswith("OK"), out.stdout
    assert "group_songs 3 budget 16: 3 groups [1,2,3] order [1,3,0,5,2,4]" in out.stdout
    assert "group_songs 2 budget 16: 4 groups [1,2,2,1] order [1,3,0,5,2,4]" in out.stdout
