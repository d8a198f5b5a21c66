"""The bookkeeping of the far list's carry in the Step-1 kernel (csrc/shm_far_carry.h: how many list entries the far loop runs per cluster, what stays for the next
cluster, where the list is drained) is plain C++: the kernel and this host test call the same function.  No GPU."""
import os
import subprocess

from conftest import ROOT


def test_far_carry_bookkeeping_on_host(tmp_path):
    """Random sequences of per-cluster far counts (0 ... 64) and flush thresholds, walked as the kernel walks them: every source exactly once and in order, a drain
    before every flush and at the end, flushes after the same sources as with per-cluster padding, the carry never above three, no list entry read unwritten
    (tests/native/test_far_carry.cpp)."""
    exe = str(tmp_path / "test_far_carry")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", os.path.join(ROOT, "tests", "native", "test_far_carry.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout
