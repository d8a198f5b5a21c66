"""The pass plan of the Step-1 kernel (csrc/shm_tier_passes.h: which far threshold, which test price and which set of sources each pass over a block's sources uses, and
when the pass loop ends) is plain C++: the kernel and this host test call the same functions.  No GPU."""
import os
import subprocess

from conftest import ROOT


def test_tier_pass_plan_on_host(tmp_path):
    """Every sequence of test outcomes, walked as the kernel's pass loop walks it (tests/native/test_tier_passes.cpp): ring = 0 gives the two passes of before; ring > 0
    puts one tiered pass at G + ring between them and reaches the all-fp64 pass only after two failures; never a far list in the all-fp64 pass; EXACT / fp32 handles
    make a single pass."""
    exe = str(tmp_path / "test_tier_passes")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", os.path.join(ROOT, "tests", "native", "test_tier_passes.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout


def test_hot_loops_sit_where_they_were_measured():
    """Where the heads of the fp64 solve's two hot loops fall in the 64-byte instruction lines moves Step 1 by up to 1 % with the instruction streams unchanged
    (profiles/NOTES_r09.md section E: measured at byte 8 / 4, 12 / 16 and 28 / 24).  The kernel pads them to byte 8 / 4 with no-ops at its start; code added in front of
    the loops, or another compiler, moves them silently -- this holds them there (tools/step1_isa_check.py assembles the kernel for the addresses; no GPU)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("step1_isa_check", os.path.join(ROOT, "tools", "step1_isa_check.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    r = mod.loops()
    assert r["fp64 solve near loop"].get("head_byte") == 8 and r["fp64 solve far loop"].get("head_byte") == 4, r
