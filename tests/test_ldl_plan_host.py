"""The plan of the block factorisation S = L D L^T that the direct dual solve uses in place of S^-1 (csrc/shm_ldl_plan.h: superblocks, the tiles each elimination launch
touches, the chain that inverts the diagonal superblocks, the mat-vecs of the solve, the tile-product counts) is plain C++: the kernels' launches and this host test
call the same functions.  No GPU."""
import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "test_ldl_plan.cpp")


def _run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra"] + flags + [SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout + out.stderr
    return out.stdout


def test_ldl_plan_on_host(tmp_path):
    """nb = 1 ... 63 pivot blocks (tests/native/test_ldl_plan.cpp): the superblocks partition the blocks; every trailing tile is updated exactly once per elimination
    step and no other tile is touched; every panel tile is written once; the solve reads each stored tile of L once per sweep and writes each segment once; the counted
    tile products equal the closed forms (at nb = 45: 17 875 against 50 535, 0.354); and with 1 x 1 tiles the walk solves a random SPD system."""
    out = _run(tmp_path, "test_ldl_plan", ["-O2"])
    assert "nb 45: tile products 17875" in out and "against 50535" in out, out


def test_ldl_step_kernel_fits_beside_step1():
    """The elimination kernel of the factorisation runs beside two Step-1 waves per SIMD as the Gauss-Jordan kernel does: from the compiler's report of the library
    build, at most 144 registers (accumulation registers included), none spilled, and no more LDS than gj_step_kernel (kGjStepLds doubles).  Measured: 142, 0, 37 440 bytes."""
    import re
    import subprocess
    import pytest
    path = os.path.join(ROOT, "signed-heat-3d_amd", "lib", "kernel_resources.txt")
    if not os.path.exists(path):
        pytest.skip("library was built without the resource report")
    res, cur = {}, None
    for line in open(path):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            res.setdefault(cur, {})
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur:
            res[cur][m.group(1)] = int(m.group(2))
    names = [n for n in res if "gj_ldl_step_kernel" in n or n.endswith("gj_step_kernelEPdiiiPKdS2_S0_S0_Pii")]
    dem = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.splitlines()
    by_name = {re.sub(r"\(.*", "", d): res[n] for n, d in zip(names, dem)}
    ldl, gj = by_name["shm::gj_ldl_step_kernel"], by_name["shm::gj_step_kernel"]
    assert ldl["VGPRs"] + ldl.get("AGPRs", 0) <= 144 and ldl.get("VGPRs Spill", 0) == 0 and ldl.get("ScratchSize", 0) == 0, ldl
    assert ldl["LDS Size"] <= gj["LDS Size"], (ldl, gj)


def test_ldl_plan_on_host_sanitized(tmp_path):
    """The same stand-alone program under the address and undefined-behaviour sanitizers: the walk indexes tiles, panels and vector segments by the plan's numbers."""
    _run(tmp_path, "test_ldl_plan_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
