"""csrc/shm_tri_dist.h, the pair distance of shm_grid_redistance_exact, is plain C++: the scatter kernel and this host test call the same function.  No GPU.

tests/native/test_tri_dist.cpp holds it to a long double evaluation of the same formula on random triangles and to closed forms on the degenerate families (a
point triangle, a segment triangle, a needle of aspect 1e-12, a query on a vertex, on an edge, and on the plane outside the triangle); the bounds and their
reasons are at its checks.  It is built once plain and once under AddressSanitizer and UBSan, and run stand-alone."""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "test_tri_dist.cpp")


def _build(tmp_path_factory, name, flags):
    exe = str(tmp_path_factory.mktemp(name) / "test_tri_dist")
    subprocess.check_call(["g++", *flags, "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory, "tri_dist", ["-O2"])


@pytest.fixture(scope="module")
def exe_san(tmp_path_factory):
    return _build(tmp_path_factory, "tri_dist_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout[-2000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-3000:] + out.stderr[-3000:]


def test_tri_dist_on_host(exe):
    _run(exe)


def test_tri_dist_under_sanitizers(exe_san):
    """The same program under AddressSanitizer and UBSan, stand-alone: no address outside an array, no undefined arithmetic (no division by a zero ee or nn)."""
    _run(exe_san)
