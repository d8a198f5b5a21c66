"""The host assembly of the constraint set-up (csrc/shm_constraints.h: rows, shift items, node index, G = A A^T, B = A K A^T, slab lists, the two-level
partition, the Schur row order, the active tiles) is plain C++: Solver::build_constraints and this host test call the same functions.  No GPU.

tests/native/test_constraints.cpp reads a problem from a raw file, writes the rows back and checks everything else itself against brute force (the bounds and
their derivations are at its checks: G to 1e-14 relative -- at most 8 non-negative products per entry; B to 1e-11 / cell^2 -- at most 56 terms of magnitude
<= 6 / cell^2)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden

SRC = os.path.join(ROOT, "tests", "native", "test_constraints.cpp")
CASES = ["bunny_small_n16", "bunny_small_n32", "bunny_pc_n32", "polygon_bear_n16", "synthetic"]


def _synthetic():
    """A slab of 14 x 14 x 5 cells of a 32^3 grid with one source in every cell and a second one in every seventh: boxes of 4 and of 8 both get several
    full boxes, separator planes in x and y, and (box 4) in z."""
    rng = np.random.default_rng(7)
    n, cell, bbox_min = 32, 0.37, np.array([-1.5, 0.25, 2.0])
    k, j, i = np.meshgrid(np.arange(2, 7), np.arange(1, 15), np.arange(1, 15), indexing="ij")
    cells = np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1)
    cells = np.concatenate([cells[rng.permutation(len(cells))], cells[::7]])
    pos = bbox_min + cell * (cells + rng.uniform(0.05, 0.95, cells.shape))
    return dict(n=n, cell=cell, bbox_min=bbox_min, pos=pos, area=rng.uniform(0.5, 2.0, len(pos)), m=14 * 14 * 5)


def _problem(case):
    return _synthetic() if case == "synthetic" else load_golden(case)


def _build(tmp_path_factory, name, flags):
    exe = str(tmp_path_factory.mktemp(name) / "test_constraints")
    subprocess.check_call(["g++", *flags, "-std=c++17", "-Wall", "-Wextra", SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory, "constraints", ["-O2"])


@pytest.fixture(scope="module")
def exe_san(tmp_path_factory):
    return _build(tmp_path_factory, "constraints_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


def _run(exe, case, tmp_path):
    d = _problem(case)
    pos = np.ascontiguousarray(d["pos"], dtype=np.float64)
    head = np.concatenate([[float(d["n"]), float(len(pos)), float(d["cell"])], np.asarray(d["bbox_min"], dtype=np.float64)])
    np.concatenate([head, pos.ravel(), np.asarray(d["area"], dtype=np.float64)]).tofile(tmp_path / "in.f64")
    must_fit = case in ("bunny_small_n32", "synthetic")   # the two-level partition has to exist for these (box requests 4 and 8)
    out = subprocess.run([exe, str(tmp_path / "in.f64"), str(tmp_path / "out"), str(int(must_fit))], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-3000:] + out.stderr[-3000:]
    nodes = np.fromfile(tmp_path / "out.nodes.i64", dtype=np.int64).reshape(-1, 8)
    coeffs = np.fromfile(tmp_path / "out.coeffs.f64", dtype=np.float64).reshape(-1, 8)
    assert nodes.shape[0] == int(d["m"])
    return d, nodes, coeffs


@pytest.mark.parametrize("case", CASES)
def test_constraint_assembly_on_host(exe, case, tmp_path):
    """Rows bit for bit against the fixture (the claim of test_gpu_parity.py::test_constraint_rows_bit_exact, without a GPU); the program's own checks of the
    shift items, G, B, the slab lists, the two-level partition, the Schur row order and the active tiles pass."""
    d, nodes, coeffs = _run(exe, case, tmp_path)
    if case != "synthetic":
        assert np.array_equal(nodes, d["c_nodes"])          # index work: bit exact
        assert np.array_equal(coeffs, d["c_coeffs"])        # same expression order -> bit exact


@pytest.mark.parametrize("case", ["bunny_small_n32", "synthetic"])
def test_constraint_assembly_under_sanitizers(exe_san, case, tmp_path):
    """The same program under AddressSanitizer and UBSan, stand-alone: no address outside an allocation is formed, no undefined arithmetic."""
    _run(exe_san, case, tmp_path)
