"""The slot layout and the chunk plan of the host query entries' staging pipeline (csrc/shm_query_stage.h) are plain C++: Solver::query_stream and this host
test call the same functions.  No GPU."""
import os
import subprocess

from conftest import ROOT


def test_query_stage_layout_and_chunks_on_host(tmp_path):
    """tests/native/test_query_stage.cpp: for the column sets of sample, raycast, closest_point and mesh_raycast, every combination of optional outputs and
    C in {1, 63, 64, 65, 2^20}, the columns lie inside the slot without overlap at multiples of 8 bytes, absent columns have no address and the slot at 2^20 is
    at most 7, 10, 10, 11 doubles per query; for Q around one and two chunks of 2^20 the chunks tile [0, Q) once, in order, only the last short, none for Q = 0."""
    exe = str(tmp_path / "test_query_stage")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "native", "test_query_stage.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout
