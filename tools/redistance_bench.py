"""Time of shm_grid_redistance on a solved grid, with band = inf and band = 8 cells.

For each case (bunny_small 256^3 and 512^3 in fp64, rocker 512^3 in fp32) and each band: one warm-up, then --reps repetitions; ms is the call's own device
time (shm_redistance_stats.ms: events around initialisation, rounds and finalisation, host polls included), median, minimum and maximum.  Beside it the
rounds, the block updates per 8^3 block, and the bytes the call moves by the kernels' own access counts --
    initialisation   N reads of phi (the halo reads hit in cache) + N writes of u
    a block update   (8^3 + 6 * 8^2) reads + at most 8^3 writes
    finalisation     N reads of phi + N reads of u + N writes of psi
-- against the floor of one read of phi and one write of psi at the copy rate measured here on a buffer of phi's size.  A stated ratio of bytes and of
times, not a share of any peak.  The numpy restatement (tests/redistance_ref.py) on the 64^3 golden is timed once on the host, for scale.
One JSON line per case and band.  Not part of bench.py.

    python tools/redistance_bench.py [--reps 5] [--cases bunny_small:256:64,bunny_small:512:64,rocker:512:32] [--iso 0] [--band-cells 8]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import shm_import  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="bunny_small:256:64,bunny_small:512:64,rocker:512:32")
    ap.add_argument("--iso", type=float, default=0.0)
    ap.add_argument("--band-cells", type=float, default=8.0)
    a = ap.parse_args()
    import torch
    shm = shm_import.load()
    from signed_heat_3d_amd.host_abi import HostSolver
    for case in a.cases.split(","):
        mesh, n_want, prec = case.split(":")
        n_want, prec = int(n_want), int(prec)
        pre = HostSolver(os.path.join(ROOT, "data", mesh + ".obj")).preprocess(hCoef=float(np.log2(n_want / 2) - 3))
        n, h = pre["n"], pre["cell"]
        assert n == n_want
        s = shm.GridSolver(precision=shm.SHM_F64 if prec == 64 else shm.SHM_F32)
        s.set_problem(pre["pos"], pre["wnormal"], pre["area"], pre["lam"], n, pre["bbox_min"], h)
        s.solve()
        esz = 8 if prec == 64 else 4
        N = n ** 3
        nbytes = N * esz
        src = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
        dst = torch.empty_like(src)
        cp = []
        for r in range(a.reps + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dst.copy_(src)
            torch.cuda.synchronize()
            if r >= 2:
                cp.append((time.perf_counter() - t0) * 1e3)
        copy_ms = float(np.median(cp))   # one read and one write of a buffer of phi's size: the floor
        del src, dst
        for band in (float("inf"), a.band_cells * h):
            s.redistance(a.iso, band)   # warm-up: allocations, code objects
            ms, wall = [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                st = s.redistance(a.iso, band)
                wall.append((time.perf_counter() - t0) * 1e3)
                ms.append(st["ms"])
            nblocks = ((n + 7) // 8) ** 3
            moved = esz * (2 * N + st["n_block_updates"] * (2 * 512 + 6 * 64) + 3 * N)
            med = float(np.median(ms))
            res = dict(mesh=mesh, n=n, precision=prec, iso=a.iso, band_cells=None if band == float("inf") else a.band_cells, reps=a.reps,
                       median_ms=round(med, 3), min_ms=round(float(np.min(ms)), 3), max_ms=round(float(np.max(ms)), 3), wall_median_ms=round(float(np.median(wall)), 3),
                       n_rounds=st["n_rounds"], rounds_cap=24 * ((n + 7) // 8) + 16, n_block_updates=st["n_block_updates"],
                       updates_per_block=round(st["n_block_updates"] / nblocks, 2), n_frozen=st["n_frozen"], n_reached=st["n_reached"], max_abs=st["max_abs"],
                       bytes_moved=moved, floor_bytes=2 * nbytes, bytes_over_floor=round(moved / (2 * nbytes), 2),
                       copy_rate_GBps=round(2 * nbytes / (copy_ms * 1e-3) / 1e9, 1), floor_ms=round(copy_ms, 4), ms_over_floor=round(med / copy_ms, 1),
                       moved_GBps=round(moved / (med * 1e-3) / 1e9, 1))
            print(json.dumps(res), flush=True)
        s.close()
    import redistance_ref as ref
    d = np.load(os.path.join(ROOT, "tests", "golden", "bunny_small_n64.npz"))
    t0 = time.perf_counter()
    _, info = ref.redistance(d["phi"], int(d["n"]), float(d["cell"]), a.iso)
    print(json.dumps(dict(restatement="numpy Jacobi, host", mesh="bunny_small", n=int(d["n"]), iso=a.iso, seconds=round(time.perf_counter() - t0, 2),
                          iterations=info["iterations"])), flush=True)


if __name__ == "__main__":
    main()
