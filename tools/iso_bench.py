"""Time of the isosurface paths on a solved grid: (a) the host-welded path, shm_grid_isosurface + shm_grid_get_isosurface; (b) the device-built indexed mesh
and its host getter; (c) the same build and its device getter (torch tensors).

For each case (bunny_small 256^3 and 512^3 in fp64, rocker 512^3 in fp32): one warm-up of every path, then --reps alternating repetitions a, b, c, a, b, c ...
in one process, each timed with a host clock around calls that return synchronised; median, minimum and maximum per path.  The build alone (no getter) is
timed the same way and set against the time of reading phi once, N * sizeof(T) bytes at the copy rate measured here (a device-to-device copy of a buffer of
phi's size moves twice its bytes): a stated number of phi reads, not a share of any peak.  (a) and (b) are compared at the timed size the way
tests/test_iso_indexed.py compares them: triangle by triangle, in order, as position triples.  One JSON line per case.  Not part of bench.py.

    python tools/iso_bench.py [--reps 5] [--cases bunny_small:256:64,bunny_small:512:64,rocker:512:32] [--paths abc] [--iso 0]

--paths c runs the device path alone (for a kernel trace: rocprofv3 --kernel-trace --stats -- python tools/iso_bench.py --paths c ...).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import shm_import  # noqa: E402


def stats(ms):
    return dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(float(np.min(ms)), 3), max_ms=round(float(np.max(ms)), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="bunny_small:256:64,bunny_small:512:64,rocker:512:32")
    ap.add_argument("--paths", default="abc")
    ap.add_argument("--iso", type=float, default=0.0)
    a = ap.parse_args()
    import torch
    shm = shm_import.load()
    from signed_heat_3d_amd.host_abi import HostSolver
    for case in a.cases.split(","):
        mesh, n_want, prec = case.split(":")
        n_want, prec = int(n_want), int(prec)
        pre = HostSolver(os.path.join(ROOT, "data", mesh + ".obj")).preprocess(hCoef=float(np.log2(n_want / 2) - 3))
        n, b, h = pre["n"], pre["bbox_min"], pre["cell"]
        assert n == n_want
        s = shm.GridSolver(precision=shm.SHM_F64 if prec == 64 else shm.SHM_F32)
        s.set_problem(pre["pos"], pre["wnormal"], pre["area"], pre["lam"], n, b, h)
        s.solve()
        nv, nt = C.c_int64(), C.c_int64()

        def build():
            s._chk(s._lib.shm_grid_isosurface_indexed(s._h, a.iso, C.byref(nv), C.byref(nt)))
        paths = {"a": lambda: s.isosurface(a.iso), "b": lambda: s.isosurface_indexed(a.iso), "c": lambda: s.isosurface_indexed(a.iso, device=True),
                 "build": build}
        order = [p for p in "abc" if p in a.paths] + ["build"]
        out = {}
        for p in order:
            out[p] = paths[p]()   # warm-up: first-use allocations, code objects
        ms = {p: [] for p in order}
        for _ in range(a.reps):
            for p in order:
                t0 = time.perf_counter()
                paths[p]()
                ms[p].append((time.perf_counter() - t0) * 1e3)
        res = dict(mesh=mesh, n=n, precision=prec, iso=a.iso, reps=a.reps, vertices=nv.value, triangles=nt.value)
        for p in order:
            res[p] = stats(ms[p])
        # the copy rate of this device on a buffer of phi's size
        nbytes = n ** 3 * (8 if prec == 64 else 4)
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
        copy_ms = float(np.median(cp))
        res["phi_bytes"] = nbytes
        res["copy_rate_GBps"] = round(2 * nbytes / (copy_ms * 1e-3) / 1e9, 1)
        res["phi_read_ms"] = round(copy_ms / 2, 4)
        res["build_in_phi_reads"] = round(res["build"]["median_ms"] / (copy_ms / 2), 2)
        del src, dst
        if "a" in out and "b" in out:
            (Vo, Fo), (V, F) = out["a"], out["b"]
            assert V.shape == Vo.shape and F.shape == Fo.shape, (V.shape, Vo.shape, F.shape, Fo.shape)
            B = float(np.abs(b).max()) + (n - 1) * h
            err = float(np.abs(V[F] - Vo[Fo]).max()) if len(F) else 0.
            assert err <= 8 * 2.0 ** -53 * B, (err, B)
            res["old_vs_new_max_abs"] = err
            res["speedup_b_over_a"] = round(res["a"]["median_ms"] / res["b"]["median_ms"], 2)
            if "c" in out:
                res["speedup_c_over_a"] = round(res["a"]["median_ms"] / res["c"]["median_ms"], 2)
        print(json.dumps(res), flush=True)
        s.close()


if __name__ == "__main__":
    main()
