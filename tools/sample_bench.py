"""Throughput of the point queries (shm_grid_sample_device / shm_grid_sample) on bunny_small.obj.

For each grid (256^3 fp64, 512^3 fp64, 512^3 fp32), point set (uniform in the box; near the surface: source positions plus a jitter of one cell) and
with / without the gradient: points per second of the device entry point (torch events around the call, after a warm-up), the time of the host entry
point for the same Q, and the fraction of the compulsory-traffic bound, (bytes of points in + outputs out) / 8 TB/s.  Then one host sample of 10^6
points against one get_phi of the same grid.  One JSON line per case.  Not part of bench.py.

    python tools/sample_bench.py [--q-log2 24] [--reps 5] [--cases 256:64,512:64,512:32]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import shm_import  # noqa: E402

HBM_BPS = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--q-log2", type=int, default=24)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="256:64,512:64,512:32")
    ap.add_argument("--host", type=int, default=1, help="also time the host entry point (0: device entry point only, e.g. under a profiler)")
    a = ap.parse_args()
    import torch
    shm = shm_import.load()
    from signed_heat_3d_amd.host_abi import HostSolver
    Q = 1 << a.q_log2
    for case in a.cases.split(","):
        n_want, prec = (int(x) for x in case.split(":"))
        pre = HostSolver(os.path.join(ROOT, "data", "bunny_small.obj")).preprocess(hCoef=float(np.log2(n_want / 2) - 3))
        n, b, h = pre["n"], pre["bbox_min"], pre["cell"]
        assert n == n_want
        s = shm.GridSolver(precision=prec)
        s.set_problem(pre["pos"], pre["wnormal"], pre["area"], pre["lam"], n, b, h)
        s.solve()
        dt_np = np.float64 if prec == 64 else np.float32
        rng = np.random.default_rng(0)
        sets = {"uniform": rng.uniform(b, (n - 1) * h + b, (Q, 3)),
                "near_surface": pre["pos"][rng.integers(0, len(pre["pos"]), Q)] + rng.uniform(-h, h, (Q, 3))}
        for name, pts in sets.items():
            t = torch.from_numpy(pts.astype(dt_np)).to("cuda:0")
            for grad in (False, True):
                for _ in range(2):
                    s.sample_device(t, grad=grad)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ms = []
                for _ in range(a.reps):
                    e0.record()
                    s.sample_device(t, grad=grad)
                    e1.record()
                    e1.synchronize()
                    ms.append(e0.elapsed_time(e1))
                dev_ms = float(np.median(ms))
                host_ms = None
                if a.host:
                    p64 = pts.astype(dt_np).astype(np.float64)
                    s.sample(p64[:1024], grad=grad)
                    t0 = time.perf_counter()
                    s.sample(p64, grad=grad)
                    host_ms = (time.perf_counter() - t0) * 1e3
                sz = np.dtype(dt_np).itemsize
                nbytes = Q * sz * (3 + (4 if grad else 1))
                print(json.dumps(dict(n=n, precision=prec, points=name, grad=grad, Q=Q, device_ms=round(dev_ms, 4),
                                      points_per_s=Q / (dev_ms * 1e-3), bound_fraction=round(nbytes / HBM_BPS / (dev_ms * 1e-3), 4),
                                      host_ms=None if host_ms is None else round(host_ms, 2))), flush=True)
            del t
        if a.host:
            p = sets["near_surface"][:1000000]
            s.sample(p[:1024], grad=True)
            t0 = time.perf_counter()
            s.sample(p, grad=True)
            t1 = time.perf_counter()
            s.get_phi()
            t2 = time.perf_counter()
            print(json.dumps(dict(n=n, precision=prec, host_sample_1e6_grad_ms=round((t1 - t0) * 1e3, 2), get_phi_ms=round((t2 - t1) * 1e3, 2))), flush=True)
        s.close()


if __name__ == "__main__":
    main()
