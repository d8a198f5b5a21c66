"""Cost of Taubin smoothing of the resident indexed mesh on the device (shm_grid_smooth_mesh_device) beside the two ways of doing it without the stage:
a torch index_add_ float umbrella on the same device (not reproducible: the adds arrive in any order) and fetching the mesh to smooth it in numpy.
bunny_small at 256^3 and 512^3, an SHM_F64 handle, isovalues 0 and 0.25 max phi, warm, one process.

Per mesh, `reps` rounds; every device call is synchronous, so the host clock around it is what a caller waits:
    build_ms     smooth_mesh_device with iterations = 0 and no normals: load, index check, frame, the vertex -> incidence lists, store -- everything but passes
    taubin10_ms  10 Taubin iterations (20 passes) with normals
    taubin20_ms  20 Taubin iterations (40 passes) with normals
    pass_ms      (taubin20_ms - taubin10_ms) / 20: one pass
    pass_MB      the bytes of one pass if every array were read once: positions read and written (48 nv), list offsets (8 nv), lists (8 per incidence);
                 the neighbours' positions are a gather that the caches serve and are not counted
    pass_share   pass_MB / pass_ms over copy_GBs, the rate a device-to-device copy of 256 MiB reaches in the same process
    torch10_ms   10 Taubin iterations of the float umbrella with index_add_ on the device (positions only)
    numpy10_ms   get_isosurface_indexed to the host and 10 Taubin iterations of the float umbrella there with np.add.at
One JSON line per row; --out writes the table to profiles/mesh_smooth.txt.  Not part of bench.py; asserts nothing but that the stage's two calls agree.

    python tools/mesh_smooth_bench.py [--sizes 256,512] [--reps 5] [--out profiles/mesh_smooth.txt]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def problem(HostSolver, name, n):
    pre = HostSolver(os.path.join(ROOT, "data", name)).preprocess(hCoef=float(np.log2(n / 2) - 3))
    assert pre["n"] == n
    return pre


def wall(f, reps):
    f()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.mean(ts)), r


def torch_umbrella(V, F, iterations, lam=0.5, mu=-0.53):
    X = V.clone()
    idx = torch.cat([F[:, 0], F[:, 1], F[:, 2]])
    nb = torch.cat([F[:, 1], F[:, 2], F[:, 0]]), torch.cat([F[:, 2], F[:, 0], F[:, 1]])
    c = torch.zeros(len(V), dtype=V.dtype, device=V.device).index_add_(0, idx, torch.full((len(idx),), 2.0, dtype=V.dtype, device=V.device))
    live = c > 0
    c = torch.where(live, c, torch.ones_like(c))
    for _ in range(iterations):
        for f in (lam, mu):
            S = torch.zeros_like(X).index_add_(0, idx, X[nb[0]] + X[nb[1]])
            X = torch.where(live[:, None], X + f * (S / c[:, None] - X), X)
    return X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import shm_import
    shm = shm_import.load()
    from signed_heat_3d_amd.host_abi import HostSolver
    import mesh_smooth_ref as ref

    big = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(big)
    ms, _ = wall(lambda: dst.copy_(big), 10)
    copy_gbs = 2 * big.numel() / ms / 1e6   # read + write
    del big, dst
    rows = [dict(row="copy", copy_GBs=round(copy_gbs, 1))]
    print(json.dumps(rows[0]), flush=True)
    for n in [int(x) for x in a.sizes.split(",")]:
        pre = problem(HostSolver, "bunny_small.obj", n)
        s = shm.GridSolver()
        s.set_problem(pre["pos"], pre["wnormal"], pre["area"], pre["lam"], pre["n"], pre["bbox_min"], pre["cell"])
        s.solve()
        phimax = float(s.get_phi()[0].max())
        for iso_name, iso in (("0", 0.0), ("0.25max", 0.25 * phimax)):
            V, F = s.isosurface_indexed(iso, device=True)
            nv, nt = len(V), len(F)
            inc = 3 * nt
            build_ms, _ = wall(lambda: s.smooth_mesh_device(V, F, 0), a.reps)
            t10, r10 = wall(lambda: s.smooth_mesh_device(V, F, 10, normals=True), a.reps)
            t20, _ = wall(lambda: s.smooth_mesh_device(V, F, 20, normals=True), a.reps)
            again = s.smooth_mesh_device(V, F, 10, normals=True)
            assert torch.equal(again[0], r10[0]) and torch.equal(again[1], r10[1])
            pass_ms = (t20 - t10) / 20
            pass_mb = (48 * nv + 8 * nv + 8 * inc) / 1e6
            tt, rt = wall(lambda: torch_umbrella(V, F, 10), a.reps)

            t0 = time.perf_counter()   # (once, cold: seconds)
            Vh, Fh = s.get_isosurface_indexed(nv, nt)
            ref.float_umbrella(Vh, Fh, 10)
            th = (time.perf_counter() - t0) * 1e3
            row = dict(row="mesh", n=n, iso=iso_name, nv=nv, nt=nt, build_ms=round(build_ms, 3), taubin10_ms=round(t10, 3), taubin20_ms=round(t20, 3),
                       pass_ms=round(pass_ms, 4), pass_MB=round(pass_mb, 2), pass_share=round(pass_mb / 1e3 / pass_ms * 1e3 / copy_gbs, 3),
                       torch10_ms=round(tt, 3), numpy10_ms=round(th, 1), max_diff_vs_torch=float((r10[0] - rt).abs().max()))
            rows.append(row)
            print(json.dumps(row), flush=True)
        s.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("Taubin smoothing of the indexed mesh on the device: tools/mesh_smooth_bench.py (columns explained there), MI355X, SHM_F64, bunny_small\n")
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
