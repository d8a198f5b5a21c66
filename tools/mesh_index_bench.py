"""Cost of closest-point queries against the attached mesh (shm_grid_attach_mesh_device / shm_grid_attached_closest_point_device) beside the existing path against
the resident indexed mesh (shm_grid_closest_point_device at max_dist = 8 cell: the yardstick), in one process.  bunny_small at 256^3 and 512^3, an SHM_F64
handle, the contour at 0.25 max phi, warm.  Every call is synchronous, so the host clock around it is what a caller waits.

Per grid size:
    attach rows  the attach time (wall, and the device time the info reports) with the index's counts, for (a) the contour at the automatic c, (b) the contour
                 at index cell = grid cell (c = the box's longest side in grid cells, rounded up, at most 512), (c) the smoothed mesh (10 Taubin iterations)
                 at the automatic c
    query rows   2^20 near-surface queries (mesh vertices displaced by 0.3 cell of Gaussian noise, in vertex order) and 2^20 uniform queries in the solve
                 grid's box (in Morton order of 8^3 blocks, so that neighbours in space are neighbours in the array), max_dist = 8 cell, against each of (a),
                 (b), (c) and against the resident path; answered = answered queries, vs_resident = ms over the resident path's ms on the same queries
    deviation    256^3 only: one-sided deviation contour -> input faces and smoothed -> input faces (max and mean over the vertices, in cells),
                 max_dist = inf, against the input surface attached at the automatic c
    cpu row      the same deviation from the numpy restatement at 64^3 (contour built by the numpy marching cubes from the device's phi, every 8th vertex),
                 so that a reader without a GPU can see the quantity
One JSON line per row; --out writes the table to profiles/mesh_index.txt.  Not part of bench.py; asserts only that (a), (b) answer as the resident path does.

    python tools/mesh_index_bench.py [--sizes 256,512] [--reps 5] [--out profiles/mesh_index.txt]
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


def wall(f, reps):
    f()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), r


def read_obj(path):
    V, F = [], []
    for line in open(path):
        p = line.split()
        if p and p[0] == "v":
            V.append([float(x) for x in p[1:4]])
        elif p and p[0] == "f":
            ids = [int(x.split("/")[0]) - 1 for x in p[1:]]
            F += [[ids[0], ids[k], ids[k + 1]] for k in range(1, len(ids) - 1)]
    return np.array(V), np.array(F, dtype=np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import shm_import
    shm = shm_import.load()
    from signed_heat_3d_amd.host_abi import HostSolver
    import mesh_index_ref as mir
    import mesh_smooth_ref as msr
    import redistance_exact_ref as rx

    Vi, Fi = read_obj(os.path.join(ROOT, "data", "bunny_small.obj"))
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    dev = torch.device("cuda", 0)
    for n in [int(x) for x in a.sizes.split(",")]:
        pre = HostSolver(os.path.join(ROOT, "data", "bunny_small.obj")).preprocess(hCoef=float(np.log2(n / 2) - 3))
        assert pre["n"] == n
        s = shm.GridSolver()
        s.set_problem(pre["pos"], pre["wnormal"], pre["area"], pre["lam"], pre["n"], pre["bbox_min"], pre["cell"])
        s.solve()
        h, bb = float(pre["cell"]), np.asarray(pre["bbox_min"], dtype=np.float64)
        iso = 0.25 * float(s.get_phi()[0].max())
        V, F = s.isosurface_indexed(iso, device=True)
        Xs = s.isosurface_smoothed(10, device=True)
        nv, nt = len(V), len(F)
        ext = float((V.max(dim=0).values - V.min(dim=0).values).max())
        c_grid = min(512, int(np.ceil(ext / h)))
        g = torch.Generator(device=dev).manual_seed(n)
        Q = a.queries
        near = (V[torch.arange(Q, device=dev) * nv // Q] + 0.3 * h * torch.randn((Q, 3), generator=g, device=dev, dtype=torch.float64)).contiguous()
        side = int(np.ceil(Q ** (1 / 3)))
        ijk = torch.stack(torch.meshgrid(*[torch.arange(side, device=dev)] * 3, indexing="ij"), dim=-1).reshape(-1, 3)
        key = ((ijk[:, 2] // 8) * (side // 8 + 1) + ijk[:, 1] // 8) * (side // 8 + 1) + ijk[:, 0] // 8       # blocks of 8^3 together
        ijk = ijk[torch.argsort(key, stable=True)][:Q]
        uni = (torch.from_numpy(bb).to(dev) + (ijk.double() + torch.rand((Q, 3), generator=g, device=dev, dtype=torch.float64)) * ((n - 1) * h / side)).contiguous()
        md = 8.0 * h
        res = {}
        for qname, pts in (("near", near), ("uniform", uni)):
            ms, r = wall(lambda: s.closest_point_device(pts, md), a.reps)
            res[qname] = r
            emit(dict(row="query", n=n, mesh="resident", queries=qname, Q=Q, ms=round(ms, 3), answered=int(r[3])))
        for mname, (Vm, cells) in (("contour_auto", (V, 0)), ("contour_gridcell", (V, c_grid)), ("smoothed_auto", (Xs, 0))):
            ms, info = wall(lambda: s.attach_mesh_device(Vm, F, cells=cells), a.reps)
            emit(dict(row="attach", n=n, mesh=mname, nv=nv, nt=nt, wall_ms=round(ms, 3), device_ms=round(info["ms"], 3), cells=info["cells"],
                      n_occupied=info["n_occupied"], n_references=info["n_references"], n_big=info["n_big"], MB=round(info["bytes"] / 1e6, 1)))
            for qname, pts in (("near", near), ("uniform", uni)):
                ms, r = wall(lambda: s.attached_closest_point_device(pts, md), a.reps)
                if mname != "smoothed_auto":
                    assert all(torch.equal(x, y) or bool((torch.isnan(x) == torch.isnan(y)).all() and torch.equal(torch.nan_to_num(x), torch.nan_to_num(y)))
                               for x, y in zip(r[:3], res[qname][:3])), (mname, qname)
                emit(dict(row="query", n=n, mesh=mname, queries=qname, Q=Q, ms=round(ms, 3), answered=int(r[3]),
                          vs_resident=round(ms / [x for x in rows if x["row"] == "query" and x["n"] == n and x["mesh"] == "resident" and x["queries"] == qname][0]["ms"], 2)))
        if n == 256:
            s.attach_mesh(Vi, Fi)
            for tag, P in (("contour", V), ("smoothed", Xs)):
                ms, r = wall(lambda: s.attached_closest_point_device(P.contiguous(), float("inf"), cp=False, tri=False), 1)
                emit(dict(row="deviation", n=n, of=tag, to="input faces", points=len(P), max_cells=round(float(r[0].max()) / h, 4), mean_cells=round(float(r[0].mean()) / h, 4),
                          ms=round(ms, 3)))
        s.detach_mesh()
        s.close()
    # the same quantity without a GPU kernel in the loop: the restatement at 64^3
    pre = HostSolver(os.path.join(ROOT, "data", "bunny_small.obj")).preprocess(hCoef=2.0)
    s = shm.GridSolver()
    s.set_problem(pre["pos"], pre["wnormal"], pre["area"], pre["lam"], pre["n"], pre["bbox_min"], pre["cell"])
    s.solve()
    phi = s.get_phi()[0]
    s.close()
    X = rx.mesh(phi, 64, pre["bbox_min"], float(pre["cell"]), 0.25 * float(phi.max()))
    Vc, inv = np.unique(X.reshape(-1, 3), axis=0, return_inverse=True)
    Fc = inv.reshape(-1, 3).astype(np.int64)
    Vs = np.asarray(msr.smooth(Vc, Fc, 10)).reshape(-1, 3)
    idx = mir.build(Vi, Fi, 0)
    for tag, P in (("contour", Vc), ("smoothed", Vs)):
        mx, mean = mir.deviation(idx, P[::8])
        emit(dict(row="cpu", n=64, of=tag, to="input faces", points=len(P[::8]), max_cells=round(mx / float(pre["cell"]), 4), mean_cells=round(mean / float(pre["cell"]), 4)))
    if a.out:
        with open(a.out, "w") as f:
            f.write("Closest-point queries against the attached mesh: tools/mesh_index_bench.py (rows explained there), MI355X, SHM_F64, bunny_small, contour at 0.25 max phi\n")
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
