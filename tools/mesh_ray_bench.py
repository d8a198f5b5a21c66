"""Time of shm_grid_mesh_raycast_device on a solved grid, beside shm_grid_raycast_device on the same rays from the same build, for scale.

For each grid (bunny_small at 256^3 and 512^3, fp64), each mesh (the phi contour at 0 and at 0.25 max phi, each unfiltered and after keep_largest = 1) and each
ray set:
    primary     the camera rays of tools/ray_render.py, --size^2 of them in 8 x 8 pixel tiles, closest hit only (no count): the walk stops behind the first hit
    parity      one ray along +x from every node of every 4th grid plane in y and z (along grid lines, through the mesh's vertices), with count: the walk runs
                to the end of the box
one warm-up, then --reps repetitions; every time is the median of the wall time of the synchronous device call.  Recorded per row:
    build_ms            the index build, from the handle's own events (the verbose log line of the first cast of a mesh)
    cast_ms, Mrays_per_s  one call on the resident index
    tests_per_ray       triangle tests per ray, from the same log line
    phi_cast_ms         shm_grid_raycast_device at the mesh's isovalue on the same rays (the trilinear level set: another surface, the same order of work)
One JSON line per row, and --out writes the table.  Not part of bench.py; asserts nothing.

    python tools/mesh_ray_bench.py [--reps 5] [--cases bunny_small:256:64,bunny_small:512:64] [--size 1024] [--out profiles/mesh_raycast.txt]
"""
import argparse
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LOG = re.compile(r"mesh_raycast: (\d+) rays, (\d+) hits, (\d+) triangle tests, (\d+) slivers, index build ([0-9.]+) ms")


def logged(f):
    """f() with the process's stderr (the library logs there) captured: (result, the last mesh_raycast log line's fields)."""
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            out = f()
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        m = LOG.findall(tmp.read().decode(errors="replace"))
    return out, ([float(x) for x in m[-1]] if m else None)


def median_ms(f, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def run(a):
    import torch
    import shm_import
    import ray_render
    shm = shm_import.load()
    from signed_heat_3d_amd.host_abi import HostSolver
    rows = []
    for case in a.cases.split(","):
        mesh, n_want, prec = case.split(":")
        n_want, prec = int(n_want), int(prec)
        pre = HostSolver(os.path.join(ROOT, "data", mesh + ".obj")).preprocess(hCoef=float(np.log2(n_want / 2) - 3))
        n, h, bb = pre["n"], pre["cell"], np.asarray(pre["bbox_min"], dtype=np.float64)
        assert n == n_want
        s = shm.GridSolver(precision=shm.SHM_F64 if prec == 64 else shm.SHM_F32, verbose=True)
        s.set_problem(pre["pos"], pre["wnormal"], pre["area"], pre["lam"], n, pre["bbox_min"], h)
        logged(lambda: s.solve())
        hi = float(s.get_phi()[0].max())
        tdt = torch.float64 if prec == 64 else torch.float32
        O, D, _ = ray_render.camera_rays(torch, n, bb, h, a.size, dtype=tdt)
        ax = [torch.arange(n, device="cuda", dtype=torch.float64) * h + float(bb[k]) for k in range(3)]
        z, y, x = torch.meshgrid(ax[2][::4], ax[1][::4], ax[0], indexing="ij")
        PO = torch.stack([x, y, z], dim=-1).reshape(-1, 3).to(tdt).contiguous()
        PD = torch.zeros_like(PO)
        PD[:, 0] = 1.0
        for label, iso, keep in (("iso0", 0.0, None), ("iso0_keep1", 0.0, 1), ("quarter_max", 0.25 * hi, None), ("quarter_max_keep1", 0.25 * hi, 1)):
            for rname, o, d, count in (("primary", O, D, False), ("parity", PO, PD, True)):
                V, F = s.isosurface_indexed(iso, keep_largest=keep)          # a fresh mesh in the slot: the next cast builds the index
                cast = lambda: s.mesh_raycast_device(o, d, tri=True, bary=False, count=count)    # noqa: E731
                (out, info) = logged(cast)
                build_ms = info[4]
                (out, info) = logged(cast)
                cast_ms = median_ms(cast, a.reps)
                s.raycast_device(o, d, iso)
                phi_ms = median_ms(lambda: s.raycast_device(o, d, iso), a.reps)
                Q = len(o)
                host_ms = None
                if a.host:
                    o64, d64 = o.cpu().numpy().astype(np.float64), d.cpu().numpy().astype(np.float64)
                    host_cast = lambda: s.mesh_raycast(o64, d64, tri=True, bary=False, count=count)    # noqa: E731
                    host_cast()
                    host_ms = round(median_ms(host_cast, 1), 2)
                row = dict(case=case, mesh=label, n_triangles=int(len(F)), n_slivers=int(info[3]), rays=rname, n_rays=Q, hits=int(info[1]), build_ms=round(build_ms, 3),
                           cast_ms=round(cast_ms, 3), Mrays_per_s=round(Q / cast_ms / 1e3, 2), tests_per_ray=round(info[2] / Q, 2), phi_cast_ms=round(phi_ms, 3),
                           host_ms=host_ms)
                print(json.dumps(row), flush=True)
                rows.append(row)
        s.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="bunny_small:256:64,bunny_small:512:64")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--out", default="")
    ap.add_argument("--host", type=int, default=0, help="also time the host entry point on the same rays, once after a warm-up call (host_ms)")
    a = ap.parse_args()
    rows = run(a)
    if a.out:
        keys = ["case", "mesh", "n_triangles", "rays", "n_rays", "hits", "build_ms", "cast_ms", "Mrays_per_s", "tests_per_ray", "phi_cast_ms"]
        with open(a.out, "w") as f:
            f.write("mesh ray casts, median of %d after a warm-up (tools/mesh_ray_bench.py)\n" % a.reps)
            f.write("  ".join(keys) + "\n")
            for r in rows:
                f.write("  ".join(str(r[k]) for k in keys) + "\n")
            f.write("\nrows as JSON\n")
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
