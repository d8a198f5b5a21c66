"""Time of shm_grid_closest_point_device on a solved grid, beside what a caller had before it: shm_grid_redistance_exact at the same band, psi fetched to the
host, and a numpy trilinear blend of psi at the same points.

For each case (bunny_small 256^3 and 512^3 in fp64, rocker 512^3 in fp32), each mesh (isovalue 0 after keep_largest = 1, and 0.25 max phi unfiltered), each query
set of 2^20 points (the mesh's own vertices jittered by 0.5 cell, in mesh order -- neighbours in space are neighbours in the array --, and uniform in the box)
and each max_dist (2, 4 and 8 cells): one warm-up, then --reps repetitions; every time is the median of the wall time of the synchronous device call.
Recorded per row:
    build_ms            the index build, from the handle's own events (the verbose log line of the first query of a mesh)
    query_ms, Mq_per_s  one call on the resident index; queries per second
    tests_per_query     triangle tests per query, from the same log line
    build_share         build_ms / (build_ms + query_ms): what the first call of a mesh pays for the index
    old_ms              redistance_exact (its own device time) + get_redistanced to the host + the numpy blend: the way to a distance at these points before
    blend_err_max/mean  |blend of psi| against the exact dist, in cells, over the queries that are answered and whose eight nodes are all inside the band
                        (for the filtered mesh psi still measures the unfiltered one: the rows say which)
One JSON line per row, and --out writes the table.  Not part of bench.py.

    python tools/closest_point_bench.py [--reps 5] [--cases bunny_small:256:64,bunny_small:512:64,rocker:512:32] [--max-dists 2,4,8] [--out profiles/closest_point.txt]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

LOG = re.compile(r"closest_point: (\d+) queries, (\d+) answered, (\d+) triangle tests, (\d+) slivers, index build ([0-9.]+) ms")


def logged(f):
    """f() with the process's stderr (the library logs there) captured: (result, the last closest_point log line's fields)."""
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


def blend(psi, n, bb, h, pts):
    """numpy trilinear interpolation of psi [n^3] at pts inside the box; NaN outside."""
    u = (pts - bb) / h
    inside = ((u >= 0) & (u <= n - 1)).all(axis=1)
    c = np.clip(np.floor(u).astype(np.int64), 0, n - 2)
    t = u - c
    P = psi.reshape(n, n, n)
    out = np.zeros(len(pts))
    corners = []
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                v = P[c[:, 2] + dz, c[:, 1] + dy, c[:, 0] + dx]
                corners.append(v)
                out += v * (t[:, 0] if dx else 1 - t[:, 0]) * (t[:, 1] if dy else 1 - t[:, 1]) * (t[:, 2] if dz else 1 - t[:, 2])
    out[~inside] = np.nan
    return out, np.abs(np.stack(corners)).max(axis=0)


def run(a):
    import torch
    import shm_import
    shm = shm_import.load()
    from signed_heat_3d_amd.host_abi import HostSolver
    rows = []
    Q = 1 << 20
    rng = np.random.default_rng(7)
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
        for label, iso, keep in (("iso0_keep1", 0.0, 1), ("quarter_max", 0.25 * hi, None)):
            for md_cells in [float(x) for x in a.max_dists.split(",")]:
                md = md_cells * h
                # the way before: exact psi at the nodes, fetched, blended on the host
                st = s.redistance_exact(iso, md)
                t0 = time.perf_counter()
                psi = s.get_redistanced()
                t_fetch = (time.perf_counter() - t0) * 1e3
                V, F = s.isosurface_indexed(iso, keep_largest=keep)
                vq = np.repeat(V, -(-Q // len(V)), axis=0)[:Q] if len(V) < Q else V[:Q]      # fewer vertices than queries: each several times, still in mesh order
                sets = {"vertices_jittered": vq + (rng.random((Q, 3)) - 0.5) * h, "uniform": bb + rng.random((Q, 3)) * (n - 1) * h}
                for qname, pts in sets.items():
                    t = torch.tensor(pts, dtype=tdt, device="cuda")
                    p64 = t.cpu().numpy().astype(np.float64)
                    s.isosurface_indexed(iso, keep_largest=keep)          # a fresh mesh in the slot: the next query builds the index
                    (out, info) = logged(lambda: s.closest_point_device(t, md))
                    build_ms, n_sliver = info[4], int(info[3])
                    times, tests = [], 0
                    for _ in range(a.reps):
                        t0 = time.perf_counter()
                        (out, info) = logged(lambda: s.closest_point_device(t, md))
                        times.append((time.perf_counter() - t0) * 1e3)
                        tests = info[2]
                    query_ms = float(np.median(times))
                    host_ms = None
                    if a.host:
                        s.closest_point(p64, md)
                        t0 = time.perf_counter()
                        s.closest_point(p64, md)
                        host_ms = round((time.perf_counter() - t0) * 1e3, 2)
                    dist = out[0].cpu().numpy().astype(np.float64)
                    ans = np.isfinite(dist)
                    t0 = time.perf_counter()
                    b, cmax = blend(psi, n, bb, h, p64)
                    t_blend = (time.perf_counter() - t0) * 1e3
                    both = ans & np.isfinite(b) & (cmax < md)
                    err = np.abs(np.abs(b[both]) - dist[both]) / h if both.any() else np.zeros(1)
                    row = dict(case=case, mesh=label, n_triangles=int(len(F)), n_slivers=n_sliver, queries=qname, max_dist_cells=md_cells, answered=int(ans.sum()),
                               build_ms=round(build_ms, 3), query_ms=round(query_ms, 3), Mq_per_s=round(Q / query_ms / 1e3, 2), tests_per_query=round(tests / Q, 2),
                               build_share=round(build_ms / (build_ms + query_ms), 3), old_ms=round(st["ms"] + t_fetch + t_blend, 1),
                               old_parts_ms=[round(st["ms"], 2), round(t_fetch, 1), round(t_blend, 1)], blend_compared=int(both.sum()),
                               blend_err_max=round(float(err.max()), 4), blend_err_mean=round(float(err.mean()), 5), psi_of="unfiltered mesh" if keep else "the same mesh",
                               host_ms=host_ms)
                    print(json.dumps(row), flush=True)
                    rows.append(row)
        s.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="bunny_small:256:64,bunny_small:512:64,rocker:512:32")
    ap.add_argument("--max-dists", default="2,4,8")
    ap.add_argument("--out", default="")
    ap.add_argument("--host", type=int, default=0, help="also time the host entry point on the same queries, once after a warm-up call (host_ms)")
    a = ap.parse_args()
    rows = run(a)
    if a.out:
        keys = ["case", "mesh", "n_triangles", "queries", "max_dist_cells", "answered", "build_ms", "query_ms", "Mq_per_s", "tests_per_query", "build_share", "old_ms",
                "blend_err_max", "blend_err_mean"]
        with open(a.out, "w") as f:
            f.write("closest-point queries, 2^20 queries per row, median of %d after a warm-up (tools/closest_point_bench.py)\n" % a.reps)
            f.write("  ".join(keys) + "\n")
            for r in rows:
                f.write("  ".join(str(r[k]) for k in keys) + "\n")
            f.write("\nrows as JSON\n")
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
