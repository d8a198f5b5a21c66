"""Time of shm_grid_redistance_exact and of the offset contour on a solved grid, beside the first-order shm_grid_redistance at the same band.

For each case (bunny_small 256^3 and 512^3 in fp64, rocker 512^3 in fp32), each isovalue (0 and 0.25 max phi) and each band (2, 4 and 8 cells): one warm-up,
then --reps repetitions; every time is the median.  Recorded per case:
    exact_ms            the call's own device time (shm_redistance_exact_stats.ms: the mesh build, init, cells, scatter and final passes)
    n_candidate_pairs   (cell, node) pairs that passed the geometric cull; pairs_per_s = n_candidate_pairs / exact_ms
    scatter_share       1 - (the same call with the scatter launch left out) / exact_ms: the timing knob SHM_RDX_NO_SCATTER, read with SHM_DEBUG_KNOBS=1 by a
                        child process this tool starts first (a knob is read once per process)
    no_atomic_ms        the whole call with the scatter pass's reads and atomicMins left out (SHM_RDX_NO_ATOMIC, a second child): the arithmetic alone
    first_order_ms      shm_grid_redistance on the same handle at the same band
    offset_ms           isosurface_indexed_psi(distance = 1 cell), wall time of the call with its counts fetched, beside
    phi_contour_ms      isosurface_indexed of phi at the isovalue itself (the offset surface of a closed shape has a comparable triangle count); both triangle
                        counts are recorded
One JSON line per case, isovalue and band, and --out writes the table.  Not part of bench.py.

    python tools/redistance_exact_bench.py [--reps 5] [--cases bunny_small:256:64,bunny_small:512:64,rocker:512:32] [--bands 2,4,8] [--out profiles/redistance_exact.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def med(f, reps):
    f()   # warm-up: allocations, code objects
    out = []
    for _ in range(reps):
        out.append(f())
    return float(np.median(out)), out


def run(a, rest_only):
    import torch  # noqa: F401  (before the library: see tests/test_sample.py)
    import shm_import
    shm = shm_import.load()
    from signed_heat_3d_amd.host_abi import HostSolver
    rows = []
    for case in a.cases.split(","):
        mesh, n_want, prec = case.split(":")
        n_want, prec = int(n_want), int(prec)
        pre = HostSolver(os.path.join(ROOT, "data", mesh + ".obj")).preprocess(hCoef=float(np.log2(n_want / 2) - 3))
        n, h = pre["n"], pre["cell"]
        assert n == n_want
        s = shm.GridSolver(precision=shm.SHM_F64 if prec == 64 else shm.SHM_F32)
        s.set_problem(pre["pos"], pre["wnormal"], pre["area"], pre["lam"], n, pre["bbox_min"], h)
        s.solve()
        hi = float(s.get_phi()[0].max())
        for frac in (0.0, 0.25):
            iso = frac * hi
            for b in [float(x) for x in a.bands.split(",")]:
                band = b * h
                last = {}

                def exact():
                    last["st"] = s.redistance_exact(iso, band)
                    return last["st"]["ms"]
                ex_ms, _ = med(exact, a.reps)
                row = dict(mesh=mesh, n=n, precision=prec, iso_frac=frac, band_cells=b, reps=a.reps, exact_ms=round(ex_ms, 3),
                           n_triangles=last["st"]["n_triangles"], n_candidate_pairs=last["st"]["n_candidate_pairs"], n_reached=last["st"]["n_reached"])
                if not rest_only:
                    def wall(f):
                        def g():
                            t0 = time.perf_counter()
                            g.res = f()
                            return (time.perf_counter() - t0) * 1e3
                        return g
                    off = wall(lambda: s._lib.shm_grid_isosurface_indexed_psi(s._h, h, None, None))
                    row["offset_ms"] = round(med(off, a.reps)[0], 3)
                    row["offset_triangles"] = len(s.isosurface_indexed_psi(h)[1])
                    row["first_order_ms"] = round(med(lambda: s.redistance(iso, band)["ms"], a.reps)[0], 3)
                    phi_c = wall(lambda: s._lib.shm_grid_isosurface_indexed(s._h, iso, None, None))
                    row["phi_contour_ms"] = round(med(phi_c, a.reps)[0], 3)
                    row["pairs_per_s"] = float("%.4g" % (row["n_candidate_pairs"] / (ex_ms * 1e-3)))
                rows.append(row)
                print(json.dumps(row), flush=True)
        s.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="bunny_small:256:64,bunny_small:512:64,rocker:512:32")
    ap.add_argument("--bands", default="2,4,8")
    ap.add_argument("--out", default="")
    ap.add_argument("--rest-only", action="store_true", help="(the child) time the call without its scatter launch")
    a = ap.parse_args()
    if a.rest_only:
        run(a, True)
        return
    # the children first, one after the other, before this process opens the device: the same cases with the scatter launch left out, and with the scatter
    # pass's atomics left out
    def child(knob):
        env = dict(os.environ, SHM_DEBUG_KNOBS="1", **{knob: "1"})
        c = subprocess.run([sys.executable, os.path.abspath(__file__), "--rest-only", "--reps", str(a.reps), "--cases", a.cases, "--bands", a.bands], env=env,
                           capture_output=True, text=True)
        if c.returncode != 0:
            sys.stderr.write(c.stdout + c.stderr)
            sys.exit(1)
        out = {}
        for line in c.stdout.splitlines():
            if line.startswith("{"):
                r = json.loads(line)
                out[(r["mesh"], r["n"], r["precision"], r["iso_frac"], r["band_cells"])] = r["exact_ms"]
        return out
    rest = child("SHM_RDX_NO_SCATTER")
    noat = child("SHM_RDX_NO_ATOMIC")
    rows = run(a, False)
    lines = ["%-12s %4s %4s %5s %5s %9s %13s %10s %11s %8s %10s %10s %9s %9s %10s %10s" % ("mesh", "n", "fp", "iso", "band", "triangles", "cand. pairs", "exact ms", "pairs/s",
                                                                                           "scatter", "no-atom ms", "1st-ord ms", "exact/1st", "offset ms", "offset tri", "phi-ctr ms")]
    for r in rows:
        r["rest_ms"] = rest[(r["mesh"], r["n"], r["precision"], r["iso_frac"], r["band_cells"])]
        r["no_atomic_ms"] = noat[(r["mesh"], r["n"], r["precision"], r["iso_frac"], r["band_cells"])]
        r["scatter_share"] = round(1.0 - r["rest_ms"] / r["exact_ms"], 3)
        lines.append("%-12s %4d %4d %5.2f %5.1f %9d %13d %10.3f %11.3g %8.3f %10.3f %10.3f %9.2f %9.3f %10d %10.3f" % (
            r["mesh"], r["n"], r["precision"], r["iso_frac"], r["band_cells"], r["n_triangles"], r["n_candidate_pairs"], r["exact_ms"], r["pairs_per_s"],
            r["scatter_share"], r["no_atomic_ms"], r["first_order_ms"], r["exact_ms"] / r["first_order_ms"], r["offset_ms"], r["offset_triangles"], r["phi_contour_ms"]))
    print("\n".join(lines), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n\n" + "\n".join(json.dumps(r) for r in rows) + "\n")


if __name__ == "__main__":
    main()
