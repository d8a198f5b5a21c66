"""Time of labelling, measuring and filtering the connected components of the resident indexed isosurface on the device, beside the indexed build of that mesh
and the host route it replaces (fetch the mesh, label it with scipy.sparse.csgraph.connected_components -- or a numpy union-find where scipy is missing).

For each case (bunny_small 256^3 and 512^3 in fp64, rocker 512^3 in fp32) and each isovalue (0 and 0.25 max phi): one warm-up of every path, then --reps
alternating repetitions in one process, each timed with a host clock around calls that return synchronised; median, minimum and maximum per path.
  build       shm_grid_isosurface_indexed alone
  components  shm_grid_isosurface_components alone (labels + records; the mesh of the build before it)
  keep        shm_grid_isosurface_keep_components with the largest component only (the build and the labelling before it are not in the time)
  fetch       shm_grid_get_isosurface_indexed into numpy arrays
  host_label  the labelling of the fetched mesh on the host
The device's component count is checked against the host's.  One JSON line per case and isovalue, and a table; both go to --out as well.  Not part of bench.py.

    python tools/iso_components_bench.py [--reps 5] [--cases bunny_small:256:64,bunny_small:512:64,rocker:512:32] [--out profiles/iso_components.txt]
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

try:
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
except ImportError:
    connected_components = None


def host_label(nv, F):
    """Number of components and the label of every vertex, on the host."""
    if connected_components is not None:
        e = np.concatenate([F[:, [0, 1]], F[:, [0, 2]]])
        g = coo_matrix((np.ones(len(e), dtype=np.int8), (e[:, 0], e[:, 1])), shape=(nv, nv))
        return connected_components(g, directed=False)
    r = np.arange(nv, dtype=np.int64)   # numpy union-find: hook the labels of every triangle's corners to their minimum, jump, repeat
    while True:
        before = r.copy()
        L = r[F]
        m = np.repeat(L.min(axis=1), 3)
        np.minimum.at(r, F.reshape(-1), m)
        np.minimum.at(r, L.reshape(-1), m)
        while True:
            j = r[r]
            if np.array_equal(j, r):
                break
            r = j
        if np.array_equal(r, before):
            return int((r == np.arange(nv)).sum()), r


def stats(ms):
    return dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(float(np.min(ms)), 3), max_ms=round(float(np.max(ms)), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="bunny_small:256:64,bunny_small:512:64,rocker:512:32")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iso_components.txt"))
    ap.add_argument("--device-only", action="store_true", help="skip the host route (for a kernel trace)")
    a = ap.parse_args()
    import torch  # noqa: F401  (before the library is loaded)
    shm = shm_import.load()
    from signed_heat_3d_amd.host_abi import HostSolver
    lines, rows = [], []
    for case in a.cases.split(","):
        mesh, n_want, prec = case.split(":")
        n_want, prec = int(n_want), int(prec)
        pre = HostSolver(os.path.join(ROOT, "data", mesh + ".obj")).preprocess(hCoef=float(np.log2(n_want / 2) - 3))
        n = pre["n"]
        assert n == n_want
        s = shm.GridSolver(precision=shm.SHM_F64 if prec == 64 else shm.SHM_F32)
        s.set_problem(pre["pos"], pre["wnormal"], pre["area"], pre["lam"], n, pre["bbox_min"], pre["cell"])
        s.solve()
        phi_max = float(s.get_phi()[0].max())
        for iso_name, iso in (("0", 0.0), ("0.25 max", 0.25 * phi_max)):
            nv, nt, nc, kv, kt = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()

            def build():
                s._chk(s._lib.shm_grid_isosurface_indexed(s._h, iso, C.byref(nv), C.byref(nt)))

            def components():
                s._chk(s._lib.shm_grid_isosurface_components(s._h, C.byref(nc)))
            build()
            components()
            rec = s.isosurface_components()
            mask = shm.largest_components_mask(rec, keep_largest=1)

            def keep():
                s._chk(s._lib.shm_grid_isosurface_keep_components(s._h, mask.ctypes.data, C.byref(kv), C.byref(kt)))
            V = np.empty((nv.value, 3))
            F = np.empty((nt.value, 3), dtype=np.int64)

            def fetch():
                s._chk(s._lib.shm_grid_get_isosurface_indexed(s._h, V.ctypes.data, F.ctypes.data))
            keep()        # warm-up of the compaction's first-use allocations
            build()
            fetch()
            names = ["build", "components", "keep"] + ([] if a.device_only else ["fetch", "host_label"])
            ms = {p: [] for p in names}
            host_nc = None
            for _ in range(a.reps):
                t0 = time.perf_counter()
                build()
                t1 = time.perf_counter()
                components()
                t2 = time.perf_counter()
                keep()
                t3 = time.perf_counter()
                ms["build"].append((t1 - t0) * 1e3)
                ms["components"].append((t2 - t1) * 1e3)
                ms["keep"].append((t3 - t2) * 1e3)
                if not a.device_only:
                    build()
                    t0 = time.perf_counter()
                    fetch()
                    t1 = time.perf_counter()
                    host_nc = host_label(nv.value, F)[0]
                    t2 = time.perf_counter()
                    ms["fetch"].append((t1 - t0) * 1e3)
                    ms["host_label"].append((t2 - t1) * 1e3)
            assert host_nc is None or host_nc == len(rec), (host_nc, len(rec))
            res = dict(mesh=mesh, n=n, precision=prec, iso=iso_name, isovalue=iso, reps=a.reps, vertices=nv.value, triangles=nt.value, components=len(rec),
                       largest_triangles=int(rec["n_triangles"].max()), largest_share=round(float(rec["n_triangles"].max()) / max(1, nt.value), 5),
                       kept_vertices=kv.value, kept_triangles=kt.value, host_labelling="scipy" if connected_components is not None else "numpy")
            for p in names:
                res[p] = stats(ms[p])
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)
            f = lambda p: "%8.3f [%7.3f, %7.3f]" % (res[p]["median_ms"], res[p]["min_ms"], res[p]["max_ms"]) if p in res else "%26s" % "-"   # noqa: E731
            rows.append("%-12s %4d^3 fp%d  %-8s %8d %8d %6d  %8.5f   %s  %s  %s  %s  %s" % (mesh, n, prec, iso_name, nv.value, nt.value, len(rec), res["largest_share"],
                                                                                          f("build"), f("components"), f("keep"), f("fetch"), f("host_label")))
        s.close()
    head = "%-12s %-9s      %-8s %8s %8s %6s  %8s   %-26s  %-26s  %-26s  %-26s  %-26s" % ("case", "", "iso", "nv", "nt", "comps", "largest", "build median [min, max] ms",
                                                                                         "components", "keep (largest only)", "fetch to host", "host labelling")
    text = "\n".join([head] + rows + ["", "The JSON lines:", ""] + lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
