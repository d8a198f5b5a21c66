"""Cost of the C1 cubic read of the resident phi (shm_grid_sample_cubic_device) beside the trilinear read (shm_grid_sample_device, with gradient) on the same
points.  bunny_small at 256^3, an SHM_F64 and an SHM_F32 handle, device entries, warm, one process.

Point sets
    random    2^22 uniform points in the box: a gather, served from the caches -- its share of HBM peak says nothing and is not printed
    raster    2048^2 points on the plane z = centre + 0.37 cell, row-major in (y, x): the coherent case of an image or slice
    vertices  the vertices of the indexed mesh at isovalue 0 in their canonical order (however many there are)
Per point set, `reps` rounds of four calls in turn -- cubic value, cubic value + gradient, cubic value + gradient + Hessian, trilinear value + gradient --
each between two device events and inside a host clock.  The entries are synchronous (they return after their stream has drained), so the pair of events
brackets the whole call -- launch, kernel, the counter's copy back and the host's wait -- on the device's clock: ev_ms is a call's time, not a kernel's.
Reported per call: ev_ms (mean of the event times), wall_ms (mean of the host clock: what a caller waits, the binding's allocation of the outputs
included), Mpts_per_s = Q / ev_ms, ratio = ev_ms over the trilinear call's, and
    min_MB    the bytes the algorithm must move at least: the distinct 128-byte lines of phi the windows touch (counted here on the host from the points,
              taking the array as 128-byte aligned) plus the points read and the outputs written
    hbm_share min_MB / ev_ms over the 8.0 TB/s HBM peak of the MI355X (6.3 TB/s is what a streaming copy achieves): a lower bound of the traffic over a
              call's whole time, not a kernel's measured bandwidth.
One JSON line per row; --out writes profiles/sample_cubic.txt with the table, the kernels' registers and, with --device-diff FILE, the output of
    bash tools/device_code_diff.sh <lib/obj of a build of the parent commit> signed-heat-3d_amd/lib/obj > FILE
(that comparison needs a build of the parent, which this script does not make).  Not part of bench.py; asserts nothing.

    python tools/sample_cubic_bench.py [--n 256] [--reps 10] [--device-diff FILE] [--rows LOG] [--out profiles/sample_cubic.txt]
"""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12
LINE = 128


def problem(HostSolver, name, n):
    pre = HostSolver(os.path.join(ROOT, "data", name)).preprocess(hCoef=float(np.log2(n / 2) - 3))
    assert pre["n"] == n
    return dict(pos=pre["pos"], wnormal=pre["wnormal"], area=pre["area"], lam=float(pre["lam"]), n=n, bbox_min=np.asarray(pre["bbox_min"], dtype=np.float64),
                cell=float(pre["cell"]))


def point_sets(d, logq=22, seed=0):
    n, b, h = d["n"], d["bbox_min"], d["cell"]
    hi = b + (n - 1) * h
    rng = np.random.default_rng(seed)
    side = 1 << (logq // 2)
    x = b[0] + (np.arange(side) + 0.5) / side * (hi[0] - b[0])
    y = b[1] + (np.arange(side) + 0.5) / side * (hi[1] - b[1])
    Y, X = np.meshgrid(y, x, indexing="ij")
    raster = np.stack([X, Y, np.full_like(X, 0.5 * (b[2] + hi[2]) + 0.37 * h)], -1).reshape(-1, 3)
    return {"random": b + rng.random((1 << logq, 3)) * (hi - b), "raster": raster}


def lines_touched(pts, n, b, h, esize, cubic):
    """Distinct 128-byte lines of an n^3 array of esize-byte nodes (x fastest, taken as line-aligned) that the windows of the in-box points touch: the
    cubic's 3 or 4 nodes per axis with the faces folded, or the trilinear cell's 2."""
    pts = pts[np.all((pts >= b) & (pts <= b + (n - 1) * h), axis=1)]
    idx = np.minimum(np.floor((pts - b) / h).astype(np.int64), n - 2)
    if cubic:
        lo = np.where(idx <= 0, 0, np.where(idx >= n - 2, n - 3, idx - 1))
        cnt = np.where((idx <= 0) | (idx >= n - 2), 3, 4)
    else:
        lo, cnt = idx, np.full_like(idx, 2)
    seen = np.zeros((n ** 3 * esize + LINE - 1) // LINE, dtype=bool)
    for kz in range(4 if cubic else 2):
        for r in range(4 if cubic else 2):
            ok = (kz < cnt[:, 2]) & (r < cnt[:, 1])
            row = ((lo[ok, 2] + kz) * n + (lo[ok, 1] + r)) * n
            first, last = (row + lo[ok, 0]) * esize // LINE, ((row + lo[ok, 0] + cnt[ok, 0] - 1) * esize + esize - 1) // LINE
            seen[first] = True
            seen[last] = True   # (a row of at most four nodes spans at most two lines)
    return int(seen.sum())


def run(a):
    import torch
    import shm_import
    shm = shm_import.load()
    from signed_heat_3d_amd.host_abi import HostSolver
    if not torch.cuda.is_available():
        raise SystemExit("sample_cubic_bench: no HIP device")
    d = problem(HostSolver, "bunny_small.obj", a.n)
    n, b, h = d["n"], d["bbox_min"], d["cell"]
    rows = []
    for precision in (64, 32):
        esize = precision // 8
        s = shm.GridSolver(precision=shm.SHM_F64 if precision == 64 else shm.SHM_F32)
        s.set_problem(d["pos"], d["wnormal"], d["area"], d["lam"], n, b, h)
        s.solve(tol=1e-10 if precision == 64 else 0.0)
        sets = point_sets(d, a.logq)
        V, _ = s.isosurface_indexed(0.0)
        sets["vertices"] = np.ascontiguousarray(V, dtype=np.float64)
        dt = torch.float64 if precision == 64 else torch.float32
        for name, pts in sets.items():
            t = torch.from_numpy(pts).to("cuda:0").to(dt).contiguous()
            p64 = t.cpu().numpy().astype(np.float64)
            Q = len(pts)
            calls = [("cubic value", lambda: s.sample_cubic_device(t), 1, True), ("cubic value+grad", lambda: s.sample_cubic_device(t, grad=True), 4, True),
                     ("cubic value+grad+hess", lambda: s.sample_cubic_device(t, grad=True, hess=True), 10, True),
                     ("trilinear value+grad", lambda: s.sample_device(t, grad=True), 4, False)]
            for _, f, _, _ in calls:
                f()   # warm: code objects, torch's allocator
            ev = [[] for _ in calls]
            wall = [[] for _ in calls]
            for _ in range(a.reps):
                for c, (_, f, _, _) in enumerate(calls):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0 = time.perf_counter()
                    e0.record()
                    f()
                    e1.record()
                    e1.synchronize()
                    wall[c].append((time.perf_counter() - t0) * 1e3)
                    ev[c].append(e0.elapsed_time(e1))
            tri_ms = float(np.mean(ev[3]))
            touched = {cubic: lines_touched(p64, n, b, h, esize, cubic) for cubic in (True, False)}
            for c, (label, _, width, cubic) in enumerate(calls):
                ms = float(np.mean(ev[c]))
                lines = touched[cubic]
                min_bytes = lines * LINE + Q * (3 + width) * esize
                row = dict(precision=precision, points=name, Q=Q, call=label, ev_ms=round(ms, 4), ev_ms_min=round(float(np.min(ev[c])), 4), wall_ms=round(float(np.mean(wall[c])), 4),
                           Mpts_per_s=round(Q / ms / 1e3, 1), ratio_to_trilinear=round(ms / tri_ms, 3), lines_128B=lines, min_MB=round(min_bytes / 1e6, 2),
                           hbm_share=None if name == "random" else round(min_bytes / (ms * 1e-3) / HBM_PEAK, 4))
                print(json.dumps(row), flush=True)
                rows.append(row)
        s.close()
    return rows


def report(rows, a):
    out = ["shm_grid_sample_cubic_device beside shm_grid_sample_device (written by tools/sample_cubic_bench.py)", "",
           "One MI355X, one process, bunny_small at %d^3, device entries, warm, %d rounds of the four calls in turn.  ev_ms: mean time between two device events" % (a.n, a.reps),
           "around one synchronous call, launch and the host's wait included: a call's time, not a kernel's (min over the rounds beside it); wall_ms: mean host",
           "clock around the same call; Mpts/s = Q / ev_ms; ratio: ev_ms over the",
           "trilinear call's on the same points; min_MB: distinct 128-byte lines of phi the windows touch (counted on the host from the points) plus points read and",
           "outputs written; hbm_share: min_MB / ev_ms over the 8.0 TB/s HBM peak -- a lower bound of the traffic over the whole call, not a measured bandwidth.  The",
           "random set is a gather served from the caches: no share is given for it.", "",
           "prec  points    Q         call                    ev_ms     (min)     wall_ms   Mpts/s    ratio   lines_128B  min_MB    hbm_share"]
    for r in rows:
        out.append("%-5d %-9s %-9d %-23s %-9.4f %-9.4f %-9.4f %-9.1f %-7.3f %-11d %-9.2f %s" % (
            r["precision"], r["points"], r["Q"], r["call"], r["ev_ms"], r["ev_ms_min"], r["wall_ms"], r["Mpts_per_s"], r["ratio_to_trilinear"], r["lines_128B"], r["min_MB"],
            "-" if r["hbm_share"] is None else "%.4f" % r["hbm_share"]))
    res_path = os.path.join(ROOT, "signed-heat-3d_amd", "lib", "kernel_resources.txt")
    if os.path.exists(res_path):
        res = open(res_path).read()
        out += ["", "Registers (the compiler's resource report of this library build; template arguments: node type, point type, outputs 0 value / 1 + gradient / 2 + Hessian)",
                "kernel                                  VGPRs  scratch  VGPR spills  waves/SIMD  LDS"]
        seen = set()
        for m in re.finditer(r"Function Name: \S*(sample_cubic_kernelI(\w)(\w)Li(\d)E|13sample_kernelI(\w)(\w)Lb1E)\S*(.*?)(?=Function Name:|\Z)", res, flags=re.S):
            g = lambda k: int(re.search(r"%s: (\d+)" % k, m.group(7)).group(1))    # noqa: E731
            ty = {"d": "double", "f": "float"}
            name = "sample_cubic_kernel<%s, %s, %s>" % (ty[m.group(2)], ty[m.group(3)], m.group(4)) if m.group(2) else "sample_kernel<%s, %s, true>" % (ty[m.group(5)], ty[m.group(6)])
            if name in seen:
                continue
            seen.add(name)
            out.append("%-39s %-6d %-8d %-12d %-11d %d" % (name, g("    VGPRs"), g(r"ScratchSize \[bytes/lane\]"), g("VGPRs Spill"), g(r"Occupancy \[waves/SIMD\]"), g(r"LDS Size \[bytes/block\]")))
    if a.device_diff:
        d = open(a.device_diff).read().splitlines()
        out += ["", "Device code of the existing kernels: tools/device_code_diff.sh <objects of a build of the parent commit> <objects of this build>", "   " + d[-1],
                "   DIFFERENT: %d;  only in the parent: %d;  only in this build: %d, of which sample_cubic_kernel instantiations: %d" % (
                    sum(l.startswith("DIFFERENT") for l in d), sum(l.startswith("only in A") for l in d), sum(l.startswith("only in B") for l in d),
                    sum(l.startswith("only in B") and "sample_cubic_kernel" in l for l in d)),
                "   literal only (nothing but the 32-bit literal of a PC-relative address differs: code now stands in front of a constant table):"]
        out += ["     " + l.split(": ", 1)[1] for l in d if l.startswith("literal only")]
    out += ["", "rows as JSON"] + [json.dumps(r) for r in rows]
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--logq", type=int, default=22)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--device-diff", dest="device_diff", default="", help="output of tools/device_code_diff.sh (parent's objects against this build's) to record")
    ap.add_argument("--rows", default="", help="do not measure: format the JSON rows of this file (a log of an earlier run of this script)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rows = [json.loads(l) for l in open(a.rows) if l.startswith("{")] if a.rows else run(a)
    if a.out:
        with open(a.out, "w") as f:
            f.write(report(rows, a))


if __name__ == "__main__":
    main()
