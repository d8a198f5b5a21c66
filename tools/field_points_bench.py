"""Rates of shm_grid_field_at_points (Steps 1-2 at arbitrary points), beside the project's own all-fp64 grid kernel on the same sources, with the accuracy the
rates were bought at.  One visit, everything warmed, every timed window at least --window seconds of synchronous calls.

Per source file (bunny_small.obj, rocker.obj, SprayBottle.pc; the sources and lambda of the 64^3 problem), per point family
    box       uniform in the grid box
    surface   a source position plus half a cell of N(0, 1): clustered at the surface
per Q in 2^12, 2^16, 2^20, 2^22 and per arith (exact, auto at the default budget):
    dev_ms, host_ms      one call of the device entry / of the host entry (wall time of the synchronous call, mean over the window)
    kernel_ms            shm_field_stats.ms of the device entry: the kernels alone
    Gpairs_per_s         Q * S / dev_ms -- (point, source) pairs ANSWERED per second of the device entry's wall time, dropped ones included: what a caller gets
    dropped, redone      pairs_dropped / (Q * S), points_redone
    err_over_bound       max |dY| / price (exact) or / (budget + price) (auto) over 256 seeded rows of the call, against the numpy restatement of
                         tests/field_points_ref.py (a row does not depend on Q, so 256 rows stand for the call)
Then points per wave P = 1, 2, 4, 8 (SHM_FIELD_P) on rocker at Q = 2^20, and the yardstick: run_conv(step1="exact") at 64^3 and 128^3 on the same files,
pairs = n^3 * S over the wall time of the call, and the ratio of the pair rates (new entry, exact, box, largest Q, over the grid kernel at 128^3): both sides
by the same clock, the wall time of a synchronous call.
One JSON line per row.  --out writes the whole of profiles/field_points.txt: the tables, the registers of the new kernels from the library build's resource
report (lib/kernel_resources.txt) and, with --device-diff FILE, the output of
    bash tools/device_code_diff.sh <lib/obj of a build of the parent commit> signed-heat-3d_amd/lib/obj > FILE
(that comparison needs a build of the parent, which this script does not make).  Not part of bench.py; asserts nothing.

    python tools/field_points_bench.py [--window 0.3] [--files bunny_small.obj,rocker.obj,SprayBottle.pc] [--logq 12,16,20,22] [--device-diff FILE]
                                       [--out profiles/field_points.txt]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("SHM_DEBUG_KNOBS", "1")    # SHM_FIELD_P is an experiment knob


def timed(f, window):
    """Mean wall ms of f() over at least `window` seconds (f ends in a device synchronise), and the last result."""
    n, t0 = 0, time.perf_counter()
    while True:
        out = f()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= window:
            return dt * 1e3 / n, out


def problem(HostSolver, name, n):
    pre = HostSolver(os.path.join(ROOT, "data", name)).preprocess(hCoef=float(np.log2(n / 2) - 3))
    assert pre["n"] == n
    return dict(pos=pre["pos"], wnormal=pre["wnormal"], area=pre["area"], lam=float(pre["lam"]), n=n, bbox_min=np.asarray(pre["bbox_min"], dtype=np.float64),
                cell=float(pre["cell"]))


def points(d, fam, Q, seed):
    rng = np.random.default_rng(seed)
    lo = d["bbox_min"]
    hi = lo + (d["n"] - 1) * d["cell"]
    if fam == "box":
        return lo + rng.random((Q, 3)) * (hi - lo)
    return d["pos"][rng.integers(0, len(d["pos"]), Q)] + 0.5 * d["cell"] * rng.standard_normal((Q, 3))


def run(a):
    import torch
    import shm_import
    import field_points_ref as ref
    shm = shm_import.load()
    from signed_heat_3d_amd.host_abi import HostSolver
    rows, grid_rate, field_rate = [], {}, {}
    for name in a.files.split(","):
        d = problem(HostSolver, name, 64)
        S = len(d["area"])
        s = shm.GridSolver()
        s.set_problem(d["pos"], d["wnormal"], d["area"], d["lam"], d["n"], d["bbox_min"], d["cell"])
        for fam in ("box", "surface"):
            for lq in [int(x) for x in a.logq.split(",")]:
                Q = 1 << lq
                pts = points(d, fam, Q, seed=lq)
                t = torch.from_numpy(pts).to("cuda:0")
                sub = np.random.default_rng(99).choice(Q, min(Q, 256), replace=False)
                y = ref.yardstick(d["pos"], d["wnormal"], d["lam"], pts[sub])
                ok = y["finite"] & (y["lam_rmin"] < ref.ZONE)
                for arith, budget in (("exact", 0.0), ("auto", 1e-8)):
                    dev = lambda: s.field_at_points_device(t, arith=arith, stats=True)    # noqa: E731
                    dev()
                    dev_ms, (Yd, st) = timed(dev, a.window)
                    host = lambda: s.field_at_points(pts, arith=arith)    # noqa: E731
                    host()
                    host_ms, Yh = timed(host, a.window)
                    err = np.abs(Yh[sub] - y["Y"]).max(axis=1)[ok] / (budget + y["price"][ok])
                    row = dict(file=name, S=S, **{"lambda": round(d["lam"], 3)}, points=fam, Q=Q, arith=arith, dev_ms=round(dev_ms, 3), host_ms=round(host_ms, 3),
                               kernel_ms=round(st["ms"], 3), Gpairs_per_s=round(Q * S / dev_ms / 1e6, 2), dropped=round(st["pairs_dropped"] / (Q * S), 4),
                               redone=int(st["points_redone"]), out_of_zone=int(st["out_of_zone"]), rows_checked=int(ok.sum()), err_over_bound=round(float(err.max()), 4),
                               host_equals_device=bool(np.array_equal(Yd.cpu().numpy(), Yh, equal_nan=True)))
                    print(json.dumps(row), flush=True)
                    rows.append(row)
                    if fam == "box" and arith == "exact":
                        field_rate[name] = row["Gpairs_per_s"]
        if name == a.p_file:
            pts = points(d, "box", 1 << 20, seed=20)
            t = torch.from_numpy(pts).to("cuda:0")
            for P in (1, 2, 4, 8):
                os.environ["SHM_FIELD_P"] = str(P)
                for arith in ("exact", "auto"):
                    dev = lambda: s.field_at_points_device(t, arith=arith, stats=True)    # noqa: E731
                    dev()
                    ms, (_, st) = timed(dev, a.window)
                    row = dict(file=name, S=S, points="box", Q=1 << 20, arith=arith, P=P, dev_ms=round(ms, 3), kernel_ms=round(st["ms"], 3),
                               Gpairs_per_s=round((1 << 20) * S / ms / 1e6, 2))
                    print(json.dumps(row), flush=True)
                    rows.append(row)
            del os.environ["SHM_FIELD_P"]
        s.close()
        for n in (64, 128):
            g = problem(HostSolver, name, n)
            s = shm.GridSolver()
            s.set_problem(g["pos"], g["wnormal"], g["area"], g["lam"], n, g["bbox_min"], g["cell"])
            s.run_conv(step1="exact_f64")
            ms, _ = timed(lambda: s.run_conv(step1="exact_f64"), a.window)
            row = dict(file=name, S=S, yardstick="run_conv(step1=exact_f64)", n=n, **{"lambda": round(g["lam"], 3)}, call_ms=round(ms, 3),
                       Gpairs_per_s=round(n ** 3 * S / ms / 1e6, 2))
            print(json.dumps(row), flush=True)
            rows.append(row)
            grid_rate[name] = row["Gpairs_per_s"]
            s.close()
        row = dict(file=name, ratio_of_pair_rates=round(field_rate[name] / grid_rate[name], 3), field_Gpairs_per_s=field_rate[name], grid_Gpairs_per_s=grid_rate[name])
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def demangle(sym):
    return re.sub(r"\(.*", "", subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip()).replace("void shm::", "")


def report(rows, a):
    """The text of profiles/field_points.txt."""
    out = ["shm_grid_field_at_points: rates, accuracy and what the change left alone (written by tools/field_points_bench.py)", "",
           "1. Rates: one MI355X, one visit, warmed, every window at least %.1f s of synchronous calls; sources and lambda of each file's 64^3 problem." % a.window,
           "   Gpairs/s = Q * S / dev_ms / 1e6: (point, source) pairs ANSWERED per second of the device entry's wall time, dropped ones included; kernel_ms: the",
           "   kernels alone (hipEvents); host_ms: the host entry; err/bound: max |dY| / price (exact) or / (budget + price) (auto, budget 1e-8) over 256 seeded",
           "   rows against the numpy restatement; host=dev: the host entry's rows equal the device entry's bit for bit.", "",
           "file             S      lambda  points   Q        arith  kernel_ms  dev_ms    host_ms   Gpairs/s  dropped  redone  out_of_zone  err/bound  host=dev"]
    for r in rows:
        if "arith" in r and "P" not in r:
            out.append("%-16s %-6d %-7.3f %-8s %-8d %-6s %-10.3f %-9.3f %-9.3f %-9.2f %-8.4f %-7d %-12d %-10.4f %s" % (
                r["file"], r["S"], r["lambda"], r["points"], r["Q"], r["arith"], r["kernel_ms"], r["dev_ms"], r["host_ms"], r["Gpairs_per_s"], r["dropped"], r["redone"],
                r["out_of_zone"], r["err_over_bound"], r["host_equals_device"]))
    out += ["", "2. Points per wave (SHM_FIELD_P; box, Q = 2^20).  No bit of any row depends on P (tests/test_field_points.py holds that); the library takes 8 for exact and",
            "   4 for auto, fewer for a short list.", "file             P  arith  kernel_ms  dev_ms    Gpairs/s"]
    for r in rows:
        if "P" in r:
            out.append("%-16s %-2d %-6s %-10.3f %-9.3f %.2f" % (r["file"], r["P"], r["arith"], r["kernel_ms"], r["dev_ms"], r["Gpairs_per_s"]))
    out += ["", "3. The yardstick: the project's own all-fp64 grid kernel, run_conv(step1=exact_f64), same files, same script; pairs = n^3 * S over the call's wall time",
            "file             S      n    call_ms   Gpairs/s"]
    for r in rows:
        if "yardstick" in r:
            out.append("%-16s %-6d %-4d %-9.3f %.2f" % (r["file"], r["S"], r["n"], r["call_ms"], r["Gpairs_per_s"]))
    out += ["", "ratio of pair rates: new entry (exact, box, largest Q) over the grid kernel at 128^3, both by the wall time of a synchronous call"]
    for r in rows:
        if "ratio_of_pair_rates" in r:
            out.append("%-16s %.3f   (%.2f / %.2f Gpairs/s)" % (r["file"], r["ratio_of_pair_rates"], r["field_Gpairs_per_s"], r["grid_Gpairs_per_s"]))
    res_path = os.path.join(ROOT, "signed-heat-3d_amd", "lib", "kernel_resources.txt")
    if os.path.exists(res_path):
        res = open(res_path).read()
        out += ["", "4. Registers of the new kernels (the compiler's resource report of this library build, lib/kernel_resources.txt)",
                "kernel                                      VGPRs  SGPR spills  VGPR spills  waves/SIMD  LDS"]
        seen = set()
        for m in re.finditer(r"Function Name: (\S*field_points_kernel\S*)(.*?)(?=Function Name:|\Z)", res, flags=re.S):
            name = demangle(m.group(1))
            if name in seen:
                continue
            seen.add(name)
            g = lambda k: int(re.search(r"%s: (\d+)" % k, m.group(2)).group(1))    # noqa: E731
            out.append("%-43s %-6d %-12d %-12d %-11d %d" % (name, g("    VGPRs"), g("SGPRs Spill"), g("VGPRs Spill"), g(r"Occupancy \[waves/SIMD\]"), g(r"LDS Size \[bytes/block\]")))
        spills = sum(int(x) for x in re.findall(r"VGPRs Spill: (\d+)", res))
        out.append("vector registers spilled over every kernel of the library: %d" % spills)
    if a.device_diff:
        d = open(a.device_diff).read().splitlines()
        out += ["", "5. Device code of the existing kernels: tools/device_code_diff.sh <objects of a build of the parent commit> <objects of this build>", "   " + d[-1],
                "   DIFFERENT: %d;  only in the parent: %d;  only in this build: %d, of which field_points_kernel instantiations: %d" % (
                    sum(l.startswith("DIFFERENT") for l in d), sum(l.startswith("only in A") for l in d), sum(l.startswith("only in B") for l in d),
                    sum(l.startswith("only in B") and "field_points_kernel" in l for l in d)),
                "   literal only (nothing but the 32-bit literal of a PC-relative address differs: code now stands in front of a constant table):"]
        for l in d:
            if l.startswith("literal only"):
                unit, sym = l.split(": ", 1)[1].split(".", 1)
                out.append("     %s  %s" % (unit, demangle(sym)))
    out += ["", "rows as JSON"] + [json.dumps(r) for r in rows]
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--files", default="bunny_small.obj,rocker.obj,SprayBottle.pc")
    ap.add_argument("--logq", default="12,16,20,22")
    ap.add_argument("--p-file", dest="p_file", default="rocker.obj")
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
