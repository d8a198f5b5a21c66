"""A/B of builds of the library on Step 1, the way the Step-1 notes measure it: the builds alternate, one fresh process per build and measurement, K alternations on one
box.  Per alternation and build: Step 1 alone (shm_grid_run_conv, wall clock, minimum of four; tools/ab.py's child) on the listed workloads, and `python bench.py`'s
ms_per_step.  A build is a name and a library path (empty: the in-tree library); the FIRST one is the baseline whose own max - min spread the others are held against.
    python tools/step1_ab.py [--alternations 5] [--cases file:hCoef:precision,...] parent=signed-heat-3d_amd/lib/variants/parent/libshm_grid.so new=
Prints every child's line as it comes, then a table: mean (spread) per build and workload, the difference to the baseline in ms, % and baseline spreads."""
import json
import os
import re
import subprocess
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = "bunny_small.obj:4:64,bunny_small.obj:5:64,rocker.obj:4:64"


def run(cmd, lib):
    env = dict(os.environ, SHM_DEBUG_KNOBS="1")
    env.pop("SHM_GRID_LIB", None)
    if lib:
        env["SHM_GRID_LIB"] = os.path.abspath(lib)
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, cwd=R)
    if p.returncode != 0:   # (a child that died took the device with it or not: nothing more is started on it)
        sys.exit("child failed (%d): %s\n%s" % (p.returncode, " ".join(cmd), p.stderr[-600:]))
    return p.stdout


def main():
    args = sys.argv[1:]
    alternations, cases = 5, CASES
    while args and args[0].startswith("--"):
        if args[0] == "--alternations":
            alternations = int(args[1])
        elif args[0] == "--cases":
            cases = args[1]
        else:
            sys.exit(__doc__)
        args = args[2:]
    builds = [a.split("=", 1) for a in args]
    rows = {}   # (workload, build) -> values
    for k in range(alternations):
        for name, lib in builds:
            for case in cases.split(","):
                f, hc, prec = case.split(":")
                line = run([sys.executable, os.path.join(R, "tools", "ab.py"), "--child", f, hc, prec, name], lib).strip()
                print(line, flush=True)
                m = re.search(r"n=(\d+).* conv_alone ([\d.]+)", line)
                rows.setdefault(("Step 1 alone %s %s^3 fp%s" % (f, m.group(1), prec), name), []).append(float(m.group(2)))
            out = run([sys.executable, os.path.join(R, "bench.py")], lib)
            res = json.loads([l for l in out.strip().split("\n") if l.startswith("{")][-1])
            print("%-10s bench.py ms_per_step %.3f value %.4e" % (name, res["ms_per_step"], res["value"]), flush=True)
            rows.setdefault(("bench.py ms_per_step", name), []).append(float(res["ms_per_step"]))
    base = builds[0][0]
    print("\n%-44s %-10s %9s %8s   %s" % ("workload", "build", "mean ms", "spread", "vs %s: ms, %%, x its spread" % base))
    for w in dict.fromkeys(k[0] for k in rows):
        b = rows[(w, base)]
        bm, bs = sum(b) / len(b), max(b) - min(b)
        for name, _ in builds:
            v = rows[(w, name)]
            vm, vs = sum(v) / len(v), max(v) - min(v)
            tail = "" if name == base else "   %+.3f  %+.2f %%  %.1f x" % (vm - bm, 100.0 * (vm - bm) / bm, (bm - vm) / max(bs, 1e-9))
            print("%-44s %-10s %9.3f %8.3f%s" % (w, name, vm, vs, tail))


if __name__ == "__main__":
    main()
