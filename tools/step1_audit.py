"""What the shipped Step 1 costs on Y, measured by the device audit (shm_grid_audit_step1) where the host oracle takes minutes:
  samples: a 4096-node stratified sample of every BASELINE.json configuration at full size, one process per configuration;
  planes:  whole z-planes, STEP1_WORST_PLANES of tests/test_gpu_parity.py (read by importing the module) among them.
Every record holds max_dy, the smallest |X| / L1 the nodes reached, the audit's device time beside ms_conv of the solve, and the pair ratio
count * S / (N * S) -- what the audit evaluates against what Step 1 nominally does.  Appends to profiles/step1_audit.txt (or --out).
    python tools/step1_audit.py                 # everything: one child process per record
    python tools/step1_audit.py sample rocker_512_f32
    python tools/step1_audit.py planes knot.obj 4.0"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: (file, hCoef, precision) -- BASELINE.json configs[0..4] as bench.py runs them on one GPU
CONFIGS = {"bunny_small_64_f64": ("data/bunny_small.obj", 2.0, 64), "bunny_small_256_f64": ("data/bunny_small.obj", 4.0, 64), "rocker_512_f32": ("data/rocker.obj", 5.0, 32),
           "bunny_pc_512_f64": ("data/bunny.pc", 5.0, 64), "spraybottle_pc_1024_f32": ("data/SprayBottle.pc", 6.0, 32)}
PLANE_CASES = [("bunny_small.obj", 4.0), ("knot.obj", 4.0)]   # whole planes at 256^3 (65536 nodes each); the 512^3 / 1024^3 cases: pass them on the command line


def _solved(path, hcoef, precision):
    import shm_import
    shm = shm_import.load()
    from signed_heat_3d_amd.host_abi import HostSolver
    pre = HostSolver(os.path.join(ROOT, path)).preprocess(hCoef=hcoef)
    s = shm.GridSolver(precision=precision)
    s.set_problem(pre["pos"], pre["wnormal"], pre["area"], pre["lam"], pre["n"], pre["bbox_min"], pre["cell"])
    s.solve(scrub=not path.endswith(".pc"))            # once to warm up, once for the record
    st = s.solve(scrub=not path.endswith(".pc"))
    return s, pre, st


def _record(label, pre, st, a, count):
    verdict = {1: "within budget", 0: "OVER BUDGET", -1: "no budget in this mode"}[a["within_budget"]]
    return ("%s n=%d S=%d: max_dy %.3e budget %.1e %s | worst node %d (|X|/L1 %.3e) min |X|/L1 %.3e | audited %d out_of_zone %d nonfinite %d mismatch %d | "
            "audit %.3f ms, ms_conv %.3f, pair ratio %.3e (count %d / N %d)"
            % (label, pre["n"], pre["S"], a["max_dy"], a["budget"], verdict, a["worst_node"], a["worst_ratio"], a["min_ratio"], a["n_audited"], a["n_out_of_zone"],
               a["n_nonfinite"], a["n_finite_mismatch"], a["ms"], st.ms_conv, count / float(pre["n"]) ** 3, count, pre["n"] ** 3))


def sample(name):
    path, hcoef, precision = CONFIGS[name]
    s, pre, st = _solved(path, hcoef, precision)
    a = s.audit_step1(count=4096, seed=0)
    return _record("sample %s" % name, pre, st, a, 4096)


def planes(fname, hcoef):
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_parity import STEP1_WORST_PLANES
    s, pre, st = _solved(os.path.join("data", fname), hcoef, 64)
    n = pre["n"]
    ks = list(STEP1_WORST_PLANES.get((fname, hcoef), [])) + [n // 2]
    out = []
    for k in dict.fromkeys(ks):
        nodes = np.arange(k * n * n, (k + 1) * n * n, dtype=np.int64)
        out.append(_record("plane %s hCoef %g k=%d" % (fname, hcoef, k), pre, st, s.audit_step1(nodes=nodes), len(nodes)))
    return "\n".join(out)


if __name__ == "__main__":
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "step1_audit.txt")
    if "--out" in args:
        out_path = args[args.index("--out") + 1]
        del args[args.index("--out"):args.index("--out") + 2]
    if args and args[0] == "sample":
        print(sample(args[1]))
    elif args and args[0] == "planes":
        print(planes(args[1], float(args[2])))
    else:
        jobs = [["sample", name] for name in CONFIGS] + [["planes", f, str(h)] for f, h in PLANE_CASES]
        with open(out_path, "a") as f:
            for job in jobs:   # one process per record: a handle's pools and a 1024^3 grid do not outlive their record
                p = subprocess.run([sys.executable, os.path.abspath(__file__)] + job, capture_output=True, text=True, timeout=900)
                text = p.stdout.strip() if p.returncode == 0 else "%s: FAILED (exit %d) %s" % (" ".join(job), p.returncode, p.stderr.strip()[-300:])
                print(text)
                f.write(text + "\n")
                f.flush()
                if p.returncode != 0:
                    sys.exit(p.returncode)   # nothing more is started on the device after a failure
