"""Bit-identity of Step 1 between two builds of the library: sha256 of Y0 / Y1 / Y2 after shm_grid_run_conv and the three pair counters of a solve, one child
process per build (the library is chosen by SHM_GRID_LIB when it is loaded), compared line by line.  The other build is a variant beside the library, e.g. the parent
commit's sources built with  make -C signed-heat-3d_amd/csrc OUT=../lib/variants/parent .
    python tools/step1_identity.py signed-heat-3d_amd/lib/variants/parent/libshm_grid.so [file:hCoef:precision,... [library to compare instead of the in-tree one]]
Exit status 0 when every line agrees."""
import hashlib
import os
import subprocess
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = "bunny_small.obj:4:64,rocker.obj:4:64,SprayBottle.pc:4:32"


def child(cases):
    import numpy as np
    sys.path.insert(0, R)
    import shm_import
    shm = shm_import.load()
    from signed_heat_3d_amd.host_abi import HostSolver
    for case in cases.split(","):
        f, hc, prec = case.split(":")
        pre = HostSolver(os.path.join(R, "data", f)).preprocess(hCoef=float(hc))
        s = shm.GridSolver(precision=int(prec))
        s.set_problem(pre["pos"], pre["wnormal"], pre["area"], pre["lam"], pre["n"], pre["bbox_min"], pre["cell"])
        s.run_conv()
        h = hashlib.sha256()
        for k in (0, 1, 2):
            h.update(np.ascontiguousarray(s.get_field(k)).tobytes())
        st = s.solve(scrub=not f.endswith(".pc"), allow_noconv=True)
        print("%-16s n=%d fp%s S=%d  Y sha256 %s  pairs fp64 %.0f packed fp32 %.0f redone %.0f" % (
            f, pre["n"], prec, len(pre["area"]), h.hexdigest()[:32], st.pairs_fp64, st.pairs_fp32, st.pairs_redone), flush=True)
        s.close()


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child(sys.argv[2])
        sys.exit(0)
    other = os.path.abspath(sys.argv[1])
    cases = sys.argv[2] if len(sys.argv) > 2 else CASES
    this = os.path.abspath(sys.argv[3]) if len(sys.argv) > 3 else None
    out = {}
    for name, lib in (("other build", other), ("this build", this)):
        env = dict(os.environ)
        env.pop("SHM_GRID_LIB", None)
        if lib:
            env["SHM_GRID_LIB"] = lib
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", cases], env=env, capture_output=True, text=True)
        if p.returncode != 0:
            print("%s: child failed (%d)\n%s" % (name, p.returncode, p.stderr[-600:]))
            sys.exit(2)
        out[name] = p.stdout.strip().split("\n")
        print("--- %s (%s)" % (name, os.path.relpath(lib, R) if lib else "signed-heat-3d_amd/lib/libshm_grid.so"))
        print(p.stdout.strip(), flush=True)
    same = out["other build"] == out["this build"]
    print("IDENTICAL: every hash and every counter agrees" if same else "DIFFERENT")
    sys.exit(0 if same else 1)
