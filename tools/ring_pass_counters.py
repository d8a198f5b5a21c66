"""Pair counters of Step 1 on the cancelling sheets and double shells of tests/test_ring_pass_gpu.py with the ring pass off and on (G = 8, ring = 2; a fresh handle per
setting: the knobs are read at set_problem).  Wrote profiles/r09_ring_counters.txt (taken BEFORE the ring pass was skipped where the dropped bound alone fails).
    python tools/ring_pass_counters.py [OUT]"""
import os, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
os.environ["SHM_DEBUG_KNOBS"] = "1"
import numpy as np
import shm_import
shm = shm_import.load()
from test_far_carry_gpu import cancelling_sheets
from test_ring_pass_gpu import double_shell
from test_gpu_parity import make_solver
out = open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, "a")
def say(s):
    print(s, flush=True); out.write(s + "\n"); out.flush()
def run(d, g, ring):
    os.environ["SHM_CONV_TIER_LOG"] = repr(g); os.environ["SHM_CONV_TIER_RING"] = repr(ring)
    s = make_solver(shm, d)
    st = s.solve(max_iters=2, allow_noconv=True)
    s.close()
    return st
cases = []
for lamc in (1.0, 2.0, 3.0):
    for sep in (0.5, 0.4, 0.3, 0.2, 0.15, 0.1):
        d = cancelling_sheets(48, sep_cells=sep); d["lam"] = lamc / d["cell"]
        cases.append(("sheets48 lamc %.1f sep %.2f" % (lamc, sep), d))
cases.append(("shell48 3000+600", double_shell(48, 3000)))
cases.append(("shell48 3000+600 r.25", double_shell(48, 3000, r_inner=0.25)))
cases.append(("shell48 3000+600 sep.3", double_shell(48, 3000, sep_cells=0.3)))
cases.append(("shell32 195+150", double_shell(32, 195, S_inner=150, radii=(0.36, 0.31, 0.27))))
cases.append(("shell37 194+150", double_shell(37, 194, S_inner=150, radii=(0.36, 0.31, 0.27))))
cases.append(("shell97 197+150 lam.5", double_shell(97, 197, S_inner=150, lam_cell=0.5, radii=(0.36, 0.31, 0.27))))
for name, d in cases:
    S = len(d["area"]); n = int(d["n"])
    for g in (8.0,):
        a = run(d, g, 0.0); b = run(d, g, 2.0)
        say("%-30s S %5d G %g | ring 0: fp64 %.4e fp32 %.4e redone %.4e | ring 2: fp64 %.4e fp32 %.4e redone %.4e | blocks redone(off)/(128 S) %.1f" % (
            name, S, g, a.pairs_fp64, a.pairs_fp32, a.pairs_redone, b.pairs_fp64, b.pairs_fp32, b.pairs_redone, a.pairs_redone / (128.0 * S)))
