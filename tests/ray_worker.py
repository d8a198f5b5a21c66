"""Worker of tests/test_raycast.py::test_two_ranks_are_refused: the ranks of a `world`-rank solve as threads of this one process (one solver handle each), their
RCCL calls going through the shared-memory test double (tests/native/rccl_mock.c, SHM_RCCL_LIB), as in tests/sample_worker.py.  Every rank solves the golden
case, asks for a ray cast and writes the status and message it got; the cast is refused before anything collective, so no rank waits for another.
Arguments: world, mock unique id (hex), golden case, output directory."""
import ctypes as C
import os
import sys
import threading
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import shm_import  # noqa: E402


def run_rank(rank, world, uid_hex, case, out_dir):
    shm = shm_import.load()
    d = np.load(os.path.join(ROOT, "tests", "golden", case + ".npz"))
    s = shm.GridSolver(device=0, rank=rank, world=world, rccl_unique_id=bytes.fromhex(uid_hex))
    s.set_problem(d["pos"], d["wnormal"], d["area"], float(d["lam"]), int(d["n"]), d["bbox_min"], float(d["cell"]))
    s.solve(tol=1e-10)
    o = np.tile(np.asarray(d["bbox_min"], dtype=np.float64) - 1.0, (8, 1))
    dd = np.ones((8, 3))
    t = np.zeros(8)
    nh = C.c_int64()
    rc = s._lib.shm_grid_raycast(s._h, 8, o.ctypes.data, dd.ctypes.data, 0.0, 0.0, float("inf"), t.ctypes.data, None, C.byref(nh))
    with open(os.path.join(out_dir, "ray_%d.txt" % rank), "w") as f:
        f.write("%d\n%s" % (rc, s._lib.shm_grid_last_error(s._h).decode()))
    s.sample(o)   # the ranks are still in step: a collective call after the refusal completes
    s.close()


def main():
    world = int(sys.argv[1])
    args = sys.argv[2:5]
    shm_import.load()

    def body(rank):
        try:
            run_rank(rank, world, *args)
        except BaseException:
            # a failed rank leaves its peers waiting in a collective: report it and take the whole process down at once
            traceback.print_exc()
            sys.stdout.flush()
            sys.stderr.flush()
            os._exit(1)

    threads = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()


if __name__ == "__main__":
    main()
