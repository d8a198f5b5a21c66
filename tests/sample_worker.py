"""Worker of tests/test_sample.py::test_sample_two_ranks: the ranks of a `world`-rank solve as threads of this one process (one solver handle each), their
RCCL calls going through the shared-memory test double (tests/native/rccl_mock.c, SHM_RCCL_LIB).  Every rank solves the golden case, samples the same
points (shm_grid_sample is collective: its ghost exchange is) and saves its phi planes and its sample output.
Arguments: world, mock unique id (hex), golden case, points file (.npy), output directory."""
import os
import sys
import threading
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import shm_import  # noqa: E402


def run_rank(rank, world, uid_hex, case, pts_path, out_dir):
    shm = shm_import.load()
    d = np.load(os.path.join(ROOT, "tests", "golden", case + ".npz"))
    s = shm.GridSolver(device=0, rank=rank, world=world, rccl_unique_id=bytes.fromhex(uid_hex))
    s.set_problem(d["pos"], d["wnormal"], d["area"], float(d["lam"]), int(d["n"]), d["bbox_min"], float(d["cell"]))
    s.solve(tol=1e-10)
    phi, (k0, k1) = s.get_phi()
    v, g, na = s.sample(np.load(pts_path), grad=True)
    np.save(os.path.join(out_dir, "phi_%d.npy" % rank), phi)
    np.save(os.path.join(out_dir, "sample_%d.npy" % rank), v)
    np.save(os.path.join(out_dir, "grad_%d.npy" % rank), g)
    np.save(os.path.join(out_dir, "meta_%d.npy" % rank), np.array([k0, k1, na]))
    s.close()


def main():
    world = int(sys.argv[1])
    args = sys.argv[2:6]
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
