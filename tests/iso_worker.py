"""Worker of tests/test_iso_indexed.py::test_two_ranks: the ranks of a `world`-rank solve as threads of this one process (one solver handle each), their
RCCL calls going through the shared-memory test double (tests/native/rccl_mock.c, SHM_RCCL_LIB).  Every rank solves the golden case, builds the indexed
isosurface at every isovalue (shm_grid_isosurface_indexed is collective: its ghost exchange is) and saves its phi planes, its plane range and its meshes.
Arguments: world, mock unique id (hex), golden case, isovalues (comma separated), output directory, local slabs per rank."""
import os
import sys
import threading
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import shm_import  # noqa: E402


def run_rank(rank, world, uid_hex, case, isos, out_dir, local_slabs):
    shm = shm_import.load()
    d = np.load(os.path.join(ROOT, "tests", "golden", case + ".npz"))
    s = shm.GridSolver(device=0, rank=rank, world=world, local_slabs=int(local_slabs), rccl_unique_id=bytes.fromhex(uid_hex))
    s.set_problem(d["pos"], d["wnormal"], d["area"], float(d["lam"]), int(d["n"]), d["bbox_min"], float(d["cell"]))
    s.solve(tol=1e-10)
    phi, (k0, k1) = s.get_phi()
    np.save(os.path.join(out_dir, "phi_%d.npy" % rank), phi)
    np.save(os.path.join(out_dir, "meta_%d.npy" % rank), np.array([k0, k1]))
    for a, iso in enumerate(float(v) for v in isos.split(",")):
        V, F = s.isosurface_indexed(iso)
        np.save(os.path.join(out_dir, "V_%d_%d.npy" % (a, rank)), V)
        np.save(os.path.join(out_dir, "F_%d_%d.npy" % (a, rank)), F)
    s.close()


def main():
    world = int(sys.argv[1])
    args = sys.argv[2:7]
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
