"""One application of the iterative dual solver's operator S = A K^+ A^T through the grid, held by itself: scatter_rows_to_nodes_kernel, the five sparse sweeps
of launch_precond_sparse (x and y on the active tiles and planes, the fused z sweep under the plane mask below n = 256, zsolve_sparse_kernel with its
zero-line workgroup from 256 on), gather_rows_kernel -- through GridSolver.apply_kplus_sparse (the sweeps alone) and GridSolver.apply_schur_grid (the chain).
A whole solve cannot see an error in this operator below about 1e-7: CG solves with the operator it is given and reports the residual of that operator.

THE BOUND IS MEASURED ON THE REFERENCE, NEVER ON THE DEVICE.  For every case E is the L-infinity error of scipy's DCT chain in the handle's precision against
the same chain in long double (tests/dual_operator_ref.py), on the device's own input (rounded to the handle's precision first: the rule of
test_stage_edges.py), taken on the touched nodes or on the m outputs; the device is held to FACTOR x E, stage E's factor in test_stage_edges.py for the reason
given there (the kernel's twiddles come from a multiplication tree and two real lines share a complex FFT: a few more roundings per pass than pocketfft's; a
defect gives 1e-2 ... 1 of max|ref|).  tests/test_dual_operator_host.py holds the premise for the z recursion, which is no DCT: it is at least as accurate as
the float64 chain.  For S on an fp32 handle the chain E is measured on makes the handle's own roundings: A^T v is summed in float64 and stored once per
touched node as float32, and the float32 result is gathered in float64.  Every test prints the device's error, E, their ratio and the margin."""
import os
import subprocess
import sys

import numpy as np
import pytest

try:
    import torch  # noqa: F401  (first, so that it and libshm_grid.so share one HIP runtime)
except ImportError:
    torch = None

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dual_operator_ref as ref
from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu

FACTOR = 8
DTYPE = {64: np.float64, 32: np.float32}
THREADS = min(16, os.cpu_count() or 1)
SHM_ERR_INVALID, SHM_ERR_STATE = 1, 7


def _round_to(v, precision):
    return v.astype(np.float32).astype(np.float64) if precision == 32 else np.asarray(v, dtype=np.float64)


# ---- problems: what matters here is which nodes the rows touch ------------------------------------------------------------------------------------------------------
def _bunny(n):
    """The 16^3 bunny fixture with the cell rescaled to n - 1 intervals (as test_stage_edges.py)."""
    g = load_golden("bunny_small_n16")
    return dict(pos=g["pos"], wnormal=g["wnormal"], area=g["area"], lam=float(g["lam"]), n=n, bbox_min=g["bbox_min"], cell=float(g["cell"]) * 15 / (n - 1))


def _from_positions(n, pos, seed):
    """A problem on the box [-1, 1]^3 with n nodes per axis from source positions; normals and areas are arbitrary (neither entry point reads them)."""
    rng = np.random.default_rng(seed)
    S = len(pos)
    nrm = rng.standard_normal((S, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    area = rng.uniform(0.5, 1.5, S) * 0.05
    return dict(pos=np.asarray(pos, dtype=np.float64), wnormal=nrm * area[:, None], area=area, lam=6.0, n=n, bbox_min=np.array([-1.0, -1.0, -1.0]), cell=2.0 / (n - 1))


def _from_cells(n, cells, seed=0):
    """One source inside each cell (i, j, k), at a random offset in (0.2, 0.8)^3 of the cell: its row touches the cell's eight corners, planes k and k + 1."""
    rng = np.random.default_rng(1000 + seed)
    cells = np.asarray(cells, dtype=np.float64).reshape(-1, 3)
    return _from_positions(n, -1.0 + (cells + rng.uniform(0.2, 0.8, cells.shape)) * (2.0 / (n - 1)), seed)


def _gapped48(n, seed=1):
    """The 48 scattered points of test_dual_z_recursion_against_primal_dct_with_gapped_planes (test_gpu_parity.py), positions only."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-0.93, 0.93, (48, 3))
    pos[:4, 2] = [-0.98, -0.975, 0.97, 0.985]
    return _from_positions(n, pos, seed)


def _with_planes(n, count):
    """Cells giving exactly `count` active planes: separate cells, 14 planes apart, give two planes each; for an odd count two cells stacked in z give three."""
    rng = np.random.default_rng(count)
    ks = [3 + 14 * a for a in range(count // 2 - (count & 1))]
    if count & 1:
        ks += [ks[-1] + 14, ks[-1] + 15]
    assert ks[-1] <= n - 2
    return _from_cells(n, [(int(rng.integers(0, n - 1)), int(rng.integers(0, n - 1)), k) for k in ks], seed=count)


def _problem(n, case):
    if case == "origin":
        return _from_cells(n, [(0, 0, 0)])
    if case == "far":
        return _from_cells(n, [(n - 2, n - 2, n - 2)])
    if case == "bunny":
        return _bunny(n)
    if case == "column":
        return _from_cells(n, [(n // 2 + 1, 5, k) for k in range(n - 1)])
    if case == "one":
        return _from_cells(n, [(100, 37, 129)])
    if case == "ends":
        return _from_cells(n, [(17, 200, 0), (201, 90, n - 2)])
    if case == "gapped48":
        return _gapped48(n)
    if case.startswith("planes"):
        return _with_planes(n, int(case[6:]))
    raise KeyError(case)


EXPECTED_PLANES = {"origin": lambda n: 2, "far": lambda n: 2, "column": lambda n: n, "one": lambda n: 2, "ends": lambda n: 4, "planes16": lambda n: 16,
                   "planes17": lambda n: 17, "planes32": lambda n: 32, "planes33": lambda n: 33}


def _solver(shm, d, precision=64, **kw):
    s = shm.GridSolver(precision=precision, **kw)
    s.set_problem(d["pos"], d["wnormal"], d["area"], float(d["lam"]), int(d["n"]), d["bbox_min"], float(d["cell"]))
    return s


def _rows(s, n):
    nodes, coeffs = s.get_constraints()
    return ref.ConstraintRows(nodes, coeffs, n)


def _node_inputs(A, n, precision):
    """The four inputs of the K^+ entry, as N-vectors: the values on the touched nodes, and noise on every other node -- the entry must not read it."""
    rng = np.random.default_rng(n + A.m)
    t = A.touched
    k = t // (n * n)
    single = np.zeros(t.size)
    single[t.size // 2] = 1.5
    for name, vals in zip(INPUTS, (rng.standard_normal(t.size), np.ones(t.size), np.where(k & 1, -1.0, 1.0), single)):
        v = 1e3 * rng.standard_normal(n ** 3)
        v[t] = vals
        yield name, _round_to(v, precision)


def _report(what, items):
    print("\n%s" % what)
    for name, err, E in items:
        print("   %-12s device error %.3e, E %.3e, ratio %.2f (bound %d, margin %.1fx)" % (name, err, E, err / max(E, 1e-300), FACTOR, FACTOR * E / max(err, 1e-300)))


# ---- K^+ by the sparse sweeps ------------------------------------------------------------------------------------------------------------------------------------------
INPUTS = ("normal", "ones", "alternating", "single")
# (n = 256: one input per test -- the long-double chain takes a second there)
KPLUS_CASES = [(n, c, "all") for n in (16, 32, 64, 128) for c in ("origin", "far", "bunny", "column")] + \
              [(256, c, i) for c in ("one", "ends", "gapped48", "planes16", "planes17", "planes32", "planes33", "column", "bunny") for i in INPUTS]


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("n,case,inputs", KPLUS_CASES)
def test_kplus_sparse_sweeps_against_the_long_double_chain(shm, n, case, inputs, precision):
    """apply_kplus_sparse on the touched nodes against the long-double chain at FACTOR x E, for four inputs (random normal; the constant 1, whose non-zero mean
    the zero line removes; alternating sign per plane; one non-zero node), and exact zeros on every other node of the result.  n < 256: the fused z sweep
    under the plane mask; n = 256: zsolve_sparse_kernel -- two adjacent planes, a gap of 253, scattered planes, the 16-plane chunk seams (16, 17, 32, 33
    planes), all planes, a surface.
    Measured on an MI355X, worst device error / E over the cases and inputs of one n (profiles/dual_operator.txt has every case): fp64 2.34, 1.37, 1.74, 2.29 at
    n = 16 ... 128 and 4.18 at 256; fp32 1.40, 2.58, 2.32, 1.85 and 2.76.  The 4.18 is "ends", alternating, fp64, the one case above half the bound: every
    cell's corners sum to zero, the low modes -- where the float64 chain and the device share the rounding of the eigenvalue table -- drop out, and E is a
    thirtieth of the same set's E for the other inputs (3.5e-21; the device's error, 1.4e-20, is below theirs).  The next largest at 256 is 2.76."""
    d = _problem(n, case)
    s = _solver(shm, d, precision)
    A = _rows(s, n)
    if case in EXPECTED_PLANES:
        assert A.planes.size == EXPECTED_PLANES[case](n), (case, A.planes)
    if case in ("ends",):
        assert list(A.planes) == [0, 1, n - 2, n - 1]
    h = float(d["cell"])
    planes = A.planes if n >= 256 else None                       # (256: x and y transforms of the active planes only, see dual_operator_ref.kplus)
    untouched = np.ones(n ** 3, dtype=bool)
    untouched[A.touched] = False
    items = []
    for name, v in _node_inputs(A, n, precision):
        if inputs not in ("all", name):
            continue
        got = s.apply_kplus_sparse(v)
        assert not got[untouched].any(), "%s: a node outside the touched set is not zero" % name
        w = np.zeros(n ** 3)
        w[A.touched] = v[A.touched]
        exact = ref.kplus(w, n, h, ref.LD, planes, THREADS)[A.touched]
        chain = ref.kplus(w, n, h, DTYPE[precision], planes, THREADS)[A.touched]
        E = float(np.abs(chain - exact).max())
        items.append((name, float(np.abs(got[A.touched] - exact).max()), E))
    s.close()
    _report("K^+ sparse n=%d %s fp%d, %d touched nodes on %d planes" % (n, case, precision, A.touched.size, A.planes.size), items)
    for name, err, E in items:
        assert err <= FACTOR * E, (n, case, precision, name, err, E)


# ---- S v through the grid ----------------------------------------------------------------------------------------------------------------------------------------------
def _row_inputs(m):
    e0, e1 = np.zeros(m), np.zeros(m)
    e0[0] = e1[m - 1] = 1.0
    return [("normal", np.random.default_rng(m).standard_normal(m)), ("ones", np.ones(m)), ("e_0", e0), ("e_{m-1}", e1)]


_SCHUR_EXACT = {}                  # (n, case, input) -> the long-double S v: the m-vectors are doubles on either handle, so both precisions share it
SCHUR_SLABS = {32: 2, 64: 4}       # several slabs run the dense sweeps and the all-reduce; the line transforms serve a power-of-two number of equal slabs


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("n,case", [(32, "bunny"), (64, "bunny"), (256, "bunny"), (256, "gapped48")])
def test_schur_through_the_grid_against_the_long_double_chain(shm, n, case, precision, monkeypatch):
    """apply_schur_grid(v) for v random, the constant 1, e_0 and e_{m-1}: the sparse and the dense sweeps each at FACTOR x E of the long-double chain
    A K^+ A^T v; several slabs (n = 32: 2, n = 64: 4; dense sweeps and the all-reduce of the gather) at the same bound; against get_schur() @ v within the sum of
    this bound and the one test_schur_edges.py holds S to (1e-10 of each column's largest entry, summed over |v|); and u . (S v) = v . (S u) within
    |u|_1 bound(v) + |v|_1 bound(u).
    Measured on an MI355X, worst device error / E over the four inputs: n = 32: fp64 2.27, fp32 1.46 (sparse, dense and two slabs alike to the digits shown);
    n = 64: fp64 1.00, fp32 1.63 (four slabs alike); n = 256: fp64 0.90 sparse, 1.00 dense; fp32 1.68 sparse, 2.38 dense.  A ratio of 1.00 on an fp64 handle: the
    rounding of the eigenvalue table, 2 - 2 cos(pi k / n) formed in double by the library and by the float64 chain alike, dominates both errors."""
    d = _problem(n, case)
    h = float(d["cell"])
    s = _solver(shm, d, precision)
    A = _rows(s, n)
    inputs = _row_inputs(A.m)
    E, exact, got = {}, {}, {}
    for name, v in inputs:
        if (n, case, name) not in _SCHUR_EXACT:
            _SCHUR_EXACT[n, case, name] = A.schur_apply(v, n, h, "ld", THREADS)
        exact[name] = _SCHUR_EXACT[n, case, name]
        E[name] = float(np.abs(A.schur_apply(v, n, h, precision, THREADS) - exact[name]).max())
        for sweeps in ("sparse", "dense"):
            got[name, sweeps] = s.apply_schur_grid(v, sweeps)
    many = None
    if n in SCHUR_SLABS:
        many = _solver(shm, d, precision, local_slabs=SCHUR_SLABS[n])
        for name, v in inputs:
            got[name, "dense, %d slabs" % SCHUR_SLABS[n]] = many.apply_schur_grid(v, "dense")
        with pytest.raises(shm.ShmError) as e:
            many.apply_schur_grid(inputs[0][1], "sparse")
        assert e.value.status == SHM_ERR_INVALID
        many.close()
    err = {key: float(np.abs(g - exact[key[0]]).max()) for key, g in got.items()}
    for sweeps in sorted({key[1] for key in got}):
        _report("S v through the grid, %s sweeps, n=%d %s fp%d, m=%d" % (sweeps, n, case, precision, A.m), [(name, err[name, sweeps], E[name]) for name, _ in inputs])
    for (name, sweeps), e_dev in err.items():
        assert e_dev <= FACTOR * E[name], (n, case, precision, name, sweeps, e_dev, E[name])
    # the explicit S, where the plan assembles one (a plan knob read per call: grids this small assemble S only for the direct solve)
    monkeypatch.setenv("SHM_DUAL_DENSE_S_ALWAYS", "1")
    S = s.get_schur()
    col = np.abs(S).max(axis=0)
    for name, v in inputs:
        diff = float(np.abs(S @ v - got[name, "sparse"]).max())
        bound = FACTOR * E[name] + 1e-10 * float((col * np.abs(v)).sum())
        print("   explicit S @ %-8s differs from the sparse sweeps by %.3e (bound %.3e)" % (name, diff, bound))
        assert diff <= bound, (n, case, precision, name, diff, bound)
    # symmetry
    (nu, u), (nv, v) = inputs[0], inputs[1]
    lhs, rhs = float(u @ got[nv, "sparse"]), float(v @ got[nu, "sparse"])
    bound = FACTOR * (np.abs(u).sum() * E[nv] + np.abs(v).sum() * E[nu])
    print("   u . (S v) - v . (S u) = %.3e (bound %.3e)" % (lhs - rhs, bound))
    assert abs(lhs - rhs) <= bound
    s.close()


# ---- state -----------------------------------------------------------------------------------------------------------------------------------------------------------
def _both(s, A, n, precision, seed):
    """(K^+ entry, S entry) of fixed inputs."""
    rng = np.random.default_rng(seed)
    return s.apply_kplus_sparse(_round_to(rng.standard_normal(n ** 3), precision)), s.apply_schur_grid(rng.standard_normal(A.m))


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("n", [64, 256])
def test_the_entry_points_keep_no_state(shm, n, precision):
    """Equal bits for: the same input twice; x, then y, then x again; P1, then set_problem(P2) on planes disjoint from P1's, against a fresh handle on P2 (S1
    must hold exact zeros outside P2's active tiles, p outside P2's touched nodes).  A zero input returns exact zeros."""
    p1 = _from_cells(n, [(3, 9, 5), (n - 3, 2, 20), (n // 2, n // 2, 21)], seed=1)
    p2 = _from_cells(n, [(3, 9, 40), (n - 4, 2, 50), (7, n - 2, n - 2)], seed=2)
    s = _solver(shm, p1, precision)
    A1 = _rows(s, n)
    x = _both(s, A1, n, precision, 1)
    assert all(np.isfinite(a).all() and a.any() for a in x)
    again = _both(s, A1, n, precision, 1)
    y = _both(s, A1, n, precision, 2)
    third = _both(s, A1, n, precision, 1)
    for a, b, c, other in zip(x, again, third, y):
        assert np.array_equal(a, b) and np.array_equal(a, c) and not np.array_equal(a, other)
    assert not s.apply_kplus_sparse(np.zeros(n ** 3)).any() and not s.apply_schur_grid(np.zeros(A1.m)).any()
    s.set_problem(p2["pos"], p2["wnormal"], p2["area"], float(p2["lam"]), n, p2["bbox_min"], float(p2["cell"]))
    A2 = _rows(s, n)
    assert not np.intersect1d(A1.planes, A2.planes).size
    moved = _both(s, A2, n, precision, 3)
    s.close()
    fresh = _solver(shm, p2, precision)
    want = _both(fresh, A2, n, precision, 3)
    fresh.close()
    for a, b in zip(moved, want):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("precision", [64, 32])
def test_a_solve_is_not_disturbed(shm, precision):
    """solve() in the direct form, both entry points, solve() again: the two phi are bit-equal, and the entries between them gave what a fresh handle gives."""
    n = 32
    d = _bunny(n)
    s = _solver(shm, d, precision)
    st = s.solve(tol=1e-10 if precision == 64 else 1e-5)
    assert st.solver == 2 and st.cg_form == 2, (st.solver, st.cg_form)
    phi = s.get_phi()[0]
    A = _rows(s, n)
    between = _both(s, A, n, precision, 4)
    with pytest.raises(shm.ShmError):
        s.get_phi()                                                # (the entries leave no phi behind, as apply_preconditioner)
    st = s.solve(tol=1e-10 if precision == 64 else 1e-5)
    assert st.cg_form == 2 and np.array_equal(s.get_phi()[0], phi)
    s.close()
    fresh = _solver(shm, d, precision)
    for a, b in zip(between, _both(fresh, A, n, precision, 4)):
        assert np.array_equal(a, b)
    fresh.close()


def _refused(shm, call, status):
    with pytest.raises(shm.ShmError) as e:
        call()
    assert e.value.status == status and str(e.value), (e.value.status, str(e.value))


def test_refusals(shm):
    """No problem: SHM_ERR_STATE.  n = 24 (no FFT line transforms), three slabs (not a power of two) and a wrong sweeps value: SHM_ERR_INVALID, for both entries."""
    s = shm.GridSolver()
    _refused(shm, lambda: s.apply_kplus_sparse(np.zeros(8)), SHM_ERR_STATE)
    out = np.zeros(8)
    assert s._lib.shm_grid_apply_schur_grid(s._h, out.ctypes.data, 0, out.ctypes.data) == SHM_ERR_STATE
    s.close()
    s = _solver(shm, _bunny(24))
    m = len(s.get_constraints()[0])
    _refused(shm, lambda: s.apply_kplus_sparse(np.zeros(24 ** 3)), SHM_ERR_INVALID)
    for sweeps in ("sparse", "dense"):
        _refused(shm, lambda: s.apply_schur_grid(np.zeros(m), sweeps), SHM_ERR_INVALID)
    s.close()
    s = _solver(shm, _bunny(32), local_slabs=3)
    m = len(s.get_constraints()[0])
    _refused(shm, lambda: s.apply_kplus_sparse(np.zeros(32 ** 3)), SHM_ERR_INVALID)
    _refused(shm, lambda: s.apply_schur_grid(np.zeros(m), "dense"), SHM_ERR_INVALID)
    s.close()
    s = _solver(shm, _bunny(32), local_slabs=2)
    _refused(shm, lambda: s.apply_kplus_sparse(np.zeros(32 ** 3)), SHM_ERR_INVALID)      # the sparse sweeps serve one slab
    v = np.zeros(m)
    assert s._lib.shm_grid_apply_schur_grid(s._h, v.ctypes.data, 2, v.ctypes.data) == SHM_ERR_INVALID
    assert s._lib.shm_grid_apply_schur_grid(s._h, None, 0, v.ctypes.data) == SHM_ERR_INVALID
    assert s._lib.shm_grid_apply_kplus_sparse(s._h, None, v.ctypes.data) == SHM_ERR_INVALID
    s.close()


def test_two_ranks_are_refused(shm, tmp_path):
    """world = 2 through the librccl double: SHM_ERR_INVALID on both ranks for both entries, with a message."""
    so = str(tmp_path / "librccl_mock.so")
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", os.path.join(ROOT, "tests", "native", "rccl_mock.c"), "-o", so, "-I/opt/rocm/include",
                           "-D__HIP_PLATFORM_AMD__", "-L/opt/rocm/lib", "-lamdhip64", "-lrt", "-lpthread"])
    uid = ("/shmmock_%d_do_2" % os.getpid()).encode().ljust(128, b"\x00")
    log = open(tmp_path / "worker.log", "w+")
    p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "worker", uid.hex(), str(tmp_path)], env=dict(os.environ, SHM_RCCL_LIB=so), stdout=log,
                         stderr=subprocess.STDOUT)
    try:
        p.wait(timeout=300)
    except subprocess.TimeoutExpired:
        p.kill()
        p.wait()
    log.seek(0)
    assert p.returncode == 0, log.read()
    for r in range(2):
        for entry in ("kplus", "schur"):
            status, msg = open(tmp_path / ("%s_%d.txt" % (entry, r))).read().split("\n", 1)
            assert int(status) == SHM_ERR_INVALID and "single-process" in msg, (r, entry, status, msg)


# ---- the worker of test_two_ranks_are_refused ------------------------------------------------------------------------------------------------------------------------
def _worker(uid_hex, out_dir):
    import threading
    import traceback
    import shm_import
    shm = shm_import.load()
    n = 32

    def run_rank(rank):
        d = _bunny(n)
        s = shm.GridSolver(device=0, rank=rank, world=2, rccl_unique_id=bytes.fromhex(uid_hex))
        s.set_problem(d["pos"], d["wnormal"], d["area"], float(d["lam"]), n, d["bbox_min"], float(d["cell"]))
        v, out = np.zeros(n ** 3), np.zeros(n ** 3)
        for entry, call in (("kplus", lambda: s._lib.shm_grid_apply_kplus_sparse(s._h, v.ctypes.data, out.ctypes.data)),
                            ("schur", lambda: s._lib.shm_grid_apply_schur_grid(s._h, v.ctypes.data, 1, out.ctypes.data))):
            rc = call()
            with open(os.path.join(out_dir, "%s_%d.txt" % (entry, rank)), "w") as fh:
                fh.write("%d\n%s" % (rc, s._lib.shm_grid_last_error(s._h).decode()))
        s.close()

    def body(rank):
        try:
            run_rank(rank)
        except BaseException:
            traceback.print_exc()
            sys.stdout.flush()
            sys.stderr.flush()
            os._exit(1)

    threads = [threading.Thread(target=body, args=(r,)) for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()


if __name__ == "__main__" and len(sys.argv) == 4 and sys.argv[1] == "worker":
    sys.path.insert(0, ROOT)
    _worker(sys.argv[2], sys.argv[3])
