"""Redistancing of the resident phi on the device (shm_grid_redistance and its two getters, include/shm_grid.h; kernels in csrc/shm_redistance.hip.h), through
the kernels, the C ABI, the Python bindings, the C++ host mirror and the CLI.

Reference: tests/redistance_ref.py, a numpy Jacobi iteration of the scheme run until nothing changes, fed the device's own phi cast to the handle's precision.
The discrete solution is unique, so the device (blocks, two colours, in-LDS iterations) and the restatement must agree to rounding:
    TOL = n eps_T max|psi|      eps_T the epsilon of the handle's precision: an update costs a few ulp and a causal chain is at most 3 n nodes long.
The +-inf patterns (unreached nodes, empty level sets) are compared exactly.  The rule for non-finite phi (a wall for the neighbours, NaN in psi, counted) is
held by the restatement and a CPU test of it here, and on the device in tests/test_injected_phi.py, which injects such a phi through shm_grid_set_phi.

Run as a script (`test_redistance.py worker <world> <uid hex> <case> <dir>`) this file is the worker of test_two_ranks_are_refused: the ranks of a solve as
threads of one process over the shared-memory RCCL double, as tests/ray_worker.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

# before the library is loaded: see tests/test_sample.py
try:
    import torch  # noqa: F401
except ImportError:
    torch = None

from conftest import ROOT, load_golden

import redistance_ref as ref

SHM_ERR_INVALID, SHM_ERR_NOCONV, SHM_ERR_STATE = 1, 5, 7
INF = float("inf")


def rounds_cap(n):
    return 24 * ((n + 7) // 8) + 16


# ---- CPU: the restatement itself ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,frac", [("bunny_small_n16", 0.0), ("bunny_small_n16", 0.25), ("bunny_small_n24", 0.0), ("bunny_small_n24", 0.25)])
def test_order_independence(case, frac):
    """Jacobi to its fixed point against Gauss-Seidel sweeping to its own, on the LU goldens: <= TOL / 4."""
    d = load_golden(case)
    n, h, phi = int(d["n"]), float(d["cell"]), np.asarray(d["phi"], dtype=np.float64)
    iso = frac * float(phi.max())
    psi, info = ref.redistance(phi, n, h, iso)
    gs = ref.gauss_seidel(phi, n, h, iso)
    assert info["n_frozen"] > 0 and np.isfinite(psi).all() and np.isfinite(gs).all()
    err, lim = float(np.abs(psi - gs).max()), ref.tol(n, np.float64, psi) / 4
    print("order independence %s iso %.3g: %.3e (limit %.3e)" % (case, iso, err, lim))
    assert err <= lim, (err, lim)
    assert np.array_equal(psi < 0, phi - iso < 0)


def test_axis_aligned_plane():
    n, h, x0 = 20, 0.1, 0.8371
    x = np.arange(n) * h
    f = np.broadcast_to(3.0 * (x - x0), (n, n, n)).reshape(-1)
    psi, info = ref.redistance(f, n, h)
    assert info["n_frozen"] == 2 * n * n
    want = np.broadcast_to(x - x0, (n, n, n)).reshape(-1)
    err, lim = float(np.abs(psi - want).max()), ref.tol(n, np.float64, psi)
    print("plane: %.3e (limit %.3e)" % (err, lim))
    assert err <= lim, (err, lim)


def _sphere():
    n, h, ctr, R = 32, 0.1, (1.53, 1.61, 1.47), 0.92
    x = np.arange(n) * h
    r2 = (x[None, None, :] - ctr[0]) ** 2 + (x[None, :, None] - ctr[1]) ** 2 + (x[:, None, None] - ctr[2]) ** 2
    return n, h, (r2 - R * R).reshape(-1), (np.sqrt(r2) - R).reshape(-1)


def test_sphere():
    """f = r^2 - R^2 is far from a distance (|grad f| = 2 r); psi is the distance to first order."""
    n, h, f, dist = _sphere()
    psi, info = ref.redistance(f, n, h)
    e = np.abs(psi - dist)
    print("sphere: error at frozen nodes %.3f h, everywhere %.3f h" % (e[info["frozen"]].max() / h, e.max() / h))
    assert e[info["frozen"]].max() <= 0.15 * h
    assert e.max() <= 1.0 * h


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_band_and_sign(dtype):
    n, h, f, _ = _sphere()
    if dtype == np.float32:
        f = f.astype(np.float32).astype(np.float64)
    full, _ = ref.redistance(f, n, h, dtype=dtype)
    B = 6 * h
    banded, info = ref.redistance(f, n, h, band=B, dtype=dtype)
    Bt = float(dtype(B))
    assert np.array_equal(banded, np.clip(full, -Bt, Bt))            # exactly: a node below the band has only parents below the band
    assert 0 < info["n_reached"] < n ** 3 and info["n_reached"] == int((np.abs(full) < B).sum())
    assert np.array_equal(full < 0, f < 0) and np.array_equal(banded < 0, f < 0)
    gs = ref.gauss_seidel(f, n, h, band=B, dtype=dtype) if dtype == np.float32 else None
    if gs is not None:
        assert np.array_equal(gs, banded)                              # rounded to fp32 on every store, the two orders meet bit for bit


def test_nonfinite_nodes_are_walls():
    """A node whose phi is not finite: NaN in psi, counted, +inf for its neighbours, and never an end of a cut edge."""
    n, h, f, _ = _sphere()
    f = f.reshape(n, n, n).copy()
    f[:, :, 20] = np.nan          # a wall across the grid, through the sphere: the part behind it keeps its own frozen nodes
    f[3, 4, 5] = np.inf
    f[16, 16, 16:19] = -np.inf    # inside the sphere
    psi, info = ref.redistance(f.reshape(-1), n, h)
    psi = psi.reshape(n, n, n)
    bad = ~np.isfinite(f)
    assert info["n_nonfinite"] == int(bad.sum()) and np.isnan(psi[bad]).all() and np.isfinite(psi[~bad]).all()
    assert np.array_equal(psi[~bad] < 0, f[~bad] < 0)
    # the two sides of the wall do not see each other: each side alone gives the same values
    left = f.copy()
    left[:, :, 21:] = np.nan
    psi_left, _ = ref.redistance(left.reshape(-1), n, h)
    assert np.array_equal(psi_left.reshape(n, n, n)[:, :, :20], psi[:, :, :20], equal_nan=True)
    # no cut edge ends at a wall: a grid whose only sign change is across non-finite nodes has no frozen node
    g = np.ones((8, 8, 8))
    g[:, :, :3] = -1.0
    g[:, :, 3] = np.nan
    psi2, info2 = ref.redistance(g.reshape(-1), 8, 1.0, band=2.5)
    assert info2["n_frozen"] == 0 and info2["n_reached"] == 0
    assert np.array_equal(psi2[np.isfinite(psi2)], np.where(g < 0, -2.5, 2.5)[np.isfinite(g)])


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def solved(shm, case, n, precision=64, slabs=1, **solve_kw):
    """(problem, handle, phi cast to the handle's precision) through the helpers of tests/test_iso_indexed.py; polygon_bear has a 16^3 golden of its own."""
    import test_iso_indexed as iso
    if case != "polygon_bear":
        return iso.solved(shm, case, n, precision, slabs, **solve_kw)
    key = (case, n, precision, slabs)
    if key not in _CACHE:
        d = dict(load_golden("polygon_bear_n16"))
        assert n == 16 and slabs == 1
        s = shm.GridSolver(precision=shm.SHM_F64 if precision == 64 else shm.SHM_F32)
        s.set_problem(d["pos"], d["wnormal"], d["area"], float(d["lam"]), int(d["n"]), d["bbox_min"], float(d["cell"]))
        s.solve(**(dict(tol=1e-10) if precision == 64 else {}))
        phi = s.get_phi()[0]
        if precision == 32:
            phi = phi.astype(np.float32).astype(np.float64)
        _CACHE[key] = (d, s, phi)
    return _CACHE[key]


def isovalues(phi):
    import test_iso_indexed as iso
    return iso.isovalues(phi)


def dt(precision):
    return np.float64 if precision == 64 else np.float32


def same_infinities(a, b):
    fa, fb = np.isfinite(a), np.isfinite(b)
    return np.array_equal(fa, fb) and np.array_equal(a[~fa], b[~fb])


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("case,n", [("bunny_small", 16), ("bunny_small", 20), ("bunny_small", 33), ("polygon_bear", 16), ("bunny_pc", 24)])
def test_parity_with_the_restatement(shm, case, n, precision):
    d, s, phi = solved(shm, case, n, precision)
    h = float(d["cell"])
    for name, iso in isovalues(phi).items():
        st = s.redistance(iso)
        psi = s.get_redistanced()
        want, info = ref.redistance(phi, n, h, iso, dtype=dt(precision))
        assert same_infinities(psi, want), name
        fin = np.isfinite(want)
        lim = ref.tol(n, dt(precision), want)
        err = float(np.abs(psi[fin] - want[fin]).max()) if fin.any() else 0.0
        print("parity %s %d fp%d %s: err %.3e TOL %.3e max|psi| %.4g frozen %d rounds %d updates %d" % (
            case, n, precision, name, err, lim, info["max_abs"], st["n_frozen"], st["n_rounds"], st["n_block_updates"]))
        assert err <= lim, (name, err, lim)
        assert np.array_equal(psi < 0, phi - iso < 0), name
        assert st["n_frozen"] == info["n_frozen"] and st["n_reached"] == info["n_reached"] and st["n_nonfinite"] == 0, (name, st)
        assert abs(st["max_abs"] - info["max_abs"]) <= lim and st["isovalue"] == iso and st["band"] == INF
        assert st["n_rounds"] <= rounds_cap(n)
        if name in ("below", "above"):
            assert st["n_frozen"] == 0 and st["n_rounds"] == 0 and st["n_block_updates"] == 0
            assert (psi == (-INF if name == "above" else INF)).all()
        else:
            assert st["n_frozen"] > 0 and fin.all()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [64, 32])
def test_fixed_point(shm, precision):
    """Independently of the path the restatement takes: psi_dev is left where it is by one update, and its frozen nodes hold the init formula."""
    n = 33
    d, s, phi = solved(shm, "bunny_small", n, precision)
    h = float(d["cell"])
    for name in ("zero", "quarter_max", "box"):
        iso = isovalues(phi)[name]
        s.redistance(iso)
        u = np.abs(s.get_redistanced()).reshape(n, n, n)
        u0, frozen, wall = ref.frozen_init(phi.reshape(n, n, n) - iso, h, dt(precision))
        assert not wall.any() and np.isfinite(u).all()
        lim = ref.tol(n, dt(precision), u)
        t = ref.godunov(u, h)
        lowered = float((u - t)[~frozen].max())
        raised = float((t - u)[~frozen].max())
        e0 = float(np.abs(u - u0)[frozen].max())
        print("fixed point fp%d %s: one update lowers by %.3e, would raise by %.3e, frozen differ by %.3e (TOL %.3e)" % (precision, name, lowered, raised, e0, lim))
        assert lowered <= lim and e0 <= lim
        assert raised <= lim      # and every value is supported by its neighbours: nothing was left too low


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [64, 32])
def test_band(shm, precision):
    n = 33
    d, s, phi = solved(shm, "bunny_small", n, precision)
    h = float(d["cell"])
    iso = isovalues(phi)["quarter_max"]
    full_st = s.redistance(iso)
    full = s.get_redistanced()
    lim = ref.tol(n, dt(precision), full)
    for B in (1.5 * h, 6 * h):
        st = s.redistance(iso, band=B)
        psi = s.get_redistanced()
        Bt = float(dt(precision)(B))
        err = float(np.abs(psi - np.clip(full, -Bt, Bt)).max())
        print("band %.1f h fp%d: err %.3e TOL %.3e rounds %d (full %d, cap %d) updates %d (full %d) reached %d" % (
            B / h, precision, err, lim, st["n_rounds"], full_st["n_rounds"], rounds_cap(n), st["n_block_updates"], full_st["n_block_updates"], st["n_reached"]))
        assert err <= lim, (B, err, lim)
        assert st["band"] == B and st["n_reached"] == int((np.abs(full) < B).sum()) and st["max_abs"] < B
        assert st["n_block_updates"] < full_st["n_block_updates"]
        # well under the cap: a front crosses at most 3 ceil(n/8) blocks, one per round; a quarter of the cap leaves as much again for blocks revisited
        assert st["n_rounds"] <= rounds_cap(n) // 4 and full_st["n_rounds"] <= rounds_cap(n) // 4


@pytest.mark.gpu
def test_determinism(shm):
    d, s, phi = solved(shm, "bunny_small", 33)
    iso = isovalues(phi)["zero"]
    a_st = s.redistance(iso)
    a = s.get_redistanced()
    s.redistance(0.5 * iso + 0.1)   # another level in between: nothing of it may stay behind
    b_st = s.redistance(iso)
    b = s.get_redistanced()
    assert np.array_equal(a, b)
    a_st.pop("ms"), b_st.pop("ms")
    assert a_st == b_st


@pytest.mark.gpu
def test_slabs(shm):
    """psi does not depend on local_slabs.  Handles with 1, 2 and 3 slabs each solve for themselves, and their phi differ in the last bits (measured here:
    max|phi_2 - phi_1| = 9.3e-13 with one set of solver options; tests/test_iso_indexed.py met the same), so their psi cannot be the same bits (measured:
    3.2e-12 apart).  What can be held: every handle's psi is the restatement's of that handle's own phi to TOL (4e-15 here, hundreds of times finer than the
    difference between the handles, so a plane taken from the wrong slab cannot hide), with the same frozen count; and where two handles do hold the same
    phi, their psi are the same bits."""
    n = 20
    out = {}
    for slabs in (1, 2, 3):
        d, s, phi = solved(shm, "bunny_small", n, 64, slabs, solver="primal", precond="none", tol=1e-10)
        res = []
        for name in ("zero", "quarter_max", "box"):
            iso = isovalues(out[1][0] if 1 in out else phi)[name]   # one set of levels for the three handles
            st = s.redistance(iso)
            psi = s.get_redistanced()
            want, info = ref.redistance(phi, n, float(d["cell"]), iso)
            lim = ref.tol(n, np.float64, want)
            err = float(np.abs(psi - want).max())
            print("slabs %d %s: err %.3e TOL %.3e" % (slabs, name, err, lim))
            assert err <= lim and st["n_frozen"] == info["n_frozen"] and st["n_reached"] == n ** 3, (slabs, name, err, lim)
            st2 = s.redistance(iso)
            assert np.array_equal(s.get_redistanced(), psi) and st2["n_block_updates"] == st["n_block_updates"]   # two calls on a slabbed handle
            res.append(psi)
        out[slabs] = (phi, res)
    for slabs in (2, 3):
        dphi = float(np.abs(out[slabs][0] - out[1][0]).max())
        dpsi = max(float(np.abs(a - b).max()) for a, b in zip(out[slabs][1], out[1][1]))
        print("slabs %d against 1: max|dphi| %.3e max|dpsi| %.3e" % (slabs, dphi, dpsi))
        if dphi == 0.0:
            assert dpsi == 0.0 and all(np.array_equal(a, b) for a, b in zip(out[slabs][1], out[1][1]))


@pytest.mark.gpu
def test_state_and_errors(shm):
    import test_iso_indexed as iso_t
    d = iso_t.problem("bunny_small", 16)
    N = 16 ** 3
    s = shm.GridSolver()
    st = shm.ShmRedistanceStats()
    buf = np.full(N, -7.0)
    run = lambda iso=0.0, band=INF, p=None: s._lib.shm_grid_redistance(s._h, float(iso), float(band), p)   # noqa: E731
    get = lambda: s._lib.shm_grid_get_redistanced(s._h, buf.ctypes.data)                                    # noqa: E731
    getd = lambda: s._lib.shm_grid_get_redistanced_device(s._h, None)                                       # noqa: E731
    assert run() == SHM_ERR_STATE                            # no problem
    s.set_problem(d["pos"], d["wnormal"], d["area"], float(d["lam"]), int(d["n"]), d["bbox_min"], float(d["cell"]))
    assert run() == SHM_ERR_STATE                            # before a solve
    assert get() == SHM_ERR_STATE and getd() == SHM_ERR_STATE
    s.solve(tol=1e-10)
    assert get() == SHM_ERR_STATE and getd() == SHM_ERR_STATE   # a getter before a redistance
    for iso, band in ((float("nan"), INF), (INF, INF), (-INF, INF), (0.0, 0.0), (0.0, -1.0), (0.0, float("nan")), (0.0, -INF)):
        assert run(iso, band) == SHM_ERR_INVALID and s._lib.shm_grid_last_error(s._h)
    assert get() == SHM_ERR_STATE and (buf == -7).all()
    # everything derived from phi is left as it was
    phi = s.get_phi()[0]
    pts = np.asarray(d["bbox_min"]) + (np.random.default_rng(5).random((257, 3)) * 15.0) * float(d["cell"])
    smp = s.sample(pts, grad=True)
    V, F = s.isosurface_indexed(0.25 * phi.max())
    Vo, Fo = s.isosurface(0.0)
    t_ray = s.raycast(pts, np.ones_like(pts))[0]
    assert run(0.0, INF, C.byref(st)) == 0 and st.n_frozen > 0 and st.n_reached == N and st.n_nonfinite == 0 and st.n_rounds > 0 and st.ms > 0
    assert run() == 0                                        # out may be NULL
    assert get() == 0 and np.isfinite(buf).all()
    assert s._lib.shm_grid_get_redistanced(s._h, None) == SHM_ERR_INVALID and getd() == SHM_ERR_INVALID
    assert np.array_equal(s.get_phi()[0], phi)
    smp2 = s.sample(pts, grad=True)
    assert np.array_equal(smp2[0], smp[0]) and np.array_equal(smp2[1], smp[1]) and smp2[2] == smp[2]
    Vg, Fg = np.empty_like(V), np.empty_like(F)
    assert s._lib.shm_grid_get_isosurface_indexed(s._h, Vg.ctypes.data, Fg.ctypes.data) == 0        # the resident meshes are still there
    assert np.array_equal(Vg, V) and np.array_equal(Fg, F)
    Vg, Fg = np.empty_like(Vo), np.empty_like(Fo)
    assert s._lib.shm_grid_get_isosurface(s._h, Vg.ctypes.data, Fg.ctypes.data) == 0
    assert np.array_equal(Vg, Vo) and np.array_equal(Fg, Fo)
    V2, F2 = s.isosurface_indexed(0.25 * phi.max())
    assert np.array_equal(V2, V) and np.array_equal(F2, F)
    assert np.array_equal(s.raycast(pts, np.ones_like(pts))[0], t_ray, equal_nan=True)
    # a failed call leaves the resident psi alone; anything that replaces phi invalidates it
    psi = buf.copy()
    assert run(float("nan")) == SHM_ERR_INVALID and get() == 0 and np.array_equal(buf, psi)
    s.solve(tol=1e-10)
    assert get() == SHM_ERR_STATE and getd() == SHM_ERR_STATE
    assert run() == 0 and get() == 0 and np.array_equal(buf, psi)       # the same phi again: the same psi
    s.apply_laplacian(np.zeros(N))                            # a stage entry point that overwrites phi
    assert get() == SHM_ERR_STATE and run() == SHM_ERR_STATE
    s.solve(tol=1e-10)
    assert run() == 0
    s.set_problem(d["pos"], d["wnormal"], d["area"], float(d["lam"]), int(d["n"]), d["bbox_min"], float(d["cell"]))
    assert get() == SHM_ERR_STATE and getd() == SHM_ERR_STATE and run() == SHM_ERR_STATE
    header = open(os.path.join(ROOT, "include", "shm_grid.h")).read()
    for name in ("shm_grid_redistance", "shm_grid_get_redistanced", "shm_grid_get_redistanced_device"):
        assert hasattr(s._lib, name) and ("shm_status %s(" % name) in header and name in shm.grid_abi.ABI_SYMBOLS
    assert s._lib.shm_grid_abi_version() == 5 and "#define SHM_GRID_ABI_VERSION 5" in header
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [64, 32])
def test_device_getter(shm, precision):
    n = 20
    d, s, phi = solved(shm, "bunny_small", n, precision)
    N = n ** 3
    s.redistance(isovalues(phi)["box"], band=5 * float(d["cell"]))
    host = s.get_redistanced()
    dev = s.get_redistanced(device=True)
    assert dev.is_cuda and dev.shape == (N,) and dev.dtype == (torch.float64 if precision == 64 else torch.float32)
    assert np.array_equal(dev.cpu().numpy(), host.astype(dt(precision)))
    assert np.array_equal(host.astype(dt(precision)).astype(np.float64), host)       # the host getter promotes the handle's values
    # bad buffers: SHM_ERR_INVALID before anything is written (exact-size allocations of their own, as in tests/test_iso_indexed.py)
    hip = C.CDLL("libamdhip64.so")
    esz = 8 if precision == 64 else 4
    sizes = dict(ok=N * esz, short=(N - 1) * esz)
    ptr = {}
    for k, nbytes in sizes.items():
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
        assert hip.hipMemset(p, 0xA5, C.c_size_t(nbytes)) == 0
        ptr[k] = p
    assert hip.hipDeviceSynchronize() == 0
    host_buf = np.full(N, -7.0)
    get = s._lib.shm_grid_get_redistanced_device
    for p in (ptr["short"], host_buf.ctypes.data, None):
        assert get(s._h, p) == SHM_ERR_INVALID and s._lib.shm_grid_last_error(s._h)
    assert hip.hipDeviceSynchronize() == 0
    back = np.zeros(sizes["short"], dtype=np.uint8)
    assert hip.hipMemcpy(C.c_void_p(back.ctypes.data), ptr["short"], C.c_size_t(back.nbytes), 2) == 0   # hipMemcpyDeviceToHost
    assert (back == 0xA5).all() and (host_buf == -7).all()
    assert get(s._h, ptr["ok"]) == 0
    back = np.zeros(N, dtype=dt(precision))
    assert hip.hipMemcpy(C.c_void_p(back.ctypes.data), ptr["ok"], C.c_size_t(back.nbytes), 2) == 0
    assert np.array_equal(back, host.astype(dt(precision)))
    for p in ptr.values():
        assert hip.hipFree(p) == 0


@pytest.mark.gpu
def test_host_mirror_and_cli_equal_the_abi(shm, tmp_path):
    from signed_heat_3d_amd.host_abi import HostSolver
    obj = os.path.join(ROOT, "data", "bunny_small.obj")
    host = HostSolver(obj, tol=1e-10)
    phi, _ = host.compute_distance(hCoef=1.0)
    pre = host.preprocess(hCoef=1.0)
    s = shm.GridSolver()
    s.set_problem(pre["pos"], pre["wnormal"], pre["area"], pre["lam"], pre["n"], pre["bbox_min"], pre["cell"])
    s.solve(tol=1e-10)
    assert np.array_equal(s.get_phi()[0], phi)              # the same library on the same input
    iso, B = 0.25 * float(phi.max()), 7.5 * float(pre["cell"])
    for band in (INF, B):
        st = s.redistance(iso, band)
        psi_h, st_h = host.redistance(iso, band)
        assert np.array_equal(psi_h, s.get_redistanced())
        st.pop("ms"), st_h.pop("ms")
        assert st_h == st and st["n_frozen"] > 0
    exe = os.path.join(ROOT, "signed-heat-3d_amd", "bin", "shm_grid_cli")
    f_phi, f_psi = str(tmp_path / "phi.bin"), str(tmp_path / "psi.bin")
    p = subprocess.run([exe, obj, "--g", "--h", "1", "--tol", "1e-10", "--out", f_phi, "--iso", repr(iso), "--redistance", "--band", repr(B), "--out-psi", f_psi],
                       capture_output=True, text=True)
    assert p.returncode == 0 and "psi written to" in p.stderr, p.stderr
    assert np.array_equal(np.fromfile(f_phi), phi)
    assert np.array_equal(np.fromfile(f_psi), s.get_redistanced())
    p = subprocess.run([exe, obj, "--g", "--redistance"], capture_output=True, text=True)
    assert p.returncode != 0 and "go together" in p.stderr
    p = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert "--redistance" in p.stdout and "--out-psi" in p.stdout and "--band" in p.stdout
    host.close()
    s.close()


@pytest.mark.gpu
def test_two_ranks_are_refused(shm, tmp_path):
    """world = 2 through the librccl double: SHM_ERR_STATE on both ranks, with a message, and the ranks go on to finish (as for the ray casts)."""
    so = str(tmp_path / "librccl_mock.so")
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", os.path.join(ROOT, "tests", "native", "rccl_mock.c"), "-o", so, "-I/opt/rocm/include",
                           "-D__HIP_PLATFORM_AMD__", "-L/opt/rocm/lib", "-lamdhip64", "-lrt", "-lpthread"])
    uid = ("/shmmock_%d_rd_2" % os.getpid()).encode().ljust(128, b"\x00")
    log = open(tmp_path / "worker.log", "w+")
    p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "worker", "2", uid.hex(), "bunny_small_n16", str(tmp_path)],
                         env=dict(os.environ, SHM_RCCL_LIB=so), stdout=log, stderr=subprocess.STDOUT)
    try:
        p.wait(timeout=300)
    except subprocess.TimeoutExpired:
        p.kill()
        p.wait()
    log.seek(0)
    assert p.returncode == 0, log.read()
    for r in range(2):
        status, msg = open(tmp_path / ("rd_%d.txt" % r)).read().split("\n", 1)
        assert int(status) == SHM_ERR_STATE and "world > 1" in msg, (r, status, msg)


# ---- the worker of test_two_ranks_are_refused ------------------------------------------------------------------------------------------------------------------
def _worker(world, uid_hex, case, out_dir):
    import threading
    import traceback
    import shm_import
    shm = shm_import.load()

    def run_rank(rank):
        d = load_golden(case)
        s = shm.GridSolver(device=0, rank=rank, world=world, rccl_unique_id=bytes.fromhex(uid_hex))
        s.set_problem(d["pos"], d["wnormal"], d["area"], float(d["lam"]), int(d["n"]), d["bbox_min"], float(d["cell"]))
        s.solve(tol=1e-10)
        rc = s._lib.shm_grid_redistance(s._h, 0.0, INF, None)
        with open(os.path.join(out_dir, "rd_%d.txt" % rank), "w") as f:
            f.write("%d\n%s" % (rc, s._lib.shm_grid_last_error(s._h).decode()))
        s.sample(np.asarray(d["bbox_min"], dtype=np.float64).reshape(1, 3))   # the ranks are still in step: a collective call after the refusal completes
        s.close()

    def body(rank):
        try:
            run_rank(rank)
        except BaseException:
            # a failed rank leaves its peer waiting in a collective: report it and take the whole process down at once
            traceback.print_exc()
            sys.stdout.flush()
            sys.stderr.flush()
            os._exit(1)

    threads = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()


if __name__ == "__main__" and len(sys.argv) == 6 and sys.argv[1] == "worker":
    _worker(int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5])
