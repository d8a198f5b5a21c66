"""Taubin smoothing and vertex normals of an indexed mesh on the device: shm_grid_smooth_mesh_device and shm_grid_get_isosurface_smoothed[_device]
(include/shm_grid.h; kernels in csrc/shm_mesh_smooth.hip.h), through the kernels, the C ABI, the Python bindings, the C++ host mirror and the CLI.

Reference: tests/mesh_smooth_ref.py, the numpy restatement that tests/test_mesh_smooth_host.py holds to the stage's promises.  Positions are compared bit for
bit: every neighbour sum is an integer sum, and everything around it is a handful of correctly rounded fp64 operations in a stated order.  Normals are
compared within 1 ulp per component (of the handle's precision): the device's sqrt and division are correctly rounded too, so 0 differing entries are
expected, and the count is printed.

Run as a script (`test_mesh_smooth.py worker <world> <uid hex> <case> <dir>`) this file is the worker of test_two_ranks_are_refused, as in
tests/test_iso_components.py."""
import ctypes as C
import itertools
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

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import ROOT, load_golden  # noqa: E402

import components_ref as cref  # noqa: E402
import mesh_smooth_ref as ref  # noqa: E402
from test_iso_components import isovalues, problem, solved, _read_obj  # noqa: E402

gpu = pytest.mark.gpu

SHM_ERR_INVALID, SHM_ERR_STATE = 1, 7


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def ulp_diff(a, b):
    """Entries of a and b (one float dtype) that differ, and whether every difference is at most 1 ulp."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    differ = ~((a == b) | (np.isnan(a) & np.isnan(b)))
    within = np.abs(a - b) <= np.spacing(np.maximum(np.abs(a), np.abs(b)))
    return int(differ.sum()), bool(within[differ].all())


def check_normals(N, want, tag):
    cnt, ok = ulp_diff(N, want)
    print("%s: normals differing from the restatement: %d of %d" % (tag, cnt, want.size))
    assert ok, tag


# ---- synthetic meshes ---------------------------------------------------------------------------------------------------------------------------------------------
def strip(nv, seed=0):
    rng = np.random.default_rng(seed)
    i = np.arange(nv)
    V = np.stack([0.5 * i, (i % 2).astype(np.float64), 0.0 * i], axis=1) + 0.2 * rng.standard_normal((nv, 3))
    t = np.arange(nv - 2)
    F = np.stack([t, np.where(t % 2 == 0, t + 1, t + 2), np.where(t % 2 == 0, t + 2, t + 1)], axis=1)
    return V, F.astype(np.int64)


def fan(k=4096, seed=1):
    """One vertex in k triangles: a closed ring of k vertices around vertex 0."""
    rng = np.random.default_rng(seed)
    a = 2 * np.pi * np.arange(k) / k
    ring = np.stack([np.cos(a), np.sin(a), 0.1 * rng.standard_normal(k)], axis=1)
    V = np.concatenate([[[0.03, -0.02, 0.5]], ring])
    r = 1 + np.arange(k)
    F = np.stack([np.zeros(k, dtype=np.int64), r, 1 + (np.arange(k) + 1) % k], axis=1)
    return V, F.astype(np.int64)


MESHES = {"one_triangle": lambda: (np.array([[0.0, 0, 0], [1.0, 0.25, 0], [0.125, 1.0, 0.5]]), np.array([[0, 1, 2]], dtype=np.int64)),
          "octahedron": lambda: (ref.OCTA_V.copy(), ref.OCTA_F.copy()), "fan4096": fan}
for _nv in (63, 64, 65, 255, 256, 257):
    MESHES["strip%d" % _nv] = (lambda m: lambda: strip(m))(_nv)


def shuffled(F, seed=7):
    rng = np.random.default_rng(seed)
    F2 = F[rng.permutation(len(F))]
    r = rng.integers(0, 3, len(F2))
    return np.stack([np.roll(t, int(k)) for t, k in zip(F2, r)]).astype(np.int64) if len(F2) else F2


@pytest.fixture(scope="module")
def handles(shm):
    hs = {64: shm.GridSolver(), 32: shm.GridSolver(precision=shm.SHM_F32)}
    yield hs
    for s in hs.values():
        s.close()


def device_smooth(s, V, F, it, mu, cap, alias, normals, fixed=None, lam=0.5):
    Vd = torch.from_numpy(np.ascontiguousarray(V)).cuda()                 # (V comes in the handle's dtype)
    Fd = torch.from_numpy(np.ascontiguousarray(F, dtype=np.int64)).cuda()
    fd = torch.from_numpy(np.ascontiguousarray(fixed, dtype=np.uint8)).cuda() if fixed is not None else None
    keep = Vd.clone()
    r = s.smooth_mesh_device(Vd, Fd, it, lam=lam, mu=mu, fixed=fd, max_displacement=cap, normals=normals, out=Vd if alias else None)
    X, N = r if normals else (r, None)
    if alias:
        assert X.data_ptr() == Vd.data_ptr()
    else:
        assert torch.equal(Vd, keep) or bool(torch.isnan(Vd).any())     # the input is only read
    return X.cpu().numpy(), (N.cpu().numpy() if normals else None)


@gpu
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("name", sorted(MESHES))
def test_synthetic_meshes(handles, name, precision):
    """Every launch and list edge: iterations 0, 1, 7; mu = 0 and -0.53; cap on and off; output aliasing the input; normals on and off; and a shuffled copy
    of the triangle list (permuted, corners rotated), which gives the same bits."""
    s = handles[precision]
    ft = np.float64 if precision == 64 else np.float32
    V, F = MESHES[name]()
    V = V.astype(ft)
    Vp = V.astype(np.float64)
    F2 = shuffled(F)
    edge = float(np.linalg.norm(Vp[F] - Vp[np.roll(F, 1, axis=1)], axis=2).mean())
    nd = 0
    for k, (it, mu, cap) in enumerate(itertools.product((0, 1, 7), (0.0, -0.53), (0.0, 0.1 * edge))):   # a tenth of the mean edge: the cap acts
        Xr, Nr = ref.smooth(Vp, F, it, mu=mu, max_displacement=cap, normals=True)
        Nr2 = ref.normals_of(Xr, F2)
        for alias, normals in itertools.product((False, True), (False, True)):
            X, N = device_smooth(s, V, F, it, mu, cap, alias, normals)
            assert bits_equal(X, Xr.astype(ft)), (name, it, mu, cap, alias, normals)
            if normals:
                c, ok = ulp_diff(N, Nr.astype(ft))
                nd += c
                assert ok, (name, it, mu, cap)
        X2, N2 = device_smooth(s, V, F2, it, mu, cap, k % 2 == 0, True)
        assert bits_equal(X2, Xr.astype(ft)), (name, it, mu, cap, "shuffled")
        c, ok = ulp_diff(N2, Nr2.astype(ft))
        nd += c
        assert ok
        if it == 7 and cap > 0:
            assert (np.linalg.norm(Xr - Vp, axis=1) > 0.999 * cap).any()   # the cap acts
    print("%s fp%d: nv %d nt %d; normal entries differing from the restatement: %d" % (name, precision, len(V), len(F), nd))


@gpu
def test_empty_meshes_and_special_vertices(handles):
    s = handles[64]
    z3, zf = np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64)
    X, N = device_smooth(s, z3, zf, 3, -0.53, 0.0, False, True)
    assert X.shape == (0, 3) and N.shape == (0, 3)
    V = np.random.default_rng(2).standard_normal((5, 3))
    X, N = device_smooth(s, V, zf, 3, -0.53, 0.1, False, True)
    assert bits_equal(X, V) and bits_equal(N, np.zeros((5, 3)))
    # NaN and infinite vertices, repeated corners, a lone vertex, duplicate triangles, fixed bits with -0
    V, F = strip(65, seed=4)
    V[7, 1] = np.nan
    V[20, 0] = np.inf
    V[33, 2] = -0.0
    V = np.concatenate([V, [[9.0, 9.0, 9.0]]])
    F = np.concatenate([F, [[3, 3, 4], [5, 6, 5], [40, 41, 42], [40, 41, 42], [11, 11, 11]]]).astype(np.int64)
    fixed = (np.arange(len(V)) % 8).astype(np.uint8)
    fixed[33] = 4
    for it, cap in ((0, 0.0), (1, 0.0), (7, 0.3)):
        Xr, Nr = ref.smooth(V, F, it, fixed=fixed, max_displacement=cap, normals=True)
        X, N = device_smooth(s, V, F, it, -0.53, cap, False, True, fixed=fixed)
        assert bits_equal(X, Xr)
        check_normals(N, Nr, "special vertices, %d iterations" % it)
        assert np.isnan(X[7, 1]) and np.isinf(X[20, 0]) and bits_equal(X[33, 2], V[33, 2]) and bits_equal(X[65], V[65])
        for a in range(3):
            m = (fixed >> a) & 1 == 1
            assert bits_equal(X[m, a], V[m, a])


# ---- the resident mesh ----------------------------------------------------------------------------------------------------------------------------------------------
CONFIGS = [(24, 64, 1), (32, 64, 3), (24, 32, 3), (32, 32, 1)]
_RESIDENT = {}


def resident(shm, n, precision, slabs):
    """(problem, handle, the handle's phi): the fp64 solve of bunny_small at n^3 made resident on a handle of the given precision and slab count."""
    d, s64, phi = solved(shm, "bunny_small", n, 64, 1)
    if (precision, slabs) == (64, 1):
        return d, s64, phi
    key = (n, precision, slabs)
    if key not in _RESIDENT:
        s = shm.GridSolver(precision=shm.SHM_F64 if precision == 64 else shm.SHM_F32, local_slabs=slabs)
        s.set_problem(d["pos"], d["wnormal"], d["area"], float(d["lam"]), int(d["n"]), d["bbox_min"], float(d["cell"]))
        s.set_phi(phi)
        _RESIDENT[key] = s
    s = _RESIDENT[key]
    return d, s, s.get_phi()[0]


def resident_checks(s, d, precision, tag, it=6, cap_cells=0.0):
    """The mesh in the slot: the resident entries (host and device, sliding or not) against the restatement of the fetched fp64 mesh, and against the device
    entry fed the fetched mesh and the touches_box mask."""
    n, cell = int(d["n"]), float(d["cell"])
    ft = np.float64 if precision == 64 else np.float32
    V, F = s.get_isosurface_indexed(*s._iso_counts)
    cap = cap_cells * cell
    mask = ref.box_mask(V, n, d["bbox_min"], cell)
    for slide in (True, False):
        fx = mask if slide else None
        Xr, Nr = ref.smooth(V, F, it, fixed=fx, max_displacement=cap, normals=True)
        X, N = s.isosurface_smoothed(it, max_displacement=cap, slide_on_box=slide, normals=True)
        assert bits_equal(X, Xr), (tag, slide)
        check_normals(N, Nr, "%s slide %d host" % (tag, slide))
        assert bits_equal(s.isosurface_smoothed(it, max_displacement=cap, slide_on_box=slide), X)           # two calls, and without normals
        Xd, Nd = s.isosurface_smoothed(it, max_displacement=cap, slide_on_box=slide, normals=True, device=True)
        assert Xd.is_cuda and bits_equal(Xd.cpu().numpy(), Xr.astype(ft))
        check_normals(Nd.cpu().numpy(), Nr.astype(ft), "%s slide %d device" % (tag, slide))
        if len(V):
            # the device entry fed the fetched mesh (rounded to the handle's precision there) and the mask
            Vf = V.astype(ft)
            Xg, Ng = device_smooth(s, Vf, F, it, -0.53, cap, False, True, fixed=fx)
            Xq, Nq = ref.smooth(Vf.astype(np.float64), F, it, fixed=fx, max_displacement=cap, normals=True)
            assert bits_equal(Xg, Xq.astype(ft))
            check_normals(Ng, Nq.astype(ft), "%s slide %d generic" % (tag, slide))
            if precision == 64:
                assert bits_equal(Xg, X) and bits_equal(Ng, N)
        if slide:
            for a in range(3):
                m = (mask >> a) & 1 == 1
                assert bits_equal(X[m, a], V[m, a])                                                         # every face coordinate is kept bitwise
    return V, F, mask


@gpu
@pytest.mark.parametrize("n,precision,slabs", CONFIGS)
def test_goldens(shm, n, precision, slabs):
    d, s, phi = resident(shm, n, precision, slabs)
    iso = isovalues(phi)
    pts = np.asarray(d["bbox_min"]) + float(d["cell"]) * np.random.default_rng(3).uniform(1, n - 2, (64, 3))
    dirs = np.random.default_rng(4).standard_normal((64, 3))
    for name in ("zero", "quarter_max", "box", "above"):
        s.isosurface_indexed(iso[name])
        before = [np.asarray(x) for x in s.closest_point(pts) + s.mesh_raycast(pts, dirs)] if len(s.get_isosurface_indexed(*s._iso_counts)[1]) else []
        V, F, mask = resident_checks(s, d, precision, "bunny_small %d^3 fp%d slabs %d %s" % (n, precision, slabs, name), cap_cells=0.5 if name == "quarter_max" else 0.0)
        if name == "above":
            assert len(V) == 0 and s.isosurface_smoothed(3, normals=True)[1].shape == (0, 3)
            assert s._lib.shm_grid_get_isosurface_smoothed(s._h, C.byref(shm.ShmSmoothOpts(3, 0, 0.5, -0.53, 0.0)), 1, None, None) == 0
        if name == "box":
            assert mask.any()                                                                                # the surface runs into the box
            free = s.isosurface_smoothed(6, slide_on_box=False)
            off = np.abs(free - V)[(mask[:, None] >> np.arange(3)) & 1 == 1].max() / float(d["cell"])
            print("unmasked, the rim leaves its face by %.3f cell" % off)
            assert off > 0
        # the slot was only read: the getters, closest_point and mesh_raycast answer as before
        V2, F2 = s.get_isosurface_indexed(len(V), len(F))
        assert bits_equal(V2, V) and bits_equal(F2, F)
        after = [np.asarray(x) for x in s.closest_point(pts) + s.mesh_raycast(pts, dirs)] if len(F) else []
        assert len(before) == len(after) and all(bits_equal(x, y) for x, y in zip(before, after))
    # after keep_largest
    s.isosurface_indexed(iso["zero"], keep_largest=1)
    V, F, _ = resident_checks(s, d, precision, "keep_largest")
    assert cref.boundary_edges(F) == 0
    # on a psi offset mesh
    s.redistance_exact(0.0)
    s.isosurface_indexed_psi(0.5 * float(d["cell"]))
    resident_checks(s, d, precision, "psi offset")
    s.isosurface_indexed(iso["zero"])


# ---- errors ---------------------------------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_limits_and_bad_buffers(handles, shm):
    """Each limit, a host pointer, a short allocation, and an index >= nv with the sentinel-filled outputs untouched.  Buffers are exact-size device allocations
    of their own (the library bounds by the allocation; a torch tensor sits in a larger segment of the caching allocator)."""
    s = handles[64]
    hip = C.CDLL("libamdhip64.so")
    V, F = strip(257, seed=8)
    nv, nt = len(V), len(F)

    def dev(arr=None, nbytes=None):
        nbytes = arr.nbytes if arr is not None else nbytes
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
        if arr is not None:
            assert hip.hipMemcpy(p, C.c_void_p(arr.ctypes.data), C.c_size_t(nbytes), 1) == 0
        else:
            assert hip.hipMemset(p, 0xA5, C.c_size_t(nbytes)) == 0
        return p

    def back(p, count, dt=np.float64):
        out = np.zeros(count, dtype=dt)
        assert hip.hipDeviceSynchronize() == 0
        assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), p, C.c_size_t(out.nbytes), 2) == 0
        return out
    sentinel = np.frombuffer(b"\xa5" * 8, dtype=np.float64)[0]
    O = shm.ShmSmoothOpts
    good = O(3, 0, 0.5, -0.53, 0.0)
    call = s._lib.shm_grid_smooth_mesh_device
    d_V, d_F, d_out, d_N, d_fix = dev(V), dev(F), dev(nbytes=24 * nv), dev(nbytes=24 * nv), dev(np.zeros(nv, dtype=np.uint8))
    untouched = lambda: (back(d_out, 3 * nv).tobytes() == back(d_N, 3 * nv).tobytes() == np.full(3 * nv, sentinel).tobytes())   # noqa: E731
    for o in (O(-1, 0, 0.5, -0.53, 0.0), O(1001, 0, 0.5, -0.53, 0.0), O(3, 0, 0.0, -0.53, 0.0), O(3, 0, 1.5, -0.53, 0.0), O(3, 0, np.nan, -0.53, 0.0),
              O(3, 0, 0.5, 0.1, 0.0), O(3, 0, 0.5, -1.5, 0.0), O(3, 0, 0.5, np.nan, 0.0), O(3, 0, 0.5, -0.53, -1.0), O(3, 0, 0.5, -0.53, np.inf),
              O(3, 0, 0.5, -0.53, np.nan)):
        assert call(s._h, nv, nt, d_V, d_F, None, C.byref(o), d_out, d_N) == SHM_ERR_INVALID and s._lib.shm_grid_last_error(s._h)
    assert call(s._h, nv, nt, d_V, d_F, None, None, d_out, d_N) == SHM_ERR_INVALID
    for a, b in ((-1, nt), (nv, -1), (2 ** 31, nt), (nv, 2 ** 31)):
        assert call(s._h, a, b, d_V, d_F, None, C.byref(good), d_out, d_N) == SHM_ERR_INVALID
    assert untouched()
    for bad_value, where in [(-1, (17, 1)), (nv, (nt - 1, 2)), (nv, (0, 0)), (2 ** 40, (100, 0)), (-2 ** 62, (5, 2))]:
        bad = F.copy()
        bad[where] = bad_value
        d_bad = dev(bad)
        assert call(s._h, nv, nt, d_V, d_bad, None, C.byref(good), d_out, d_N) == SHM_ERR_INVALID
        assert b"outside [0, nv)" in s._lib.shm_grid_last_error(s._h)
        assert untouched()
        assert hip.hipFree(d_bad) == 0
    assert call(s._h, 0, nt, None, d_F, None, C.byref(good), None, None) == SHM_ERR_INVALID                  # no vertex: every index is out of range
    host_V, host_F, host_out, host_fix = V.copy(), F.copy(), np.zeros((nv, 3)), np.zeros(nv, dtype=np.uint8)
    d_short, d_short_F, d_short_fix = dev(nbytes=24 * nv - 8), dev(nbytes=24 * nt - 8), dev(nbytes=nv - 1)
    for pv, pf, pfix, po, pn in [(host_V.ctypes.data, d_F, None, d_out, d_N), (d_V, host_F.ctypes.data, None, d_out, d_N), (d_V, d_F, host_fix.ctypes.data, d_out, d_N),
                                 (d_V, d_F, None, host_out.ctypes.data, d_N), (d_V, d_F, None, d_out, host_out.ctypes.data), (d_short, d_F, None, d_out, d_N),
                                 (d_V, d_short_F, None, d_out, d_N), (d_V, d_F, d_short_fix, d_out, d_N), (d_V, d_F, None, d_short, d_N), (d_V, d_F, None, d_out, d_short),
                                 (None, d_F, None, d_out, d_N), (d_V, None, None, d_out, d_N), (d_V, d_F, None, None, d_N)]:
        assert call(s._h, nv, nt, pv, pf, pfix, C.byref(good), po, pn) == SHM_ERR_INVALID and s._lib.shm_grid_last_error(s._h)
    assert untouched() and not host_out.any()
    # more than 2^20 incidences at one vertex
    k = (1 << 20) + 1
    big = np.stack([np.zeros(k, dtype=np.int64), 1 + np.arange(k) % 256, 1 + (np.arange(k) + 1) % 256], axis=1)
    d_big = dev(big)
    assert call(s._h, nv, k, d_V, d_big, None, C.byref(good), d_out, d_N) == SHM_ERR_INVALID and b"2^20" in s._lib.shm_grid_last_error(s._h)
    assert untouched()
    assert call(s._h, nv, k - 1, d_V, d_big, None, C.byref(O(1, 0, 0.5, 0.0, 0.0)), d_out, None) == 0      # at the limit: accepted
    # and the good call
    assert call(s._h, nv, nt, d_V, d_F, d_fix, C.byref(good), d_out, d_N) == 0
    Xr, Nr = ref.smooth(V, F, 3, normals=True)
    assert bits_equal(back(d_out, 3 * nv).reshape(-1, 3), Xr)
    check_normals(back(d_N, 3 * nv).reshape(-1, 3), Nr, "raw call")
    for p in (d_V, d_F, d_out, d_N, d_fix, d_short, d_short_F, d_short_fix, d_big):
        assert hip.hipFree(p) == 0


@gpu
def test_state_rules(shm):
    d = problem("bunny_small", 16)
    s = shm.GridSolver()
    o = shm.ShmSmoothOpts(2, 0, 0.5, -0.53, 0.0)
    buf = np.zeros((4096, 3))
    host = lambda oo=o, slide=1, p=buf.ctypes.data: s._lib.shm_grid_get_isosurface_smoothed(s._h, C.byref(oo), slide, p, None)     # noqa: E731
    devc = lambda: s._lib.shm_grid_get_isosurface_smoothed_device(s._h, C.byref(o), 1, None, None)                               # noqa: E731
    assert host() == SHM_ERR_STATE and devc() == SHM_ERR_STATE                                                                   # no problem
    s.set_problem(d["pos"], d["wnormal"], d["area"], float(d["lam"]), int(d["n"]), d["bbox_min"], float(d["cell"]))
    assert host() == SHM_ERR_STATE
    s.solve(tol=1e-10)
    assert host() == SHM_ERR_STATE and devc() == SHM_ERR_STATE                                                                   # no indexed mesh yet
    assert b"shm_grid_isosurface_indexed" in s._lib.shm_grid_last_error(s._h)
    V, F = s.isosurface_indexed(0.0)
    assert len(V) <= 4096 and host() == 0 and bits_equal(buf[:len(V)], ref.smooth(V, F, 2, fixed=ref.box_mask(V, 16, d["bbox_min"], float(d["cell"]))))
    assert host(p=None) == SHM_ERR_INVALID and devc() == SHM_ERR_INVALID                                                         # NULL for a non-empty mesh
    assert host(slide=2) == SHM_ERR_INVALID and host(oo=shm.ShmSmoothOpts(2, 0, 0.0, -0.53, 0.0)) == SHM_ERR_INVALID
    assert s._lib.shm_grid_get_isosurface_smoothed(s._h, None, 1, buf.ctypes.data, None) == SHM_ERR_INVALID
    assert s._lib.shm_grid_get_isosurface_smoothed_device(s._h, C.byref(o), 1, buf.ctypes.data, None) == SHM_ERR_INVALID         # a host pointer
    s.solve(tol=1e-10)                                                                                                           # a new solve
    assert host() == SHM_ERR_STATE and devc() == SHM_ERR_STATE
    s.isosurface_indexed(0.0)
    assert host() == 0
    # the generic entry needs no problem and no phi
    s2 = shm.GridSolver()
    X = device_smooth(s2, ref.OCTA_V, ref.OCTA_F, 1, 0.0, 0.0, False, False)[0]
    assert bits_equal(X, 0.5 * ref.OCTA_V)
    s2.close()
    header = open(os.path.join(ROOT, "include", "shm_grid.h")).read()
    for name in ("shm_grid_smooth_mesh_device", "shm_grid_get_isosurface_smoothed", "shm_grid_get_isosurface_smoothed_device"):
        assert hasattr(s._lib, name) and ("shm_status %s(" % name) in header and name in shm.grid_abi.ABI_SYMBOLS
    assert s._lib.shm_grid_abi_version() == 5 and "#define SHM_GRID_ABI_VERSION 5" in header and C.sizeof(shm.ShmSmoothOpts) == 32
    s.close()


@gpu
def test_two_ranks_are_refused(shm, tmp_path):
    """world = 2 through the librccl double: the resident entries are SHM_ERR_STATE on both ranks, the generic entry works there, and the ranks go on."""
    so = str(tmp_path / "librccl_mock.so")
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", os.path.join(ROOT, "tests", "native", "rccl_mock.c"), "-o", so, "-I/opt/rocm/include",
                           "-D__HIP_PLATFORM_AMD__", "-L/opt/rocm/lib", "-lamdhip64", "-lrt", "-lpthread"])
    uid = ("/shmmock_%d_smooth_2" % os.getpid()).encode().ljust(128, b"\x00")
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
        status, generic, msg = open(tmp_path / ("smooth_%d.txt" % r)).read().split("\n", 2)
        assert int(status) == SHM_ERR_STATE and "world > 1" in msg and generic == "ok", (r, status, generic, msg)


# ---- the other layers -------------------------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_host_mirror_equals_the_abi(shm):
    from signed_heat_3d_amd.host_abi import HostSolver
    host = HostSolver(os.path.join(ROOT, "data", "bunny_small.obj"), tol=1e-10)
    phi, _ = host.compute_distance(hCoef=1.0)
    pre = host.preprocess(hCoef=1.0)
    s = shm.GridSolver()
    s.set_problem(pre["pos"], pre["wnormal"], pre["area"], pre["lam"], pre["n"], pre["bbox_min"], pre["cell"])
    s.solve(tol=1e-10)
    assert np.array_equal(s.get_phi()[0], phi)
    for iso, kw in ((0.0, dict(keep_largest=1)), (0.6 * float(phi.max()), dict())):
        V, F = s.isosurface_indexed(iso, **kw)
        Vh, Fh = host.isosurface_indexed(iso, **kw)
        assert bits_equal(Vh, V) and bits_equal(Fh, F)
        for opts in (dict(iterations=10), dict(iterations=4, lam=0.6, mu=0.0, max_displacement=0.3 * pre["cell"], slide_on_box=False)):
            X, N = s.isosurface_smoothed(normals=True, **opts)
            Xh, Nh = host.isosurface_smoothed(normals=True, **opts)
            assert bits_equal(Xh, X) and bits_equal(Nh, N), (iso, opts)
            assert bits_equal(host.isosurface_smoothed(**opts), X)
    host.close()
    s.close()


@gpu
def test_cli_smooth(tmp_path, shm):
    from signed_heat_3d_amd.host_abi import HostSolver
    exe = os.path.join(ROOT, "signed-heat-3d_amd", "bin", "shm_grid_cli")
    mesh = os.path.join(ROOT, "data", "bunny_small.obj")

    def run(extra):
        obj = str(tmp_path / "out.obj")
        p = subprocess.run([exe, mesh, "--g", "--h", "1", "--iso", "0", "--export", obj, "--iso-indexed", "--keep-largest", "1"] + extra, capture_output=True, text=True)
        assert p.returncode == 0 and "Isosurface written to" in p.stderr, p.stderr
        vn = np.array([[float(x) for x in ln.split()[1:4]] for ln in open(obj) if ln.startswith("vn ")])
        return _read_obj(obj), vn
    (V, F), vn0 = run([])
    assert len(vn0) == 0                                                     # without the flag: today's output
    (X, F1), vn = run(["--smooth", "10"])
    (Xc, F2), vnc = run(["--smooth", "5", "--smooth-lambda", "0.6", "--smooth-mu", "0", "--smooth-cap", "0.01"])
    assert np.array_equal(F1, F) and np.array_equal(F2, F) and vn.shape == X.shape == V.shape and vnc.shape == V.shape
    host = HostSolver(mesh, tol=1e-10)
    host.compute_distance(hCoef=1.0)
    Vh, Fh = host.isosurface_indexed(0.0, keep_largest=1)
    assert np.array_equal(Fh, F) and np.array_equal(Vh, V)                   # (the OBJ carries 17 significant digits)
    Xh, Nh = host.isosurface_smoothed(iterations=10, normals=True)
    assert np.array_equal(X, Xh) and np.array_equal(vn, Nh)
    Xh, Nh = host.isosurface_smoothed(iterations=5, lam=0.6, mu=0.0, max_displacement=0.01, normals=True)
    assert np.array_equal(Xc, Xh) and np.array_equal(vnc, Nh)
    assert ref.roughness(X, F) < ref.roughness(V, F)
    host.close()
    p = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert all(f in p.stdout for f in ("--smooth <it>", "--smooth-lambda", "--smooth-mu", "--smooth-cap"))
    p = subprocess.run([exe, mesh, "--smooth", "3"], capture_output=True, text=True)
    assert p.returncode != 0 and "--iso-indexed" in p.stderr


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
        V, F = s.isosurface_indexed(0.0)                                     # (collective)
        buf = np.zeros((len(V) + 1, 3))
        o = shm.ShmSmoothOpts(2, 0, 0.5, -0.53, 0.0)
        rc = s._lib.shm_grid_get_isosurface_smoothed(s._h, C.byref(o), 1, buf.ctypes.data, None)
        msg = s._lib.shm_grid_last_error(s._h).decode()
        rc2 = s._lib.shm_grid_get_isosurface_smoothed_device(s._h, C.byref(o), 1, None, None)
        X = s.smooth_mesh_device(torch.from_numpy(ref.OCTA_V).cuda(), torch.from_numpy(ref.OCTA_F).cuda(), 1, mu=0.0)
        generic = "ok" if rc2 == rc and np.array_equal(X.cpu().numpy(), 0.5 * ref.OCTA_V) and not buf.any() else "bad"
        with open(os.path.join(out_dir, "smooth_%d.txt" % rank), "w") as f:
            f.write("%d\n%s\n%s" % (rc, generic, msg))
        s.sample(np.asarray(d["bbox_min"], dtype=np.float64).reshape(1, 3))   # the ranks are still in step: a collective call after the refusal completes
        s.close()

    def body(rank):
        try:
            run_rank(rank)
        except BaseException:
            # a failed rank leaves its peer waiting in a collective: report it and take the whole process down at once
            traceback.print_exc()
            sys.stdout.flush()
            os._exit(1)

    threads = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()


if __name__ == "__main__" and len(sys.argv) == 6 and sys.argv[1] == "worker":
    _worker(int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5])
