"""The indexed, welded marching-cubes mesh built on the device in a canonical order (shm_grid_isosurface_indexed and its two getters, include/shm_grid.h;
kernels in csrc/shm_iso_indexed.hip.h), through the kernels, the C ABI, the Python bindings, the C++ host mirror and the CLI.

References: a numpy restatement of the order and of the vertex formula (below), tests/iso_ref.py for the triangles, and the host-welded path
(shm_grid_isosurface), which the new path leaves untouched.  Indices and orders are always compared exactly.  Positions are held to
    B = max|bbox_min| + (n-1) cell;   8 * 2^-53 * B  against iso_ref (pos(a) + t (pos(b) - pos(a)): three roundings each way) and against the old device path
                                      (the same expressions: bit-equality is expected, the bound only forgives a different fused-multiply-add contraction);
                                      2^-23 * B  for fp32 device buffers against float32(old path): one more rounding."""
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

import iso_ref

pytestmark = pytest.mark.gpu

SHM_ERR_INVALID, SHM_ERR_STATE = 1, 7
ISO_NAMES = ["zero", "quarter_max", "box", "half_min", "below", "above"]


def isovalues(phi):
    """0 (closed), 0.25 max, 0.6 max (the surface runs into the box: edges owned by nodes with i, j, k = n-1), 0.5 min (a few dozen vertices), two empty."""
    lo, hi = float(phi.min()), float(phi.max())
    return dict(zip(ISO_NAMES, [0.0, 0.25 * hi, 0.6 * hi, 0.5 * lo, lo - 1.0, hi + 1.0]))


def problem(case, n):
    """The golden's sources on an n^3 grid over the golden's box: cell = 31 cell_32 / (n - 1) (16 and 32 are the goldens' own grids)."""
    d = dict(load_golden(case + "_n32"))
    if n == 16 and case == "bunny_small":
        return dict(load_golden("bunny_small_n16"))
    if n != 32:
        d["cell"] = 31.0 * float(d["cell"]) / (n - 1)
        d["n"] = n
    return d


def bound(d):
    return float(np.abs(d["bbox_min"]).max()) + (int(d["n"]) - 1) * float(d["cell"])


_CACHE = {}


def solved(shm, case, n, precision=64, slabs=1, **solve_kw):
    """(problem, handle, phi of the handle cast to its precision): one solve per configuration for the whole module."""
    key = (case, n, precision, slabs, tuple(sorted(solve_kw.items())))
    if key not in _CACHE:
        d = problem(case, n)
        s = shm.GridSolver(precision=shm.SHM_F64 if precision == 64 else shm.SHM_F32, local_slabs=slabs)
        s.set_problem(d["pos"], d["wnormal"], d["area"], float(d["lam"]), int(d["n"]), d["bbox_min"], float(d["cell"]))
        if slabs > 1:
            solve_kw = dict(dict(solver="primal", precond="none", tol=1e-10), **solve_kw)
        elif precision == 64:
            solve_kw = dict(dict(tol=1e-10), **solve_kw)
        s.solve(**solve_kw)
        phi = s.get_phi()[0]
        if precision == 32:
            phi = phi.astype(np.float32).astype(np.float64)   # the reference is fed the device's own input
        _CACHE[key] = (d, s, phi)
    return _CACHE[key]


# ---- the restatement: canonical vertex keys and positions of a plane range -----------------------------------------------------------------------------------
def restate_vertices(planes, n, kb, bbox_min, cell, iso):
    """planes: phi of the planes kb .. ktop (ktop = min(ke, n-1)), [nz, n, n].  Returns (keys ascending, positions): key = 3 g + axis, g = i + j n + k n^2."""
    P = np.asarray(planes, dtype=np.float64).reshape(-1, n, n)
    nz = P.shape[0]
    inside = P < iso
    k, j, i = np.meshgrid(np.arange(kb, kb + nz, dtype=np.int64), np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64), indexing="ij")
    g = i + j * n + k * n * n
    cx = np.zeros_like(inside)
    cy = np.zeros_like(inside)
    cz = np.zeros_like(inside)
    cx[:, :, :-1] = inside[:, :, :-1] != inside[:, :, 1:]
    cy[:, :-1, :] = inside[:, :-1, :] != inside[:, 1:, :]
    cz[:-1] = inside[:-1] != inside[1:]
    keys = np.sort(np.concatenate([3 * g[cx], 3 * g[cy] + 1, 3 * g[cz] + 2]))
    gg, ax = keys // 3, keys % 3
    ii, jj, kk = gg % n, (gg // n) % n, gg // (n * n)
    va = P[kk - kb, jj, ii]
    vb = P[kk - kb + (ax == 2), jj + (ax == 1), ii + (ax == 0)]
    tt = (iso - va) / (vb - va)
    pos = np.stack([ii * cell + bbox_min[0], jj * cell + bbox_min[1], kk * cell + bbox_min[2]], axis=1)
    pos[np.arange(len(keys)), ax] += tt * cell
    return keys, pos


_TRI_CACHE = {}


def restate_triangles(tag, planes, n, kb, bbox_min, cell, iso):
    """iso_ref.marching_cubes on the plane range, in its own iteration order ((k, j, i, tr) ascending): (triangles as vertex keys [nt, 3], positions [nt, 3, 3])."""
    if tag not in _TRI_CACHE:
        P = np.asarray(planes, dtype=np.float64).reshape(-1, n, n)
        pts, tris = iso_ref.marching_cubes(P.reshape(-1), n, bbox_min, cell, iso, nz=P.shape[0])
        off = kb * n * n   # iso_ref numbers the nodes from the range's first plane
        axis = {1: 0, n: 1, n * n: 2}
        K = np.array([[3 * (a + off) + axis[b - a] for (a, b) in t] for t in tris], dtype=np.int64).reshape(-1, 3)
        X = np.array([[pts[e] for e in t] for t in tris], dtype=np.float64).reshape(-1, 3, 3)
        _TRI_CACHE[tag] = (K, X)
    return _TRI_CACHE[tag]


def boundary_edges(F):
    e = np.sort(np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]]), axis=1)
    _, cnt = np.unique(e, axis=0, return_counts=True)
    return int((cnt == 1).sum())


def check_against_restatement(V, F, planes, n, kb, bbox_min, cell, iso, tol, tri_tag=None):
    keys, pos = restate_vertices(planes, n, kb, bbox_min, cell, iso)
    assert V.shape == (len(keys), 3)                                   # one vertex per cut edge ...
    if len(keys):
        err = float(np.abs(V - pos).max())
        assert err <= tol, (err, tol)                                   # ... in exactly the canonical order
    assert F.dtype == np.int64 and (F.size == 0) == (len(keys) == 0)
    if F.size:
        assert F.min() >= 0 and F.max() < len(keys)
        assert np.unique(F).size == len(keys)                           # every vertex is referenced
    if tri_tag is not None:
        K, X = restate_triangles(tri_tag, planes, n, kb, bbox_min, cell, iso)
        assert F.shape == K.shape
        if len(K):
            assert np.array_equal(keys[F], K)                           # the triangles, their order and the order of their corners
            if kb == 0:   # (iso_ref places a plane range at z = bbox_min: its positions are the grid's only for a range that starts at plane 0)
                err = float(np.abs(V[F] - X).max())
                assert err <= tol, (err, tol)
    return keys


# ---- A. canonical order against the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("n", [16, 32, 11, 33])
def test_canonical_order_matches_the_restatement(shm, n, precision):
    """Vertices in ascending 3 g + axis at the formula's positions, triangles as iso_ref lists them, at every isovalue; n = 11 and 33 leave partial waves
    and workgroups.  The box case must really reach the box: its mesh has boundary edges, the closed cases of the goldens' own grids have none."""
    d, s, phi = solved(shm, "bunny_small", n, precision)
    tol = 8 * 2.0 ** -53 * bound(d)
    for name, iso in isovalues(phi).items():
        V, F = s.isosurface_indexed(iso)
        assert V.dtype == np.float64 and F.dtype == np.int64
        keys = check_against_restatement(V, F, phi, n, 0, d["bbox_min"], float(d["cell"]), iso, tol, tri_tag=("A", n, precision, name))
        print("n %d fp%d %-11s iso %+.4f: %5d vertices %5d triangles, %d boundary edges" % (n, precision, name, iso, len(V), len(F), boundary_edges(F) if len(F) else 0))
        if name in ("below", "above"):
            assert len(V) == 0 and len(F) == 0
        else:
            assert len(keys) > 0
        if name == "box":
            assert boundary_edges(F) > 0
            gg = keys // 3
            assert ((gg % n == n - 1) | ((gg // n) % n == n - 1) | (gg // (n * n) == n - 1)).any()   # edges owned by nodes on the upper faces
        if name == "zero" and n in (16, 32):
            assert boundary_edges(F) == 0


# ---- B. against the host-welded path ----------------------------------------------------------------------------------------------------------------------------
def check_against_old_path(s, d, phi, iso, tol):
    Vo, Fo = s.isosurface(iso)
    V, F = s.isosurface_indexed(iso)
    assert V.shape == Vo.shape and F.shape == Fo.shape
    if len(F):
        err = float(np.abs(V[F] - Vo[Fo]).max())     # triangle by triangle, in order: the meshes differ by a renumbering of the vertices only
        assert err <= tol, (err, tol)
        # the renumbering is a bijection
        m = np.full(len(V), -1, dtype=np.int64)
        m[F.reshape(-1)] = Fo.reshape(-1)
        assert np.array_equal(m[F], Fo) and np.unique(m).size == len(V)
    return V, F


@pytest.mark.parametrize("case,n,precision", [("bunny_small", 32, 64), ("bunny_pc", 32, 64), ("bunny_small", 32, 32), ("bunny_small", 90, 64),
                                              ("bunny_small", 136, 32)])
def test_matches_the_host_welded_path(shm, case, n, precision):
    """The same handle, both paths.  n = 90: 729 000 nodes, hundreds of tiles in the totals scan; n = 136: more tiles than the scan has threads, so each
    thread owns a run of them.  Where the python loop of iso_ref is too slow the vectorised vertex restatement stands beside the old path."""
    d, s, phi = solved(shm, case, n, precision)
    tol = 8 * 2.0 ** -53 * bound(d)
    isos = isovalues(phi)
    for name in (ISO_NAMES if n == 32 else ["zero", "box", "above"]):
        V, F = check_against_old_path(s, d, phi, isos[name], tol)
        check_against_restatement(V, F, phi, n, 0, d["bbox_min"], float(d["cell"]), isos[name], tol)
        print("%s n %d fp%d %-11s: %d vertices %d triangles" % (case, n, precision, name, len(V), len(F)))
        if name in ("zero", "box"):
            assert len(F) > 0


# ---- C. independence of the slab plan -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [32, 33])
def test_result_does_not_depend_on_local_slabs(shm, n):
    """local_slabs 1, 3 and 5, solver="primal", precond="none" on every handle.  The surface must really cross a seam: counted per plane range of the
    slab plan (shm_plan_slab), the cut edges (seam planes counted on both sides) exceed those of the whole grid -- 582 against 572 at n = 32, iso 0, three slabs.

    The mesh is a function of phi, and the three handles do not hold the same phi: their solves sum their dot products in different orders and return
    phi that differ in the last bits (measured: max |phi_s - phi_1| = 4.7e-13 / 3.9e-13 at n = 32 and 7.1e-13 / 4.6e-13 at n = 33 for 3 / 5 slabs, and 1e-15 ... 1e-13
    with fast integration; no entry point puts a caller's field into the handle).  So V of two handles cannot be compared bit for bit.  What is held instead:
      * F is bit-identical to the one-slab F (numbering, triangle order and corner order do not depend on the slab plan);
      * V is the restatement of the handle's OWN phi in the canonical order, to 8 * 2^-53 * B, like the one-slab handle's (test A);
      * V differs from the one-slab V by no more than phi explains: tt = (iso - va) / (vb - va) with both nodes moved by at most d = max |phi_s - phi_1| moves by
        at most 3 d / |vb - va| to first order (held at 4 d / |vb - va|), so the vertex moves by at most cell times that, plus the two roundings' 8 * 2^-53 * B;
      * two builds on the multi-slab handle are bit-identical."""
    d, s1, phi1 = solved(shm, "bunny_small", n, 64, 1, solver="primal", precond="none", tol=1e-10)
    cell = float(d["cell"])
    tol = 8 * 2.0 ** -53 * bound(d)
    isos = isovalues(phi1)
    for name in ("zero", "box", "half_min"):
        iso = isos[name]
        V1, F1 = s1.isosurface_indexed(iso)
        keys1 = restate_vertices(phi1, n, 0, d["bbox_min"], cell, iso)[0]
        whole = len(keys1)
        assert whole == len(V1) > 0
        parts = {}
        for slabs in (3, 5):
            parts[slabs] = 0
            for sl in range(slabs):
                k0, k1 = shm.plan_slab(n, slabs, sl)
                parts[slabs] += len(restate_vertices(phi1.reshape(n, n, n)[k0:min(k1, n - 1) + 1], n, k0, d["bbox_min"], cell, iso)[0])
        # the closed surface at n = 33 lies between the seams of the three-slab plan (planes 11 and 22) and crosses those of the five-slab plan
        if name == "box" or (name == "zero" and n == 32):
            assert parts[3] > whole and parts[5] > whole, (parts, whole)
        elif name == "zero":
            assert parts[5] > whole, (parts, whole)
        # |vb - va| of every vertex's edge, from the one-slab phi
        gg, ax = keys1 // 3, keys1 % 3
        gap = np.abs(phi1[gg + np.where(ax == 0, 1, np.where(ax == 1, n, n * n))] - phi1[gg])
        for slabs in (3, 5):
            _, s, phi = solved(shm, "bunny_small", n, 64, slabs)
            V, F = s.isosurface_indexed(iso)
            dphi = float(np.abs(phi - phi1).max())
            print("n %d %-8s slabs %d: %d vertices (its plane ranges apart: %d, whole %d), max |phi - phi_1| = %.2e, max |V - V_1| = %.2e" %
                  (n, name, slabs, len(V), parts[slabs], whole, dphi, np.abs(V - V1).max() if V.shape == V1.shape else -1))
            check_against_restatement(V, F, phi, n, 0, d["bbox_min"], cell, iso, tol)
            assert np.array_equal(F, F1)
            assert V.shape == V1.shape
            moved = np.abs(V - V1).max(axis=1)
            assert (moved <= tol + cell * 4 * dphi / gap).all(), float((moved - cell * 4 * dphi / gap).max())
            V2, F2 = s.isosurface_indexed(iso)
            assert np.array_equal(V2, V) and np.array_equal(F2, F)


# ---- D. two ranks ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_two_ranks(shm, tmp_path, local_slabs=1):
    """world = 2 on one GPU through the shared-memory double of librccl (tests/iso_worker.py): each rank's piece is the restatement of its own plane range
    (its top cell layer reads the other rank's first plane from the ghost layer), and the two triangle lists in rank order are the one-process list.
    The two-rank solve is the gathered whole-grid one and returns the one-process phi bit for bit: so here -- unlike between the separate solves of
    test_result_does_not_depend_on_local_slabs -- the buffers have a common input, and every piece is held to the one-process buffers bit for bit."""
    so = str(tmp_path / "librccl_mock.so")
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", os.path.join(ROOT, "tests", "native", "rccl_mock.c"), "-o", so, "-I/opt/rocm/include",
                           "-D__HIP_PLATFORM_AMD__", "-L/opt/rocm/lib", "-lamdhip64", "-lrt", "-lpthread"])
    n = 32
    d, s1, phi1 = solved(shm, "bunny_small", n, 64)
    tol = 8 * 2.0 ** -53 * bound(d)
    isos = [0.0, 0.6 * float(phi1.max())]
    uid = ("/shmmock_%d_iso_2_%d" % (os.getpid(), local_slabs)).encode().ljust(128, b"\x00")
    log = open(tmp_path / "worker.log", "w+")
    p = subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "iso_worker.py"), "2", uid.hex(), "bunny_small_n32", ",".join(repr(v) for v in isos),
                          str(tmp_path), str(local_slabs)], env=dict(os.environ, SHM_RCCL_LIB=so), stdout=log, stderr=subprocess.STDOUT)
    try:
        p.wait(timeout=300)
    except subprocess.TimeoutExpired:
        p.kill()
        p.wait()
    log.seek(0)
    assert p.returncode == 0, log.read()
    ranges = [tuple(int(v) for v in np.load(tmp_path / ("meta_%d.npy" % r))) for r in range(2)]
    phi = np.concatenate([np.load(tmp_path / ("phi_%d.npy" % r)) for r in range(2)]).reshape(n, n, n)
    assert ranges[0][0] == 0 and ranges[0][1] == ranges[1][0] and ranges[1][1] == n
    print("two ranks: planes %s, max |phi - phi_1| = %.2e" % (ranges, np.abs(phi.reshape(-1) - phi1).max()))
    assert np.array_equal(phi.reshape(-1), phi1)   # (both come from the whole-grid solver; this is what lets the pieces be compared bit for bit below)
    for a, iso in enumerate(isos):
        V1, F1 = s1.isosurface_indexed(iso)
        keys1 = restate_vertices(phi1, n, 0, d["bbox_min"], float(d["cell"]), iso)[0]
        pieces = []
        for r, (kb, ke) in enumerate(ranges):
            V, F = np.load(tmp_path / ("V_%d_%d.npy" % (a, r))), np.load(tmp_path / ("F_%d_%d.npy" % (a, r)))
            planes = phi[kb:min(ke, n - 1) + 1]
            keys = check_against_restatement(V, F, planes, n, kb, d["bbox_min"], float(d["cell"]), iso, tol, tri_tag=("D", a, kb, ke))
            assert len(F) > 0
            pieces.append(keys[F])
            # the gathered two-rank solve returns the one-process phi bit for bit, so the piece is the one-process mesh restricted to the range, bit for bit
            assert np.array_equal(V, V1[np.searchsorted(keys1, keys)])
        assert np.array_equal(np.concatenate(pieces), keys1[F1])
        seam = np.intersect1d(np.unique(pieces[0]), np.unique(pieces[1]))
        assert len(seam) > 0                                            # seam vertices are duplicated between the ranks


# ---- E. device buffers ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [64, 32])
def test_device_buffers(shm, precision):
    d, s, phi = solved(shm, "bunny_small", 32, precision)
    B = bound(d)
    isos = isovalues(phi)
    for name in ("zero", "box"):
        iso = isos[name]
        Vh, Fh = s.isosurface_indexed(iso)
        V, F = s.isosurface_indexed(iso, device=True)
        assert V.is_cuda and F.is_cuda and F.dtype == torch.int64 and V.dtype == (torch.float64 if precision == 64 else torch.float32)
        assert np.array_equal(F.cpu().numpy(), Fh)
        if precision == 64:
            assert np.array_equal(V.cpu().numpy(), Vh)
        else:
            assert np.array_equal(V.cpu().numpy(), Vh.astype(np.float32))   # the fp64 position rounded once on the store
            Vo, Fo = s.isosurface(iso)
            err = float(np.abs(V.cpu().numpy().astype(np.float64)[Fh] - Vo.astype(np.float32).astype(np.float64)[Fo]).max())
            assert err <= 2.0 ** -23 * B, (err, 2.0 ** -23 * B)
        V2, F2 = s.isosurface_indexed(iso, device=True)
        assert torch.equal(V, V2) and torch.equal(F, F2)                   # two builds: bit-identical
        if precision == 64:
            # the vertices lie on the level set of the trilinear interpolant along their edge
            v, na = s.sample_device(V.contiguous())
            assert na == len(Vh)
            err = float((v - iso).abs().max())
            lim = 16 * 2.0 ** -53 * float(np.abs(phi).max())
            assert err <= lim, (err, lim)
    # bad buffers: SHM_ERR_INVALID before anything is written.  The buffers are exact-size device allocations of their own (a torch tensor sits in a
    # segment of the caching allocator, which may be larger than the tensor: the library bounds by the allocation), filled with a sentinel byte.
    Vh, Fh = s.isosurface_indexed(0.0)
    hip = C.CDLL("libamdhip64.so")
    esz = 8 if precision == 64 else 4
    sizes = dict(V=3 * len(Vh) * esz, F=3 * len(Fh) * 8, short_V=(3 * len(Vh) - 1) * esz, short_F=(3 * len(Fh) - 1) * 8)
    dev = {}
    for k, nbytes in sizes.items():
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
        assert hip.hipMemset(p, 0xA5, C.c_size_t(nbytes)) == 0
        dev[k] = p
    assert hip.hipDeviceSynchronize() == 0
    host_V = np.full(3 * len(Vh), -7.0)
    host_F = np.full(3 * len(Fh), -7, dtype=np.int64)
    get = s._lib.shm_grid_get_isosurface_indexed_device
    for pv, pf in [(dev["short_V"], dev["F"]), (dev["V"], dev["short_F"]), (host_V.ctypes.data, dev["F"]), (dev["V"], host_F.ctypes.data),
                   (None, dev["F"]), (dev["V"], None)]:
        assert get(s._h, pv, pf) == SHM_ERR_INVALID
        assert s._lib.shm_grid_last_error(s._h)
    assert hip.hipDeviceSynchronize() == 0
    for k, nbytes in sizes.items():
        back = np.zeros(nbytes, dtype=np.uint8)
        assert hip.hipMemcpy(C.c_void_p(back.ctypes.data), dev[k], C.c_size_t(nbytes), 2) == 0   # hipMemcpyDeviceToHost
        assert (back == 0xA5).all(), k
    assert (host_V == -7).all() and (host_F == -7).all()
    assert get(s._h, dev["V"], dev["F"]) == 0
    back = np.zeros(3 * len(Fh), dtype=np.int64)
    assert hip.hipMemcpy(C.c_void_p(back.ctypes.data), dev["F"], C.c_size_t(back.nbytes), 2) == 0
    assert np.array_equal(back.reshape(-1, 3), Fh)
    for p in dev.values():
        assert hip.hipFree(p) == 0


# ---- F. state -------------------------------------------------------------------------------------------------------------------------------------------------------
def test_state_rules(shm):
    d = problem("bunny_small", 16)
    s = shm.GridSolver()
    nv, nt = C.c_int64(-1), C.c_int64(-1)
    buf = np.zeros(8)
    ibuf = np.zeros(8, dtype=np.int64)
    build = lambda iso: s._lib.shm_grid_isosurface_indexed(s._h, float(iso), C.byref(nv), C.byref(nt))   # noqa: E731
    get = lambda: s._lib.shm_grid_get_isosurface_indexed(s._h, buf.ctypes.data, ibuf.ctypes.data)        # noqa: E731
    getd = lambda: s._lib.shm_grid_get_isosurface_indexed_device(s._h, None, None)                        # noqa: E731
    assert build(0.0) == SHM_ERR_STATE                      # no problem
    s.set_problem(d["pos"], d["wnormal"], d["area"], float(d["lam"]), int(d["n"]), d["bbox_min"], float(d["cell"]))
    assert build(0.0) == SHM_ERR_STATE                      # a build before a solve
    assert get() == SHM_ERR_STATE and getd() == SHM_ERR_STATE
    s.solve(tol=1e-10)
    assert get() == SHM_ERR_STATE and getd() == SHM_ERR_STATE   # a getter before a build
    phi = s.get_phi()[0]
    # empty surfaces: SHM_OK, 0, 0, and the getters accept NULL
    for iso in (phi.min() - 1.0, phi.max() + 1.0):
        assert build(iso) == 0 and nv.value == 0 and nt.value == 0
        assert s._lib.shm_grid_get_isosurface_indexed(s._h, None, None) == 0 and getd() == 0
    # the old path's resident mesh and the new one do not disturb each other
    Vo, Fo = s.isosurface(0.0)
    V, F = s.isosurface_indexed(0.25 * phi.max())
    Vo2 = np.empty_like(Vo)
    Fo2 = np.empty_like(Fo)
    assert s._lib.shm_grid_get_isosurface(s._h, Vo2.ctypes.data, Fo2.ctypes.data) == 0
    assert np.array_equal(Vo2, Vo) and np.array_equal(Fo2, Fo)
    Vo3, Fo3 = s.isosurface(0.0)
    assert np.array_equal(Vo3, Vo) and np.array_equal(Fo3, Fo)
    Vg = np.empty_like(V)
    Fg = np.empty_like(F)
    assert s._lib.shm_grid_get_isosurface_indexed(s._h, Vg.ctypes.data, Fg.ctypes.data) == 0        # still the new path's mesh after an old-path build
    assert np.array_equal(Vg, V) and np.array_equal(Fg, F)
    assert np.array_equal(s.get_phi()[0], phi)                                                      # phi is left as it was
    # anything that replaces phi invalidates the mesh
    s.solve(tol=1e-10)
    assert get() == SHM_ERR_STATE and getd() == SHM_ERR_STATE
    assert build(0.0) == 0 and nv.value == len(Vo) and nt.value == len(Fo)
    s.apply_laplacian(np.zeros(16 ** 3))                    # a stage entry point that overwrites q
    assert get() == SHM_ERR_STATE and build(0.0) == SHM_ERR_STATE
    s.solve(tol=1e-10)
    assert build(0.0) == 0
    s.set_problem(d["pos"], d["wnormal"], d["area"], float(d["lam"]), int(d["n"]), d["bbox_min"], float(d["cell"]))
    assert get() == SHM_ERR_STATE and getd() == SHM_ERR_STATE
    # the entry points are exported, declared, and the version stays 5
    header = open(os.path.join(ROOT, "include", "shm_grid.h")).read()
    for name in ("shm_grid_isosurface_indexed", "shm_grid_get_isosurface_indexed", "shm_grid_get_isosurface_indexed_device"):
        assert hasattr(s._lib, name) and ("shm_status %s(" % name) in header
    assert s._lib.shm_grid_abi_version() == 5 and "#define SHM_GRID_ABI_VERSION 5" in header
    s.close()


# ---- G. the C++ mirror and the CLI -----------------------------------------------------------------------------------------------------------------------------------
def test_host_mirror_equals_the_abi(shm):
    from signed_heat_3d_amd.host_abi import HostSolver
    host = HostSolver(os.path.join(ROOT, "data", "bunny_small.obj"), tol=1e-10)
    phi, _ = host.compute_distance(hCoef=1.0)
    pre = host.preprocess(hCoef=1.0)
    s = shm.GridSolver()
    s.set_problem(pre["pos"], pre["wnormal"], pre["area"], pre["lam"], pre["n"], pre["bbox_min"], pre["cell"])
    s.solve(tol=1e-10)
    assert np.array_equal(s.get_phi()[0], phi)              # the same library on the same input
    for iso in (0.0, 0.6 * float(phi.max())):
        V, F = s.isosurface_indexed(iso)
        Vh, Fh = host.isosurface_indexed(iso)
        assert len(F) > 0 and np.array_equal(Fh, F) and np.array_equal(Vh, V)
    host.close()
    s.close()


def _read_obj(path):
    V, F = [], []
    for line in open(path):
        t = line.split()
        if t and t[0] == "v":
            V.append([float(x) for x in t[1:4]])
        elif t and t[0] == "f":
            F.append([int(x.split("/")[0]) - 1 for x in t[1:4]])
    return np.array(V), np.array(F, dtype=np.int64)


def test_cli_iso_indexed(tmp_path):
    """--export with and without --iso-indexed: the same triangles as position triples in the same order.  At iso = 1 the level set of the 32^3 bunny is one
    sphere-like closed surface (F = 2 V - 4; at iso = 0 it is several closed pieces, each of which adds 4)."""
    exe = os.path.join(ROOT, "signed-heat-3d_amd", "bin", "shm_grid_cli")
    d = load_golden("bunny_small_n32")

    def run(iso, extra):
        obj = str(tmp_path / "out.obj")
        p = subprocess.run([exe, os.path.join(ROOT, "data", "bunny_small.obj"), "--g", "--h", "1", "--iso", iso, "--export", obj] + extra, capture_output=True, text=True)
        assert p.returncode == 0 and "Isosurface written to" in p.stderr, p.stderr
        return _read_obj(obj)
    Vo, Fo = run("0", [])
    V, F = run("0", ["--iso-indexed"])
    assert V.shape == Vo.shape and F.shape == Fo.shape and len(F) > 0
    assert float(np.abs(V[F] - Vo[Fo]).max()) <= 8 * 2.0 ** -53 * bound(d)
    assert (len(F) - 2 * len(V)) % 4 == 0 and boundary_edges(F) == 0          # closed pieces of genus 0
    assert (np.diff(V[:, 2]) >= -1.5 * float(d["cell"])).all()                # canonical order: the vertices ascend with their edge's lower node, z slowest
    V, F = run("1", ["--iso-indexed"])
    assert len(F) == 2 * len(V) - 4 and len(V) > 1000 and boundary_edges(F) == 0   # one closed genus-0 surface
    p = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert "--iso-indexed" in p.stdout
