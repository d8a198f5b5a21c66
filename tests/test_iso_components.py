"""Connected components of the indexed isosurface on the device: shm_grid_label_mesh_device, shm_grid_isosurface_components and its getter,
shm_grid_isosurface_keep_components (include/shm_grid.h; kernels in csrc/shm_iso_components.hip.h), through the kernels, the C ABI, the Python bindings, the
C++ host mirror and the CLI.

Reference: tests/components_ref.py, a plain-numpy restatement (labels by min-propagation to the fixed point, records by the header's fixed-point formulas),
itself held to an independent breadth-first search on the goldens.  Labels, counts, lo / hi and every index are compared exactly.  Area and volume are
compared as their int64 images (value / quantum): one llrint per triangle may flip where the device's A_t or V_t differs from numpy's in the last bit, so the
images may differ by at most n_triangles; 0 is what is expected and what the tests print.

Run as a script (`test_iso_components.py worker <world> <uid hex> <case> <dir>`) this file is the worker of test_two_ranks_are_refused, as in
tests/test_redistance.py."""
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

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import ROOT, load_golden  # noqa: E402

import components_ref as cref  # noqa: E402
import iso_ref  # noqa: E402

gpu = pytest.mark.gpu

SHM_ERR_INVALID, SHM_ERR_STATE = 1, 7
ISO_NAMES = ["zero", "quarter_max", "box", "half_min", "below", "above"]


def isovalues(phi):
    """The six isovalues of tests/test_iso_indexed.py: 0, 0.25 max, 0.6 max (the surface runs into the box), 0.5 min (a few dozen vertices), two empty."""
    lo, hi = float(phi.min()), float(phi.max())
    return dict(zip(ISO_NAMES, [0.0, 0.25 * hi, 0.6 * hi, 0.5 * lo, lo - 1.0, hi + 1.0]))


def problem(case, n):
    """The golden's sources on an n^3 grid over the golden's box: cell = 31 cell_32 / (n - 1) (16 and 32 are the goldens' own grids)."""
    if n == 16 and case in ("bunny_small", "polygon_bear", "bunny_pc"):
        return dict(load_golden(case + "_n16"))
    d = dict(load_golden(case + "_n32"))
    if n != 32:
        d["cell"] = 31.0 * float(d["cell"]) / (n - 1)
        d["n"] = n
    return d


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
            phi = phi.astype(np.float32).astype(np.float64)
        _CACHE[key] = (d, s, phi)
    return _CACHE[key]


# ---- CPU: the restatement itself, on the goldens --------------------------------------------------------------------------------------------------------------
_MESH = {}


def golden_mesh(name, iso_name):
    """(V, F, golden) of the marching-cubes surface of a golden's phi in the canonical order, from tests/iso_ref.py: vertices ascend in 3 g + axis of their
    edge, triangles in iso_ref's own (cell, table position) order."""
    if (name, iso_name) not in _MESH:
        d = load_golden(name)
        n, cell, phi = int(d["n"]), float(d["cell"]), np.asarray(d["phi"], dtype=np.float64)
        iso = isovalues(phi)[iso_name]
        pts, tris = iso_ref.marching_cubes(phi, n, d["bbox_min"], cell, iso)
        axis = {1: 0, n: 1, n * n: 2}
        key = {e: 3 * e[0] + axis[e[1] - e[0]] for e in pts}
        order = sorted(pts, key=lambda e: key[e])
        vid = {e: a for a, e in enumerate(order)}
        V = np.array([pts[e] for e in order], dtype=np.float64).reshape(-1, 3)
        F = np.array([[vid[e] for e in t] for t in tris], dtype=np.int64).reshape(-1, 3)
        _MESH[(name, iso_name)] = (V, F, d)
    return _MESH[(name, iso_name)]


# golden at isovalue 0: vertices, triangles, components, triangles of the largest
TABLE = {"bunny_small_n24": (356, 660, 14, 476), "bunny_small_n32": (572, 1116, 10, 1004), "bunny_pc_n32": (626, 1184, 17, 1040),
         "polygon_bear_n16": (188, 364, 4, 316), "bunny_small_n16": (156, 312, 2, 304), "bunny_pc_n16": (174, 348, 2, 324)}


@pytest.mark.parametrize("name", sorted(TABLE))
def test_restatement_on_the_goldens(name):
    """roots() against the breadth-first search, the counts of the issue's table at isovalue 0, one component at 0.25 max, and what the records promise of a
    component that does not touch the box: it is closed, and its fixed-point volume does not depend on the origin by more than one quantum per triangle."""
    V, F, d = golden_mesh(name, "zero")
    n, cell = int(d["n"]), float(d["cell"])
    r = cref.roots(len(V), F)
    assert np.array_equal(r, cref.roots_bfs(len(V), F))
    rec, tcomp, vcomp, sa, sv = cref.records(V, F, n, d["bbox_min"], cell)
    print("%s iso 0: nv %d nt %d components %d largest %d, the rest %s" % (name, len(V), len(F), len(rec), rec["n_triangles"].max(),
                                                                         sorted(rec["n_triangles"].tolist())[:-1]))
    assert (len(V), len(F), len(rec), int(rec["n_triangles"].max())) == TABLE[name]
    assert (np.diff(rec["first_vertex"]) > 0).all() and rec["n_triangles"].sum() == len(F) and rec["n_vertices"].sum() == len(V)
    assert np.array_equal(rec["first_vertex"][vcomp], r)
    for c in range(len(rec)):
        assert rec["touches_box"][c] == 0                                   # every piece of the zero set lies inside the box ...
        Fc = F[tcomp == c]
        assert cref.boundary_edges(Fc) == 0                                 # ... and is closed
        own = cref.triangle_quanta(V, Fc, cell, V[rec["first_vertex"][c]])[1].sum()
        assert abs(int(own) - int(sv[c])) <= len(Fc), (c, own, sv[c])       # (measured: <= 5 quanta)
        assert rec["area"][c] > 0
    V, F, d = golden_mesh(name, "quarter_max")
    rec = cref.records(V, F, n, d["bbox_min"], cell)[0]
    assert len(rec) == 1 and len(F) > 0 and rec["volume"][0] > 0


@pytest.mark.parametrize("name", ["bunny_small_n16", "bunny_small_n32"])
def test_restatement_box_isovalue(name):
    V, F, d = golden_mesh(name, "box")
    rec, tcomp, _, _, _ = cref.records(V, F, int(d["n"]), d["bbox_min"], float(d["cell"]))
    big = int(np.argmax(rec["n_triangles"]))
    assert rec["touches_box"][big] == 1 and cref.boundary_edges(F[tcomp == big]) > 0


def test_restatement_small_cases():
    assert np.array_equal(cref.roots(5, np.zeros((0, 3), dtype=np.int64)), np.arange(5))
    assert np.array_equal(cref.roots(6, [[5, 4, 4], [1, 1, 1], [2, 4, 2]]), [0, 1, 2, 3, 2, 2])
    m = cref.largest_mask(np.array([(0, 3, 8, 0, 0, [0] * 3, [0] * 3, 0, 0), (3, 3, 9, 0, 0, [0] * 3, [0] * 3, 0, 0), (6, 3, 9, 0, 0, [0] * 3, [0] * 3, 0, 0)],
                                   dtype=cref.DTYPE), keep_largest=1)
    assert m.tolist() == [False, True, False]                               # ties: the smaller first_vertex


# ---- GPU, the generic entry: index arrays built in numpy, root compared exactly ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handle(shm):
    s = shm.GridSolver()
    yield s
    s.close()


def label(s, F, nv):
    t = torch.from_numpy(np.ascontiguousarray(F, dtype=np.int64)).cuda()
    root, nc = s.label_mesh_device(t, nv)
    root2, nc2 = s.label_mesh_device(t, nv)
    assert torch.equal(root, root2) and nc == nc2                           # two calls: bit-identical
    return root.cpu().numpy(), nc


def _bitrev(count):
    bits = int(count - 1).bit_length()
    key = np.array([int(format(a, "0%db" % bits)[::-1], 2) for a in range(count)])
    return np.argsort(key, kind="stable")


NT_STRIP = 70000


@gpu
@pytest.mark.parametrize("order", ["ascending", "descending", "bit_reversed", "permuted"])
def test_label_strip(handle, order):
    """One component through chains far longer than a wave or a workgroup."""
    nv = NT_STRIP + 2
    p = {"ascending": np.arange(nv), "descending": np.arange(nv)[::-1], "bit_reversed": _bitrev(nv),
         "permuted": np.random.default_rng(7).permutation(nv)}[order].astype(np.int64)
    F = np.stack([p[:-2], p[1:-1], p[2:]], axis=1)
    root, nc = label(handle, F, nv)
    assert nc == 1 and np.array_equal(root, np.zeros(nv, dtype=np.int64))
    assert np.array_equal(root, cref.roots(nv, F))


@gpu
def test_label_disjoint_triangles_and_isolated_vertices(handle):
    nt, iso = 50000, 1000
    nv = 3 * nt + iso
    p = np.random.default_rng(11).permutation(nv).astype(np.int64)
    F = p[:3 * nt].reshape(nt, 3)
    root, nc = label(handle, F, nv)
    want = cref.roots(nv, F)
    assert nc == nt + iso == np.unique(want).size
    assert np.array_equal(root, want)
    assert np.array_equal(root[p[3 * nt:]], p[3 * nt:])                     # a vertex in no triangle is its own component


@gpu
def test_label_star_on_the_largest_id(handle):
    """65 536 triangles share the vertex with the largest id: every hook contends for one root."""
    nt = 65536
    nv = 2 * nt + 1
    F = np.stack([np.full(nt, nv - 1), np.arange(nt), nt + np.arange(nt)], axis=1).astype(np.int64)
    root, nc = label(handle, F, nv)
    assert nc == 1 and not root.any()


@gpu
def test_label_duplicates_repeated_corners_and_empty(handle):
    F = np.array([[5, 4, 4], [1, 1, 1], [2, 4, 2], [5, 4, 4], [7, 8, 9], [9, 8, 7], [7, 8, 9]], dtype=np.int64)
    root, nc = label(handle, F, 11)
    assert np.array_equal(root, cref.roots(11, F)) and root.tolist() == [0, 1, 2, 3, 2, 2, 6, 7, 7, 7, 10] and nc == 7
    root, nc = label(handle, np.zeros((0, 3), dtype=np.int64), 9)           # nt = 0: nv components of one vertex each
    assert nc == 9 and np.array_equal(root, np.arange(9))
    root, nc = label(handle, np.zeros((0, 3), dtype=np.int64), 0)           # nv = 0
    assert nc == 0 and root.size == 0
    assert handle._lib.shm_grid_label_mesh_device(handle._h, 0, 0, None, None, None) == 0


@gpu
def test_label_refuses_bad_indices_and_bad_buffers(handle):
    """An index outside [0, nv): SHM_ERR_INVALID with the sentinel-filled root buffer untouched.  Buffers are exact-size device allocations of their own (a torch
    tensor sits in a segment of the caching allocator, which may be larger than the tensor: the library bounds by the allocation)."""
    s = handle
    hip = C.CDLL("libamdhip64.so")
    nv, nt = 1000, 4000
    rng = np.random.default_rng(3)
    good = rng.integers(0, nv, size=(nt, 3)).astype(np.int64)

    def dev(arr=None, nbytes=None):
        nbytes = arr.nbytes if arr is not None else nbytes
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
        if arr is not None:
            assert hip.hipMemcpy(p, C.c_void_p(arr.ctypes.data), C.c_size_t(nbytes), 1) == 0
        else:
            assert hip.hipMemset(p, 0xA5, C.c_size_t(nbytes)) == 0
        return p

    def back(p, count):
        out = np.zeros(count, dtype=np.int64)
        assert hip.hipDeviceSynchronize() == 0
        assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), p, C.c_size_t(out.nbytes), 2) == 0
        return out
    sentinel = np.frombuffer(b"\xa5" * 8, dtype=np.int64)[0]
    call = s._lib.shm_grid_label_mesh_device
    nc = C.c_int64(-1)
    d_root = dev(nbytes=8 * nv)
    d_good = dev(good)
    for bad_value, where in [(-1, (17, 1)), (nv, (nt - 1, 2)), (nv, (0, 0)), (2 ** 40, (2000, 0)), (-2 ** 62, (5, 2))]:
        bad = good.copy()
        bad[where] = bad_value
        d_bad = dev(bad)
        assert call(s._h, nv, nt, d_bad, d_root, C.byref(nc)) == SHM_ERR_INVALID
        assert b"outside [0, nv)" in s._lib.shm_grid_last_error(s._h)
        assert (back(d_root, nv) == sentinel).all()
        assert hip.hipFree(d_bad) == 0
    host_F = good.copy()
    host_root = np.full(nv, -7, dtype=np.int64)
    d_short_root = dev(nbytes=8 * nv - 8)
    d_short_F = dev(nbytes=24 * nt - 8)
    for pf, pr in [(host_F.ctypes.data, d_root), (d_good, host_root.ctypes.data), (d_good, d_short_root), (d_short_F, d_root), (None, d_root), (d_good, None)]:
        assert call(s._h, nv, nt, pf, pr, C.byref(nc)) == SHM_ERR_INVALID
        assert s._lib.shm_grid_last_error(s._h)
    assert call(s._h, -1, nt, d_good, d_root, C.byref(nc)) == SHM_ERR_INVALID
    assert call(s._h, nv, -1, d_good, d_root, C.byref(nc)) == SHM_ERR_INVALID
    assert (back(d_root, nv) == sentinel).all() and (host_root == -7).all() and (back(d_short_root, nv - 1) == sentinel).all()
    assert call(s._h, nv, nt, d_good, d_root, C.byref(nc)) == 0
    want = cref.roots(nv, good)
    assert np.array_equal(back(d_root, nv), want) and nc.value == np.unique(want).size
    for p in (d_root, d_good, d_short_root, d_short_F):
        assert hip.hipFree(p) == 0


# ---- GPU, the resident mesh ----------------------------------------------------------------------------------------------------------------------------------------
def check_records(s, d, iso, tag=""):
    """Build, label, fetch; hold everything to the restatement of the device's own fetched mesh.  Returns (V, F, rec, tcomp, vcomp)."""
    n, cell = int(d["n"]), float(d["cell"])
    V, F = s.isosurface_indexed(iso)
    rec, tc, vc = s.isosurface_components(labels=True)
    want, wtc, wvc, sa, sv = cref.records(V, F, n, d["bbox_min"], cell)
    assert rec.dtype == cref.DTYPE and len(rec) == len(want)
    for k in ("first_vertex", "n_vertices", "n_triangles", "touches_box", "reserved"):
        assert np.array_equal(rec[k], want[k]), k
    assert rec["lo"].tobytes() == want["lo"].tobytes() and rec["hi"].tobytes() == want["hi"].tobytes()      # bitwise the resident vertices' doubles
    assert np.array_equal(tc, wtc) and np.array_equal(vc, wvc) and tc.dtype == np.int64 and vc.dtype == np.int64
    qA, qV = cref.quanta(n, cell)
    da = np.abs(np.rint(rec["area"] / qA).astype(np.int64) - sa)
    dv = np.abs(np.rint(rec["volume"] / qV).astype(np.int64) - sv)
    print("%s iso %+.4f: %d vertices %d triangles %d components (largest %d); area / volume images differ by at most %d / %d quanta" %
          (tag, iso, len(V), len(F), len(rec), rec["n_triangles"].max() if len(rec) else 0, da.max() if len(rec) else 0, dv.max() if len(rec) else 0))
    assert (da <= rec["n_triangles"]).all() and (dv <= rec["n_triangles"]).all()
    assert (np.diff(rec["first_vertex"]) > 0).all()                         # records ascend in first_vertex
    assert rec["n_triangles"].sum() == len(F) and rec["n_vertices"].sum() == len(V)
    rec2, tc2, vc2 = s.isosurface_components(labels=True)                   # two calls: bit-identical
    assert rec2.tobytes() == rec.tobytes() and np.array_equal(tc2, tc) and np.array_equal(vc2, vc)
    return V, F, rec, tc, vc


CASES = [("bunny_small", 16), ("bunny_small", 20), ("bunny_small", 24), ("bunny_small", 33), ("polygon_bear", 16), ("bunny_pc", 24), ("bunny_pc", 32)]


@gpu
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("case,n", CASES)
def test_records_match_the_restatement(shm, case, n, precision):
    d, s, phi = solved(shm, case, n, precision)
    for name, iso in isovalues(phi).items():
        V, F, rec, tc, vc = check_records(s, d, iso, "%s n %d fp%d %-11s" % (case, n, precision, name))
        if name in ("below", "above"):
            assert len(rec) == 0 and len(V) == 0
        else:
            assert len(rec) >= 1
        if name == "box":
            big = int(np.argmax(rec["n_triangles"]))
            assert rec["touches_box"][big] == 1 and cref.boundary_edges(F[tc == big]) > 0
        if name == "quarter_max" and precision == 64:
            assert rec["volume"][int(np.argmax(rec["n_triangles"]))] > 0      # a blob of inside
        for c in np.flatnonzero(rec["touches_box"] == 0):
            assert cref.boundary_edges(F[tc == c]) == 0


@gpu
def test_many_components_at_isovalue_zero(shm):
    """bunny_small 24^3 at isovalue 0: 14 components on the golden phi -- a shell and a cloud of closed specks.  The count asserted is the restatement's on the
    device's own phi."""
    d, s, phi = solved(shm, "bunny_small", 24, 64)
    V, F, rec, tc, vc = check_records(s, d, 0.0, "bunny_small n 24")
    n = 24
    pts, tris = iso_ref.marching_cubes(phi, n, d["bbox_min"], float(d["cell"]), 0.0)
    ids = {e: a for a, e in enumerate(sorted(pts))}
    want = np.unique(cref.roots(len(ids), np.array([[ids[e] for e in t] for t in tris], dtype=np.int64))).size
    assert len(rec) == want >= 10, (len(rec), want)
    assert rec["n_triangles"].max() > 0.5 * len(F) and (np.sort(rec["n_triangles"])[:-1] <= 64).all()


def masks(rec):
    nc = len(rec)
    big = int(np.lexsort((rec["first_vertex"], -rec["n_triangles"]))[0]) if nc else 0
    only = np.zeros(nc, dtype=np.uint8)
    if nc:
        only[big] = 1
    return {"all": np.ones(nc, dtype=np.uint8), "none": np.zeros(nc, dtype=np.uint8), "largest": only, "all_but_largest": 1 - only,
            "alternating": (np.arange(nc) % 2).astype(np.uint8) * 3}       # (any non-zero byte keeps)


@gpu
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("case,n,iso_name", [("bunny_small", 24, "zero"), ("bunny_pc", 32, "zero"), ("bunny_small", 33, "box"), ("bunny_small", 16, "above")])
def test_keep_components(shm, case, n, iso_name, precision):
    d, s, phi = solved(shm, case, n, precision)
    iso = isovalues(phi)[iso_name]
    V, F, rec, tc, vc = check_records(s, d, iso, "%s n %d fp%d" % (case, n, precision))
    for name, mask in masks(rec).items():
        s.isosurface_indexed(iso)
        assert len(s.isosurface_components()) == len(rec)
        nv2, nt2 = s.isosurface_keep(mask)
        Vw, Fw = cref.keep_mesh(V, F, vc, tc, mask)
        assert (nv2, nt2) == (len(Vw), len(Fw)), name
        Vk, Fk = s.get_isosurface_indexed(nv2, nt2)
        assert np.array_equal(Fk, Fw) and Vk.tobytes() == Vw.tobytes(), name                 # indices exactly, positions bitwise
        Vd, Fd = s.get_isosurface_indexed(nv2, nt2, device=True)
        assert np.array_equal(Fd.cpu().numpy(), Fw)
        assert Vd.cpu().numpy().tobytes() == (Vw if precision == 64 else Vw.astype(np.float32)).tobytes(), name
        # the survivors: the same integers
        assert s._lib.shm_grid_get_isosurface_components(s._h, None, None, None) == SHM_ERR_STATE   # the records were dropped
        rec2, tc2, vc2 = s.isosurface_components(labels=True)
        kept = np.flatnonzero(mask)
        assert len(rec2) == len(kept)
        for k in ("n_vertices", "n_triangles", "touches_box"):
            assert np.array_equal(rec2[k], rec[k][kept]), (name, k)
        for k in ("area", "volume", "lo", "hi"):
            assert rec2[k].tobytes() == rec[k][kept].tobytes(), (name, k)
        newid = np.cumsum(mask[vc] != 0) - 1
        assert np.array_equal(rec2["first_vertex"], newid[rec["first_vertex"][kept]])
        assert np.array_equal(tc2, np.searchsorted(kept, tc[mask[tc] != 0])) and np.array_equal(vc2, np.searchsorted(kept, vc[mask[vc] != 0]))
        print("%s n %d fp%d %-15s: %d of %d components, %d of %d triangles kept" % (case, n, precision, name, len(kept), len(rec), nt2, len(F)))
    Vf, Ff = s.isosurface_indexed(iso)                                       # a rebuild returns the full mesh
    assert np.array_equal(Ff, F) and Vf.tobytes() == V.tobytes()


@gpu
@pytest.mark.parametrize("slabs", [1, 2, 3])
def test_local_slabs(shm, slabs):
    """Each handle is held to the restatement of its own mesh (the handles' phi differ in the last bits: tests/test_iso_indexed.py, test C)."""
    d, s, phi = solved(shm, "bunny_small", 24, 64, slabs, solver="primal", precond="none", tol=1e-10)
    isos = isovalues(phi)
    for name in ("zero", "box"):
        V, F, rec, tc, vc = check_records(s, d, isos[name], "slabs %d %-4s" % (slabs, name))
        assert len(rec) >= 1
    mask = masks(rec)["largest"]
    nv2, nt2 = s.isosurface_keep(mask)
    Vw, Fw = cref.keep_mesh(V, F, vc, tc, mask)
    Vk, Fk = s.get_isosurface_indexed(nv2, nt2)
    assert np.array_equal(Fk, Fw) and Vk.tobytes() == Vw.tobytes()


@gpu
def test_state_and_error_rules(shm):
    d = problem("bunny_small", 16)
    s = shm.GridSolver()
    nc, nv, nt = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    comps = lambda: s._lib.shm_grid_isosurface_components(s._h, C.byref(nc))                                   # noqa: E731
    get = lambda p=None: s._lib.shm_grid_get_isosurface_components(s._h, p, None, None)                       # noqa: E731
    keep = lambda p=None: s._lib.shm_grid_isosurface_keep_components(s._h, p, C.byref(nv), C.byref(nt))       # noqa: E731
    assert comps() == SHM_ERR_STATE and get() == SHM_ERR_STATE and keep() == SHM_ERR_STATE                    # no problem
    s.set_problem(d["pos"], d["wnormal"], d["area"], float(d["lam"]), int(d["n"]), d["bbox_min"], float(d["cell"]))
    assert comps() == SHM_ERR_STATE
    s.solve(tol=1e-10)
    assert get() == SHM_ERR_STATE and keep() == SHM_ERR_STATE and comps() == SHM_ERR_STATE                    # no indexed mesh yet
    assert b"shm_grid_isosurface_indexed" in s._lib.shm_grid_last_error(s._h)
    phi = s.get_phi()[0]
    V, F = s.isosurface_indexed(0.0)
    assert get() == SHM_ERR_STATE and keep() == SHM_ERR_STATE                                                 # a mesh, no labelling yet
    assert comps() == 0 and nc.value >= 1
    buf = np.zeros(nc.value, dtype=cref.DTYPE)
    assert get(None) == SHM_ERR_INVALID and keep(None) == SHM_ERR_INVALID                                     # NULL with a positive count
    assert get(buf.ctypes.data) == 0 and buf["n_triangles"].sum() == len(F)
    assert s._lib.shm_grid_isosurface_components(s._h, None) == 0                                             # the count is optional
    # an empty mesh: SHM_OK with 0 components, NULL accepted everywhere
    for iso in (phi.min() - 1.0, phi.max() + 1.0):
        s.isosurface_indexed(iso)
        assert get() == SHM_ERR_STATE                                                                         # a rebuild drops the labelling
        assert comps() == 0 and nc.value == 0 and get(None) == 0
        assert keep(None) == 0 and nv.value == 0 and nt.value == 0
        assert s._lib.shm_grid_get_isosurface_indexed(s._h, None, None) == 0
    # a filter drops the labelling, the mesh stays
    s.isosurface_indexed(0.0)
    assert comps() == 0
    mask = np.ones(nc.value, dtype=np.uint8)
    assert keep(mask.ctypes.data) == 0 and (nv.value, nt.value) == (len(V), len(F))
    assert get(buf.ctypes.data) == SHM_ERR_STATE and keep(mask.ctypes.data) == SHM_ERR_STATE
    assert comps() == 0
    # anything that replaces or invalidates phi
    s.solve(tol=1e-10)
    assert comps() == SHM_ERR_STATE and get(buf.ctypes.data) == SHM_ERR_STATE
    s.isosurface_indexed(0.0)
    assert comps() == 0
    s.apply_laplacian(np.zeros(16 ** 3))
    assert comps() == SHM_ERR_STATE and get(buf.ctypes.data) == SHM_ERR_STATE and keep(mask.ctypes.data) == SHM_ERR_STATE
    s.solve(tol=1e-10)
    s.isosurface_indexed(0.0)
    assert comps() == 0
    s.set_problem(d["pos"], d["wnormal"], d["area"], float(d["lam"]), int(d["n"]), d["bbox_min"], float(d["cell"]))
    assert comps() == SHM_ERR_STATE and get(buf.ctypes.data) == SHM_ERR_STATE
    # declared, exported, and the version stays 5
    header = open(os.path.join(ROOT, "include", "shm_grid.h")).read()
    for name in ("shm_grid_label_mesh_device", "shm_grid_isosurface_components", "shm_grid_get_isosurface_components", "shm_grid_isosurface_keep_components"):
        assert hasattr(s._lib, name) and ("shm_status %s(" % name) in header and name in shm.grid_abi.ABI_SYMBOLS
    assert s._lib.shm_grid_abi_version() == 5 and C.sizeof(shm.ShmIsoComponent) == 96 == cref.DTYPE.itemsize
    s.close()


@gpu
def test_everything_else_is_left_as_it_was(shm):
    """One sample, psi, a ray cast and the soup mesh, bit-identical before and after labelling and filtering."""
    d = problem("bunny_small", 16)
    s = shm.GridSolver()
    s.set_problem(d["pos"], d["wnormal"], d["area"], float(d["lam"]), int(d["n"]), d["bbox_min"], float(d["cell"]))
    s.solve(tol=1e-10)
    n, cell, b = int(d["n"]), float(d["cell"]), np.asarray(d["bbox_min"], dtype=np.float64)
    pts = b[None, :] + cell * np.array([[3.3, 7.1, 8.6], [9.5, 4.4, 2.2]])
    org = np.array([[b[0] - cell, b[1] + 7.3 * cell, b[2] + 7.9 * cell]])
    s.redistance(0.0)
    s.isosurface_indexed(0.0)

    def snapshot():
        Vs, Fs = np.empty((len(soup[0]), 3)), np.empty((len(soup[1]), 3), dtype=np.int64)
        assert s._lib.shm_grid_get_isosurface(s._h, Vs.ctypes.data, Fs.ctypes.data) == 0
        return [s.get_phi()[0], s.sample(pts, grad=True)[0], s.sample(pts, grad=True)[1], s.get_redistanced(), s.raycast(org, np.array([[1.0, 0.0, 0.0]]), grad=True)[0],
                Vs, Fs, s.get_field(s.FIELD_Y0)]
    soup = s.isosurface(0.0)
    before = snapshot()
    rec = s.isosurface_components()
    s.isosurface_keep(masks(rec)["largest"])
    s.isosurface_components()
    after = snapshot()
    for x, y in zip(before, after):
        assert x.tobytes() == y.tobytes()
    s.close()


@gpu
def test_python_conveniences(shm):
    d, s, phi = solved(shm, "bunny_small", 24, 64)
    V, F = s.isosurface_indexed(0.0)
    rec, tc, vc = s.isosurface_components(labels=True)
    assert len(rec) >= 2
    for kw in (dict(keep_largest=1), dict(keep_largest=3), dict(min_triangles=16), dict(keep_largest=2, min_triangles=10 ** 6), dict(keep_largest=0)):
        mask = cref.largest_mask(rec, **kw)
        assert np.array_equal(shm.largest_components_mask(rec, **kw) != 0, mask)
        Vw, Fw = cref.keep_mesh(V, F, vc, tc, mask)
        Vk, Fk = s.isosurface_indexed(0.0, **kw)
        assert np.array_equal(Fk, Fw) and Vk.tobytes() == Vw.tobytes(), kw
        Vd, Fd = s.isosurface_indexed(0.0, device=True, **kw)
        assert Vd.is_cuda and np.array_equal(Fd.cpu().numpy(), Fw) and Vd.cpu().numpy().tobytes() == Vw.tobytes()
    Vk, Fk = s.isosurface_indexed(0.0, keep_largest=1)
    assert cref.boundary_edges(Fk) == 0 and len(np.unique(cref.roots(len(Vk), Fk))) == 1 and len(Fk) == rec["n_triangles"].max()
    V2, F2 = s.isosurface_indexed(0.0)                                       # the defaults: today's behaviour
    assert np.array_equal(F2, F) and V2.tobytes() == V.tobytes()
    # the resident mesh labelled through the generic entry gives the records' names
    Fd = s.isosurface_indexed(0.0, device=True)[1]
    root, nc = s.label_mesh_device(Fd, len(V))
    assert nc == len(rec) and np.array_equal(root.cpu().numpy(), rec["first_vertex"][vc])


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
    for iso in (0.0, 0.6 * float(phi.max())):
        s.isosurface_indexed(iso)
        rec = s.isosurface_components()
        assert len(rec) >= 1 and host.isosurface_components(iso).tobytes() == rec.tobytes()
        for kw in (dict(keep_largest=1), dict(min_triangles=20), dict(keep_largest=2, min_triangles=9)):
            V, F = s.isosurface_indexed(iso, **kw)
            Vh, Fh = host.isosurface_indexed(iso, **kw)
            assert np.array_equal(Fh, F) and Vh.tobytes() == V.tobytes(), (iso, kw)
    assert len(s.isosurface_indexed(0.0, keep_largest=1)[1]) < len(s.isosurface_indexed(0.0)[1])   # (the 32^3 bunny carries specks at isovalue 0)
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


@gpu
def test_cli_keep_largest(tmp_path):
    import re
    exe = os.path.join(ROOT, "signed-heat-3d_amd", "bin", "shm_grid_cli")

    def run(extra):
        obj = str(tmp_path / "out.obj")
        p = subprocess.run([exe, os.path.join(ROOT, "data", "bunny_small.obj"), "--g", "--h", "1", "--iso", "0", "--export", obj, "--iso-indexed"] + extra,
                           capture_output=True, text=True)
        assert p.returncode == 0 and "Isosurface written to" in p.stderr, p.stderr
        lines = re.findall(r"^component (\d+): first_vertex (\d+) nv (\d+) nt (\d+) area (\S+) volume (\S+) touches_box ([01])$", p.stderr, flags=re.M)
        return _read_obj(obj), lines
    (V, F), none = run([])
    assert not none                                                          # without the flags: today's output
    (V1, F1), lines = run(["--keep-largest", "1"])
    assert len(lines) >= 2 and [int(x[0]) for x in lines] == list(range(len(lines)))
    nts = [int(x[3]) for x in lines]
    assert sum(nts) == len(F) and sum(int(x[2]) for x in lines) == len(V) and len(F1) == max(nts)
    assert cref.boundary_edges(F1) == 0 and (len(F1) - 2 * len(V1)) % 4 == 0 and np.unique(cref.roots(len(V1), F1)).size == 1   # one closed surface (the shell has handles)
    assert all(float(x[4]) > 0 and x[6] == "0" for x in lines)
    (V2, F2), _ = run(["--min-triangles", str(max(nts))])
    assert np.array_equal(F2, F1) and np.array_equal(V2, V1)
    p = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert "--keep-largest" in p.stdout and "--min-triangles" in p.stdout
    p = subprocess.run([exe, os.path.join(ROOT, "data", "bunny_small.obj"), "--keep-largest", "1"], capture_output=True, text=True)
    assert p.returncode != 0 and "--iso-indexed" in p.stderr


@gpu
def test_two_ranks_are_refused(shm, tmp_path):
    """world = 2 through the librccl double: SHM_ERR_STATE on both ranks, with a message, and the ranks go on to finish."""
    so = str(tmp_path / "librccl_mock.so")
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", os.path.join(ROOT, "tests", "native", "rccl_mock.c"), "-o", so, "-I/opt/rocm/include",
                           "-D__HIP_PLATFORM_AMD__", "-L/opt/rocm/lib", "-lamdhip64", "-lrt", "-lpthread"])
    uid = ("/shmmock_%d_cmp_2" % os.getpid()).encode().ljust(128, b"\x00")
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
        status, msg = open(tmp_path / ("cmp_%d.txt" % r)).read().split("\n", 1)
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
        s.isosurface_indexed(0.0)                                            # (collective)
        rc = s._lib.shm_grid_isosurface_components(s._h, None)
        with open(os.path.join(out_dir, "cmp_%d.txt" % rank), "w") as f:
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
            os._exit(1)

    threads = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()


if __name__ == "__main__" and len(sys.argv) == 6 and sys.argv[1] == "worker":
    _worker(int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5])
