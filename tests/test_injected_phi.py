"""Every reader of the resident phi -- the two soup contours, the indexed mesh and its psi variant, component labelling, sample, raycast, redistance and
redistance_exact -- on fields no solve produces, put in place through shm_grid_set_phi (include/shm_grid.h): random signs (all 256 marching-cubes cases),
isolated specks, nodes exactly on the isovalue, affine and trilinear fields with closed-form answers, and a sphere with NaN / +-inf nodes (tests/phi_fields.py).

Rules.  Every reference is fed get_phi() of the handle, the device's own input (tests/test_stage_edges.py).  Every tolerance is the one of the module that
owns the reader, none is fitted to the kernels' output, and each is printed beside the worst value:
    positions   8 * 2^-53 * B, B = max|bbox_min| + (n-1) cell; 2^-23 * B for fp32 device buffers            (tests/test_iso_indexed.py)
    rays        ray_ref.agree at 1e-9 cell / |d|, the gradient bound of tests/test_raycast.py's check_family, at most 0.1 % of a family in dispute
    psi         redistance_ref.tol = n eps_T max|psi|; fp32 exact distance: one fp32 ulp at <= 1e-3 of the reached nodes (tests/test_redistance_exact.py)
    samples     1e-13 max|phi|                                                                               (tests/test_sample.py)
Rays are chosen by the restatement alone: a ray is cast only if the float64 restatement's own gap exceeds 1e-6 max|phi|.  Grid-line rays on `on_iso` hit
nodes exactly (gap 0): those whose answer follows in integers are kept, those that start on the level set or touch it at their last node are not.
test_restatement_is_stable_on_the_injected_rays holds the float64 restatement to x87 long double on every ray that is cast.

Run as a script (`test_injected_phi.py worker <uid hex> <dir>`) this file is the worker of test_set_phi_is_refused_on_two_ranks."""
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

from conftest import ROOT

import components_ref as cref
import iso_ref
import phi_fields as pf
import ray_ref
import redistance_exact_ref as xref
import redistance_ref as rref

SHM_ERR_INVALID, SHM_ERR_STATE = 1, 7
INF = float("inf")
N = 20           # see tests/phi_fields.py
N_BRUTE = 12
FINITE = ["random_sign", "specks", "on_iso"]
PREC = [64, 32]


def dt(precision):
    return np.float64 if precision == 64 else np.float32


def build(name, n):
    if name == "affine_axis":
        return pf.affine(n, *pf.AFFINE_AXIS)
    return getattr(pf, name)(n)


def box(n):
    """The box of tests/test_iso_indexed.py's problem: the bunny's, with sources inside it for the 'camera' rays.  Loaded without a device."""
    import test_iso_indexed as iso_t
    d = iso_t.problem("bunny_small", n)
    return d, np.asarray(d["bbox_min"], dtype=np.float64), float(d["cell"])


_HANDLES = {}


def inject(shm, name, n, precision=64, slabs=1):
    """(problem, handle, the handle's phi): one handle per (n, precision, slabs) for the module; set_phi every time, the handle is shared."""
    key = (n, precision, slabs)
    if key not in _HANDLES:
        assert hasattr(shm.load_library(), "shm_grid_set_phi"), "libshm_grid.so does not export shm_grid_set_phi"
        d = box(n)[0]
        s = shm.GridSolver(precision=shm.SHM_F64 if precision == 64 else shm.SHM_F32, local_slabs=slabs)
        s.set_problem(d["pos"], d["wnormal"], d["area"], float(d["lam"]), int(d["n"]), d["bbox_min"], float(d["cell"]))
        _HANDLES[key] = (d, s)
    d, s = _HANDLES[key]
    s.set_phi(build(name, n))
    return d, s, s.get_phi()[0]


def same_values(a, b):
    """Equal where finite, the same NaN pattern with the same sign bits, the same infinities."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


def bound_B(d):
    return float(np.abs(d["bbox_min"]).max()) + (int(d["n"]) - 1) * float(d["cell"])


# ---- the mesh restatement with the non-finite rule --------------------------------------------------------------------------------------------------------------
_MESH = {}


def mesh_ref(tag, phi, n, b, h, iso=0.0):
    """(keys ascending, positions [nv, 3], triangles as keys [nt, 3], triangle corners [nt, 3, 3]) of iso_ref under the rule of include/shm_grid.h."""
    if tag not in _MESH:
        keys = iso_ref.cut_edges(phi, n, iso)
        P = np.asarray(phi, dtype=np.float64).reshape(n, n, n)
        gg, ax = keys // 3, keys % 3
        ii, jj, kk = gg % n, (gg // n) % n, gg // (n * n)
        va, vb = P[kk, jj, ii], P[kk + (ax == 2), jj + (ax == 1), ii + (ax == 0)]
        pos = np.stack([ii * h + b[0], jj * h + b[1], kk * h + b[2]], axis=1)
        pos[np.arange(len(keys)), ax] += (iso - va) / (vb - va) * h
        pts, tris = iso_ref.marching_cubes(np.asarray(phi, dtype=np.float64), n, b, h, iso)
        axis = {1: 0, n: 1, n * n: 2}
        K = np.array([[3 * a + axis[c - a] for (a, c) in t] for t in tris], dtype=np.int64).reshape(-1, 3)
        X = np.array([[pts[e] for e in t] for t in tris], dtype=np.float64).reshape(-1, 3, 3)
        _MESH[tag] = (keys, pos, K, X)
    return _MESH[tag]


def check_indexed(V, F, ref, tol, tag):
    """Keys, order and indices exactly, positions within tol, nothing non-finite.  Returns the number of vertices no triangle references."""
    keys, pos, K, X = ref
    assert V.dtype == np.float64 and F.dtype == np.int64 and V.shape == (len(keys), 3) and F.shape == K.shape, (tag, V.shape, len(keys), F.shape, K.shape)
    assert np.isfinite(V).all(), tag
    err = float(np.abs(V - pos).max()) if len(keys) else 0.0
    assert np.array_equal(keys[F], K), tag
    err = max(err, float(np.abs(V[F] - X).max()) if len(K) else 0.0)
    print("%s: %d vertices %d triangles, position error %.3e (bound %.3e, margin %.1fx)" % (tag, len(V), len(F), err, tol, tol / err if err > 0 else INF))
    assert err <= tol, (tag, err, tol)
    return len(keys) - np.unique(F).size


def check_edges(keys, F, n, tag):
    """Every directed edge is used once, and its reverse once unless the edge lies in a face of the box (both vertices sit on grid edges inside one face:
    decided from the vertices' keys, in integers)."""
    e = np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]])
    code = e[:, 0] * (len(keys) + 1) + e[:, 1]
    assert np.unique(code).size == len(code), tag
    rev = np.isin(e[:, 1] * (len(keys) + 1) + e[:, 0], code)
    g, ax = keys // 3, keys % 3
    idx = np.stack([g % n, (g // n) % n, g // (n * n)], axis=1)
    off_axis = np.arange(3)[None, :] != ax[:, None]
    on = np.concatenate([(idx == 0) & off_axis, (idx == n - 1) & off_axis], axis=1)
    assert (on[e[~rev, 0]] & on[e[~rev, 1]]).any(axis=1).all(), tag
    return int((~rev).sum())


# ---- CPU: the restatements and the fields themselves -----------------------------------------------------------------------------------------------------------
def test_fields_are_what_they_claim():
    """All 256 cases at both grid sizes; specks isolated, on faces, edges, corners and seams; nodes on the isovalue; the holed layout."""
    for n in (N, N_BRUTE):
        cnt = np.bincount(iso_ref.cell_cases(pf.random_sign(n).reshape(n, n, n), 0.0).reshape(-1), minlength=256)
        print("random_sign n %d: rarest case occurs %d times" % (n, cnt.min()))
        assert (cnt > 0).all()
        nodes = pf.speck_nodes(n)
        f = pf.specks(n).reshape(n, n, n)
        assert (f < 0).sum() == len(nodes) >= 17 and len(np.unique(nodes, axis=0)) == len(nodes)
        dist = np.abs(nodes[:, None, :] - nodes[None, :, :]).max(axis=2) + 3 * np.eye(len(nodes), dtype=np.int64)
        assert dist.min() >= 3
        edge = ((nodes == 0) | (nodes == n - 1)).sum(axis=1)
        assert (edge == 3).sum() >= 2 and (edge == 2).sum() >= 3 and (edge == 1).sum() >= 6
        for seam in (shm_plan(n, 3, 1)[0], shm_plan(n, 3, 2)[0]):
            assert (nodes[:, 2] == seam).any() and (nodes[:, 2] == seam - 1).any()
        assert (pf.on_iso(n) == 0).sum() > n and np.array_equal(pf.on_iso(n), np.rint(pf.on_iso(n)))
        g = pf.holed(n).reshape(n, n, n)
        L = pf.holed_layout(n)
        assert np.isnan(g).any() and (g == INF).any() and (g == -INF).any() and np.signbit(g[np.isnan(g)]).any() and not np.signbit(g[np.isnan(g)]).all()
        wall = g[L["wall"]]
        assert np.isfinite(wall).sum() == 1 and np.isfinite(wall[L["hole"][1], L["hole"][0]])
        assert (g[L["wall"] + 1:] > 0).all()                                   # nothing is cut behind the wall
        fin = np.isfinite(g)
        assert (g[fin] < 0).any()
    for name in ("affine", "affine_axis", "trilinear", "on_iso"):              # exact in fp32: both handles hold the same function
        f = build(name, N)
        assert np.array_equal(f.astype(np.float32).astype(np.float64), f), name
    assert not (pf.affine(N) == 0).any()


def shm_plan(n, nslabs, slab):
    q, r = divmod(n, nslabs)
    b = slab * q + min(slab, r)
    return b, b + q + (1 if slab < r else 0)


def test_iso_ref_is_unchanged_on_finite_fields():
    """The rule is a no-op on the goldens' contours: with and without it iso_ref returns the same dictionaries, for both methods, and cut_edges lists exactly the
    edges the triangles use."""
    from conftest import load_golden
    for case, method in (("bunny_small_n16", "marching_cubes"), ("bunny_small_n16", "marching_tets"), ("polygon_bear_n16", "marching_cubes"),
                         ("bunny_small_n24", "marching_cubes")):
        d = load_golden(case)
        n, phi = int(d["n"]), np.asarray(d["phi"], dtype=np.float64)
        for iso in (0.0, 0.25 * float(phi.max())):
            a = getattr(iso_ref, method)(phi, n, d["bbox_min"], float(d["cell"]), iso, drop_nonfinite=False)
            c = getattr(iso_ref, method)(phi, n, d["bbox_min"], float(d["cell"]), iso)
            assert a[1] == c[1] and a[0].keys() == c[0].keys() and all(np.array_equal(a[0][k], c[0][k]) for k in a[0]) and len(a[1]) > 0
            if method == "marching_cubes":
                axis = {1: 0, n: 1, n * n: 2}
                used = np.unique([3 * p + axis[q - p] for (p, q) in a[0].keys()])
                assert np.array_equal(used, iso_ref.cut_edges(phi, n, iso)) and np.array_equal(used, iso_ref.cut_edges(phi, n, iso, drop_nonfinite=False))


def test_iso_ref_rule_on_the_holed_field():
    """With the rule: no NaN position, no triangle from a cell with a non-finite corner, every referenced vertex among cut_edges, and some vertex of cut_edges
    referenced by no triangle (the orphan edge).  Without it the same field gives NaN positions -- the gap this module closes.  redistance_exact_ref.mesh is
    the same mesh."""
    for n in (N, N_BRUTE):
        phi = pf.holed(n)
        b, h = np.zeros(3), 1.0
        pts, tris = iso_ref.marching_cubes(phi, n, b, h, 0.0)
        assert len(tris) > 100 and all(np.isfinite(p).all() for p in pts.values())
        for m in ("marching_cubes", "marching_tets"):
            with np.errstate(invalid="ignore"):
                raw = getattr(iso_ref, m)(phi, n, b, h, 0.0, drop_nonfinite=False)
            assert any(not np.isfinite(p).all() for p in raw[0].values()), m
            ruled = getattr(iso_ref, m)(phi, n, b, h, 0.0)
            assert all(np.isfinite(p).all() for p in ruled[0].values()) and 0 < len(ruled[1]) < len(raw[1]), m
        keys, pos, K, X = mesh_ref(("cpu holed", n), phi, n, b, h)
        assert np.isfinite(pos).all() and np.isin(K, keys).all()
        orphan = np.setdiff1d(keys, K)
        io, m_, kz = pf.holed_layout(n)["orphan"]
        assert 3 * (io + m_ * n + kz * n * n) in orphan
        table, _ = iso_ref._mc_table()
        per_cell = np.array([len(t) for t in table])[iso_ref.cell_cases(phi.reshape(n, n, n), 0.0)]
        assert len(X) == int((per_cell * iso_ref.finite_cells(phi.reshape(n, n, n))).sum()) < int(per_cell.sum())     # the finite cells' triangles, no others
        assert np.array_equal(xref.mesh(phi, n, b, h, 0.0), X)
        assert xref.candidate_pairs(phi, n, h, 0.0, 2.5) < xref.candidate_pairs(np.where(np.isfinite(phi), phi, 1.0), n, h, 0.0, 2.5)


def test_redistance_restatement_reaches_the_far_side_through_the_hole_only():
    n = N
    phi, L = pf.holed(n), pf.holed_layout(n)
    psi, info = rref.redistance(phi, n, 1.0)
    far = psi.reshape(n, n, n)[L["wall"] + 1:]
    assert np.isfinite(far).all() and info["n_nonfinite"] == int((~np.isfinite(phi)).sum())
    k, j, i = np.unravel_index(np.argmin(far), far.shape)
    assert (i, j, k) == (L["hole"][0], L["hole"][1], 0)
    plugged = phi.reshape(n, n, n).copy()
    plugged[L["wall"]] = np.nan
    psi2, _ = rref.redistance(plugged.reshape(-1), n, 1.0)
    assert (psi2.reshape(n, n, n)[L["wall"] + 1:] == INF).all()


# ---- rays: chosen by the restatement alone -----------------------------------------------------------------------------------------------------------------------
RAY_FIELDS = ["random_sign", "specks", "on_iso", "holed"]
RAYS_PER_FAMILY = 375


def scale_of(phi):
    return float(np.abs(phi[np.isfinite(phi)]).max())


def hole_rays(phi, n, b, h):
    """One +z ray from below the box through every cell column that holds a cell with a non-finite corner, off the cell's centre."""
    bad = ~iso_ref.finite_cells(np.asarray(phi).reshape(n, n, n))
    j, i = np.nonzero(bad[:pf.holed_layout(n)["wall"] - 1].any(axis=0))      # (the NaN plane makes every column one: only the layers below it choose)
    O = np.stack([(i + 0.37) * h + b[0], (j + 0.61) * h + b[1], np.full(len(i), b[2] - 1.5 * h)], axis=1)
    D = np.tile(np.array([0.0, 0.0, 1.0]), (len(i), 1))
    return O, D, bad, i, j


def on_iso_grid_line_answers(phi, n, b, h, O, D):
    """Grid-line rays on on_iso, in integers: f moves by one per node, so a ray from a node with f0 != 0 that passes the node with f = 0 and goes on at least
    one node further crosses there, at t = |f0| cell exactly; one that never reaches 0 misses.  Rays that start on 0 or only touch it at the last node are
    marginal by construction (the restatement disputes them with itself) and are left out.  Returns (selected, t or NaN)."""
    idx = np.rint((O - b) / h).astype(np.int64)
    ax = np.argmax(np.abs(D), axis=1)
    sgn = D[np.arange(len(D)), ax]
    f0 = np.asarray(phi).reshape(n, n, n)[idx[:, 2], idx[:, 1], idx[:, 0]]
    steps = np.where(sgn > 0, n - 1 - idx[np.arange(len(D)), ax], idx[np.arange(len(D)), ax])
    fend = f0 + sgn * steps
    hit = (f0 != 0) & (f0 * fend < 0)
    miss = (f0 != 0) & (f0 * fend > 0)
    return hit | miss, np.where(hit, np.abs(f0) * h, np.nan)


def ray_families(name, phi, d, n, b, h):
    """[(family, O, D, selected, restatement)]: tests/test_raycast.py's families on this field, and which rays the float64 restatement alone leaves beyond
    dispute.  On `holed` the two families that run inside grid planes are left out: beside a non-finite node the answer of such a ray depends on which of the
    adjacent cells is walked, which include/shm_grid.h leaves to the implementation."""
    import test_raycast as ray_t
    out = []
    fams = list(ray_t.FAMILIES) if name != "holed" else ["camera", "inside", "through_holes"]
    scale = scale_of(phi)
    neg = np.where(np.isfinite(phi), phi, 1.0)                 # 'inside' starts at finite negative nodes
    for fam in fams:
        O, D = hole_rays(phi, n, b, h)[:2] if fam == "through_holes" else ray_t.rays(d, neg, fam, RAYS_PER_FAMILY, 100 + len(out))
        r = ray_ref.raycast_ref(phi, n, b, h, O, D, 0.0)
        sel = r["gap"] > 1e-6 * scale
        if name == "on_iso" and fam == "grid_lines":
            sel = on_iso_grid_line_answers(phi, n, b, h, O, D)[0]
        out.append((fam, O, D, sel, r))
    return out


@pytest.mark.parametrize("precision", PREC)
@pytest.mark.parametrize("name", RAY_FIELDS)
def test_restatement_is_stable_on_the_injected_rays(name, precision):
    """float64 against x87 long double on the rays the device tests cast, for the field as either handle holds it: no dispute, and (but for the grid-line rays
    that hit nodes of on_iso exactly) no gap below 1e-6 max|phi|; most rays survive the selection and most of those hit."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("long double is double on this platform")
    n = N
    d, b, h = box(n)
    phi = build(name, n).astype(dt(precision)).astype(np.float64)
    for fam, O, D, sel, r64 in ray_families(name, phi, d, n, b, h):
        r80 = ray_ref.raycast_ref(phi, n, b, h, O[sel], D[sel], 0.0, dtype=np.longdouble)
        ok = ray_ref.agree(r64["t"][sel], r80["t"].astype(np.float64), h, D[sel])
        hits = int(np.isfinite(r64["t"][sel]).sum())
        print("%s fp%d %-13s: %d of %d rays selected, %d hit, min gap %.3g max|phi|" % (name, precision, fam, sel.sum(), len(sel), hits,
                                                                                       float(r64["gap"][sel].min()) / scale_of(phi)))
        assert ok.all(), (name, fam, np.nonzero(~ok)[0][:10])
        assert sel.sum() >= (0.75 if (name, fam) == ("on_iso", "grid_lines") else 0.9) * len(sel) and hits > 0, (name, fam, int(sel.sum()), hits)
        if (name, fam) == ("on_iso", "grid_lines"):
            want = on_iso_grid_line_answers(phi, n, b, h, O, D)[1][sel]
            assert ray_ref.agree(r64["t"][sel], want, h, D[sel]).all() and (r64["gap"][sel] == 0).any()


# ---- GPU: the entry point ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("precision", PREC)
@pytest.mark.parametrize("slabs", [1, 3])
@pytest.mark.parametrize("n", [20, 21])
def test_get_phi_returns_the_rounded_input(shm, n, slabs, precision):
    """Bit for bit, sign bits of NaN included, on a field with every kind of value; a second set_phi replaces the first."""
    d = box(n)[0]
    s = shm.GridSolver(precision=shm.SHM_F64 if precision == 64 else shm.SHM_F32, local_slabs=slabs)
    s.set_problem(d["pos"], d["wnormal"], d["area"], float(d["lam"]), n, d["bbox_min"], float(d["cell"]))
    rng = np.random.default_rng(n + slabs)
    for f in (pf.holed(n) * rng.uniform(0.5, 2.0, n ** 3), rng.standard_normal(n ** 3) * 10.0 ** rng.integers(-30, 30, n ** 3)):
        s.set_phi(f)
        got, (k0, k1) = s.get_phi()
        with np.errstate(over="ignore"):
            want = f.astype(dt(precision)).astype(np.float64)
        assert (k0, k1) == (0, n) and same_values(got, want)
        assert np.array_equal(s.get_field(s.FIELD_PHI), got, equal_nan=True)
    s.close()


@pytest.mark.gpu
def test_set_phi_errors_and_state(shm):
    """SHM_ERR_STATE without a problem, SHM_ERR_INVALID for NULL; what was derived from the old phi is dropped; Y and a later solve are untouched."""
    lib = shm.load_library()
    from signed_heat_3d_amd.grid_abi import ABI_SYMBOLS
    header = open(os.path.join(ROOT, "include", "shm_grid.h")).read()
    assert "shm_grid_set_phi" in ABI_SYMBOLS and hasattr(lib, "shm_grid_set_phi") and "shm_status shm_grid_set_phi(" in header and lib.shm_grid_abi_version() == 5
    n = N
    d = box(n)[0]
    f = pf.random_sign(n)
    s = shm.GridSolver()
    assert lib.shm_grid_set_phi(s._h, f.ctypes.data) == SHM_ERR_STATE and lib.shm_grid_last_error(s._h)
    assert lib.shm_grid_set_phi(None, f.ctypes.data) == SHM_ERR_INVALID
    s.set_problem(d["pos"], d["wnormal"], d["area"], float(d["lam"]), n, d["bbox_min"], float(d["cell"]))
    assert lib.shm_grid_set_phi(s._h, None) == SHM_ERR_INVALID and lib.shm_grid_last_error(s._h)
    buf = np.empty(n ** 3)
    assert lib.shm_grid_get_phi(s._h, buf.ctypes.data, None, None) == SHM_ERR_STATE            # a refused call set nothing
    # Y of an earlier run_conv stays, before and after
    s.run_conv()
    Y0 = s.get_field(s.FIELD_Y0)
    s.set_phi(f)
    assert np.array_equal(s.get_field(s.FIELD_Y0), Y0)
    # build everything that hangs on phi, then replace phi: every getter refuses
    V, F = s.isosurface_indexed(0.0)
    s.isosurface_components()
    s.redistance(0.0)
    assert len(F) > 0 and lib.shm_grid_get_isosurface_indexed(s._h, V.ctypes.data, F.ctypes.data) == 0
    s.set_phi(pf.specks(n))
    assert lib.shm_grid_get_isosurface_indexed(s._h, V.ctypes.data, F.ctypes.data) == SHM_ERR_STATE
    assert lib.shm_grid_get_isosurface_indexed_device(s._h, None, None) == SHM_ERR_STATE
    assert lib.shm_grid_get_isosurface_components(s._h, None, None, None) == SHM_ERR_STATE
    nc = C.c_int64()
    assert lib.shm_grid_isosurface_components(s._h, C.byref(nc)) == SHM_ERR_STATE
    assert lib.shm_grid_get_redistanced(s._h, buf.ctypes.data) == SHM_ERR_STATE
    assert lib.shm_grid_isosurface_indexed_psi(s._h, 0.0, None, None) == SHM_ERR_STATE
    # ... and the rebuilt ones belong to the new phi
    V2, F2 = s.isosurface_indexed(0.0)
    assert len(F2) < len(F)
    assert np.array_equal(s.get_field(s.FIELD_Y0), Y0)
    # the brick extrema fall with phi: after the plane k = 7.25 (every brick above it skippable) the rays of on_iso still find its plane, at the integers' answers
    import test_raycast as ray_t
    b, h = np.asarray(d["bbox_min"], dtype=np.float64), float(d["cell"])
    O, D = ray_t.rays(d, f, "grid_lines", 300, 5)
    s.set_phi(build("affine_axis", n))
    s.raycast(O, D)
    s.set_phi(pf.on_iso(n))
    sel, want = on_iso_grid_line_answers(pf.on_iso(n), n, b, h, O, D)
    t, nh = s.raycast(O[sel], D[sel])
    assert ray_ref.agree(t, want[sel], h, D[sel]).all() and nh == np.isfinite(want[sel]).sum() > 20
    # a solve after set_phi gives the phi it gives without it
    s2 = shm.GridSolver()
    s2.set_problem(d["pos"], d["wnormal"], d["area"], float(d["lam"]), n, d["bbox_min"], float(d["cell"]))
    s2.solve(tol=1e-10)
    s.solve(tol=1e-10)
    assert np.array_equal(s.get_phi()[0], s2.get_phi()[0])
    s.close()
    s2.close()


@pytest.mark.gpu
def test_set_phi_is_refused_on_two_ranks(shm, tmp_path):
    """world = 2 through the librccl double: SHM_ERR_INVALID on both ranks, with a message."""
    so = str(tmp_path / "librccl_mock.so")
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", os.path.join(ROOT, "tests", "native", "rccl_mock.c"), "-o", so, "-I/opt/rocm/include",
                           "-D__HIP_PLATFORM_AMD__", "-L/opt/rocm/lib", "-lamdhip64", "-lrt", "-lpthread"])
    uid = ("/shmmock_%d_sp_2" % os.getpid()).encode().ljust(128, b"\x00")
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
        status, msg = open(tmp_path / ("sp_%d.txt" % r)).read().split("\n", 1)
        assert int(status) == SHM_ERR_INVALID and "single-process" in msg, (r, status, msg)


# ---- GPU: contours ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("precision", PREC)
@pytest.mark.parametrize("name", FINITE)
def test_contours_on_finite_fields(shm, name, precision):
    """Soup marching cubes against iso_ref triangle by triangle; the indexed mesh (keys, order, indices exact; host and device getters); indexed against soup
    as a renumbering; two builds and three slabs bit-identical; every directed edge once."""
    import test_iso_indexed as iso_t
    n = N
    d, s, phi = inject(shm, name, n, precision)
    b, h = np.asarray(d["bbox_min"], dtype=np.float64), float(d["cell"])
    B = bound_B(d)
    tol = 8 * 2.0 ** -53 * B
    ref = mesh_ref((name, n, precision), phi, n, b, h)
    if name == "random_sign":
        cnt = np.bincount(iso_ref.cell_cases(phi.reshape(n, n, n), 0.0).reshape(-1), minlength=256)
        assert (cnt > 0).all()                                                 # all 256 cases, from the reference, before the comparison is trusted
    tag = "%s n %d fp%d" % (name, n, precision)
    V, F = s.isosurface_indexed(0.0)
    assert check_indexed(V, F, ref, tol, tag + " indexed") == 0 and len(F) > 0
    iso_t.check_against_restatement(V, F, phi, n, 0, b, h, 0.0, tol)          # the neighbouring module's own comparison
    Vs, Fs = s.isosurface(0.0)
    assert Vs.shape == V.shape and Fs.shape == F.shape
    err = float(np.abs(Vs[Fs] - ref[3]).max())
    print("%s soup marching cubes: %d triangles, error %.3e (bound %.3e)" % (tag, len(Fs), err, tol))
    assert err <= tol
    iso_t.check_against_old_path(s, d, phi, 0.0, tol)                          # a pure renumbering
    V2, F2 = s.isosurface_indexed(0.0)
    assert np.array_equal(V2, V) and np.array_equal(F2, F)
    open_edges = check_edges(ref[0], F, n, tag)
    print("%s: %d edges without a reverse, all in faces of the box" % (tag, open_edges))
    assert open_edges > 0                                                      # every one of these surfaces runs into the box
    if name == "on_iso":
        X = V[F]
        assert ((np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]) ** 2).sum(axis=1) == 0).any()          # zero-area triangles really occur
        assert len(np.unique(V, axis=0)) < len(V)                                                       # and coincident vertices
    if torch is not None:
        Vd, Fd = s.isosurface_indexed(0.0, device=True)
        Vd, Fd = Vd.cpu().numpy(), Fd.cpu().numpy()
        assert np.array_equal(Fd, F) and Vd.dtype == dt(precision)
        errd = float(np.abs(Vd.astype(np.float64) - ref[1]).max())
        told = tol if precision == 64 else 2.0 ** -23 * B
        print("%s device getter: error %.3e (bound %.3e)" % (tag, errd, told))
        assert errd <= told and np.array_equal(Vd, V.astype(dt(precision)))
    _, s3, phi3 = inject(shm, name, n, precision, slabs=3)
    assert same_values(phi3, phi)
    V3, F3 = s3.isosurface_indexed(0.0)
    assert np.array_equal(V3, V) and np.array_equal(F3, F)
    Vs3, Fs3 = s3.isosurface(0.0)
    assert np.array_equal(Vs3, Vs) and np.array_equal(Fs3, Fs)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PREC)
@pytest.mark.parametrize("name", FINITE + ["holed"])
def test_marching_tets_soup(shm, name, precision):
    """iso_kernel against iso_ref.marching_tets at n = 12 (the python loop over six tetrahedra per cell is the cost): the same welded vertices, the same
    triangles as position triples up to rotation, on one slab and on three; on `holed` nothing non-finite comes back."""
    n = N_BRUTE
    d, s, phi = inject(shm, name, n, precision)
    b, h = np.asarray(d["bbox_min"], dtype=np.float64), float(d["cell"])
    B = bound_B(d)
    V, F = s.isosurface(0.0, method="marching_tets")
    pts, tris = iso_ref.marching_tets(phi, n, b, h, 0.0)
    assert np.isfinite(V).all() and len(V) == len(pts) and len(F) == len(tris) > 0, (len(V), len(pts), len(F), len(tris))
    got = np.array(sorted(map(tuple, np.round(V / B, 11))))
    want = np.array(sorted(map(tuple, np.round(np.array(list(pts.values())) / B, 11))))
    err = float(np.abs(got - want).max()) * B
    tol = 8 * 2.0 ** -53 * B + 1e-11 * B                                       # (the rounding that makes the lists sortable)
    print("%s n %d fp%d marching tets: %d vertices %d triangles, error %.3e (bound %.3e)" % (name, n, precision, len(V), len(F), err, tol))
    assert err <= tol
    # triangles as unordered position triples (the kernel orients each towards increasing phi, the restatement does not)
    def canon(T):   # noqa: E306
        T = np.round(np.asarray(T) / B, 10)
        return np.array(sorted(tuple(sorted(map(tuple, t))) for t in T)).reshape(-1, 9)
    assert np.abs(canon(V[F]) - canon(np.array([[pts[k] for k in t] for t in tris]))).max() <= 2e-10
    _, s3, _ = inject(shm, name, n, precision, slabs=3)
    V3, F3 = s3.isosurface(0.0, method="marching_tets")
    assert np.array_equal(V3, V) and np.array_equal(F3, F)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PREC)
def test_contours_on_the_holed_field(shm, precision):
    """The rule of include/shm_grid.h on the device: no non-finite position from any path, the triangles of the restatement with the rule, the unreferenced
    vertices where the restatement has them and components of their own; slabs and calls bit-identical."""
    n = N
    d, s, phi = inject(shm, "holed", n, precision)
    b, h = np.asarray(d["bbox_min"], dtype=np.float64), float(d["cell"])
    B = bound_B(d)
    tol = 8 * 2.0 ** -53 * B
    assert same_values(phi, pf.holed(n).astype(dt(precision)).astype(np.float64))
    ref = mesh_ref(("holed", n, precision), phi, n, b, h)
    tag = "holed n %d fp%d" % (n, precision)
    V, F = s.isosurface_indexed(0.0)
    orphans = check_indexed(V, F, ref, tol, tag + " indexed")
    want_orphans = np.setdiff1d(ref[0], ref[2])
    print("%s: %d vertices referenced by no triangle" % (tag, orphans))
    assert orphans == len(want_orphans) > 0
    assert np.array_equal(np.setdiff1d(np.arange(len(V)), F), np.searchsorted(ref[0], want_orphans))
    # the soup path: the same triangles in the same order; it welds from the triangles, so it has no unreferenced vertex
    Vs, Fs = s.isosurface(0.0)
    assert np.isfinite(Vs).all() and Fs.shape == F.shape and len(Vs) == len(V) - orphans
    err = float(np.abs(Vs[Fs] - ref[3]).max())
    print("%s soup marching cubes: error %.3e (bound %.3e)" % (tag, err, tol))
    assert err <= tol
    m = np.full(len(V), -1, dtype=np.int64)
    m[F.reshape(-1)] = Fs.reshape(-1)
    assert np.array_equal(m[F], Fs) and np.unique(m[m >= 0]).size == len(Vs)
    # components: an unreferenced vertex is a component of its own
    rec, tc, vc = s.isosurface_components(labels=True)
    want, wtc, wvc, sa, sv = cref.records(V, F, n, b, h)
    for k in ("first_vertex", "n_vertices", "n_triangles", "touches_box"):
        assert np.array_equal(rec[k], want[k]), k
    assert rec["lo"].tobytes() == want["lo"].tobytes() and rec["hi"].tobytes() == want["hi"].tobytes() and np.array_equal(tc, wtc) and np.array_equal(vc, wvc)
    lone = rec[rec["n_triangles"] == 0]
    assert len(lone) == orphans and (lone["n_vertices"] == 1).all() and (lone["area"] == 0).all() and (lone["volume"] == 0).all()
    assert np.array_equal(lone["lo"], lone["hi"]) and np.array_equal(lone["lo"], V[lone["first_vertex"]])
    Vk, Fk = s.isosurface_indexed(0.0, keep_largest=1)
    Vw, Fw = cref.keep_mesh(V, F, wvc, wtc, cref.largest_mask(want, keep_largest=1))
    assert np.array_equal(Vk, Vw) and np.array_equal(Fk, Fw)
    V2, F2 = s.isosurface_indexed(0.0)
    assert np.array_equal(V2, V) and np.array_equal(F2, F)
    if torch is not None:
        Vd, Fd = s.isosurface_indexed(0.0, device=True)
        assert np.array_equal(Fd.cpu().numpy(), F) and np.array_equal(Vd.cpu().numpy(), V.astype(dt(precision)))
    _, s3, phi3 = inject(shm, "holed", n, precision, slabs=3)
    assert same_values(phi3, phi)
    V3, F3 = s3.isosurface_indexed(0.0)
    Vs3, Fs3 = s3.isosurface(0.0)
    assert np.array_equal(V3, V) and np.array_equal(F3, F) and np.array_equal(Vs3, Vs) and np.array_equal(Fs3, Fs)


# ---- GPU: components ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("precision", PREC)
@pytest.mark.parametrize("name", FINITE)
def test_components(shm, name, precision):
    """Labels, records and keep_components against components_ref through tests/test_iso_components.py's own check: hundreds of components and long thin ones
    (random_sign, specks), zero-area triangles in the fixed-point area (on_iso)."""
    import test_iso_components as cmp_t
    n = N
    for slabs in (1, 3):
        d, s, phi = inject(shm, name, n, precision, slabs)
        V, F, rec, tc, vc = cmp_t.check_records(s, d, 0.0, "%s fp%d slabs %d" % (name, precision, slabs))
        if name == "specks":
            nodes = pf.speck_nodes(n)
            on_box = ((nodes == 0) | (nodes == n - 1)).any(axis=1)
            assert len(rec) == len(nodes) > 100                                # one component per speck ...
            assert (rec["touches_box"] == 1).sum() == on_box.sum() >= 11       # ... open exactly where its node lies on the box, lower faces and upper
            assert (rec["volume"][rec["touches_box"] == 0] > 0).all()          # a closed blob of inside
        if name == "random_sign":
            assert len(rec) >= 50 and rec["n_triangles"].max() > 1000          # many small components and one that sprawls through the grid
        if name == "on_iso":
            qA = cref.quanta(n, float(d["cell"]))[0]
            ia = cref.triangle_quanta(V, F, float(d["cell"]), d["bbox_min"])[0]
            assert (ia == 0).any() and len(rec) >= 1 and rec["area"].sum() == qA * float(ia.sum())
        want = cref.records(V, F, n, d["bbox_min"], float(d["cell"]))[0]
        for kw in (dict(keep_largest=1), dict(keep_largest=3, min_triangles=8), dict(min_triangles=9)):
            Vk, Fk = s.isosurface_indexed(0.0, **kw)
            Vw, Fw = cref.keep_mesh(V, F, vc, tc, cref.largest_mask(want, **kw))
            assert np.array_equal(Vk, Vw) and np.array_equal(Fk, Fw), kw


# ---- GPU: sample -----------------------------------------------------------------------------------------------------------------------------------------------------
def sample_points(n, b, h, seed):
    """Interior points, nodes, points on interior planes of one, two and three axes, and points on the upper faces, edges and corner of the box."""
    rng = np.random.default_rng(seed)
    hi = np.array([(n - 1) * h + b[a] for a in range(3)])
    P = [rng.uniform(b, hi, (3000, 3)), rng.integers(0, n, (1500, 3)) * h + b]
    for axes in ((0,), (1,), (2,), (0, 1), (1, 2), (0, 2)):
        q = rng.uniform(b, hi, (400, 3))
        for a in axes:
            q[:, a] = rng.integers(0, n, 400) * h + b[a]
        P.append(q)
    for axes in ((0,), (1,), (2,), (0, 1), (1, 2), (0, 1, 2)):
        q = rng.uniform(b, hi, (200, 3))
        for a in axes:
            q[:, a] = hi[a]
        P.append(q)
    return np.concatenate(P)


@pytest.mark.gpu
@pytest.mark.parametrize("slabs", [1, 3])
@pytest.mark.parametrize("precision", PREC)
@pytest.mark.parametrize("name", ["trilinear", "affine"])
def test_sample_closed_form(shm, name, precision, slabs):
    """The interpolant reproduces the field, so value and gradient are known without eval_ref: at nodes, on interior faces, on the upper faces.  The node values
    are exact in both precisions; the bound is tests/test_sample.py's 1e-13 max|phi| (the gradient in phi per length, as there)."""
    n = N
    d, s, phi = inject(shm, name, n, precision, slabs)
    assert np.array_equal(phi, build(name, n))
    b, h = np.asarray(d["bbox_min"], dtype=np.float64), float(d["cell"])
    pts = sample_points(n, b, h, 7)
    v, g, na = s.sample(pts, grad=True)
    at = pf.trilinear_at if name == "trilinear" else pf.affine_at
    wv, wg = at((pts - b) / h)
    scale = float(np.abs(phi).max())
    ev, eg = float(np.abs(v - wv).max()), float(np.abs(g - wg / h).max())
    print("%s fp%d slabs %d: %d points, value error %.3e, gradient error %.3e (bound %.3e)" % (name, precision, slabs, len(pts), ev, eg, 1e-13 * scale))
    assert na == len(pts) and ev <= 1e-13 * scale and eg <= 1e-13 * scale


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PREC)
def test_sample_on_the_holed_field(shm, precision):
    """Against eval_ref, non-finite values included (the formula in IEEE arithmetic, no special case: include/shm_grid.h): the answer is finite exactly where
    all eight corners of the chosen cell are, zero weights included."""
    from test_sample import eval_ref
    n = N
    for slabs in (1, 3):
        d, s, phi = inject(shm, "holed", n, precision, slabs)
        b, h = np.asarray(d["bbox_min"], dtype=np.float64), float(d["cell"])
        pts = sample_points(n, b, h, 8)
        v, g, na = s.sample(pts, grad=True)
        with np.errstate(invalid="ignore"):
            rv, rg = eval_ref(phi, n, b, h, pts, grad=True)
        scale = scale_of(phi)
        idx = np.minimum(np.floor((pts - b) / h).astype(np.int64), n - 2)
        good = iso_ref.finite_cells(phi.reshape(n, n, n))[idx[:, 2], idx[:, 1], idx[:, 0]]
        assert na == len(pts) and np.array_equal(np.isfinite(v), good) and np.array_equal(np.isfinite(g).all(axis=1), good) and 0 < (~good).sum() < len(good)
        for got, want in ((v, rv), (g, rg)):
            fin = np.isfinite(want)
            assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])
            err = float(np.abs(got[fin] - want[fin]).max())
            assert err <= 1e-13 * scale, (err, 1e-13 * scale)
        print("holed fp%d slabs %d: %d of %d points in cells with a non-finite corner, all non-finite; the others within 1e-13 max|phi|" % (
            precision, slabs, (~good).sum(), len(good)))


# ---- GPU: raycast ----------------------------------------------------------------------------------------------------------------------------------------------------
def check_rays(t, g, O, D, phi, n, b, h, ref, who, exact_hits=False):
    """tests/test_raycast.py's check_family with max|phi| over the finite nodes: agreement at 1e-9 cell / |d|, a dispute only where the restatement's gap is
    below 1e-6 max|phi| and in at most 0.1 % of the family, the gradient within that module's bound."""
    tol_t = 1e-9
    scale = scale_of(phi)
    ok = ray_ref.agree(t, ref["t"], h, D, tol_t)
    disputed = ~ok
    both = np.isfinite(t) & np.isfinite(ref["t"])
    worst = float((np.abs(t - ref["t"])[both] * np.linalg.norm(D, axis=1)[both] / h).max()) if both.any() else 0.0
    print("%s: %d rays, %d hits (ref %d), %d in dispute, max |dt| %.3g cell/|d| (bound %.0e), min gap %.3g max|phi|"
          % (who, len(t), np.isfinite(t).sum(), np.isfinite(ref["t"]).sum(), disputed.sum(), worst, tol_t, float(ref["gap"].min()) / scale))
    assert (ref["gap"][disputed] <= 1e-6 * scale).all(), (who, np.nonzero(disputed)[0][:10], t[disputed][:10], ref["t"][disputed][:10])
    assert disputed.sum() <= 1e-3 * len(t), (who, int(disputed.sum()))
    miss = np.isnan(t)
    assert np.isnan(g[miss]).all() and np.isfinite(g[~miss]).all()
    m = ok & np.isfinite(t)
    if m.any():
        U = np.asarray(phi, dtype=np.float64).reshape(n, n, n)
        i, j, k = ref["cell"][m].T
        kx = U[k, j, i + 1] - U[k, j, i]
        ky = U[k, j + 1, i] - U[k, j, i]
        kxy = (U[k, j + 1, i + 1] - U[k, j + 1, i]) - kx
        kxz = (U[k + 1, j, i + 1] - U[k + 1, j, i]) - kx
        kyz = (U[k + 1, j + 1, i] - U[k + 1, j, i]) - ky
        kxyz = ((U[k + 1, j + 1, i + 1] - U[k + 1, j + 1, i]) - (U[k + 1, j, i + 1] - U[k + 1, j, i])) - kxy
        second = (np.maximum(np.maximum(np.abs(kxy), np.abs(kxz)), np.abs(kyz)) + np.abs(kxyz)) / h ** 2
        tol = 2 * tol_t * h * second + 1e-13 * scale / h
        err = np.abs(g[m] - ref["grad"][m]).max(axis=1)
        assert (err <= tol).all(), (who, float((err / tol).max()), np.nonzero(m)[0][np.argmax(err / tol)])
    return ok


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PREC)
@pytest.mark.parametrize("name", RAY_FIELDS)
def test_raycast_against_the_restatement(shm, name, precision):
    """tests/test_raycast.py's four families on each field, one slab and three; on `holed` also a ray up every cell column that holds a non-finite corner: no
    hit inside such a cell, and hits behind such cells are found."""
    n = N
    d, s, phi = inject(shm, name, n, precision)
    _, s3, _ = inject(shm, name, n, precision, slabs=3)
    b, h = np.asarray(d["bbox_min"], dtype=np.float64), float(d["cell"])
    good = iso_ref.finite_cells(phi.reshape(n, n, n))
    for fam, O, D, sel, r in ray_families(name, phi, d, n, b, h):
        O, D = O[sel], D[sel]
        ref = {k: v[sel] for k, v in r.items()}
        t, g, nh = s.raycast(O, D, 0.0, grad=True)
        who = "%s fp%d %s" % (name, precision, fam)
        ok = check_rays(t, g, O, D, phi, n, b, h, ref, who)
        assert nh == np.isfinite(t).sum() > 0
        if name == "on_iso" and fam == "grid_lines":
            want = on_iso_grid_line_answers(phi, n, b, h, O, D)[1]             # (O, D are the selected rays: all of them have an answer in integers)
            assert ok.all() and (ref["gap"] == 0).any() and ray_ref.agree(t, want, h, D).all()      # node hits: no dispute although the gap is zero
        t3, g3, _ = s3.raycast(O, D, 0.0, grad=True)
        assert same_values(t3, t) and same_values(g3, g)
        # no hit inside a cell with a non-finite corner: a hit strictly inside a cell names that cell
        u = (O + t[:, None] * D - b) / h
        inner = np.isfinite(t) & (np.abs(u - np.rint(u)) > 1e-6).all(axis=1) & (u > 0).all(axis=1) & (u < n - 1).all(axis=1)
        c = np.floor(u[inner]).astype(np.int64)
        assert good[c[:, 2], c[:, 1], c[:, 0]].all(), who
        if fam == "through_holes":
            _, _, bad, ci, cj = hole_rays(phi, n, b, h)
            ci, cj = ci[sel], cj[sel]
            hit = np.isfinite(t) & ok
            zc = np.floor(np.where(np.isfinite(t), u[:, 2], 0.0)).astype(np.int64)
            behind = np.array([hit[q] and bad[:max(zc[q], 0), cj[q], ci[q]].any() for q in range(len(t))])
            print("%s: %d hits lie behind a cell with a non-finite corner" % (who, behind.sum()))
            assert behind.sum() >= 5
            # and the holes matter: the sphere without them answers some of these rays differently
            with np.errstate(invalid="ignore"):
                L = pf.holed_layout(n)
                kk, jj, ii = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
                whole = (np.sqrt((ii - L["centre"][0]) ** 2 + (jj - L["centre"][1]) ** 2 + (kk - L["centre"][2]) ** 2) - L["R"]).reshape(-1)
            rw = ray_ref.raycast_ref(whole.astype(dt(precision)).astype(np.float64), n, b, h, O, D, 0.0)
            moved = ~ray_ref.agree(t, rw["t"], h, D)
            print("%s: %d rays answer differently from the sphere without holes" % (who, moved.sum()))
            assert moved.sum() >= 3


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PREC)
def test_raycast_closed_form_on_the_affine_field(shm, precision):
    """f is affine along every ray: t = (c - a . u_o) / (a . u_d), a hit iff it lies in the ray's interval in the box; gradient a / cell.  Rays within 1e-6 of
    an end of their interval, or within 1e-3 of grazing, are left out by the closed form alone."""
    import test_raycast as ray_t
    n = N
    a, c = np.array(pf.AFFINE_GENERIC[0]), pf.AFFINE_GENERIC[1]
    for slabs in (1, 3):
        d, s, phi = inject(shm, "affine", n, precision, slabs)
        assert np.array_equal(phi, pf.affine(n))
        b, h = np.asarray(d["bbox_min"], dtype=np.float64), float(d["cell"])
        for f, fam in enumerate(ray_t.FAMILIES):
            O, D = ray_t.rays(d, phi, fam, RAYS_PER_FAMILY, 200 + f)
            uo, ud = (O - b) / h, D / h
            den = ud @ a
            with np.errstate(divide="ignore", invalid="ignore"):
                tx = (c - uo @ a) / den
                ta, tb = (0.0 - uo) / ud, ((n - 1) - uo) / ud
                lo = np.where(ud != 0, np.minimum(ta, tb), -INF).max(axis=1)
                up = np.where(ud != 0, np.maximum(ta, tb), INF).min(axis=1)
            inbox = ((ud != 0) | ((uo >= 0) & (uo <= n - 1))).all(axis=1)
            lo = np.maximum(lo, 0.0)
            width = np.linalg.norm(ud, axis=1)                                  # cells per unit of t
            sel = (np.abs(den) > 1e-3 * np.linalg.norm(a) * width) & (np.abs(tx - lo) * width > 1e-6) & (np.abs(tx - up) * width > 1e-6)
            want = np.where(inbox & (lo <= up) & (tx > lo) & (tx < up), tx, np.nan)[sel]
            t, g, nh = s.raycast(O[sel], D[sel], 0.0, grad=True)
            ok = ray_ref.agree(t, want, h, D[sel])
            both = np.isfinite(t) & np.isfinite(want)
            worst = float((np.abs(t - want)[both] * width[sel][both]).max())
            eg = float(np.abs(g[both] - a / h).max())
            print("affine fp%d slabs %d %-11s: %d rays, %d hits, max |dt| %.3g cell/|d| (bound 1e-09), gradient error %.3e (bound %.3e)" % (
                precision, slabs, fam, sel.sum(), both.sum(), worst, eg, 1e-13 * np.abs(phi).max() / h))
            assert ok.all() and both.sum() > 0 and sel.sum() >= 0.95 * len(sel), (fam, np.nonzero(~ok)[0][:10])
            assert eg <= 1e-13 * float(np.abs(phi).max()) / h and np.isnan(g[~both]).all()


# ---- GPU: redistance -------------------------------------------------------------------------------------------------------------------------------------------------
def compare_psi(psi, want, n, precision, tag):
    assert np.array_equal(np.isnan(psi), np.isnan(want)), tag
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(psi), inf) and np.array_equal(psi[inf], want[inf]), tag
    fin = np.isfinite(want)
    lim = rref.tol(n, dt(precision), want)
    err = float(np.abs(psi[fin] - want[fin]).max()) if fin.any() else 0.0
    print("%s: err %.3e TOL %.3e (margin %.1fx)" % (tag, err, lim, lim / err if err > 0 else INF))
    assert err <= lim, (tag, err, lim)
    return lim


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PREC)
@pytest.mark.parametrize("name", ["affine_axis", "affine", "specks", "on_iso", "holed"])
def test_redistance(shm, name, precision):
    """Against redistance_ref.redistance; on the axis-aligned plane also against the exact distance; on `holed` the walls."""
    import test_redistance as rd_t
    n = N
    d, s, phi = inject(shm, name, n, precision)
    h = float(d["cell"])
    st = s.redistance(0.0)
    psi = s.get_redistanced()
    want, info = rref.redistance(phi, n, h, 0.0, dtype=dt(precision))
    tag = "redistance %s n %d fp%d" % (name, n, precision)
    lim = compare_psi(psi, want, n, precision, tag)
    bad = ~np.isfinite(phi)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(psi[~bad] < 0, phi[~bad] < 0)
    assert st["n_frozen"] == info["n_frozen"] > 0 and st["n_reached"] == info["n_reached"] and st["n_nonfinite"] == int(bad.sum()), (tag, st)
    assert abs(st["max_abs"] - info["max_abs"]) <= lim and 0 < st["n_rounds"] <= rd_t.rounds_cap(n)
    if name == "affine_axis":
        k = np.repeat(np.arange(n, dtype=np.float64), n * n)
        exact = (k - pf.AFFINE_AXIS[1]) * h
        err = float(np.abs(psi - exact).max())
        print("%s: against the exact plane distance %.3e TOL %.3e" % (tag, err, lim))
        assert err <= lim
    if name == "on_iso":
        assert (psi[phi == 0] == 0).all() and not np.signbit(psi[phi == 0]).any() and info["frozen"][phi == 0].all()      # f = 0: outside, frozen at 0
    if name == "holed":
        L = pf.holed_layout(n)
        assert np.isnan(psi[bad]).all() and np.isfinite(psi[~bad]).all()
        far = psi.reshape(n, n, n)[L["wall"] + 1:]
        kk, jj, ii = np.unravel_index(np.argmin(far), far.shape)
        assert (ii, jj, kk) == (L["hole"][0], L["hole"][1], 0)                 # the front arrives through the hole
        above = psi.reshape(n, n, n)[L["wall"] + 1, L["hole"][1], L["hole"][0]]
        assert abs(above - (psi.reshape(n, n, n)[L["wall"], L["hole"][1], L["hole"][0]] + h)) <= lim
    st2 = s.redistance(0.0)
    assert same_values(s.get_redistanced(), psi)
    for a in (st, st2):
        a.pop("ms")
    assert st2 == st
    _, s3, _ = inject(shm, name, n, precision, slabs=3)
    st3 = s3.redistance(0.0)
    assert same_values(s3.get_redistanced(), psi)
    assert (st3["n_frozen"], st3["n_reached"], st3["n_nonfinite"], st3["max_abs"]) == (st["n_frozen"], st["n_reached"], st["n_nonfinite"], st["max_abs"])


# ---- GPU: redistance_exact -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("precision", PREC)
@pytest.mark.parametrize("name,n", [("random_sign", N_BRUTE), ("specks", N), ("on_iso", N), ("holed", N)])
def test_redistance_exact(shm, name, n, precision):
    """Against redistance_exact_ref.exact_distance over the device's own mesh (and brute force at n = 12); the mesh itself against the restatement with the rule;
    n_candidate_pairs and the +-band pattern exactly; two calls and three slabs bit-identical; the psi contour at +- one cell.  `holed` is the test of the
    header's sentence: a node whose phi is not finite holds NaN and a cell with a non-finite corner contributes no triangle."""
    import test_redistance_exact as rx_t
    d, s, phi = inject(shm, name, n, precision)
    b, h = np.asarray(d["bbox_min"], dtype=np.float64), float(d["cell"])
    band = 2.5 * h
    tol = 8 * 2.0 ** -53 * bound_B(d)
    tag = "exact %s n %d fp%d" % (name, n, precision)
    st = s.redistance_exact(0.0, band)
    psi = s.get_redistanced()
    V, F = s.get_isosurface_indexed(st["n_vertices"], st["n_triangles"])
    check_indexed(V, F, mesh_ref((name, n, precision), phi, n, b, h), tol, tag + " mesh")
    X = V[F]
    want, info = xref.exact_distance(X, phi, n, b, h, 0.0, band, dt(precision))
    bad = ~np.isfinite(phi)
    assert np.array_equal(np.isnan(psi), bad) and np.array_equal(np.isnan(want), bad)
    fin = ~bad
    rx_t.compare(psi[fin], want[fin], dict(info, reached=info["reached"][fin]), precision, n, tag)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(psi[fin] < 0, phi[fin] < 0)
    assert st["n_reached"] == info["n_reached"] and st["n_candidate_pairs"] == xref.candidate_pairs(phi, n, h, 0.0, band) > 0, (tag, st)
    if n == N_BRUTE:
        wb, ib = xref.brute_force(X, phi, n, b, h, 0.0, band, dt(precision))
        rx_t.compare(psi[fin], wb[fin], dict(ib, reached=ib["reached"][fin]), precision, n, tag + " brute force")
    if name == "on_iso":
        assert ((np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]) ** 2).sum(axis=1) == 0).any()
        on = phi == 0
        assert (psi[on] >= 0).all() and (psi[on] <= tol).all()
    st2 = s.redistance_exact(0.0, band)
    assert same_values(s.get_redistanced(), psi)
    for a in (st, st2):
        a.pop("ms")
    assert st2 == st
    # the psi contour at +- one cell, under the same rule (psi is NaN where phi is not finite)
    for k in (-1.0, 1.0):
        Vp, Fp = s.isosurface_indexed_psi(k * h)
        psi_ref = mesh_ref((name, n, precision, "psi", k), psi, n, b, h, k * h)
        check_indexed(Vp, Fp, psi_ref, tol, "%s psi contour at %+.0f cell" % (tag, k))
        assert len(Fp) > 0 or name == "specks"
    _, s3, _ = inject(shm, name, n, precision, slabs=3)
    st3 = s3.redistance_exact(0.0, band)
    st3.pop("ms")
    assert same_values(s3.get_redistanced(), psi) and st3 == st


# ---- the worker of test_set_phi_is_refused_on_two_ranks --------------------------------------------------------------------------------------------------------------
def _worker(uid_hex, out_dir):
    import threading
    import traceback
    import shm_import
    shm = shm_import.load()
    n = N_BRUTE

    def run_rank(rank):
        d = box(n)[0]
        s = shm.GridSolver(device=0, rank=rank, world=2, rccl_unique_id=bytes.fromhex(uid_hex))
        s.set_problem(d["pos"], d["wnormal"], d["area"], float(d["lam"]), n, d["bbox_min"], float(d["cell"]))
        f = pf.specks(n)
        rc = s._lib.shm_grid_set_phi(s._h, f.ctypes.data)
        with open(os.path.join(out_dir, "sp_%d.txt" % rank), "w") as fh:
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
    _worker(sys.argv[2], sys.argv[3])
