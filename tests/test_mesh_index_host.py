"""The index of the attached mesh without a GPU (csrc/shm_mesh_index.h; the contract is under shm_grid_attach_mesh_device in include/shm_grid.h).

Three evaluations of one contract are held to each other BIT FOR BIT -- dist, tri and cp; there is no tolerance in this file:
    brute    tests/mesh_index_ref.brute: closest_point_ref.brute_force over the triangles with finite corners; knows nothing of cells
    ref      tests/mesh_index_ref.build / answers: the numpy restatement of the index rules
    native   tests/native/test_mesh_index.cpp: csrc/shm_mesh_index.h itself, built as a stand-alone program, plain and under AddressSanitizer + UBSan
Meshes: the 24^3 golden contour (0.25 max phi, welded) after mesh_smooth_ref.smooth(..., 10); data/bunny_small.obj's 2856 faces; a fine patch plus one quad of
two triangles spanning the whole box (the big list); a soup with repeated corners, duplicate triangles, NaN vertices and a needle of height 2^-30 cell.
Queries: closest_point_ref.families over the index's own grid, plus points 10^3 box sides away and points exactly on vertices and edge midpoints.
max_dist: 1/16 of the box side, and +inf."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden

import mesh_index_ref as mir
import mesh_smooth_ref as msr
import redistance_exact_ref as rx

PLAIN = ["-O2"]
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
CELLS = (1, 2, 7, 64, 0)
Q_FAMILY = 96


def weld(X):
    """(V, F) of unwelded triangles X [nt, 3, 3]: equal positions become one vertex."""
    V, inv = np.unique(X.reshape(-1, 3), axis=0, return_inverse=True)
    return V, inv.reshape(-1, 3).astype(np.int64)


def golden_contour(case="bunny_small_n24", frac=0.25):
    d = load_golden(case)
    n, h, phi = int(d["n"]), float(d["cell"]), np.asarray(d["phi"], dtype=np.float64)
    return weld(rx.mesh(phi, n, d["bbox_min"], h, frac * float(phi.max())))


def read_obj(path):
    """(V, F) of an OBJ file, polygons fan-triangulated from each face's first vertex."""
    V, F = [], []
    with open(path) as f:
        for line in f:
            p = line.split()
            if not p:
                continue
            if p[0] == "v":
                V.append([float(x) for x in p[1:4]])
            elif p[0] == "f":
                ids = [int(x.split("/")[0]) - 1 for x in p[1:]]
                F += [[ids[0], ids[k], ids[k + 1]] for k in range(1, len(ids) - 1)]
    return np.array(V, dtype=np.float64), np.array(F, dtype=np.int64)


def patch_and_quad():
    g = np.linspace(0.25, 0.5, 25)
    x, y = np.meshgrid(g, g, indexing="ij")
    V = np.stack([x.ravel(), y.ravel(), 0.3 + 0.05 * np.sin(9 * x.ravel()) * np.cos(7 * y.ravel())], axis=1)
    idx = np.arange(25 * 25).reshape(25, 25)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    F = np.concatenate([np.stack([a, b, c], axis=1), np.stack([a, c, d], axis=1)])
    nv = len(V)
    V = np.concatenate([V, [[0.0, 0.0, 0.0], [1.0, 0.0, 0.1], [1.0, 1.0, 1.0], [0.0, 1.0, 0.9]]])
    F = np.concatenate([F, [[nv, nv + 1, nv + 2], [nv, nv + 2, nv + 3]]])
    return V, F.astype(np.int64)


def special_soup():
    rng = np.random.default_rng(3)
    ctr = rng.random((300, 3))
    V = (ctr[:, None, :] + 0.03 * rng.standard_normal((300, 3, 3))).reshape(-1, 3)
    F = np.arange(900, dtype=np.int64).reshape(300, 3)
    V[3 * 11] = np.nan
    V[3 * 12 + 1, 2] = np.inf
    extra = [F[5], F[5], [30, 30, 31], [40, 40, 40], F[7][::-1]]                       # duplicates, a segment, a point, a flipped copy
    cell = 1.0 / 64
    nv = len(V)
    V = np.concatenate([V, [[0.5, 0.5, 0.5], [0.5 + 4 * cell, 0.5, 0.5], [0.5 + 2 * cell, 0.5 + cell * 2.0 ** -30, 0.5]]])   # the needle
    F = np.concatenate([F, extra, [[nv, nv + 1, nv + 2]]])
    return V, F.astype(np.int64)


def smoothed_contour():
    V, F = golden_contour()
    return np.asarray(msr.smooth(V, F, 10), dtype=np.float64).reshape(-1, 3), F


MESHES = {"smoothed_n24": smoothed_contour, "bunny_small": lambda: read_obj(os.path.join(ROOT, "data", "bunny_small.obj")), "patch_and_quad": patch_and_quad,
          "special_soup": special_soup}
_CASE = {}


def case(name):
    """(V, F, the automatic index, families, all queries, {max_dist: brute force}) of a mesh, computed once."""
    if name not in _CASE:
        V, F = MESHES[name]()
        X = mir.build(V, F, 0)
        fam = mir.families(V, F, X, seed=7, Q=Q_FAMILY)
        pts = np.concatenate(list(fam.values()))
        side = (X["G"]["n"] - 1) * X["G"]["cell"]
        want = {md: mir.brute(V, F, pts, md) for md in (side / 16, np.inf)}
        _CASE[name] = (V, F, X, fam, pts, want)
    return _CASE[name]


def same(got, want, tag):
    for key in ("dist", "tri", "cp"):
        a, b = np.asarray(got[key]), np.asarray(want[key])
        assert a.shape == b.shape and a.dtype == b.dtype, (tag, key)
        nan = np.isnan(a) if a.dtype.kind == "f" else np.zeros(a.shape, bool)
        assert np.array_equal(nan, np.isnan(b) if b.dtype.kind == "f" else nan) and a[~nan].tobytes() == b[~nan].tobytes(), (tag, key)


@pytest.fixture(scope="module", params=[PLAIN, SAN], ids=["plain", "sanitizers"])
def program(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mesh_index") / "test_mesh_index")
    subprocess.check_call(["g++", *request.param, "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", os.path.join(ROOT, "tests", "native", "test_mesh_index.cpp"), "-o", exe])
    return exe


def test_native(program):
    """The stand-alone program's own checks (listed at its head): box, automatic c, ranges, big and sliver rules, the host walk against brute force."""
    out = subprocess.run([program], capture_output=True, text=True)
    print(out.stdout[-2000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-3000:] + out.stderr[-3000:]


def run_program(program, tmp_path, V, F, pts, cells, max_dist):
    f_mesh, f_pts, f_out = (str(tmp_path / x) for x in ("mesh.bin", "pts.bin", "out.bin"))
    with open(f_mesh, "wb") as f:
        np.array([len(V), len(F)], dtype=np.int64).tofile(f)
        np.ascontiguousarray(V, dtype=np.float64).tofile(f)
        np.ascontiguousarray(F, dtype=np.int64).tofile(f)
    np.ascontiguousarray(pts, dtype=np.float64).tofile(f_pts)
    p = subprocess.run([program, f_mesh, f_pts, str(cells), repr(float(max_dist)), f_out], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    w = np.fromfile(f_out, dtype=np.int64)
    rc, c, npairs, nbig, Q = (int(x) for x in w[:5])
    out = dict(rc=rc, c=c)
    if rc == 0:
        o = 5
        out["pair_cell"], out["pair_tri"], out["big"] = w[o:o + npairs], w[o + npairs:o + 2 * npairs], w[o + 2 * npairs:o + 2 * npairs + nbig]
        o += 2 * npairs + nbig
        out["dist"], out["cp"], out["tri"] = w[o:o + Q].view(np.float64), w[o + Q:o + 4 * Q].view(np.float64).reshape(-1, 3), w[o + 4 * Q:o + 5 * Q]
        assert o + 5 * Q == len(w)
    return out


@pytest.mark.parametrize("cells", [0, 7, 64])
@pytest.mark.parametrize("name", list(MESHES))
def test_program_equals_restatement(program, tmp_path, name, cells):
    """The header's filed (cell, triangle) pairs, its big list, its c and its answers equal the numpy restatement's, bit for bit."""
    V, F, _, _, pts, _ = case(name)
    X = mir.build(V, F, cells)
    side = (X["G"]["n"] - 1) * X["G"]["cell"]
    for md in (side / 16, np.inf):
        got = run_program(program, tmp_path, V, F, pts, cells, md)
        assert got["rc"] == 0 and got["c"] == X["c"]
        assert np.array_equal(got["pair_cell"], X["pair_cell"]) and np.array_equal(got["pair_tri"], X["pair_tri"]) and np.array_equal(np.sort(got["big"]), X["big"])
        same(got, mir.answers(X, pts, md), (name, cells, md))


def test_program_refusals(program, tmp_path):
    """An index out of range, c > 512 and a big list that is too long are refused by the header with the codes of its enum."""
    V, F = patch_and_quad()
    bad = F.copy()
    bad[3, 1] = len(V)
    assert run_program(program, tmp_path, V, bad, np.zeros((1, 3)), 0, 1.0)["rc"] == 1
    assert run_program(program, tmp_path, V, F, np.zeros((1, 3)), 513, 1.0)["rc"] == 4
    big = np.tile(F[-2:], (2100, 1))
    assert run_program(program, tmp_path, V, big, np.zeros((1, 3)), 64, 1.0)["rc"] == 2
    with pytest.raises(mir.Refused):
        mir.build(V, big, 64)
    assert run_program(program, tmp_path, V, big, np.zeros((1, 3)), 0, 1.0)["c"] == mir.build(V, big, 0)["c"] < 5     # the automatic c is halved instead


@pytest.mark.parametrize("name", list(MESHES))
def test_restatement_equals_brute_force(name):
    """Every family, both max_dist, at the automatic c: the index loses nothing."""
    V, F, X, fam, pts, want = case(name)
    assert len(X["cand"]) > 0
    if name == "special_soup":
        assert len(X["cand"]) < len(F) and len(X["big"]) >= 1          # NaN corners are skipped; the needle is a sliver
    for md, w in want.items():
        assert w["n_answered"] > 0
        same(mir.answers(X, pts, md), w, (name, md))
    far = mir.answers(X, fam["far"], np.inf)
    assert far["answered"].all()                                         # 10^3 box sides away, max_dist = inf: answered all the same
    onv = mir.answers(X, fam["on_vertices"], np.inf)
    assert (onv["dist"] == 0).all()


@pytest.mark.parametrize("name", list(MESHES))
def test_resolution_independence(name):
    """c in {1, 2, 7, 64, automatic}: identical bits."""
    V, F, X, _, pts, want = case(name)
    for cells in CELLS[:-1]:
        Y = mir.build(V, F, cells)
        if name == "patch_and_quad" and cells == 64:
            assert len(Y["big"]) == 2                                    # the quad's two triangles span the box
        for md, w in want.items():
            same(mir.answers(Y, pts, md), w, (name, cells, md))


def test_a_seeded_defect_shows():
    """With every range shrunk by one cell on the upper side, some family disagrees with brute force: the inputs reach the rule."""
    shown = 0
    for name in MESHES:
        V, F, _, fam, _, _ = case(name)
        Y = mir.build(V, F, 64, shrink_upper=True)
        for k, pts in fam.items():
            got, want = mir.answers(Y, pts, np.inf), mir.brute(V, F, pts, np.inf)
            shown += int(not (np.array_equal(got["dist"], want["dist"], equal_nan=True) and np.array_equal(got["tri"], want["tri"])))
    assert shown > 0


def test_deviation_on_the_cpu():
    """The one-sided deviation of the 24^3 contour and of its smoothed version from bunny_small.obj's faces, in cells, from the restatement: the quantity
    tools/mesh_index_bench.py measures on the device.  The contour lies within a cell or two of the input here (0.25 max phi is not the surface itself: the
    numbers are a measurement, the assertion only that they are finite and of the grid's scale)."""
    d = load_golden("bunny_small_n24")
    Vi, Fi = read_obj(os.path.join(ROOT, "data", "bunny_small.obj"))
    X = mir.build(Vi, Fi, 0)
    Vc, Fc = golden_contour()
    Vs, _ = smoothed_contour()
    h = float(d["cell"])
    for tag, P in (("contour", Vc), ("smoothed", Vs)):
        mx, mean = mir.deviation(X, P[::4])
        print("%s -> input faces: max %.4f cell, mean %.4f cell" % (tag, mx / h, mean / h))
        assert 0 <= mean <= mx < int(d["n"]) * h
