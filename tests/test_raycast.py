"""Ray casts against a level set of the resident phi (shm_grid_raycast / shm_grid_raycast_device, include/shm_grid.h; kernels in csrc/shm_raycast.hip.h),
through the kernels, the C ABI, the Python bindings, the C++ host mirror and the CLI.

Reference: tests/ray_ref.py, a numpy restatement that walks EVERY cell a ray crosses (sorted plane parameters, the cell of each interval's midpoint) and
knows neither bricks nor a DDA.  It is fed the device's own phi.

Acceptance rule of the GPU comparisons.  A ray AGREES when both sides miss, or both hit with |t_dev - t_ref| <= 1e-9 cell / |d|: rounding of f (about 30
operations * 2^-53 * max|phi|) over the smallest |f'| the inputs show, four decades above the 7e-14 cell / |d| between the restatement in float64 and in
long double.  A ray that does not agree is IN DISPUTE, and a dispute is allowed only if the restatement certifies the ray as grazing (its gap
<= 1e-6 max|phi|) and disputes stay <= 0.1 % of the rays of the family.  test_restatement_is_stable_on_the_test_rays shows that on the goldens' phi the
test's own rays leave the restatement alone at zero disputes and no gap below 1e-6 max|phi|.
Gradient on agreeing hits: held to the restatement's gradient in its own cell at t_ref, within
    2 * 1e-9 cell * (max(|kxy|, |kxz|, |kyz|) + |kxyz|) / cell^2  +  1e-13 max|phi| / cell
-- a hit displaced by 1e-9 cell moves a component of the trilinear gradient by at most two of the cell's second derivatives (mixed second differences
/ cell^2) times the displacement; the second term is test_sample.py's bound on the formula itself."""
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

import ray_ref
from test_sample import eval_ref
from test_iso_indexed import bound, isovalues, problem, solved, ISO_NAMES

SHM_ERR_INVALID, SHM_ERR_STATE = 1, 7
FAMILIES = ["camera", "inside", "grid_lines", "face_planes"]


# ---- the ray families -----------------------------------------------------------------------------------------------------------------------------------------
def rays(d, phi, family, count, seed):
    """(origins, dirs) of one family on problem d (its phi decides where 'inside' starts)."""
    n, b, h = int(d["n"]), np.asarray(d["bbox_min"], dtype=np.float64), float(d["cell"])
    rng = np.random.default_rng(seed)
    hi = (n - 1) * h + b
    if family == "camera":   # origins on a sphere of 1.5 box radii, aimed at sources with +-2 cells of jitter; d is not normalised
        c = (b + hi) / 2
        R = 1.5 * np.linalg.norm(hi - b) / 2
        u = rng.standard_normal((count, 3))
        O = c + R * u / np.linalg.norm(u, axis=1, keepdims=True)
        tgt = np.asarray(d["pos"])[rng.integers(0, len(d["pos"]), count)] + rng.uniform(-2 * h, 2 * h, (count, 3))
        D = (tgt - O) * rng.uniform(0.2, 3.0, (count, 1))
        return O, D
    if family == "inside":   # random origins and directions inside the box, plus origins at nodes with phi < 0 (they start inside the surface)
        m = count // 2
        O = rng.uniform(b, hi, (m, 3))
        neg = np.nonzero(np.asarray(phi) < 0)[0]
        pick = neg[rng.integers(0, len(neg), count - m)] if len(neg) else rng.integers(0, n ** 3, count - m)
        nodes = np.stack([pick % n, (pick // n) % n, pick // (n * n)], axis=1)
        O = np.concatenate([O, nodes * h + b])
        D = rng.standard_normal((count, 3)) * rng.uniform(0.2, 3.0, (count, 1))
        return O, D
    if family == "grid_lines":   # origins on nodes, d = +-e_a
        nodes = rng.integers(0, n, (count, 3))
        O = nodes * h + b
        D = np.zeros((count, 3))
        D[np.arange(count), rng.integers(0, 3, count)] = rng.choice([-1.0, 1.0], count)
        return O, D
    if family == "face_planes":   # an axis-parallel ray with one other coordinate on a grid plane, the third anywhere; started outside the box
        a = rng.integers(0, 3, count)
        o2 = (a + rng.integers(1, 3, count)) % 3
        sgn = rng.choice([-1.0, 1.0], count)
        O = rng.uniform(b, hi, (count, 3))
        r = np.arange(count)
        O[r, o2] = rng.integers(0, n, count) * h + b[o2]
        O[r, a] = np.where(sgn > 0, b[a] - 1.5 * h, hi[a] + 1.5 * h)
        D = np.zeros((count, 3))
        D[r, a] = sgn
        return O, D
    raise KeyError(family)


def degenerate_rays(d):
    """(origins, dirs, expect): expect[q] is 'nan' where the contract says NaN, else None (the restatement decides).  Cast with t in [0, inf]."""
    n, b, h = int(d["n"]), np.asarray(d["bbox_min"], dtype=np.float64), float(d["cell"])
    hi = (n - 1) * h + b
    c = (b + hi) / 2
    O, D, E = [], [], []

    def add(o, dd, e):
        O.append(np.array(o, dtype=np.float64))
        D.append(np.array(dd, dtype=np.float64))
        E.append(e)
    add(c, [0, 0, 0], "nan")                                       # d = 0
    add([np.nan, c[1], c[2]], [1, 0, 0], "nan")
    add(c, [1, np.nan, 0], "nan")
    add([np.inf, c[1], c[2]], [-1, 0, 0], "nan")
    add(c, [np.inf, 0, 0], "nan")
    add(hi + h, [1, 1, 1], "nan")                                  # outside, pointing away
    add(b - h, [-1, 0.5, 0], "nan")
    for a in range(3):                                             # parallel to a face, just outside it
        for side in (np.nextafter(b[a], -np.inf), np.nextafter(hi[a], np.inf)):
            o = c.copy()
            o[a] = side
            dd = np.zeros(3)
            dd[(a + 1) % 3] = 1.0
            add(o, dd, "nan")
    for a in range(3):                                             # ... and just inside it, and on it
        for side in (b[a], hi[a]):
            o = c.copy()
            o[a] = side
            o[(a + 1) % 3] = b[(a + 1) % 3] - h
            dd = np.zeros(3)
            dd[(a + 1) % 3] = 1.0
            add(o, dd, None)
    add(hi, [-1, -1, -1], None)                                    # origin exactly on the upper corner, into the box
    add(hi, [1, 1, 1], None)                                       # ... and out of it: the box is touched at t = 0 only
    add(hi, [-1, 0, 0], None)
    add(b, [1, 1, 1], None)
    add(b - h, [1, 1, 1], None)                                    # the main diagonal: through nodes, ties on all three axes
    return np.array(O), np.array(D), E


def check_family(t, g, O, D, phi, d, iso, who, tol_t=1e-9):
    """The acceptance rule.  Returns (ref, agreeing mask)."""
    n, b, h = int(d["n"]), np.asarray(d["bbox_min"], dtype=np.float64), float(d["cell"])
    scale = float(np.abs(phi).max())
    ref = ray_ref.raycast_ref(phi, n, b, h, O, D, iso)
    ok = ray_ref.agree(t, ref["t"], h, D, tol_t)
    disputed = ~ok
    worst = float(np.nanmax(np.abs(t - ref["t"]) * np.linalg.norm(D, axis=1) / h)) if np.isfinite(t - ref["t"]).any() else 0.0
    print("%s: %d rays, %d hits (ref %d), %d in dispute, max |dt| %.3g cell/|d|, min gap %.3g max|phi|"
          % (who, len(t), np.isfinite(t).sum(), np.isfinite(ref["t"]).sum(), disputed.sum(), worst, float(ref["gap"].min()) / scale))
    assert (ref["gap"][disputed] <= 1e-6 * scale).all(), (who, np.nonzero(disputed)[0][:10], t[disputed][:10], ref["t"][disputed][:10], ref["gap"][disputed][:10] / scale)
    assert disputed.sum() <= 1e-3 * len(t), (who, int(disputed.sum()))
    if g is not None:
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
    return ref, ok


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------------------------------------
def _golden(name):
    d = dict(load_golden(name))
    return d, np.asarray(d["phi"], dtype=np.float64)


def test_restatement_matches_eval_ref_at_its_hits():
    """At every hit the restatement reports, eval_ref's trilinear value is the isovalue (to rounding of f) and eval_ref's gradient in the restatement's cell is
    the restatement's; before the hit the ray stays on one side (sampled: no earlier crossing at 64 points per cell of travel)."""
    d, phi = _golden("bunny_small_n16")
    n, b, h = int(d["n"]), d["bbox_min"], float(d["cell"])
    scale = np.abs(phi).max()
    for iso in (0.0, 0.25 * phi.max()):
        for fam in FAMILIES:
            O, D = rays(d, phi, fam, 300, 11)
            r = ray_ref.raycast_ref(phi, n, b, h, O, D, iso)
            hit = np.isfinite(r["t"])
            assert hit.any()
            P = O[hit] + r["t"][hit, None] * D[hit]
            v = eval_ref(phi, n, b, h, np.clip(P, b, (n - 1) * h + b))
            assert np.abs(v - iso).max() <= 1e-12 * scale, np.abs(v - iso).max() / scale
            # no crossing before the hit, none at all on a miss: f keeps the sign it has at the start of the clipped interval
            for q in np.nonzero(np.isfinite(O).all(1))[0][:120]:
                dn = np.linalg.norm(D[q])
                tend = r["t"][q] if hit[q] else 4 * n * h / dn
                ts = np.linspace(0, tend, int(64 * tend * dn / h) + 2)[:-1]
                vv = eval_ref(phi, n, b, h, O[q] + ts[:, None] * D[q]) - iso
                vv = vv[np.isfinite(vv)]
                if hit[q] and len(vv) > 2:
                    vv = vv[:-1]   # (the last sample may sit within rounding of the hit)
                assert len(vv) == 0 or (vv > 0).all() or (vv < 0).all(), (fam, iso, q)


def test_restatement_reproduces_marching_cubes_edge_positions():
    """A ray from a cut edge's lower node along the edge with t in [0, cell] returns (iso - va) / (vb - va) * cell to 8 * 2^-53 * cell, and the same from the
    upper node backwards."""
    d, phi = _golden("bunny_small_n32")
    n, b, h = int(d["n"]), np.asarray(d["bbox_min"]), float(d["cell"])
    U = phi.reshape(n, n, n)
    for iso in (0.0, 0.25 * phi.max()):
        O, D, T = [], [], []
        for ax in range(3):
            sl_a = [slice(None)] * 3
            sl_b = [slice(None)] * 3
            sl_a[2 - ax] = slice(0, n - 1)
            sl_b[2 - ax] = slice(1, n)
            va, vb = U[tuple(sl_a)], U[tuple(sl_b)]
            cut = (va < iso) != (vb < iso)
            k, j, i = np.nonzero(cut)
            lower = np.stack([i, j, k], axis=1) * h + b
            e = np.zeros(3)
            e[ax] = 1.0
            tt = (iso - va[cut]) / (vb[cut] - va[cut]) * h
            O += [lower, lower + h * e]
            D += [np.tile(e, (len(tt), 1)), np.tile(-e, (len(tt), 1))]
            T += [tt, h - tt]
        O, D, T = np.concatenate(O), np.concatenate(D), np.concatenate(T)
        assert len(T) > 400
        r = ray_ref.raycast_ref(phi, n, b, h, O, D, iso, 0.0, h)
        assert np.isfinite(r["t"]).all()
        err = np.abs(r["t"] - T) / h
        fwd = D.sum(1) > 0
        print("iso %.3g: %d edges, max error forward %.3g cell, backward %.3g cell" % (iso, fwd.sum(), err[fwd].max(), err[~fwd].max()))
        assert err.max() <= 8 * 2.0 ** -53, (err[fwd].max(), err[~fwd].max())


@pytest.mark.parametrize("case", ["bunny_small_n16", "bunny_small_n32"])
def test_restatement_is_stable_on_the_test_rays(case):
    """The restatement in float64 against itself in x87 long double, on the goldens' phi with the test's own ray generators: 0 disputes and no gap
    below 1e-6 max|phi| -- so on these inputs a dispute of the device with the restatement is the device's."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("long double is double on this platform")
    d, phi = _golden(case)
    n, b, h = int(d["n"]), d["bbox_min"], float(d["cell"])
    scale = np.abs(phi).max()
    for iso in (0.0, 0.25 * phi.max()):
        for fam in FAMILIES:
            O, D = rays(d, phi, fam, 350, 5)
            r64 = ray_ref.raycast_ref(phi, n, b, h, O, D, iso)
            r80 = ray_ref.raycast_ref(phi, n, b, h, O, D, iso, dtype=np.longdouble)
            ok = ray_ref.agree(r64["t"], r80["t"].astype(np.float64), h, D)
            hits = np.isfinite(r64["t"]).sum()
            print(case, iso, fam, "hits", hits, "of", len(O), "min gap", float(r64["gap"].min() / scale))
            assert ok.all(), (fam, iso, np.nonzero(~ok)[0])
            assert r64["gap"].min() > 1e-6 * scale, (fam, iso, float(r64["gap"].min() / scale), int(np.argmin(r64["gap"])))
            assert 0 < hits
            if fam == "camera":
                share = hits / len(O)
                assert (share > 0.4 and share < 0.9) if iso == 0.0 else share > 0.97, share


def test_kernel_header_on_the_host_under_sanitizers(tmp_path):
    """csrc/shm_raycast.hip.h compiled for the host (tests/native/raycast_host.cpp: one lane, launches as loops) with AddressSanitizer and UBSan, on the
    golden 16^3 phi with one and three slabs: every family and the degenerate rays at the zero, box and an empty level, plus a phi with NaN and inf nodes.
    No address outside an allocation is formed (the sanitizers abort otherwise), and the answers pass the GPU tests' acceptance rule."""
    src = open(os.path.join(ROOT, "signed-heat-3d_amd", "csrc", "shm_raycast.hip.h")).read()
    assert '#include "shm_kernels.hip.h"' in src
    (tmp_path / "shm_raycast_host.h").write_text(src.replace('#include "shm_kernels.hip.h"', ""))
    exe = str(tmp_path / "raycast_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", str(tmp_path), os.path.join(ROOT, "tests", "native", "raycast_host.cpp"), "-o", exe])
    d, phi = _golden("bunny_small_n16")
    n, b, h = int(d["n"]), np.asarray(d["bbox_min"]), float(d["cell"])
    np.concatenate([b, [h]]).tofile(tmp_path / "grid.f64")

    def cast(field, O, D, iso, slabs):
        np.asarray(field, dtype=np.float64).tofile(tmp_path / "phi.f64")
        np.concatenate([O, D], axis=1).tofile(tmp_path / "rays.f64")
        p = subprocess.run([exe, str(n), str(slabs), str(tmp_path / "phi.f64"), str(tmp_path / "rays.f64"), str(len(O)), str(tmp_path / "grid.f64"), repr(float(iso)),
                            "0", "inf", str(tmp_path / "out.f64")], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-3000:]
        raw = np.fromfile(tmp_path / "out.f64")
        return raw[:len(O)], raw[len(O):].reshape(-1, 3)
    isos = isovalues(phi)
    sets = {fam: rays(d, phi, fam, 400, 21 + f) for f, fam in enumerate(FAMILIES)}
    sets["degenerate"] = degenerate_rays(d)[:2]
    for slabs in (1, 3):
        for name in ("zero", "box", "above"):
            for fam, (O, D) in sets.items():
                t, g = cast(phi, O, D, isos[name], slabs)
                check_family(t, g, O, D, phi, d, isos[name], "host build, %d slab(s), %s %s" % (slabs, name, fam))
    bad = phi.copy()
    bad[::97] = np.nan
    bad[5::101] = np.inf
    O, D = sets["camera"]
    t, g = cast(bad, O, D, 0.0, 3)
    ref, ok = check_family(t, None, O, D, bad, d, 0.0, "host build, non-finite nodes")   # (max|phi| is not finite here: t alone, no dispute allowed)
    assert ok.all() and 0 < np.isfinite(t).sum() < len(t) and np.isfinite(g[np.isfinite(t)]).all()


def test_raycast_entry_points_are_declared_and_exported(shm):
    lib = shm.load_library()
    from signed_heat_3d_amd.grid_abi import ABI_SYMBOLS
    header = open(os.path.join(ROOT, "include", "shm_grid.h")).read()
    for name in ("shm_grid_raycast", "shm_grid_raycast_device"):
        assert name in ABI_SYMBOLS and hasattr(lib, name) and (name + "(") in header
    assert lib.shm_grid_abi_version() == 5


def test_cli_help_lists_the_ray_flags():
    exe = os.path.join(ROOT, "signed-heat-3d_amd", "bin", "shm_grid_cli")
    p = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert p.returncode == 0
    for flag in ("--rays <file>", "--rays-out <file>", "--rays-iso <v>"):
        assert flag in p.stdout, flag


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("n", [16, 24, 32, 33, 11])
def test_parity_with_the_restatement(shm, n, precision):
    """A.  15, 23, 31, 32 and 10 cells: a partial last brick of 7, one of 7 beside two full ones, 7 again, none, and two bricks with a 2-cell remainder.
    Every isovalue of test_iso_indexed (closed, into the box, a few cells, two empty ones), every family, and the degenerate rays."""
    d, s, phi = solved(shm, "bunny_small", n, precision)
    isos = isovalues(phi)
    for name in ISO_NAMES:
        iso = isos[name]
        total_hits = 0
        for f, fam in enumerate(FAMILIES):
            O, D = rays(d, phi, fam, 2000, 1000 * n + 10 * f + precision)
            t, g, nh = s.raycast(O, D, iso, grad=True)
            assert nh == np.isfinite(t).sum()
            total_hits += nh
            who = "n=%d fp%d %s %s" % (n, precision, name, fam)
            ref, ok = check_family(t, g, O, D, phi, d, iso, who)
            # hits AND misses in every family at the three levels with a surface of some size (at 0.25 max every camera ray hits; the few cells of the
            # half_min level are held to hits and misses over the families together, below)
            if name in ("zero", "quarter_max", "box"):
                assert 0 < nh, who
                assert nh < len(t) or (fam == "camera" and name == "quarter_max"), who
            if fam == "camera" and n == 32 and name in ("zero", "quarter_max"):
                share = nh / len(t)
                assert (0.4 < share < 0.9) if name == "zero" else share > 0.97, (who, share)
        if name == "half_min":
            assert 0 < total_hits < 4 * 2000, total_hits
        if name in ("below", "above"):
            assert total_hits == 0, name   # (every brick is skipped)
    # degenerate rays at iso 0, t in [0, inf]
    O, D, E = degenerate_rays(d)
    t, g, nh = s.raycast(O, D, 0.0, 0.0, np.inf, grad=True)
    for q, e in enumerate(E):
        if e == "nan":
            assert np.isnan(t[q]) and np.isnan(g[q]).all(), (q, O[q], D[q], t[q])
    check_family(t, g, O, D, phi, d, 0.0, "n=%d fp%d degenerate" % (n, precision))
    # t ranges: t_min > t_max is NaN for every ray; a range that ends before the surface misses; one that starts behind it finds what comes next
    O, D = rays(d, phi, "camera", 500, 77 + n)
    t_all = s.raycast(O, D, 0.0)[0]
    hit = np.isfinite(t_all)
    assert hit.any()
    t_bad, nh = s.raycast(O, D, 0.0, 2.0, 1.0)
    assert nh == 0 and np.isnan(t_bad).all()
    tcut = 0.9 * float(t_all[hit].min())
    t_short, nh = s.raycast(O, D, 0.0, 0.0, tcut)
    assert nh == 0 and np.isnan(t_short).all()
    tmid = float(np.median(t_all[hit]))
    t_late, g_late, nh = s.raycast(O, D, 0.0, tmid, np.inf, grad=True)
    n_, b_, h_ = int(d["n"]), d["bbox_min"], float(d["cell"])
    r_late = ray_ref.raycast_ref(phi, n_, b_, h_, O, D, 0.0, tmid, np.inf)
    ok = ray_ref.agree(t_late, r_late["t"], h_, D)
    assert (r_late["gap"][~ok] <= 1e-6 * np.abs(phi).max()).all() and (~ok).sum() <= 1e-3 * len(ok)
    assert np.nanmin(t_late) >= tmid


@pytest.mark.gpu
def test_parity_at_128_cubed(shm):
    """A, the large case: 20 000 camera rays at 128^3 (16 bricks per side, the last one of 7 cells), iso 0."""
    d, s, phi = solved(shm, "bunny_small", 128, 64)
    O, D = rays(d, phi, "camera", 20000, 128)
    t, g, nh = s.raycast(O, D, 0.0, grad=True)
    assert 0 < nh < len(t)
    check_family(t, g, O, D, phi, d, 0.0, "n=128 camera")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [32, 33])
def test_edge_rays_hit_the_indexed_mesh_vertices(shm, n):
    """B.  For every vertex of isosurface_indexed(iso), the ray along its grid edge from each end, t in [0, cell], hits within 8 * 2^-53 * bound of the
    vertex: the vertex order gives each vertex its edge (3 g + axis ascending over the cut edges), the mesh code gives its position."""
    d, s, phi = solved(shm, "bunny_small", n, 64)
    b, h = np.asarray(d["bbox_min"]), float(d["cell"])
    U = phi.reshape(n, n, n)
    for iso in (0.0, 0.25 * float(phi.max())):
        V, F = s.isosurface_indexed(iso)
        inside = U < iso
        keys = []
        g = np.arange(n ** 3).reshape(n, n, n)
        keys.append(3 * g[:, :, :-1][inside[:, :, :-1] != inside[:, :, 1:]])
        keys.append(3 * g[:, :-1, :][inside[:, :-1, :] != inside[:, 1:, :]] + 1)
        keys.append(3 * g[:-1][inside[:-1] != inside[1:]] + 2)
        keys = np.sort(np.concatenate(keys))
        assert len(keys) == len(V) > 100
        gg, ax = keys // 3, keys % 3
        lower = np.stack([gg % n, (gg // n) % n, gg // (n * n)], axis=1)
        E = np.eye(3)[ax]
        O = np.concatenate([lower * h + b, (lower + E.astype(np.int64)) * h + b])
        D = np.concatenate([E, -E])
        t, nh = s.raycast(O, D, iso, 0.0, h)
        assert nh == len(t), (nh, len(t))
        P = O + t[:, None] * D
        err = np.abs(P - np.concatenate([V, V])).max()
        assert err <= 8 * 2.0 ** -53 * bound(d), err / bound(d)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [32, 33])
@pytest.mark.parametrize("slabs", [1, 3, 5])
def test_slabs(shm, n, slabs):
    """C.  Any local_slabs: rays along z through every seam plane, rays lying in seam planes, and the families; each handle against the restatement of
    its own phi, and against the one-slab handle up to what the two solves' phi differ by: |dt| <= 4 dphi / |f'| plus the tolerance."""
    kw = dict(solver="primal", precond="none")
    d, s, phi = solved(shm, "bunny_small", n, 64, slabs, **kw)
    _, s1, phi1 = solved(shm, "bunny_small", n, 64, 1, **kw)
    b, h = np.asarray(d["bbox_min"]), float(d["cell"])
    rng = np.random.default_rng(40 + n + slabs)
    seams = [shm.plan_slab(n, slabs, sl)[0] for sl in range(1, slabs)] or [n // 2]
    m = 1500
    ij = rng.uniform(b[:2], (n - 1) * h + b[:2], (m, 2))
    Oz = np.concatenate([ij, np.full((m, 1), b[2] - h)], axis=1)
    Dz = np.tile([0.0, 0.0, 1.0], (m, 1))
    Dz[m // 2:] *= -1
    Oz[m // 2:, 2] = (n - 1) * h + b[2] + h
    Os, Ds = [], []
    for kb in seams:
        for kk in (kb, kb - 1):   # rays lying in the seam plane and in the plane below it, aimed at the sources nearest to that plane
            z = kk * h + b[2]
            near = np.argsort(np.abs(d["pos"][:, 2] - z))[:max(20, len(d["pos"]) // 10)]
            o = rng.uniform(b - h, (n - 1) * h + b + h, (200, 3))
            o[:, 2] = z
            dd = d["pos"][near[rng.integers(0, len(near), 200)]] - o
            dd[:, 2] = 0.0
            Os.append(o)
            Ds.append(dd)
    sets = {"z": (Oz, Dz), "seam_planes": (np.concatenate(Os), np.concatenate(Ds))}
    for f, fam in enumerate(FAMILIES):
        sets[fam] = rays(d, phi, fam, 800, 7 * n + f)
    dphi = float(np.abs(phi - phi1).max())
    for iso in (0.0, 0.25 * float(phi.max())):
        for name, (O, D) in sets.items():
            t, g, nh = s.raycast(O, D, iso, grad=True)
            # (the model is flat in z: at iso 0 the outer seam planes of three and five slabs pass above and below it; the 0.25 max level reaches them)
            assert 0 < nh or (name == "seam_planes" and iso == 0.0), (name, iso)
            ref, ok = check_family(t, g, O, D, phi, d, iso, "slabs=%d n=%d %s iso=%.3g" % (slabs, n, name, iso))
            t1 = s1.raycast(O, D, iso)[0]
            both = np.isfinite(t) & np.isfinite(t1) & ok
            # f' is per unit t: a change of phi by dphi moves a simple root by at most dphi / |f'| (4x: f' itself moves with phi over the displacement)
            lim = 4 * dphi / np.abs(ref["fprime"][both]) + 1e-9 * h / np.linalg.norm(D[both], axis=1)
            far = np.abs(t[both] - t1[both]) > lim
            # a ray whose first crossing is marginal under a change of dphi may find another crossing first: certified by the restatement's gap
            assert (ref["gap"][both][far] <= 4 * dphi + 1e-6 * np.abs(phi).max()).all(), (name, int(far.sum()))
            flips = np.isfinite(t) != np.isfinite(t1)
            assert (ref["gap"][flips] <= 4 * dphi + 1e-6 * np.abs(phi).max()).all(), (name, int(flips.sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [64, 32])
def test_device_entry_equals_the_host_entry(shm, precision):
    """D.  array_equal with NaNs after the host result is rounded to the tensor type; host memory and an oversize Q are refused with status 1 before any
    launch, and the handle goes on working."""
    if torch is None or not torch.cuda.is_available():
        pytest.fail("torch with a HIP device is needed for the device entry point")
    d, s, phi = solved(shm, "bunny_small", 33, precision)
    npdt = np.float64 if precision == 64 else np.float32
    O = np.concatenate([rays(d, phi, fam, 1500, 3 + f)[0] for f, fam in enumerate(FAMILIES)]).astype(npdt)
    D = np.concatenate([rays(d, phi, fam, 1500, 3 + f)[1] for f, fam in enumerate(FAMILIES)]).astype(npdt)
    Od, Dd, _ = degenerate_rays(d)
    O, D = np.concatenate([O, Od.astype(npdt)]), np.concatenate([D, Dd.astype(npdt)])
    dev = torch.device("cuda", 0)
    for iso in (0.0, 0.25 * float(phi.max())):
        th, gh, nh = s.raycast(O.astype(np.float64), D.astype(np.float64), iso, grad=True)
        td, gd, nd = s.raycast_device(torch.from_numpy(O).to(dev), torch.from_numpy(D).to(dev), iso, grad=True)
        assert td.dtype == (torch.float64 if precision == 64 else torch.float32) and td.is_cuda
        assert nd == nh and 0 < nh < len(th)
        assert np.array_equal(td.cpu().numpy(), th.astype(npdt), equal_nan=True)
        assert np.array_equal(gd.cpu().numpy(), gh.astype(npdt), equal_nan=True)
        td2, nd2 = s.raycast_device(torch.from_numpy(O).to(dev), torch.from_numpy(D).to(dev), iso)
        assert nd2 == nd and torch.equal(torch.nan_to_num(td2, nan=-1.0), torch.nan_to_num(td, nan=-1.0))
    if precision == 64:
        # more than two chunks of 2^20 rays and a short last one through the host entry: slot reuse, the last chunk and the sum of n_hits over chunks
        reps = (2 * (1 << 20) + 1) // len(O) + 1
        Ob, Db = np.tile(O, (reps, 1))[:2 * (1 << 20) + 1 + 300], np.tile(D, (reps, 1))[:2 * (1 << 20) + 1 + 300]
        tb, gb, nb = s.raycast(Ob, Db, 0.0, grad=True)
        tdb, gdb, ndb = s.raycast_device(torch.from_numpy(Ob).to(dev), torch.from_numpy(Db).to(dev), 0.0, grad=True)
        assert nb == ndb == np.isfinite(tb).sum() > 0
        assert np.array_equal(tdb.cpu().numpy(), tb, equal_nan=True) and np.array_equal(gdb.cpu().numpy(), gb, equal_nan=True)
        del tdb, gdb
    # refusals, before anything is launched
    import ctypes as C
    lib, h = s._lib, s._h
    Q = 64
    o_d, d_d = torch.from_numpy(O[:Q].copy()).to(dev), torch.from_numpy(D[:Q].copy()).to(dev)
    t_d = torch.empty(Q, dtype=o_d.dtype, device=dev)
    host = np.zeros(3 * Q, dtype=npdt)
    nh = C.c_int64(-5)
    inf = float("inf")
    assert lib.shm_grid_raycast_device(h, Q, host.ctypes.data, d_d.data_ptr(), 0.0, 0.0, inf, t_d.data_ptr(), None, C.byref(nh)) == SHM_ERR_INVALID
    assert lib.shm_grid_raycast_device(h, Q, o_d.data_ptr(), host.ctypes.data, 0.0, 0.0, inf, t_d.data_ptr(), None, C.byref(nh)) == SHM_ERR_INVALID
    assert lib.shm_grid_raycast_device(h, Q, o_d.data_ptr(), d_d.data_ptr(), 0.0, 0.0, inf, host.ctypes.data, None, C.byref(nh)) == SHM_ERR_INVALID
    assert lib.shm_grid_raycast_device(h, Q, o_d.data_ptr(), d_d.data_ptr(), 0.0, 0.0, inf, t_d.data_ptr(), host.ctypes.data, C.byref(nh)) == SHM_ERR_INVALID
    assert lib.shm_grid_raycast_device(h, 1 << 40, o_d.data_ptr(), d_d.data_ptr(), 0.0, 0.0, inf, t_d.data_ptr(), None, C.byref(nh)) == SHM_ERR_INVALID
    for big in ((1 << 61) // 3 + 1, (1 << 63) - 1):   # 24 Q wraps in 64 bits: refused by the cap on Q, never multiplied
        assert lib.shm_grid_raycast_device(h, big, o_d.data_ptr(), d_d.data_ptr(), 0.0, 0.0, inf, t_d.data_ptr(), None, C.byref(nh)) == SHM_ERR_INVALID
        assert lib.shm_grid_raycast(h, big, host.ctypes.data, host.ctypes.data, 0.0, 0.0, inf, host.ctypes.data, None, C.byref(nh)) == SHM_ERR_INVALID
    assert nh.value == -5
    t_again, n_again = s.raycast_device(o_d, d_d, 0.0)
    assert np.array_equal(t_again.cpu().numpy(), s.raycast(O[:Q].astype(np.float64), D[:Q].astype(np.float64), 0.0)[0].astype(npdt), equal_nan=True)


@pytest.mark.gpu
def test_state_rules(shm):
    """E.  Status 7 before a solve and after apply_laplacian; status 1 for Q < 0, NULL arguments and a NaN isovalue; Q = 0 is valid; a second call is
    bit-identical; a new solve with other sources is seen by the next cast (the brick cache falls with phi); phi, the indexed mesh and sample are unchanged
    around a cast."""
    import ctypes as C
    d = problem("bunny_small", 24)
    n, b, h = int(d["n"]), np.asarray(d["bbox_min"]), float(d["cell"])
    s = shm.GridSolver()
    lib, hd = s._lib, s._h
    O, D = rays(d, np.zeros(n ** 3), "camera", 3000, 1)
    t = np.empty(len(O))
    nh = C.c_int64()
    inf = float("inf")

    def call(Q, o, dd, iso, tp):
        return lib.shm_grid_raycast(hd, Q, o, dd, iso, 0.0, inf, tp, None, C.byref(nh))
    s.set_problem(d["pos"], d["wnormal"], d["area"], float(d["lam"]), n, b, h)
    assert call(len(O), O.ctypes.data, D.ctypes.data, 0.0, t.ctypes.data) == SHM_ERR_STATE   # before a solve
    s.solve(tol=1e-10)
    assert call(-1, O.ctypes.data, D.ctypes.data, 0.0, t.ctypes.data) == SHM_ERR_INVALID
    assert call(len(O), None, D.ctypes.data, 0.0, t.ctypes.data) == SHM_ERR_INVALID
    assert call(len(O), O.ctypes.data, None, 0.0, t.ctypes.data) == SHM_ERR_INVALID
    assert call(len(O), O.ctypes.data, D.ctypes.data, 0.0, None) == SHM_ERR_INVALID
    assert call(len(O), O.ctypes.data, D.ctypes.data, float("nan"), t.ctypes.data) == SHM_ERR_INVALID
    assert call(0, None, None, 0.0, None) == 0 and nh.value == 0
    phi0 = s.get_phi()[0]
    V0, F0 = s.isosurface_indexed(0.0)
    pts = O + 0.5 * D
    v0 = s.sample(pts)[0]
    t1, g1, n1 = s.raycast(O, D, 0.0, grad=True)
    t2, g2, n2 = s.raycast(O, D, 0.0, grad=True)
    assert n1 == n2 > 0 and np.array_equal(t1, t2, equal_nan=True) and np.array_equal(g1, g2, equal_nan=True)
    assert np.array_equal(s.get_phi()[0], phi0)
    V1 = np.empty_like(V0)
    F1 = np.empty_like(F0)
    s._chk(lib.shm_grid_get_isosurface_indexed(hd, V1.ctypes.data, F1.ctypes.data))   # the resident mesh survived the cast
    assert np.array_equal(V1, V0) and np.array_equal(F1, F0)
    assert np.array_equal(s.sample(pts)[0], v0, equal_nan=True)
    check_family(t1, g1, O, D, phi0, d, 0.0, "state: first phi")
    # other sources (the upper half of the model), a new solve: the cast must see the new phi
    keep = d["pos"][:, 2] > np.median(d["pos"][:, 2])
    s.set_problem(d["pos"][keep], d["wnormal"][keep], d["area"][keep], float(d["lam"]), n, b, h)
    s.solve(tol=1e-10)
    phi_b = s.get_phi()[0]
    t3, g3, n3 = s.raycast(O, D, 0.0, grad=True)
    check_family(t3, g3, O, D, phi_b, d, 0.0, "state: second phi")
    assert not np.array_equal(t3, t1, equal_nan=True)
    # the same problem solved again on the same arrays: still the new phi's answer
    s.solve(tol=1e-10)
    t4 = s.raycast(O, D, 0.0)[0]
    check_family(t4, None, O, D, s.get_phi()[0], d, 0.0, "state: third solve")
    s.apply_laplacian(np.zeros(n ** 3))
    assert call(len(O), O.ctypes.data, D.ctypes.data, 0.0, t.ctypes.data) == SHM_ERR_STATE   # phi was overwritten
    s.close()


@pytest.mark.gpu
def test_two_ranks_are_refused(shm, tmp_path):
    """E, world = 2 through the librccl double: SHM_ERR_STATE on both ranks, with a message, and the ranks go on to finish."""
    so = str(tmp_path / "librccl_mock.so")
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", os.path.join(ROOT, "tests", "native", "rccl_mock.c"), "-o", so, "-I/opt/rocm/include",
                           "-D__HIP_PLATFORM_AMD__", "-L/opt/rocm/lib", "-lamdhip64", "-lrt", "-lpthread"])
    uid = ("/shmmock_%d_ray_2" % os.getpid()).encode().ljust(128, b"\x00")
    log = open(tmp_path / "worker.log", "w+")
    p = subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "ray_worker.py"), "2", uid.hex(), "bunny_small_n16", str(tmp_path)],
                         env=dict(os.environ, SHM_RCCL_LIB=so), stdout=log, stderr=subprocess.STDOUT)
    try:
        p.wait(timeout=300)
    except subprocess.TimeoutExpired:
        p.kill()
        p.wait()
    log.seek(0)
    assert p.returncode == 0, log.read()
    for r in range(2):
        status, msg = open(tmp_path / ("ray_%d.txt" % r)).read().split("\n", 1)
        assert int(status) == SHM_ERR_STATE and "world > 1" in msg, (r, status, msg)


@pytest.mark.gpu
def test_a_real_field(shm):
    """F.  At 128^3 and iso 0, camera rays that hit enter the surface (d . grad < 0) in >= 95 % of cases, and phi sampled at the hit point is within
    1e-12 max|phi| of the isovalue."""
    d, s, phi = solved(shm, "bunny_small", 128, 64)
    O, D = rays(d, phi, "camera", 20000, 129)
    t, g, nh = s.raycast(O, D, 0.0, grad=True)
    hit = np.isfinite(t)
    assert nh == hit.sum() > 5000
    entering = (np.einsum("qa,qa->q", D[hit], g[hit]) < 0).mean()
    print("entering share", entering)
    assert entering >= 0.95, entering
    v = s.sample(O[hit] + t[hit, None] * D[hit])[0]
    assert np.isfinite(v).all()
    assert np.abs(v - 0.0).max() <= 1e-12 * np.abs(phi).max(), np.abs(v).max() / np.abs(phi).max()


@pytest.mark.gpu
def test_cli_rays(shm, tmp_path):
    """G.  --rays / --rays-out / --rays-iso reproduce HostSolver.raycast on bunny_small at hCoef 2 (two processes, two solves: t is held to the
    acceptance rule, hits and misses are the same rays), and HostSolver.raycast is held to the restatement of its own phi."""
    from signed_heat_3d_amd.host_abi import HostSolver
    exe = os.path.join(ROOT, "signed-heat-3d_amd", "bin", "shm_grid_cli")
    mesh = os.path.join(ROOT, "data", "bunny_small.obj")
    host = HostSolver(mesh)
    phi, _ = host.compute_distance(hCoef=2.0)
    gi = host.grid_info()
    d = dict(n=gi["n"], bbox_min=gi["bbox_min"], cell=gi["cell"], pos=host.preprocess(hCoef=2.0)["pos"])
    O, D = rays(d, phi, "camera", 4000, 8)
    iso = 0.1 * float(np.max(phi))
    t, g, nh = host.raycast(O, D, iso, grad=True)
    assert 0 < nh == np.isfinite(t).sum()
    assert not np.array_equal(t, host.raycast(O, D, 0.0)[0], equal_nan=True)   # (the level matters: --rays-iso has something to get wrong)
    ref, ok = check_family(t, g, O, D, phi, d, iso, "host mirror")
    np.concatenate([O, D], axis=1).astype("<f8").tofile(tmp_path / "rays.f64")
    p = subprocess.run([exe, mesh, "--h", "2", "--rays", str(tmp_path / "rays.f64"), "--rays-out", str(tmp_path / "out.f64"), "--rays-iso", repr(iso)],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    out = np.fromfile(tmp_path / "out.f64", dtype="<f8").reshape(-1, 4)
    assert out.shape == (len(O), 4)
    same = ray_ref.agree(out[:, 0], t, d["cell"], D)
    assert (ref["gap"][~same] <= 1e-6 * np.abs(phi).max()).all() and (~same).sum() <= 1e-3 * len(t), int((~same).sum())
    m = same & np.isfinite(t)
    assert np.abs(out[m, 1:] - g[m]).max() <= 1e-9 * np.abs(g[m]).max()
    assert np.isnan(out[np.isnan(out[:, 0]), 1:]).all()
