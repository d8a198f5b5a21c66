"""The mesh smoothing stage without a GPU: the per-vertex arithmetic the kernels call (csrc/shm_mesh_smooth.h, through the stand-alone program
tests/native/test_mesh_smooth.cpp, plain and under AddressSanitizer + UBSan) against the numpy restatement tests/mesh_smooth_ref.py bit for bit, and the
restatement itself held to what the stage promises: exact cases on the octahedron, independence of the triangle order, closeness to the floating-point
umbrella operator, what Taubin passes do to a golden surface, and the rules for fixed axes, the cap, non-finite vertices and degenerate triangles.

Bounds.  A fixed-point pass differs from the float umbrella by at most E 2^-39 per coordinate: every neighbour is quantised to within q / 2 <= E 2^-40, the
mean of such numbers is off by no more, |f| <= 1, and the float operations on either side round at 2^-53 of numbers below 2 E -- three orders of
magnitude below E 2^-40.  Over p passes with factors f_i the difference grows by at most prod (1 + 2 |f_i|) per pass before it (the operator I + f (M - I) has
norm <= 1 + 2 |f| in the maximum norm), which is where the octahedron's tolerance after three Taubin iterations comes from."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import components_ref as cref
import mesh_smooth_ref as ref
from test_iso_components import golden_mesh

NATIVE_FLAGS = {"plain": ["-O2"], "sanitizers": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}
_EXE = {}


def native(tmp_path_factory, kind):
    if kind not in _EXE:
        exe = str(tmp_path_factory.mktemp("mesh_smooth_" + kind) / "test_mesh_smooth")
        src = os.path.join(ROOT, "tests", "native", "test_mesh_smooth.cpp")
        subprocess.check_call(["g++", *NATIVE_FLAGS[kind], "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", src, "-o", exe])
        _EXE[kind] = exe
    return _EXE[kind]


def run_native(exe, tmp_path, V, F, iterations, lam, mu, cap=0.0, fixed=None):
    V, F = np.ascontiguousarray(V, dtype=np.float64), np.ascontiguousarray(F, dtype=np.int64)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<4q3d", len(V), len(F), iterations, int(fixed is not None), lam, mu, cap))
        f.write(V.tobytes())
        f.write(F.tobytes())
        if fixed is not None:
            f.write(np.ascontiguousarray(fixed, dtype=np.uint8).tobytes())
    out = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-2000:] + out.stderr[-3000:]
    r = np.fromfile(fout, dtype=np.float64).reshape(2, -1, 3)
    return r[0], r[1]


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.int64), np.ascontiguousarray(b, dtype=np.float64).view(np.int64))


def shell(name):
    """The largest component of a golden's zero set, renumbered: (V, F, golden)."""
    V, F, d = golden_mesh(name, "zero")
    rec, tcomp, vcomp, _, _ = cref.records(V, F, int(d["n"]), d["bbox_min"], float(d["cell"]))
    big = int(np.argmax(rec["n_triangles"]))
    keep = vcomp == big
    newid = np.cumsum(keep) - 1
    return V[keep], newid[F[tcomp == big]], d


# ---- the stand-alone program ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["plain", "sanitizers"])
def test_native_mesh_smooth(tmp_path_factory, tmp_path, kind):
    exe = native(tmp_path_factory, kind)
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout[-2000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-3000:] + out.stderr[-3000:]


@pytest.mark.parametrize("kind", ["plain", "sanitizers"])
def test_native_equals_the_restatement(tmp_path_factory, tmp_path, kind):
    """The header's arithmetic and numpy's agree bit for bit: the octahedron, and the whole 24^3 golden mesh (14 components) with a cap and a mask."""
    exe = native(tmp_path_factory, kind)
    X, N = run_native(exe, tmp_path, ref.OCTA_V, ref.OCTA_F, 3, 0.5, -0.53)
    Xr, Nr = ref.smooth(ref.OCTA_V, ref.OCTA_F, 3, normals=True)
    assert same_bits(X, Xr) and same_bits(N, Nr)
    V, F, d = golden_mesh("bunny_small_n24", "zero")
    fixed = (np.arange(len(V)) % 11 == 0).astype(np.uint8) * (1 + np.arange(len(V)) % 7).astype(np.uint8)
    for cap, fx in ((0.0, None), (0.5 * float(d["cell"]), fixed)):
        X, N = run_native(exe, tmp_path, V, F, 10, 0.5, -0.53, cap, fx)
        Xr, Nr = ref.smooth(V, F, 10, fixed=fx, max_displacement=cap, normals=True)
        assert same_bits(X, Xr) and same_bits(N, Nr)


# ---- exact cases ---------------------------------------------------------------------------------------------------------------------------------------------
def test_octahedron_exact():
    lo, q = ref.frame(ref.OCTA_V)
    assert q == 2.0 ** -38 and np.array_equal(lo, [-1, -1, -1])
    X, N = ref.smooth(ref.OCTA_V, ref.OCTA_F, 1, lam=0.5, mu=0.0, normals=True)
    assert np.array_equal(X, 0.5 * ref.OCTA_V)
    assert np.array_equal(N, ref.OCTA_V)
    X0, N0 = ref.smooth(ref.OCTA_V, ref.OCTA_F, 0, normals=True)
    assert same_bits(X0, ref.OCTA_V) and np.array_equal(N0, ref.OCTA_V)


def test_octahedron_taubin_radius():
    """Three Taubin iterations scale the radius by (0.5 * 1.53)^3: the neighbour mean of every vertex is the origin up to the quantisation, E = 2, and six
    passes with factors 0.5 and -0.53 amplify a pass's E 2^-39 by at most (2 * 2.06)^3 in all (module docstring)."""
    X = ref.smooth(ref.OCTA_V, ref.OCTA_F, 3, lam=0.5, mu=-0.53)
    want = (0.5 * 1.53) ** 3 * ref.OCTA_V
    tol = 2.0 * 2.0 ** -39 * 6 * (2 * 2.06) ** 3
    err = np.abs(X - want).max()
    print("octahedron, 3 Taubin iterations: max |X - 0.765^3 V| = %.3e (tolerance %.3e)" % (err, tol))
    assert err <= tol


# ---- order independence -------------------------------------------------------------------------------------------------------------------------------------------
def test_order_independence():
    V, F, _ = golden_mesh("bunny_small_n24", "zero")
    rng = np.random.default_rng(5)
    X, N = ref.smooth(V, F, 10, normals=True)
    F2 = F[rng.permutation(len(F))]
    F2 = np.stack([np.roll(t, int(r)) for t, r in zip(F2, rng.integers(0, 3, len(F2)))])
    X2, N2 = ref.smooth(V, F2, 10, normals=True)
    assert same_bits(X, X2)
    # (a rotated triangle's normal is another cross product of the same three points: its last bits may differ, and so may an llrint -- printed, not held)
    print("normals under permutation + rotation: max |dN| = %.3e" % np.abs(N - N2).max())
    X3, N3 = ref.smooth(V, F[rng.permutation(len(F))], 10, normals=True)
    assert same_bits(X, X3) and same_bits(N, N3)          # a permutation alone: normals bit-identical too
    # the plain float umbrella on the same input is not reproducible: the test can tell the two apart
    Y, Y2 = ref.float_umbrella(V, F, 10), ref.float_umbrella(V, F2, 10)
    d = np.abs(Y - Y2).max()
    print("float umbrella under the same permutation: max difference %.3e" % d)
    assert 0 < d < 1e-12


def test_close_to_the_float_operator():
    V, F, _ = golden_mesh("bunny_small_n24", "zero")
    lo, q = ref.frame(V)
    E = float((V.max(axis=0) - V.min(axis=0)).max())
    for f in (0.5, -0.53, 1.0):
        A = ref.one_pass(V, F, lo, q, f)
        B = ref.float_umbrella(V, F, 1, lam=f, mu=0.0)
        err = np.abs(A - B).max()
        print("one pass f = %+.2f: fixed point - float = %.2e E (bound 2^-39 = %.2e)" % (f, err / E, 2.0 ** -39))
        assert err <= E * 2.0 ** -39


# ---- golden behaviour -----------------------------------------------------------------------------------------------------------------------------------------------
def test_golden_behaviour():
    V, F, d = shell("bunny_small_n64")
    cell = float(d["cell"])
    r0, v0 = ref.roughness(V, F), ref.volume(V, F)
    X = ref.smooth(V, F, 20)
    r1, v1 = ref.roughness(X, F), ref.volume(X, F)
    disp = np.linalg.norm(X - V, axis=1).max() / cell
    P = ref.smooth(V, F, 5, lam=0.5, mu=0.0)
    v2 = ref.volume(P, F)
    print("bunny_small_n64 shell: nv %d nt %d; roughness %.3f -> %.3f rad (x %.3f); volume x %.5f; largest displacement %.3f cell; 5 plain passes: volume x %.4f"
          % (len(V), len(F), r0, r1, r1 / r0, v1 / v0, disp, v2 / v0))
    assert r1 <= 0.75 * r0
    assert abs(v1 / v0 - 1.0) <= 0.01
    assert disp < 1.25
    assert v2 / v0 < 0.95


# ---- rules ----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_rules():
    V, F, d = golden_mesh("bunny_small_n24", "zero")
    cell = float(d["cell"])
    rng = np.random.default_rng(9)
    fixed = rng.integers(0, 8, len(V)).astype(np.uint8)
    V = V.copy()
    V[3, 1] = -0.0 if fixed[3] & 2 else V[3, 1]
    cap = 0.5 * cell
    for it, fx in ((10, None), (20, None), (10, fixed)):
        X = ref.smooth(V, F, it, fixed=fx, max_displacement=cap)
        for a in range(3):
            m = (fixed >> a) & 1 == 1
            assert fx is None or same_bits(X[m, a], V[m, a])
        moved = np.linalg.norm(X - V, axis=1)
        print("cap %.4f, %d iterations%s: largest move %.6f = %.17g cap, vertices at the cap %d"
              % (cap, it, ", mask" if fx is not None else "", moved.max(), moved.max() / cap, int((moved > 0.999 * cap).sum())))
        assert (moved <= cap * (1 + 2.0 ** -50)).all()
        assert fx is not None or (moved > 0.999 * cap).any()                # without a mask the cap acts here
    # a NaN vertex stays NaN, contributes nothing and moves nobody; (a, a, b) contributes nothing; a lone vertex stays
    nv = len(V)
    W = np.concatenate([V, [[np.nan, 0.0, 0.0], V.mean(axis=0)]])
    extra = np.array([[0, 1, nv], [5, 5, 9], [7, 9, 9]], dtype=np.int64)
    A = ref.smooth(W, np.concatenate([F, extra]), 4)
    B = ref.smooth(W, F, 4)
    assert same_bits(A, B)
    assert np.isnan(A[nv, 0]) and same_bits(A[nv, 1:], [0.0, 0.0]) and same_bits(A[nv + 1], W[nv + 1])
    assert same_bits(ref.smooth(W, np.concatenate([F, extra]), 0, normals=True)[1][nv:], np.zeros((2, 3)))
