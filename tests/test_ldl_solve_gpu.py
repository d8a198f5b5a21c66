"""The direct dual solve applies S^-1 through the block factorisation S = L D L^T with inverted diagonal superblocks (csrc/shm_ldl_plan.h, gj_ldl_step_kernel, ldl_tri_kernel,
apply_ldl) where it used to form the explicit inverse (SHM_S_FORM=invert keeps that path).  Both are reached here with matrices of the test's own through
shm_grid_spd_solve (GridSolver.spd_solve): the same set-up launches and the same apply as inside a solve, at the sizes where the plan changes shape -- one block, the padding
tail, the last size with one superblock and the first with two, four equal superblocks and the first four unequal ones -- and on the real S of bunny_small.obj at 64^3."""
import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SIZES = [1, 64, 65, 256, 257, 1024, 1025]
CONDS = [1e2, 1e5]


@functools.lru_cache(maxsize=None)
def _system(m, cond):
    """Q diag(lambda) Q^T, lambda log-spaced over [1, cond], a right-hand side, and numpy's fp64 solution -- built once per case and shared."""
    rng = np.random.default_rng(1000 * m + int(np.log10(cond)))
    q, _ = np.linalg.qr(rng.standard_normal((m, m)))
    lam = np.logspace(0.0, np.log10(cond), m) if m > 1 else np.array([3.0])
    S = (q * lam) @ q.T
    S = 0.5 * (S + S.T)
    rhs = rng.standard_normal(m)
    ref = np.linalg.solve(S, rhs)
    for a in (S, rhs, ref):
        a.setflags(write=False)
    return S, rhs, ref


@pytest.fixture(scope="module")
def solver(shm):
    return shm.GridSolver()


@pytest.fixture(scope="module")
def bunny_S(shm):
    """The explicit Schur complement of bunny_small.obj at 64^3, as the dual solver assembles it (m = 1129: 18 pivot blocks, four unequal superblocks)."""
    d = np.load(os.path.join(GOLDEN, "bunny_small_n64.npz"))
    s = shm.GridSolver()
    s.set_problem(d["pos"], d["wnormal"], d["area"], float(d["lam"]), int(d["n"]), d["bbox_min"], float(d["cell"]))
    old = os.environ.get("SHM_DUAL_DENSE_S_ALWAYS")
    os.environ["SHM_DUAL_DENSE_S_ALWAYS"] = "1"   # (a plan knob read per call: at 64^3 the plan assembles S only for the direct solve)
    try:
        S = s.get_schur()
    finally:
        if old is None:
            del os.environ["SHM_DUAL_DENSE_S_ALWAYS"]
        else:
            os.environ["SHM_DUAL_DENSE_S_ALWAYS"] = old
    S = 0.5 * (S + S.T)
    rhs = np.random.default_rng(7).standard_normal(S.shape[0])
    return S, rhs, np.linalg.solve(S, rhs)


def _errors(solver, S, rhs, ref):
    out = {}
    for form in ("factor", "invert"):
        u, flag = solver.spd_solve(S, rhs, form)
        assert flag == 0, (form, flag)
        out[form] = float(np.linalg.norm(u - ref) / np.linalg.norm(ref))
    return out


@pytest.mark.parametrize("cond", CONDS)
@pytest.mark.parametrize("m", SIZES)
def test_factor_solve_matches_the_inverse_on_spd_matrices(solver, m, cond):
    """|u - u_numpy| / |u_numpy| of the factorisation is at most 4 x that of the explicit inverse on the same input, plus 1e-14: the margin is over the path it replaces,
    and the factor 4 is for the different summation order alone.  Measured (MI355X), error of the factorisation / of the inverse and their ratio:
    cond 1e2: m = 1 2.0e-16 / 2.0e-16 (1.00), 64 2.66e-15 / 2.67e-15 (0.99), 65 2.11e-15 / 2.22e-15 (0.95), 256 3.25e-15 / 3.20e-15 (1.01), 257 3.48e-15 / 3.20e-15 (1.08),
    1024 4.39e-15 / 4.40e-15 (1.00), 1025 4.19e-15 / 4.15e-15 (1.01);
    cond 1e5: m = 1 0 / 0, 64 8.58e-13 / 8.58e-13 (1.00), 65 1.37e-12 / 1.26e-12 (1.09), 256 4.95e-12 / 4.81e-12 (1.03), 257 3.88e-12 / 3.76e-12 (1.03),
    1024 2.86e-12 / 2.81e-12 (1.02), 1025 3.00e-12 / 2.96e-12 (1.01)."""
    S, rhs, ref = _system(m, cond)
    e = _errors(solver, S, rhs, ref)
    print("m %d cond %.0e: factor %.3e invert %.3e ratio %.2f" % (m, cond, e["factor"], e["invert"], e["factor"] / max(e["invert"], 1e-300)))
    assert e["factor"] <= 4.0 * e["invert"] + 1e-14, e


def test_factor_solve_matches_the_inverse_on_the_bunny_schur_complement(solver, bunny_S):
    """The same bound on the real S = A K^+ A^T of bunny_small.obj at 64^3 (m = 1129).  Measured: factorisation 5.39e-13, inverse 3.40e-13, ratio 1.59."""
    S, rhs, ref = bunny_S
    assert S.shape[0] == 1129
    e = _errors(solver, S, rhs, ref)
    print("bunny_small 64^3 m %d: factor %.3e invert %.3e ratio %.2f" % (S.shape[0], e["factor"], e["invert"], e["factor"] / max(e["invert"], 1e-300)))
    assert e["factor"] <= 4.0 * e["invert"] + 1e-14, e


@pytest.mark.parametrize("m", [65, 257, 1025])
def test_factor_solve_is_deterministic(solver, m):
    """Two runs on the same input are bit-equal: every sum of the elimination, of the superblock inverses and of the solve's mat-vecs has a fixed order."""
    S, rhs, _ = _system(m, 1e5)
    u0, f0 = solver.spd_solve(S, rhs, "factor")
    u1, f1 = solver.spd_solve(S, rhs, "factor")
    assert f0 == 0 and f1 == 0 and np.array_equal(u0, u1)


@pytest.mark.parametrize("m,where", [(65, 0), (65, 64), (257, 130), (1025, 700)])
def test_indefinite_input_raises_the_pivot_flag(solver, m, where):
    """An SPD matrix with one diagonal entry's sign flipped is indefinite: the elimination meets a pivot that is not positive and reports it through the device flag of
    the Gauss-Jordan kernels -- in the first block, in the padded last block, inside a superblock, in a late superblock -- and nothing faults; the handle then solves a
    positive definite system as before."""
    S, rhs, ref = _system(m, 1e2)
    bad = S.copy()
    bad[where, where] = -bad[where, where]
    for form in ("factor", "invert"):
        _, flag = solver.spd_solve(bad, rhs, form)
        assert flag != 0, form
    u, flag = solver.spd_solve(S, rhs, "factor")
    assert flag == 0 and np.linalg.norm(u - ref) <= 1e-12 * np.linalg.norm(ref)


def test_default_solve_factors_and_agrees_with_the_inverse(shm, monkeypatch):
    """bunny_small at 64^3 through the whole solve: the default direct dual solve (the factorisation) and SHM_S_FORM=invert take the same number of passes, the
    residual of the default is within 4 x of the other, and phi agrees to the solve's accuracy (1e-9: a hundred times eps cond(S) = 1e-16 x 7e4).  Measured: one pass
    either way, rel_residual 8.7e-15 with the factorisation against 4.6e-12 with the inverse."""
    d = np.load(os.path.join(GOLDEN, "bunny_small_n64.npz"))
    s = shm.GridSolver()
    s.set_problem(d["pos"], d["wnormal"], d["area"], float(d["lam"]), int(d["n"]), d["bbox_min"], float(d["cell"]))
    res = {}
    for form in ("factor", "invert"):
        if form == "invert":
            monkeypatch.setenv("SHM_S_FORM", "invert")   # (a plan knob, read per solve)
        else:
            monkeypatch.delenv("SHM_S_FORM", raising=False)   # the default
        st = s.solve(tol=1e-10)
        phi, _ = s.get_phi()
        res[form] = (int(st.iters), float(st.rel_residual), phi)
    print("passes %d / %d, rel_residual %.3e / %.3e" % (res["factor"][0], res["invert"][0], res["factor"][1], res["invert"][1]))
    assert res["factor"][0] == res["invert"][0]
    assert res["factor"][1] <= 4.0 * res["invert"][1] + 1e-16
    assert np.abs(res["factor"][2] - res["invert"][2]).max() <= 1e-9
    assert np.abs(res["factor"][2] - d["phi"]).max() < 1e-7
