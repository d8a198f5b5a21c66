"""The dual solver's set-up on the device -- the Green's table (cosi_lines_kernel for n = 2^k, three dgemm_rm_kernel products for every other n),
schur_assemble_kernel, the inversion of S and dual_bordered_kernel -- held stage by stage the way test_stage_edges.py holds the stages after Step 1:
  0. (CPU) the reference itself: schur_ref(nodes, coeffs, n, cell) = A K^+ A^T in fp64 from get_constraints()-shaped rows alone, K^+ the scipy DCT-II chain of
     test_stage_edges.py part E, against the dense pseudo-inverse of the matrix of shmo_laplacian_apply (n = 8, 11) and against the 6 x 6 x 6 table formula of
     test_schur_math.py on the same rows -- so the GPU tests below never compare the device with itself;
  1. every entry of S = get_schur() against schur_ref on rows placed where the assembly and the table can go wrong: boundary cells, weights exactly 0 and
     (all but) 1, every fold / merge branch of the index windows on every axis, m on both sides of the 16 x 16 tiles and of the 64-row padding, grid sides on
     both table paths and on every edge of the GEMM tiles;
  2. the inverse of S after exactly one pass of the direct form, against an fp64 LU solve of the bordered system refined with extended-precision residuals,
     fed the device's own right-hand side b;
  3. the three dual forms and the primal solver with constraint rows on the planes 0 and n - 1, against the C oracle.
The sources are synthetic (test_step1_edges._sources_in_cells: one source per chosen cell at chosen local coordinates, all exactly representable), the
reference is fed the device's own rows (1) and the device's own b (2), and no bound is fitted to what the kernels give: 1e-10 of a column's largest entry
is the figure test_explicit_schur_complement_is_A_Kplus_AT already holds (1), a stated multiple of what numpy's same-precision inverse does on the same input
(2), the tolerance of test_matches_c_oracle_odd_sizes (3).  Every test prints its worst error and its margin.  Measured: profiles/schur_edges.txt."""
import itertools
import zlib

import numpy as np
import pytest

# (as tests/test_stage_edges.py: torch first, so that it and libshm_grid.so share one HIP runtime -- the memory guard below asks torch for the free device memory)
try:
    import torch  # noqa: F401
except ImportError:
    torch = None

from conftest import c_
from test_gpu_parity import _free_memory_gb, make_solver
from test_schur_math import _fold
from test_stage_edges import _bunny, _line
from test_step1_edges import ORACLE_THREADS, _sources_in_cells

gpu = pytest.mark.gpu


# ---- the synthetic layouts ------------------------------------------------------------------------------------------------------------------------------------
T_TOP = 1.0 - 2.0 ** -30   # set_problem admits no source on a top face (floor + 1 <= n - 1): a node of index n - 1 is reached to 2^-30 of a cell


def _layout(name, n):
    """(cells (m, 3), t (m, 3)) of a named layout on an n^3 grid; lo / mid / hi = cells 0, (n - 2) // 2, n - 2.  t has 20 bits unless it is 0, 0.5 or T_TOP.
      corners   the 8 corner cells, the 12 edge-centre cells and the 6 face-centre cells: every X_a in {lo, mid, hi};
      on_nodes  sources on grid nodes (t = 0; index n - 1 as T_TOP in cell hi): the 8 corners of the grid, nodes on four faces, interior nodes next to each other,
                mixed with rows that sit on a node plane in one or two axes only and with t = 0.5 rows;
      folds     per axis two parallel lines of five consecutive cells around the middle: every pair (X, X') with X - X' in {0, +-1, +-2} and
                X + X' + 1 in {n - 3, ..., n} that parity allows occurs on every axis (test_layouts_reach_every_fold_and_merge_branch counts them);
      tilesM    M random distinct cells over the whole grid, cells (0, 0, 0) and (n - 2, n - 2, n - 2) among them when M >= 2."""
    rng = np.random.default_rng(zlib.crc32(("%s/%d" % (name, n)).encode()))
    lo, mid, hi = 0, (n - 2) // 2, n - 2

    def rand_t(m):
        return rng.integers(1, 2 ** 20, size=(m, 3)) / 2.0 ** 20

    if name == "corners":
        cells = np.array([c for c in itertools.product((lo, mid, hi), repeat=3) if c != (mid, mid, mid)])
        return cells, rand_t(len(cells))
    if name == "on_nodes":
        rows = [(tuple(hi if b else lo for b in bits), tuple(T_TOP if b else 0.0 for b in bits)) for bits in itertools.product((0, 1), repeat=3)]
        rows += [((mid, mid, mid), (0.0, 0.0, 0.0)), ((mid + 1, mid, mid), (0.0, 0.0, 0.0)),             # two interior nodes next to each other
                 ((lo, mid, mid + 1), (0.0, 0.0, 0.0)), ((mid, mid + 1, lo), (0.0, 0.0, 0.0)),           # nodes on the faces x = 0 and z = 0
                 ((mid, hi, mid + 1), (0.0, T_TOP, 0.0)), ((mid + 1, mid + 1, hi), (0.0, 0.0, T_TOP)),   # ... y = n - 1 and z = n - 1
                 ((lo, lo, mid), (0.0, 0.5, 0.5)), ((hi, mid, lo), (T_TOP, 0.5, 0.0)), ((mid, hi, hi), (0.5, 0.5, T_TOP)), ((mid, mid - 1, mid), (0.5, 0.0, 0.5)),
                 ((mid - 1, mid, mid), (0.5, 0.5, 0.5)), ((lo, hi, mid - 1), (0.5, 0.5, 0.5))]
        return np.array([c for c, _ in rows]), np.array([t for _, t in rows])
    if name == "folds":
        cells = []
        for a in range(3):
            for others in ((1, n - 3), (2, n - 3)):
                for X in range(mid - 2, mid + 3):
                    c = list(others)
                    c.insert(a, X)
                    if tuple(c) not in cells:
                        cells.append(tuple(c))
        cells = np.array(cells)
        return cells, rand_t(len(cells))
    if name.startswith("tiles"):
        m = int(name[5:])
        last = (n - 1) ** 3 - 1
        ids = rng.choice(np.arange(1, last), size=max(m - 2, 0), replace=False) if m > 2 else np.zeros(0, dtype=np.int64)
        ids = np.concatenate([[0], ids, [last]])[:max(m, 1)] if m >= 2 else np.array([rng.integers(0, last + 1)])
        cells = np.stack([ids % (n - 1), (ids // (n - 1)) % (n - 1), ids // (n - 1) ** 2], axis=1)
        return cells, rand_t(len(cells))
    raise KeyError(name)


def _problem(name, n):
    """set_problem arguments of a layout (or of the rescaled bunny fixture) on an n^3 grid."""
    if name == "bunny":
        return _bunny(n)
    cells, t = _layout(name, n)
    return _sources_in_cells(n, cells, t, seed=zlib.crc32(name.encode()) + n)


def _rows_of(cells, t, n):
    """(nodes (m, 8), coeffs (m, 8)) of one trilinear row per cell, in the order of build_rows (shm_constraints.h) and get_constraints()."""
    i, j, k = (cells[:, a].astype(np.int64) for a in range(3))
    tx, ty, tz = (t[:, a] for a in range(3))

    def ix(a, b, c):
        return a + b * n + c * n * n

    nodes = np.stack([ix(i, j, k), ix(i + 1, j, k), ix(i, j + 1, k), ix(i, j, k + 1), ix(i + 1, j + 1, k), ix(i + 1, j, k + 1), ix(i, j + 1, k + 1), ix(i + 1, j + 1, k + 1)], axis=1)
    coeffs = np.stack([(1. - tx) * (1. - ty) * (1. - tz), tx * (1. - ty) * (1. - tz), (1. - tx) * ty * (1. - tz), (1. - tx) * (1. - ty) * tz,
                       tx * ty * (1. - tz), tx * (1. - ty) * tz, (1. - tx) * ty * tz, tx * ty * tz], axis=1)
    return nodes, coeffs


# ---- 0. the host reference --------------------------------------------------------------------------------------------------------------------------------------
def _inv_symbol(n, h):
    """1 / lambda_k of the 7-point Neumann Laplacian in the DCT-II basis, 0 for the zero mode (test_stage_edges.py part E)."""
    lam1 = (2 - 2 * np.cos(np.pi * np.arange(n) / n)) / h ** 2
    LAM = lam1[:, None, None] + lam1[None, :, None] + lam1[None, None, :]
    return np.where(LAM > 0, 1 / np.where(LAM > 0, LAM, 1), 0.0)


def kplus(v, n, h, inv=None, workers=1):
    """K^+ v on the host: the scipy DCT-II chain, divide by lambda_k, zero mode -> 0."""
    from scipy.fft import dctn, idctn
    inv = _inv_symbol(n, h) if inv is None else inv
    return idctn(dctn(v.reshape(n, n, n), type=2, norm="ortho", workers=workers) * inv, type=2, norm="ortho", workers=workers).reshape(-1)


def schur_ref(nodes, coeffs, n, cell, workers=1):
    """The full m x m S = A K^+ A^T in fp64 from rows shaped like get_constraints() output alone: one dctn per row, F_r = DCT(A^T e_r), and
    S = F diag(1 / lambda) F^T (the orthonormal DCT-II diagonalises K; K^+ = V diag(1 / lambda, zero mode 0) V^T).  Symmetric by construction."""
    from scipy.fft import dctn
    m, N = nodes.shape[0], n ** 3
    inv = _inv_symbol(n, cell).reshape(-1)
    F = np.empty((m, N))
    for r in range(m):
        v = np.zeros(N)
        np.add.at(v, nodes[r], coeffs[r])
        F[r] = dctn(v.reshape(n, n, n), type=2, norm="ortho", workers=workers).reshape(-1)
    S = (F * inv) @ F.T
    return 0.5 * (S + S.T)


def _dense_A(nodes, coeffs, N):
    A = np.zeros((nodes.shape[0], N))
    for r in range(nodes.shape[0]):
        np.add.at(A[r], nodes[r], coeffs[r])
    return A


# schur_ref against the dense pseudo-inverse and against the table formula: 1e-12 of max|S|.  Every entry is a sum of at most n^3 <= 1331 products of cosines
# with the positive weights 1 / lambda_k, bounded in absolute value by the diagonal (Cauchy-Schwarz): N u max|S| = 1.5e-13 covers the summation on either side,
# and the eigen-decomposition behind the dense pseudo-inverse adds u cond(K) = u * 12 / (2 - 2 cos(pi / n)) ~ 150 u ~ 2e-14 at n = 11.
REF_BOUND = 1e-12
CPU_LAYOUTS = ["corners", "on_nodes", "folds", "tiles17"]


@pytest.mark.parametrize("layout", CPU_LAYOUTS)
@pytest.mark.parametrize("n", [8, 11])
def test_schur_ref_matches_the_dense_pseudo_inverse(oracle_c, n, layout):
    """K column by column from shmo_laplacian_apply (the operator the solvers apply), its pseudo-inverse from a symmetric eigen-decomposition with the constant
    mode removed, S = A K^+ A^T by dense products."""
    h = 0.125
    cells, t = _layout(layout, n)
    nodes, coeffs = _rows_of(cells, t, n)
    N = n ** 3
    K = np.empty((N, N))
    e, col = np.zeros(N), np.zeros(N)
    for j in range(N):
        e[j] = 1.0
        oracle_c.shmo_laplacian_apply(n, h, e, col)
        K[:, j] = -col
        e[j] = 0.0
    assert np.array_equal(K, K.T) and (np.diag(K) > 0).all()
    w, V = np.linalg.eigh(K)
    assert abs(w[0]) < 1e-10 * w[-1] and w[1] > 1e-3 * w[-1] / n ** 2 and np.abs(np.abs(V[:, 0]) - N ** -0.5).max() < 1e-10   # one zero mode: the constants
    winv = np.concatenate([[0.0], 1.0 / w[1:]])
    A = _dense_A(nodes, coeffs, N)
    AV = A @ V
    dense = (AV * winv) @ AV.T
    ref = schur_ref(nodes, coeffs, n, h)
    scale = float(np.abs(dense).max())
    err = float(np.abs(ref - dense).max())
    _line("schur_ref vs dense pseudo-inverse, n=%d %s (m %d)" % (n, layout, len(cells)),
          ["max|dS| %.2e = %.2e max|S|, bound %.0e (margin %.1fx)" % (err, err / scale, REF_BOUND, REF_BOUND * scale / max(err, 1e-300))])
    assert np.array_equal(ref, ref.T) and err <= REF_BOUND * scale, (n, layout, err, scale)


def _green_table(n, h):
    """T[d1][d2][d3] of csrc/shm_schur.hip.h, (n + 1)^3, as test_schur_math._setup builds it."""
    k = np.arange(n)
    gam = np.where(k == 0, 1 / (2 * n), 1.0 / n)
    C = np.cos(np.pi * np.outer(np.arange(n + 1), k) / n)
    W0 = gam[:, None, None] * gam[None, :, None] * gam[None, None, :] * _inv_symbol(n, h)
    return np.einsum("ai,bj,ck,ijk->abc", C, C, C, W0, optimize=True)


def _axis_windows(Xi, Xj, ti, tj, n):
    """The six (table index, weight) pairs of one axis: the difference window |D - 1|, |D|, |D + 1| and the folded sum window E, E + 1, E + 2 (test_schur_math.py)."""
    wi, wj = (1 - ti, ti), (1 - tj, tj)
    D, E = Xi - Xj, Xi + Xj + 1
    idx = [abs(D - 1), abs(D), abs(D + 1), _fold(E, n), _fold(E + 1, n), _fold(E + 2, n)]
    w = [wi[0] * wj[1], wi[0] * wj[0] + wi[1] * wj[1], wi[1] * wj[0], wi[0] * wj[0], wi[0] * wj[1] + wi[1] * wj[0], wi[1] * wj[1]]
    return np.array(idx), np.array(w)


def schur_by_table(cells, t, n, h):
    """S from the 6 x 6 x 6 table formula of test_schur_math.py::test_schur_entry_of_two_trilinear_rows, every pair of rows."""
    T = _green_table(n, h)
    m = len(cells)
    S = np.empty((m, m))
    for i in range(m):
        for j in range(i, m):
            (ix, wx), (iy, wy), (iz, wz) = (_axis_windows(int(cells[i, a]), int(cells[j, a]), t[i, a], t[j, a], n) for a in range(3))
            S[i, j] = S[j, i] = np.einsum("p,q,r,pqr->", wx, wy, wz, T[np.ix_(ix, iy, iz)])
    return S


@pytest.mark.parametrize("layout", CPU_LAYOUTS)
@pytest.mark.parametrize("n", [8, 11])
def test_schur_ref_matches_the_table_formula(n, layout):
    h = 0.125
    cells, t = _layout(layout, n)
    nodes, coeffs = _rows_of(cells, t, n)
    ref = schur_ref(nodes, coeffs, n, h)
    tab = schur_by_table(cells, t, n, h)
    scale = float(np.abs(ref).max())
    err = float(np.abs(ref - tab).max())
    _line("schur_ref vs the 6 x 6 x 6 table formula, n=%d %s (m %d)" % (n, layout, len(cells)),
          ["max|dS| %.2e = %.2e max|S|, bound %.0e (margin %.1fx)" % (err, err / scale, REF_BOUND, REF_BOUND * scale / max(err, 1e-300))])
    assert err <= REF_BOUND * scale, (n, layout, err, scale)


@pytest.mark.parametrize("n", [8, 11, 12, 16, 33])
def test_layouts_reach_every_fold_and_merge_branch(n):
    """What the layouts are for, counted: `folds` holds on every axis every pair with D = X - X' in {0, +-1, +-2} and E = X + X' + 1 in {n - 3, ..., n} that parity
    allows -- the windows |D - 1|, |D|, |D + 1| ascending, descending and merged onto two entries (D = 0), the sum windows unfolded, folded at E + 2, E + 1 and E
    (E + 1 = n merges fold(E) and fold(E + 2)) -- `corners` holds X in {0, n - 2} in every combination (E = 1 and E = 2 n - 3), `on_nodes` weights exactly 0 on
    every axis, and the synthetic positions give back their rows exactly."""
    cells, _ = _layout("folds", n)
    for a in range(3):
        X = cells[:, a]
        pairs = {(int(x - y), int(x + y + 1)) for x in X for y in X}
        want = {(D, E) for D in (-2, -1, 0, 1, 2) for E in (n - 3, n - 2, n - 1, n) if (E - 1 + D) % 2 == 0}
        assert want <= pairs, (n, a, sorted(want - pairs))
        same = [(r, q) for r in range(len(cells)) for q in range(r + 1, len(cells)) if cells[r, a] == cells[q, a]]
        assert same, "no two distinct rows share X on axis %d: D = 0 would only be seen on the diagonal" % a
    cells, _ = _layout("corners", n)
    assert {tuple(c) for c in cells.tolist()} >= set(itertools.product((0, n - 2), repeat=3)) and len(cells) == 26
    cells, t = _layout("on_nodes", n)
    for a in range(3):
        assert (t[:, a] == 0.0).any() and (t[:, a] == T_TOP).any() and (t[:, a] == 0.5).any()
        assert ((cells[:, a] == 0) & (t[:, a] == 0.0)).any() and ((cells[:, a] == n - 2) & (t[:, a] == T_TOP)).any()
    for name in ("corners", "on_nodes", "folds", "tiles1", "tiles17", "tiles65"):
        cells, t = _layout(name, n)
        d = _sources_in_cells(n, cells, t, seed=1)       # (asserts that locate_source's expressions give back cells and t exactly)
        assert len(d["area"]) == len(cells) == (int(name[5:]) if name.startswith("tiles") else len(cells))


# ---- 1. every entry of S -----------------------------------------------------------------------------------------------------------------------------------------
SCHUR_BOUND = 1e-10   # |dS_ij| <= 1e-10 max|S[:, j]|: test_explicit_schur_complement_is_A_Kplus_AT's figure, here against a reference that shares no transform with the device

TILE_LAYOUTS = ["tiles1", "tiles15", "tiles16", "tiles17", "tiles33", "tiles65"]
S_CASES = [(n, name) for n in (16, 32, 11, 12, 33) for name in ["corners", "on_nodes", "folds"] + TILE_LAYOUTS] + [(33, "bunny"), (130, "folds"), (130, "tiles48")]


def _schur_states(n):
    """(label, precision, Step-1 arithmetic to run before get_schur or None) -- how each table path is reached.  get_schur() plans with the Step-1 kernel the
    handle last selected (Solver::step1_kernel): set_problem selects the tiered kernel on either precision (select_step1_arith(AUTO)), which makes
    `narrow = plan_in.tiered()` true and the table of a non-power-of-two n three dgemm_rm_kernel<1> products; run_conv(step1="reference_f64") selects the
    untiered all-fp64 kernel, after which the same call builds the table with dgemm_rm_kernel<4>.  n = 2^k: the FFT passes, whatever the Step-1 kernel."""
    if n & (n - 1) == 0:
        return [("fp64 FFT table", 64, None), ("fp32 handle FFT table", 32, None)]
    return [("fp64 dgemm<1>", 64, None), ("fp64 dgemm<4>", 64, "reference_f64"), ("fp32 handle dgemm<1>", 32, None)]


@gpu
@pytest.mark.parametrize("n,layout", S_CASES)
def test_every_entry_of_S_at_grid_and_tile_edges(shm, monkeypatch, n, layout):
    """All m^2 entries of get_schur() against schur_ref of the handle's own rows, and S == S^T exactly.  n = 16, 32: cosi_lines_kernel (get_schur() assembles S on
    grids this small only under SHM_DUAL_DENSE_S_ALWAYS, a plan knob read per solve -- conftest.py sets SHM_DEBUG_KNOBS=1, which knob() needs); n = 11, 12: the
    dense products with K < 16, one partial chunk; 33: two chunks and one more; 130: M = n + 1 crosses the 128-row tile (48 rows at most: one dctn per row on the
    host).  Each in the states of _schur_states.  m = 1 ... 65: one partial 16 x 16 tile, the tile edge, diagonal and off-diagonal tiles, the 64-row padding of the
    inversion on either side."""
    if n & (n - 1) == 0:
        monkeypatch.setenv("SHM_DUAL_DENSE_S_ALWAYS", "1")
    if n >= 128:
        dev_gb, host_gb = _free_memory_gb()
        if dev_gb < 2 or host_gb < 4:
            pytest.skip("needs 2 GB of free device memory and 4 GB of host memory, found %.0f / %.0f GB" % (dev_gb, host_gb))
    d = _problem(layout, n)
    ref, items, worst = None, [], 0.0
    for label, precision, arith in _schur_states(n):
        s = make_solver(shm, d, precision=precision)
        if arith is not None:
            s.run_conv(step1=arith)
        S = s.get_schur()
        if ref is None:
            nodes, coeffs = s.get_constraints()
            if layout != "bunny":      # the rows are the ones the layout chose
                want_nodes, want_coeffs = _rows_of(*_layout(layout, n), n)
                assert np.array_equal(nodes, want_nodes) and np.allclose(coeffs, want_coeffs, rtol=0, atol=2.0 ** -50)
            ref = schur_ref(nodes, coeffs, n, float(d["cell"]), workers=ORACLE_THREADS)
            colmax = np.abs(ref).max(axis=0)
        s.close()
        assert S.shape == ref.shape and np.isfinite(S).all(), (n, layout, label)
        assert np.array_equal(S, S.T), "%s: S is not exactly symmetric" % label
        ratio = np.abs(S - ref) / (SCHUR_BOUND * colmax[None, :])
        i, j = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        items.append("%s max|dS| / max|S[:, j]| %.2e at (%d, %d), bound %.0e (margin %.0fx)" % (label, ratio[i, j] * SCHUR_BOUND, i, j, SCHUR_BOUND, 1 / max(ratio[i, j], 1e-300)))
        worst = max(worst, float(ratio[i, j]))
    _line("S n=%d %s (m %d) vs schur_ref of the device's rows" % (n, layout, ref.shape[0]), items)
    assert worst <= 1.0, (n, layout, items)


# ---- 2. the inverse of S after exactly one pass -------------------------------------------------------------------------------------------------------------------
# The direct form (solve_dual, dual_bordered_kernel): with g = A K^+ b, the KKT system of the dual is [[S, 1], [1^T, 0]] [mu; c] = [g; sum b]; the device starts
# from mu_0 = (sum b / m) 1, takes r = Pm(g - S mu_0) (Pm: minus the mean), u = S^-1 r and v = S^-1 1 with the explicitly inverted S, mu = mu_0 + u - (1^T u / 1^T v) v,
# then x = K^+ (A^T mu - b) and phi = -x - shift, shift = sum_s area_s (-x)(pos_s) / sum_s area_s (shift_partial_kernel, write_phi_kernel) -- the additive constant
# of x cancels.  Truth: the bordered system by LU in fp64, refined twice with residuals in np.longdouble.  The bound is a multiple of what the same method does in
# the same precision on the same input: phi_inv from np.linalg.inv(S_ref) through the device's own formulas, e_ref = max|phi_inv - phi_truth|, and
#     max|phi_dev - phi_truth| <= 16 e_ref + 64 * 2^-53 * max|phi|:
# 16 for an unpivoted blocked Gauss-Jordan against LAPACK's pivoted inverse, the floor for the two transform solves (K^+ b and K^+ (A^T mu - b)) the device does
# with its own transforms.
INV_FACTOR, INV_FLOOR = 16, 64 * 2.0 ** -53
INV_CASES = [(n, name) for n in (16, 33) for name in ("corners", "folds", "tiles65")]


def _phi_of_mu(mu, b, A, area, n, h, inv):
    minus_x = -kplus(A.T @ mu - b, n, h, inv)
    return minus_x - float((area * (A @ minus_x)).sum() / area.sum())


def _host_one_pass(S, A, b, area, n, h):
    """(phi_truth, phi_inv) for the right-hand side b: see the comment above."""
    import scipy.linalg
    m = S.shape[0]
    inv = _inv_symbol(n, h)
    g = A @ kplus(b, n, h, inv)
    sumb = float(np.sum(b.astype(np.longdouble)))
    M = np.zeros((m + 1, m + 1))
    M[:m, :m] = S
    M[:m, m] = M[m, :m] = 1.0
    rhs = np.concatenate([g, [sumb]])
    lu = scipy.linalg.lu_factor(M)
    z = scipy.linalg.lu_solve(lu, rhs)
    Ml = M.astype(np.longdouble)
    for _ in range(2):
        z = z + scipy.linalg.lu_solve(lu, (rhs.astype(np.longdouble) - Ml @ z.astype(np.longdouble)).astype(np.float64))
    phi_truth = _phi_of_mu(z[:m], b, A, area, n, h, inv)
    Sinv = np.linalg.inv(S)
    mu0 = np.full(m, sumb / m)
    r = g - S @ mu0
    r -= r.mean()
    u, v = Sinv @ r, Sinv @ np.ones(m)
    mu = mu0 + u - (u.sum() / v.sum()) * v
    return phi_truth, _phi_of_mu(mu, b, A, area, n, h, inv)


@gpu
@pytest.mark.parametrize("n,layout", INV_CASES)
def test_inverse_of_S_after_exactly_one_pass(shm, n, layout):
    """run_conv, run_divergence, b = get_field(DIV); then solve(dual, direct, max_iters = 1): cg_form 2, one pass, and phi within 16 x the error of numpy's
    inverse of S_ref on the same b (plus 64 u max|phi| for the transforms) of the refined LU solution."""
    import scipy.sparse as sp
    d = _problem(layout, n)
    h = float(d["cell"])
    s = make_solver(shm, d)
    s.run_conv()
    s.run_divergence()
    b = s.get_field(s.FIELD_DIV)
    nodes, coeffs = s.get_constraints()
    st = s.solve(tol=1e-10, solver="dual", dual_form="direct", max_iters=1, allow_noconv=True)
    phi, _ = s.get_phi()
    s.close()
    m = nodes.shape[0]
    assert (st.cg_form, st.iters, st.m) == (2, 1, m) and m == len(d["area"]) and np.isfinite(b).all() and np.isfinite(phi).all()
    A = sp.csr_matrix((coeffs.ravel(), (np.repeat(np.arange(m), 8), nodes.ravel())), shape=(m, n ** 3))
    S_ref = schur_ref(nodes, coeffs, n, h)
    phi_truth, phi_inv = _host_one_pass(S_ref, A, b, np.asarray(d["area"], dtype=np.float64), n, h)
    scale = float(np.abs(phi_truth).max())
    e_ref = float(np.abs(phi_inv - phi_truth).max())
    e_dev = float(np.abs(phi - phi_truth).max())
    bound = INV_FACTOR * e_ref + INV_FLOOR * scale
    _line("one direct pass n=%d %s (m %d, cond(S) %.1e) vs refined LU on the device's b" % (n, layout, m, np.linalg.cond(S_ref)),
          ["max|phi| %.2e; e_ref (numpy inverse) %.2e; e_dev %.2e; e_dev / e_ref = %.2f; bound 16 e_ref + 64 u max|phi| = %.2e (margin %.1fx); rel_residual %.1e"
           % (scale, e_ref, e_dev, e_dev / max(e_ref, 1e-300), bound, bound / max(e_dev, 1e-300), st.rel_residual)])
    assert e_dev <= bound, (n, layout, e_dev, e_ref, bound)


# ---- 3. the three dual forms and the primal solver on boundary rows ----------------------------------------------------------------------------------------------
PHI_ORACLE = 1e-7   # test_matches_c_oracle_odd_sizes' tolerance
FORMS = [("direct", dict(solver="dual", dual_form="direct"), 2), ("explicit_s_cg", dict(solver="dual", dual_form="explicit_s_cg"), 3),
         ("through_grid", dict(solver="dual", dual_form="through_grid"), 0), ("primal plain", dict(solver="primal", precond="none"), None),
         ("primal dct", dict(solver="primal", precond="dct"), None)]
_ORACLE_PHI = {}   # (layout, n) -> the C oracle's phi, computed once


def _oracle_phi(oracle_c, layout, n):
    if (layout, n) not in _ORACLE_PHI:
        d = _problem(layout, n)
        ref, st = np.zeros(n ** 3), np.zeros(5)
        rc = oracle_c.shmo_compute_distance(n, c_(d["bbox_min"]), float(d["cell"]), len(d["area"]), c_(d["pos"]).reshape(-1), c_(d["wnormal"]).reshape(-1),
                                            c_(d["area"]), float(d["lam"]), 1, 0, 1e-12, 100000, ref, st)
        assert rc == 0
        ref.setflags(write=False)
        _ORACLE_PHI[(layout, n)] = ref
    return _ORACLE_PHI[(layout, n)]


@gpu
@pytest.mark.parametrize("layout", ["corners", "on_nodes"])
@pytest.mark.parametrize("n", [16, 33])
def test_solver_forms_with_rows_on_the_boundary_planes(shm, oracle_c, n, layout):
    """Constraint rows in the cells 0 and n - 2 of every axis (and sources on the nodes of the planes 0 and n - 1) through the three dual forms -- at n = 16 the
    through-grid form runs the sparse-plane transforms and zsolve_sparse_kernel on the planes 0 and n - 1, at n = 33 the dense products -- and the primal CG, plain
    and DCT-preconditioned: each phi within 1e-7 of the C oracle's projected CG on the same input; the two CG forms of the dual agree in iterations within 2; the
    direct form takes at most two passes."""
    d = _problem(layout, n)
    ref = _oracle_phi(oracle_c, layout, n)
    s = make_solver(shm, d)
    items, its, errs = [], {}, {}
    for name, kw, cg_form in FORMS:
        st = s.solve(tol=1e-10, scrub=True, **kw)
        phi, _ = s.get_phi()
        errs[name] = float(np.abs(phi - ref).max())
        its[name] = int(st.iters)
        if cg_form is not None:
            assert st.solver == 2 and st.cg_form == cg_form, (name, st.solver, st.cg_form)
        else:
            assert st.solver == 1 and st.preconditioner == (2 if kw["precond"] == "dct" else 1), (name, st.solver, st.preconditioner)
        items.append("%s max|dphi| %.2e (margin %.0fx, %d iterations)" % (name, errs[name], PHI_ORACLE / max(errs[name], 1e-300), st.iters))
    s.close()
    _line("phi n=%d %s (m %d) vs the C oracle, bound %.0e" % (n, layout, len(d["area"]), PHI_ORACLE), items)
    for name, e in errs.items():
        assert e < PHI_ORACLE, (n, layout, name, e)
    assert abs(its["explicit_s_cg"] - its["through_grid"]) <= 2, its
    assert its["direct"] <= 2, its
