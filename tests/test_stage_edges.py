"""The stages after Step 1, one at a time, in both precisions and at the launch geometries the whole-solve tests only pass through:
  A. divergence (divergence_march_kernel<T, VEC>, divergence_kernel<T>) against shmo_divergence -- or, where three N-vectors on the host are too much, against the
     numpy restatement of the closed form below, itself held to shmo_divergence by a CPU test in this file;
  B. laplacian_kernel<float> against shmo_laplacian_apply;
  C. the projector against v - A^T (A A^T)^-1 A v formed on the host in fp64 from get_constraints();
  D. fast integration (bfs_plane0_kernel, bfs_z_kernel) against shmo_integrate_greedily minus shmo_source_average;
  E. the fp32 DCT preconditioner against scipy's fp64 DCT chain.
One rule throughout: THE REFERENCE IS FED THE DEVICE'S OWN INPUT -- Y as read back from the handle, or the random vector rounded to the handle's precision first (an
fp32 value promoted to fp64 is exact input for an fp64 reference) -- so every stage is isolated from the stages before it and what remains is the rounding of the
kernel under test alone.  That is what lets the bounds be derived instead of measured: each bound below is a count of roundings written beside it (A, B, C fp32, D
fp32), a figure an existing test of the project already holds (C fp64, D fp64), or a stated multiple of the error a reference implementation in the same precision
makes on the same input (E).  None is fitted to what the kernels give.  Every test prints its worst error and its margin to the bound."""
import os
import subprocess
import sys

import numpy as np
import pytest

# (as tests/test_sample.py: torch first, so that it and libshm_grid.so share one HIP runtime -- the memory guards below ask torch for the free device memory)
try:
    import torch  # noqa: F401
except ImportError:
    torch = None

from conftest import GOLDEN, ROOT, c_, load_golden
from test_gpu_parity import _free_memory_gb, make_solver
from test_step1_edges import LAYOUTS, ORACLE_THREADS, _on_grid_sources, _slab_bounds

gpu = pytest.mark.gpu

U = {64: 2.0 ** -53, 32: 2.0 ** -24}                                 # unit roundoff of the handle's number format
TINY = {64: float(np.finfo(np.float64).tiny), 32: float(np.finfo(np.float32).tiny)}   # below this a product is subnormal and its rounding error absolute


def _bunny(n):
    """The 16^3 bunny fixture with the cell rescaled to n - 1 intervals (as test_step1_edges.py)."""
    g = load_golden("bunny_small_n16")
    return dict(pos=g["pos"], wnormal=g["wnormal"], area=g["area"], lam=float(g["lam"]), n=n, bbox_min=g["bbox_min"], cell=float(g["cell"]) * 15 / (n - 1))


def _round_to(v, precision):
    """v rounded to the handle's precision, as an fp64 array (what upload_owned stores)."""
    return v.astype(np.float32).astype(np.float64) if precision == 32 else np.asarray(v, dtype=np.float64)


def _line(what, items):
    print("\n%s: %s" % (what, ", ".join(items)))


# ---- A. Divergence ---------------------------------------------------------------------------------------------------------------------------------------------
def div_restated(Y, n, cell, ka, kb, scrub=False, absolute=False):
    """b = D^T Y on the z-planes [ka, kb), (kb - ka, n, n) values, from the closed form above GridParams in shm_kernels.hip.h:
        b += ( [a>=1] Ya[a-1] + [a==n-1] Ya[a] - [a<n-1] Ya[a] - [a==n-2] Ya[a+1] ) / h     per axis a,
    each term divided by h like the oracle's scatter.  Y(f, k0, k1) returns the planes [k0, k1) of component f as (k1 - k0, n, n).  np.where picks a term or an
    exact 0: a non-finite value never meets a factor 0.  absolute: sum of |terms| (the T of the bounds) instead."""
    nz = kb - ka
    x, y = Y(0, ka, kb), Y(1, ka, kb)
    zlo, zhi = max(ka - 1, 0), min(kb + 1, n)
    z = Y(2, zlo, zhi)
    pad = np.zeros((1, n, n))
    z = np.concatenate(([pad] if ka == 0 else []) + [z] + ([pad] if kb == n else []))   # now the planes [ka - 1, kb + 1)
    ii = np.arange(n)
    axes = ((np.roll(x, 1, axis=2), x, np.roll(x, -1, axis=2), ii[None, None, :]),      # (the rolled-in values sit where the masks are false)
            (np.roll(y, 1, axis=1), y, np.roll(y, -1, axis=1), ii[None, :, None]),
            (z[0:nz], z[1:nz + 1], z[2:nz + 2], np.arange(ka, kb)[:, None, None]))
    b = np.zeros((nz, n, n))
    with np.errstate(invalid="ignore"):
        for ym, yc, yp, a in axes:
            for sign, t in ((1., np.where(a >= 1, ym, 0.)), (1., np.where(a == n - 1, yc, 0.)), (-1., np.where(a < n - 1, yc, 0.)), (-1., np.where(a == n - 2, yp, 0.))):
                b += np.abs(t) / cell if absolute else sign * (t / cell)
    if scrub:
        b[~np.isfinite(b)] = 0.
    return b


def _of_array(Y3):
    """The accessor div_restated wants, over a whole field Y3 (N, 3)."""
    n = round(Y3.shape[0] ** (1 / 3))
    comp = [np.ascontiguousarray(Y3[:, f]).reshape(n, n, n) for f in range(3)]
    return lambda f, k0, k1: comp[f][k0:k1]


# The restatement against the oracle: a node has at most nine terms y / h (three per axis where its index is n - 2), each rounded once by the division, added in
# different orders (the oracle scatters node by node, the restatement walks the axes): at most eight additions each, so the two differ by at most
# 2 * 8 * 2^-53 * T to first order, T = sum |y_t| / h.  18 covers the second-order terms.
RESTATEMENT_K = 18


@pytest.mark.parametrize("scrub", [0, 1])
@pytest.mark.parametrize("n", [4, 11, 16])
def test_divergence_restatement_matches_the_oracle(oracle_c, n, scrub):
    """div_restated equals shmo_divergence to fp64 rounding on random Y with NaN and +-inf entries, scrub on and off, with identical non-finite sets -- whole field
    and plane ranges.  And the count behind the 1 % cap of the non-finite test: one non-finite node of Y reaches at most four entries of b."""
    rng = np.random.default_rng(200 + n)
    N = n ** 3
    Y = rng.standard_normal((N, 3))
    bad = rng.choice(3 * N, size=max(3, N // 40), replace=False)
    Y.reshape(-1)[bad] = rng.choice([np.nan, np.inf, -np.inf], size=bad.size)
    cell = float(rng.uniform(0.05, 0.5))
    ref = np.zeros(N)
    oracle_c.shmo_divergence(n, cell, c_(Y).reshape(-1), scrub, ref)
    acc = _of_array(Y)
    got = div_restated(acc, n, cell, 0, n, scrub=bool(scrub)).reshape(-1)
    T = div_restated(acc, n, cell, 0, n, absolute=True).reshape(-1)
    assert not np.isfinite(Y).all() and (scrub or not np.isfinite(ref).all())
    assert np.array_equal(np.isfinite(got), np.isfinite(ref))
    if scrub:
        assert np.isfinite(ref).all() and np.array_equal(got == 0., ref == 0.)
    fin = np.isfinite(ref) & np.isfinite(T)
    assert (np.abs(got[fin] - ref[fin]) <= RESTATEMENT_K * U[64] * T[fin]).all()
    for ka, kb in ((0, 1), (1, 2), (n - 2, n - 1), (n - 1, n), (1, n - 1), (n // 2, n // 2 + 1)):      # plane ranges: the same bits as the whole field
        part = div_restated(acc, n, cell, ka, kb, scrub=bool(scrub)).reshape(-1)
        assert np.array_equal(part, got[ka * n * n:kb * n * n], equal_nan=True)
    Y1 = rng.standard_normal((N, 3))
    for node in (0, N - 1, (n // 2) * (n * n + n + 1), (n - 2) * (n * n + n + 1)):
        Yn = Y1.copy()
        Yn[node] = np.nan
        assert 1 <= int((~np.isfinite(div_restated(_of_array(Yn), n, cell, 0, n))).sum()) <= 4


# A node's value is a sum of products ih * y: two per axis inside the grid, three where the node's index on that axis is n - 2, so at most nine.  Roundings a
# term passes through in the kernels (a += ih * y, shm_kernels.hip.h): 1 / h formed in fp64 on the host (1), its conversion to T (1), the product (1), at most
# eight additions after it (8): 11 relative roundings of at most u each, so |b_dev - exact| <= 11 u T to first order with T = (1 / h) sum |y_t|.  (A contracted
# multiply-add only removes roundings.)  The oracle divides each term by h (1) and adds at most eight times (8): 9 * 2^-53 * T.  DIV_K = 12 covers both counts
# and their second-order terms; the bound is per node, no global tolerance.
DIV_K = 12


def _div_check(b, ref, T, precision, what):
    """Per node |b - ref| <= DIV_K u T + DIV_K 2^-53 T (+ the subnormal threshold of the format) on the reference's finite nodes; equal non-finite sets.
    Returns (largest error, largest error / bound)."""
    fin = np.isfinite(ref)
    bad = np.flatnonzero(np.isfinite(b) != fin)
    assert bad.size == 0, "%s: %d nodes finite in one field only (first: %s)" % (what, bad.size, bad[:5])
    ok = fin & np.isfinite(T)
    err = np.abs(b[ok] - ref[ok])
    bound = DIV_K * (U[precision] + U[64]) * T[ok] + TINY[precision]
    worst = int(np.argmax(err / bound)) if err.size else 0
    ratio = float((err / bound).max()) if err.size else 0.
    assert ratio <= 1.0, "%s: |db| = %.3e against a bound of %.3e at finite node #%d" % (what, err[worst], bound[worst], worst)
    return float(err.max()) if err.size else 0., ratio


def _device_Y(s):
    """The accessor div_restated wants, over the handle's Y."""
    return lambda f, a, b: s.get_field_planes(f, a, b).reshape(b - a, s.n, s.n)


def _div_case(shm, oracle_c, d, precision, slabs, weighted, planes=None, scrubs=(1,)):
    """One handle: run_conv, then per scrub run_divergence, b read slab by slab on the slab's owned range and compared with shmo_divergence of the handle's own Y
    (planes None: every node) or with the restatement on the given planes.  Returns {scrub: (max error, max error / bound, nodes compared)}."""
    n, cell = int(d["n"]), float(d["cell"])
    bounds = _slab_bounds(shm, d, slabs, weighted, precision)
    s = make_solver(shm, d, precision=precision, local_slabs=slabs, slab_plan=1 if weighted else 0)
    s.run_conv()
    out = {}
    if planes is None:
        Yd = np.stack([s.get_field(f) for f in (0, 1, 2)], axis=1)
        acc = _of_array(Yd)
        T = div_restated(acc, n, cell, 0, n, absolute=True).reshape(-1)
    for scrub in scrubs:
        s.run_divergence(bool(scrub))
        what = "n=%d fp%d slabs %d%s scrub %d" % (n, precision, slabs, "w" if weighted else "", scrub)
        if planes is None:
            b = np.concatenate([s.get_field_planes(s.FIELD_DIV, k0, k1) for k0, k1 in bounds])
            ref = np.zeros(n ** 3)
            oracle_c.shmo_divergence(n, cell, c_(Yd).reshape(-1), int(scrub), ref)
            if scrub:    # where the reference scrubbed, the device holds exactly 0
                raw = np.zeros(n ** 3)
                oracle_c.shmo_divergence(n, cell, c_(Yd).reshape(-1), 0, raw)
                assert np.isfinite(ref).all() and (b[~np.isfinite(raw)] == 0.).all(), what
            e, r = _div_check(b, ref, T, precision, what)
            out[scrub] = (e, r, b.size)
        else:
            e = r = 0.
            acc = _device_Y(s)
            for k in planes:
                assert any(k0 <= k < k1 for k0, k1 in bounds)
                b = s.get_field_planes(s.FIELD_DIV, k, k + 1)
                ref = div_restated(acc, n, cell, k, k + 1, scrub=bool(scrub)).reshape(-1)
                Tk = div_restated(acc, n, cell, k, k + 1, absolute=True).reshape(-1)
                ek, rk = _div_check(b, ref, Tk, precision, what + " plane %d" % k)
                e, r = max(e, ek), max(r, rk)
            out[scrub] = (e, r, len(planes) * n * n)
    s.close()
    return out, bounds


def _seam_planes(n, bounds, extra=()):
    ks = {0, 1, n // 2, n - 2, n - 1} | set(extra)
    for k0, k1 in bounds:
        ks |= {k0 - 1, k0, k0 + 1, k1 - 1}
    return sorted(k for k in ks if 0 <= k < n)


@gpu
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("n", [11, 33, 22, 90, 64])
def test_divergence_scalar_and_vector_kernels_at_slab_seams(shm, oracle_c, n, layout):
    """Every node against shmo_divergence of the handle's own Y.  n = 11, 33: the scalar kernel in both precisions; 22, 90: vectorised in fp64 (VEC 2), scalar in
    fp32 (VEC 4 does not divide n); 64: vectorised in both.  Slabs 1 / 3 / 5 and the weighted plan of 3: the Y2 ghost plane below every seam."""
    d = _bunny(n)
    slabs, weighted = LAYOUTS[layout]
    items = []
    oracle_c.shmo_set_threads(ORACLE_THREADS)
    try:
        for precision in (64, 32):
            out, bounds = _div_case(shm, oracle_c, d, precision, slabs, weighted)
            e, r, cnt = out[1]
            items.append("fp%d %s max|db| %.2e, worst error / bound %.3f (margin %.1fx, %d nodes, slabs %s)" % (
                precision, "vector" if n % (2 if precision == 64 else 4) == 0 else "scalar", e, r, 1 / max(r, 1e-300), cnt, bounds))
    finally:
        oracle_c.shmo_set_threads(min(8, os.cpu_count() or 1))
    _line("divergence n=%d slabs %s vs shmo_divergence on the device's Y" % (n, layout), items)


@gpu
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_divergence_rows_of_two_waves_fp64(shm, oracle_c, layout):
    """n = 256, fp64: a row is 128 lanes, so the second wave's first lane reloads its left neighbour ((threadIdx.x & 63) == 0).  Checked with the restatement on
    the planes k0 - 1, k0, k0 + 1, k1 - 1 of every slab and 0, 1, n / 2, n - 2, n - 1."""
    d = _bunny(256)
    slabs, weighted = LAYOUTS[layout]
    bounds = _slab_bounds(shm, d, slabs, weighted, 64)
    ks = _seam_planes(256, bounds)
    out, _ = _div_case(shm, oracle_c, d, 64, slabs, weighted, planes=ks)
    e, r, cnt = out[1]
    _line("divergence n=256 fp64 slabs %s vs restatement on the device's Y" % layout,
          ["planes %s: max|db| %.2e, worst error / bound %.3f (margin %.1fx, %d nodes)" % (ks, e, r, 1 / max(r, 1e-300), cnt)])


@gpu
def test_divergence_rows_of_two_waves_fp32(shm, oracle_c):
    """n = 512, fp32 (VEC 4): 128 lanes per row.  Planes 0, 1, n / 2, n - 2, n - 1 through get_field_planes against the restatement."""
    dev_gb, host_gb = _free_memory_gb()
    if dev_gb < 8 or host_gb < 4:
        pytest.skip("needs 8 GB of free device memory and 4 GB of host memory, found %.0f / %.0f GB" % (dev_gb, host_gb))
    n = 512
    ks = [0, 1, n // 2, n - 2, n - 1]
    out, _ = _div_case(shm, oracle_c, _bunny(n), 32, 1, False, planes=ks)
    e, r, cnt = out[1]
    _line("divergence n=512 fp32 one slab vs restatement on the device's Y",
          ["planes %s: max|db| %.2e, worst error / bound %.3f (margin %.1fx, %d nodes)" % (ks, e, r, 1 / max(r, 1e-300), cnt)])


@gpu
def test_divergence_two_x_chunks_fp64(shm, oracle_c):
    """n = 1024, fp64: 512 lanes per row in two chunks of 256 (xchunks = 2): lx == 0 of the second chunk reloads its left neighbour.  About 50 GB on the device."""
    dev_gb, host_gb = _free_memory_gb()
    if dev_gb < 120 or host_gb < 8:
        pytest.skip("needs 120 GB of free device memory and 8 GB of host memory, found %.0f / %.0f GB" % (dev_gb, host_gb))
    n = 1024
    ks = [0, 1, n // 2, n - 2, n - 1]
    out, _ = _div_case(shm, oracle_c, _bunny(n), 64, 1, False, planes=ks)
    e, r, cnt = out[1]
    _line("divergence n=1024 fp64 one slab vs restatement on the device's Y",
          ["planes %s: max|db| %.2e, worst error / bound %.3f (margin %.1fx, %d nodes)" % (ks, e, r, 1 / max(r, 1e-300), cnt)])


@gpu
@pytest.mark.parametrize("slabs", [1, 3])
@pytest.mark.parametrize("precision", [64, 32])
def test_divergence_of_a_non_finite_Y(shm, oracle_c, precision, slabs):
    """Sources exactly on nodes (the input of test_step1_sources_exactly_on_nodes_and_faces): Y is NaN there.  scrub = 0: the non-finite nodes of b are the
    reference's; scrub = 1: none, and exactly 0 where the reference scrubbed.  The finite nodes keep the bound."""
    d, _ = _on_grid_sources(3)
    n = int(d["n"])
    oracle_c.shmo_set_threads(ORACLE_THREADS)
    try:
        s = make_solver(shm, d, precision=precision, local_slabs=slabs)
        s.run_conv()
        Yd = np.stack([s.get_field(f) for f in (0, 1, 2)], axis=1)
        s.close()
        raw = np.zeros(n ** 3)
        oracle_c.shmo_divergence(n, float(d["cell"]), c_(Yd).reshape(-1), 0, raw)
        y_bad, b_bad = int((~np.isfinite(Yd).all(axis=1)).sum()), int((~np.isfinite(raw)).sum())
        assert y_bad >= 1, "the device's Y is finite everywhere: the input does not reach the scrub"
        assert 1 <= b_bad < 0.01 * n ** 3 and b_bad <= 4 * y_bad, (y_bad, b_bad)
        out, _ = _div_case(shm, oracle_c, d, precision, slabs, False, scrubs=(0, 1))
    finally:
        oracle_c.shmo_set_threads(min(8, os.cpu_count() or 1))
    _line("divergence of a non-finite Y, n=%d fp%d slabs %d: %d non-finite nodes of Y, %d of b (scrub 0), as the reference's" % (n, precision, slabs, y_bad, b_bad),
          ["scrub %d max|db| %.2e, worst error / bound %.3f (margin %.1fx)" % (sc, e, r, 1 / max(r, 1e-300)) for sc, (e, r, _) in sorted(out.items())])


# ---- B. Laplacian, fp32 -------------------------------------------------------------------------------------------------------------------------------------------
# laplacian_kernel: ((xp + yp + zp + xm + ym + zm) - 6 uc) * (T)inv_h2.  A neighbour's value passes five additions, the subtraction, the product, and the factor
# carries the conversion of 1 / h^2 to T: 8 roundings of u; the centre term 6 uc is rounded once (6 is not a power of two) and then passes three of them.  So
# |out - exact| <= 8 u T, T = (1 / h^2) (sum |neighbours| + 6 |uc|), to first order.  The oracle forms 1 / (h * h) (2), adds six times (6) and multiplies (1):
# 9 * 2^-53 * T.  LAP_K = 10 covers both and the second-order terms, per node.
LAP_K = 10


@gpu
@pytest.mark.parametrize("slabs", [1, 3])
@pytest.mark.parametrize("n", [11, 16, 33, 64])
def test_laplacian_fp32_matches_oracle(shm, oracle_c, n, slabs):
    """The instrument of the fp32 KKT tests, held itself: fp32 handle against shmo_laplacian_apply on the float32-rounded input, per node."""
    d = _bunny(n)
    cell = float(d["cell"])
    u = _round_to(np.random.default_rng(n).standard_normal(n ** 3), 32)
    s = make_solver(shm, d, precision=32, local_slabs=slabs)
    got = s.apply_laplacian(u)
    s.close()
    ref = np.empty_like(u)
    oracle_c.shmo_laplacian_apply(n, cell, u, ref)
    a = np.abs(np.pad(u.reshape(n, n, n), 1, mode="edge"))                                      # an out-of-grid neighbour is the node itself
    T = (a[2:, 1:-1, 1:-1] + a[:-2, 1:-1, 1:-1] + a[1:-1, 2:, 1:-1] + a[1:-1, :-2, 1:-1] + a[1:-1, 1:-1, 2:] + a[1:-1, 1:-1, :-2] + 6 * a[1:-1, 1:-1, 1:-1]).reshape(-1) / cell ** 2
    err = np.abs(got - ref)
    bound = LAP_K * (U[32] + U[64]) * T + TINY[32]
    r = float((err / bound).max())
    _line("laplacian fp32 n=%d slabs %d vs shmo_laplacian_apply" % (n, slabs), ["max|d| %.2e, worst error / bound %.3f (margin %.1fx)" % (err.max(), r, 1 / max(r, 1e-300))])
    assert r <= 1.0, (n, slabs, r)


# ---- C. Projector ---------------------------------------------------------------------------------------------------------------------------------------------------
PROJ_FP64 = 1e-11        # of max|v|: test_projector's own figure
PROJ_TWO_LEVEL = 1e-10   # of max|v|: test_two_level_inverse_of_AAT_matches_lu_golden's figure for A P v
# fp32 handle: gather_rows_kernel, ginv_matvec_kernel and scatter_nodes_kernel compute in fp64 from the stored fp32 values and round once, on the store:
# |d| <= 2^-24 |Pv_ref| + (the fp64 figure) max|v| at the nodes some constraint row touches; every other node is not written at all.


class _HostProjector:
    """P = I - A^T (A A^T)^-1 A in fp64 on the host, dense (m is 1129 for bunny_small at 64^3), with one step of iterative refinement of the solve."""

    def __init__(self, nodes, coeffs, N):
        import scipy.linalg
        import scipy.sparse as sp
        m = nodes.shape[0]
        self.A = sp.csr_matrix((coeffs.ravel(), (np.repeat(np.arange(m), 8), nodes.ravel())), shape=(m, N))   # (duplicate entries are summed)
        self.G = (self.A @ self.A.T).toarray()
        self.lu = scipy.linalg.lu_factor(self.G)
        self.touched = np.zeros(N, dtype=bool)
        self.touched[nodes.ravel()] = True

    def __call__(self, v):
        import scipy.linalg
        w = self.A @ v
        mu = scipy.linalg.lu_solve(self.lu, w)
        mu += scipy.linalg.lu_solve(self.lu, w - self.G @ mu)
        return v - self.A.T @ mu


def _projector_errors(P, precision, tol, v, got):
    """(worst error / bound at the touched nodes, largest error) of got = the device's P v for the uploaded v; bit-equality everywhere else."""
    ref = P(v)
    assert np.array_equal(got[~P.touched], v[~P.touched]), "a node outside every constraint stencil was changed"
    err = np.abs(got - ref)[P.touched]
    bound = (U[32] * np.abs(ref[P.touched]) if precision == 32 else 0.) + tol * np.abs(v).max()
    return float((err / bound).max()), float(err.max())


def _projector_case(s, d_n, precision, tol, with_properties, P=None):
    """P: the host projector to hold the handle to (test_ginv_edges.py passes its refined one); by default the dense one of this file."""
    n = d_n
    nodes, coeffs = s.get_constraints()
    if P is None:
        P = _HostProjector(nodes, coeffs, n ** 3)
    rng = np.random.default_rng(1)
    v = _round_to(rng.standard_normal(n ** 3), precision)
    Pv = s.apply_projector(v)
    r_rand, e_rand = _projector_errors(P, precision, tol, v, Pv)
    v0 = _round_to(P(rng.standard_normal(n ** 3)), precision)          # built in null(A) on the host, then rounded to the handle's precision
    Pv0 = s.apply_projector(v0)
    r_null, e_null = _projector_errors(P, precision, tol, v0, Pv0)
    moved = float(np.abs(Pv0 - v0).max())
    if precision == 64:
        assert moved < tol * np.abs(v0).max(), moved                  # a vector of null(A) is left alone
    if with_properties and precision == 64:                           # the three properties of test_projector, as they are there
        assert np.abs((coeffs * Pv[nodes]).sum(axis=1)).max() < 1e-11
        assert np.abs(s.apply_projector(Pv) - Pv).max() < 1e-11
        w = rng.standard_normal(nodes.shape[0])
        Atw = np.zeros(n ** 3)
        np.add.at(Atw, nodes.ravel(), (coeffs * w[:, None]).ravel())
        assert np.abs(s.apply_projector(Atw)).max() < 1e-10 * np.abs(Atw).max()
    return dict(m=nodes.shape[0], r_rand=r_rand, e_rand=e_rand, r_null=r_null, e_null=e_null, moved=moved, untouched=int((~P.touched).sum()))


def _projector_report(what, res):
    _line(what, ["fp%d m %d: random v max|d| %.2e, error / bound %.3f (margin %.1fx); null(A) v max|d| %.2e, error / bound %.3f (margin %.1fx), moved by %.2e; %d untouched nodes bit-equal"
                 % (p, r["m"], r["e_rand"], r["r_rand"], 1 / max(r["r_rand"], 1e-300), r["e_null"], r["r_null"], 1 / max(r["r_null"], 1e-300), r["moved"], r["untouched"])
                 for p, r in res])
    for p, r in res:
        assert r["r_rand"] <= 1.0 and r["r_null"] <= 1.0, (what, p, r)


@gpu
@pytest.mark.parametrize("slabs", [1, 3])
@pytest.mark.parametrize("case", ["bunny_small_n16", "bunny_small_n32", "bunny_small_n64", "bunny_pc_n32"])
def test_projector_matches_the_host_projector(shm, case, slabs):
    """P v against v - A^T (A A^T)^-1 A v from get_constraints(), for a random v and for a v of null(A), both rounded to the handle's precision first; nodes outside
    every constraint stencil come back bit-equal to what was uploaded.  A projector that returns 0, or v, fails the first or the second."""
    d = load_golden(case)
    res = []
    for precision in (64, 32):
        s = make_solver(shm, d, precision=precision, local_slabs=slabs)
        res.append((precision, _projector_case(s, int(d["n"]), precision, PROJ_FP64, True)))
        s.close()
    _projector_report("projector %s slabs %d vs the fp64 host projector" % (case, slabs), res)


_TWO_LEVEL_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import shm_import
shm = shm_import.load()
import test_stage_edges as t
d = np.load(%(fixture)r)
out = {}
for precision in (64, 32):
    s = t.make_solver(shm, d, precision=precision)
    for k, val in t._projector_case(s, int(d["n"]), precision, t.PROJ_TWO_LEVEL, True).items():
        out["%%s_%%d" %% (k, precision)] = val
    s.close()
np.savez(%(out)r, **out)
"""


@gpu
def test_projector_two_level_inverse_matches_the_host_projector(tmp_path):
    """The two-level (boxes + separator) inverse of A A^T forced onto bunny_small_n32 as test_two_level_inverse_of_AAT_matches_lu_golden forces it (the library reads
    SHM_TL_MIN_M / SHM_TL_BOX once per process: one child process, under its own time limit), held to the same host projector at that test's 1e-10."""
    out = str(tmp_path / "two_level.npz")
    code = _TWO_LEVEL_CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"), fixture=os.path.join(GOLDEN, "bunny_small_n32.npz"), out=out)
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SHM_TL_MIN_M="32", SHM_TL_BOX="4"), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    z = np.load(out)
    res = [(precision, {k: z["%s_%d" % (k, precision)].item() for k in ("m", "r_rand", "e_rand", "r_null", "e_null", "moved", "untouched")}) for precision in (64, 32)]
    _projector_report("projector bunny_small_n32, two-level inverse (SHM_TL_MIN_M=32, SHM_TL_BOX=4) vs the fp64 host projector", res)


# ---- D. Fast integration ------------------------------------------------------------------------------------------------------------------------------------------
FAST_FP64 = 1e-9   # the project's figure (test_fast_integration_matches_bfs_golden)
# fp32 handle: bfs_plane0_kernel and bfs_z_kernel accumulate phi in fp64 from the stored fp32 Y (exact input for the reference) and round phi to float on every
# store: 2^-24 |phi| per stored value.  A scan restarts from a stored value where it re-reads one: once at the end of the row j = 0 (the y scans start from it),
# once on plane 0 (the z scans start from it) and once per slab seam above the first slab (slabs - 1): a node's value carries at most 1 + 1 + 1 + (slabs - 1)
# roundings of values no larger than max|phi_greedy|, its own store included.  The shift is an average of stored values (one more, at most), and phi - shift
# is rounded on its store (one more): (slabs + 4) * 2^-24 * max|phi_ref + shift|, plus the fp64 figure for what the fp64 arithmetic in between does.


def _fast_bound(precision, slabs, greedy):
    return ((slabs + 4) * U[32] * float(np.abs(greedy).max()) if precision == 32 else 0.) + FAST_FP64


@gpu
@pytest.mark.parametrize("slabs", [1, 2, 5])
@pytest.mark.parametrize("n", [11, 23, 32, 64, 90])
def test_fast_integration_matches_oracle_on_the_device_Y(shm, oracle_c, n, slabs):
    """solve(fast=True) in both precisions against shmo_integrate_greedily on the handle's own Y, minus shmo_source_average of it."""
    d = _bunny(n)
    S = len(d["area"])
    items = []
    for precision in (64, 32):
        s = make_solver(shm, d, precision=precision, local_slabs=slabs)
        s.solve(fast=True)
        phi, _ = s.get_phi()
        try:
            Yd = np.stack([s.get_field(f) for f in (0, 1, 2)], axis=1)
        except shm.ShmError:                                             # the handle no longer holds Y: Step 1 is deterministic (test_step1_block_order_does_not_change_Y)
            s.run_conv()
            Yd = np.stack([s.get_field(f) for f in (0, 1, 2)], axis=1)
        s.close()
        assert np.isfinite(Yd).all()
        greedy = np.zeros(n ** 3)
        oracle_c.shmo_integrate_greedily(n, c_(d["bbox_min"]), float(d["cell"]), c_(Yd).reshape(-1), greedy)
        shift = oracle_c.shmo_source_average(n, c_(d["bbox_min"]), float(d["cell"]), greedy, S, c_(d["pos"]).reshape(-1), c_(d["area"]))
        err = float(np.abs(phi - (greedy - shift)).max())
        bound = _fast_bound(precision, slabs, greedy)
        items.append((precision, err, bound))
    _line("fast integration n=%d slabs %d vs shmo_integrate_greedily on the device's Y" % (n, slabs),
          ["fp%d max|dphi| %.2e, bound %.2e (margin %.1fx)" % (p, e, b, b / max(e, 1e-300)) for p, e, b in items])
    for p, e, b in items:
        assert e <= b, (n, slabs, p, e, b)


# ---- E. DCT preconditioner, fp32 -----------------------------------------------------------------------------------------------------------------------------------
# The rounding of the line transforms cannot be derived tightly, so it is measured against a reference, not against the kernel: the same chain in float32 with
# scipy (pocketfft keeps float32) has the L-infinity error E32(n) against the fp64 chain on the same float32-rounded input, and the device is held to 8 E32(n).
# Why 8: the kernel forms its inter-pass twiddles by a multiplication tree and packs two real lines into one complex FFT -- a few more roundings per pass than
# pocketfft's tabulated twiddles, over six 1-D transforms; a defect (a wrong twiddle, swapped lines, a tile or segment seam) gives 1e-2 ... 1 of max|ref|.
DCT_FACTOR = 8
# n not a power of two: six dense products with the DCT matrix, in double whatever T (launch_precond_gemm: convert_kernel<float, double> on the way in,
# <double, float> on the way out).  The input is already float32, so the output's single rounding is all there is: 2^-24 |ref|, held at 2^-23 max|ref|.
DCT_DENSE = 2.0 ** -23


def _dct_case(shm, n, slabs):
    from scipy.fft import dctn, idctn
    d = _bunny(n)
    h = float(d["cell"])
    v = _round_to(np.random.default_rng(n).standard_normal(n ** 3), 32)
    s = make_solver(shm, d, precision=32, local_slabs=slabs)
    got = s.apply_preconditioner(v)
    s.close()
    lam1 = (2 - 2 * np.cos(np.pi * np.arange(n) / n)) / h ** 2
    LAM = lam1[:, None, None] + lam1[None, :, None] + lam1[None, None, :]
    inv = np.where(LAM > 0, 1 / np.where(LAM > 0, LAM, 1), 0.0)
    del LAM
    w = ORACLE_THREADS
    ref = idctn(dctn(v.reshape(n, n, n), type=2, norm="ortho", workers=w) * inv, type=2, norm="ortho", workers=w).reshape(-1)
    ref32 = idctn(dctn(v.reshape(n, n, n).astype(np.float32), type=2, norm="ortho", workers=w) * inv.astype(np.float32), type=2, norm="ortho", workers=w)
    assert ref32.dtype == np.float32
    scale = float(np.abs(ref).max())
    e32 = float(np.abs(ref32.reshape(-1) - ref).max())
    del ref32, inv
    return float(np.abs(got - ref).max()), e32, scale


@gpu
@pytest.mark.parametrize("slabs,n", [(1, 16), (1, 32), (1, 64), (1, 128), (1, 256), (1, 512), (2, 32), (4, 64)])
def test_preconditioner_fp32_line_transforms_match_the_dct(shm, slabs, n):
    """fp32 handle, n = 2^k: dct_lines_kernel's fp32 tiles (one slab) and the multi-slab packed sweeps against scipy's fp64 chain, at 8 x the error of scipy's
    float32 chain on the same input."""
    if n >= 512:
        dev_gb, host_gb = _free_memory_gb()
        if dev_gb < 8 or host_gb < 12:
            pytest.skip("needs 8 GB of free device memory and 12 GB of host memory, found %.0f / %.0f GB" % (dev_gb, host_gb))
    err, e32, scale = _dct_case(shm, n, slabs)
    _line("fp32 DCT preconditioner n=%d slabs %d vs scipy fp64" % (n, slabs),
          ["max|d| %.2e = %.2e max|ref|; scipy float32 E32 %.2e = %.2e max|ref|; err_dev / E32 = %.2f (bound %d, margin %.1fx)"
           % (err, err / scale, e32, e32 / scale, err / e32, DCT_FACTOR, DCT_FACTOR * e32 / max(err, 1e-300))])
    assert err <= DCT_FACTOR * e32, (n, slabs, err, e32)


@gpu
@pytest.mark.parametrize("n", [22, 45, 90])
def test_preconditioner_fp32_dense_products_match_the_dct(shm, n):
    """fp32 handle, n not a power of two: the dense-product path is fp64 inside, so only the output's rounding to float remains."""
    err, e32, scale = _dct_case(shm, n, 1)
    _line("fp32 DCT preconditioner n=%d (dense products) vs scipy fp64" % n,
          ["max|d| %.2e = %.2e max|ref|, bound 2^-23 = %.2e (margin %.1fx); scipy float32 E32 %.2e max|ref|" % (err, err / scale, DCT_DENSE, DCT_DENSE * scale / max(err, 1e-300), e32 / scale)])
    assert err <= DCT_DENSE * scale, (n, err, scale)
