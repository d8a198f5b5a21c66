"""Step 1 with the far list's remainder carried from cluster to cluster (conv_tiered_kernel, csrc/shm_conv_tiered.hip.h; bookkeeping csrc/shm_far_carry.h): the far
loop takes four sources per trip, a cluster's leftover entries stay at the head of the wave's lists for the next cluster, and the list is padded and drained only
before a flush of the packed-fp32 sums, before the a-posteriori test and at the end of the fp32 solve's pass.  Every case runs Step 1 alone (shm_grid_run_conv) on a
small grid and holds Y to the C oracle on ALL planes -- the Step-1 budget of 1e-8 for an fp64 handle, the fp32 bound of test_gpu_parity.py for an fp32 one --, with
the rule of tests/test_step1_edges.py (the non-finite nodes are the oracle's; nodes with lambda r_min >= 335 are left out: none here, at most 5 % asserted), and
asserts that two default runs give the same bits.  The pair counters (of a solve with the same arithmetic) are printed and must show the tier under test at work.

Inputs (seeded; the sources are Morton-sorted into clusters of 64 by set_problem, so a block sees, cluster by cluster, anything from no far source -- a cluster next
to it: all near; one beyond the drop threshold: all dropped -- to 64 of them):
  remainders  64 k + r sources (k = 3; r = 0 ... 3 and 5) on an ellipsoid, lambda * cell = 1: the last cluster holds r real sources, the others are cut by the far
              window (8 ... ~24 e-folds below a block's nearest source) at a different place for every block -- every remainder, and empty clusters between
              occupied ones (the ellipsoid's near side: near; its flanks: far; Morton order visits near and far octants in turn);
  flush       3000 sources on a sphere 40 cells across in a 48^3 grid: from a block next to the sphere, the sources 15 ... 31 cells away are far -- about 0.46 of
              the sphere -- so the packed-fp32 sums are flushed (every 256 far sources) at least twice inside a block, with clusters of uneven far counts before
              each flush; asserted from the kernel's counter: a mean of >= 512 far sources per block;
  second pass two cancelling sheets a tenth of a cell apart (the same positions and areas, opposite normals): |X| is down to 1e-5 of the sum of |terms|, so blocks with
              far sources fail the a-posteriori test behind the end-of-pass drain and run every source again in fp64 -- pairs_redone > 0 is asserted;
  block shapes the remainders' input at the smallest side with NPT = 4 and at 32 (NPT = 2); cut blocks: a side of 37 (partial blocks in x, y and z); one fp32 handle."""
import numpy as np
import pytest

from test_gpu_parity import Y_BUDGET, Y_BUDGET_F32, make_solver
from test_near_body_gpu import _smallest_npt4_side, accurate_zone, oracle_field
from test_step1_edges import _step1_npt

pytestmark = pytest.mark.gpu

TIER_FLUSH = 256        # kTierFlush


def ellipsoid_sources(n, S, seed=20258, lam_cell=1.0, radii=(0.36, 0.31, 0.27)):
    """set_problem arguments: cell a power of two, bbox_min a multiple of it (node coordinates exact), S sources on an ellipsoid around the grid's centre."""
    rng = np.random.default_rng(seed)
    cell = 2.0 ** -5
    bbox_min = np.full(3, -np.floor((n - 1) / 2) * cell)
    ext = (n - 1) * cell
    v = rng.normal(size=(S, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    ax3 = np.array(radii) * ext
    mid = bbox_min + 0.5 * ext + np.array([0.013, -0.021, 0.017]) * ext
    pos = mid + v * ax3
    nrm = v / ax3
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    area = 4 * np.pi * (0.3 * ext) ** 2 / S * (0.5 + rng.random(S))
    return dict(pos=pos, wnormal=nrm * area[:, None], area=area, lam=lam_cell / cell, n=n, bbox_min=bbox_min, cell=cell)


_REF = {}


def _reference(oracle_c, key, make):
    """(inputs, the oracle's Y on all planes, the accurate zone): computed once per input, shared, never written to."""
    if key not in _REF:
        d = make()
        ref = oracle_field(oracle_c, d)
        ref.setflags(write=False)
        _REF[key] = (d, ref, accurate_zone(d))
    return _REF[key]


def _field(s):
    return np.stack([s.get_field(f) for f in (0, 1, 2)], axis=1)


def _check(shm, d, ref, zone, label, precision=64, expect_npt=None):
    """Two default runs of Step 1: the same bits, the oracle's non-finite nodes, max|dY| inside the bound; returns the counters of a solve with the same arithmetic."""
    n = int(d["n"])
    if expect_npt is not None:
        assert _step1_npt(n, n) == expect_npt, (n, expect_npt)
    s = make_solver(shm, d, precision=precision)
    s.run_conv()
    Y1 = _field(s)
    s.run_conv()
    Y2 = _field(s)
    st = s.solve(max_iters=2, allow_noconv=True)
    s.close()
    fin = np.isfinite(ref).all(axis=1)
    bad = np.flatnonzero(np.isfinite(Y1).all(axis=1) != fin)
    assert 1.0 - zone.mean() <= 0.05, zone.mean()
    ok = fin & zone
    err = float(np.abs(Y1[ok] - ref[ok]).max())
    bound = Y_BUDGET if precision == 64 else Y_BUDGET_F32
    nom = float(n) ** 3 * len(d["area"])
    print("\nfar carry %-28s n=%d S=%d fp%d: max|dY| vs C oracle %.3e (bound %.0e, margin %.1fx); pairs fp64 %.0f packed fp32 %.0f redone %.0f (of nominal: %.3f %.3f %.4f)" % (
        label, n, len(d["area"]), precision, err, bound, bound / max(err, 1e-300), st.pairs_fp64, st.pairs_fp32, st.pairs_redone,
        st.pairs_fp64 / nom, st.pairs_fp32 / nom, st.pairs_redone / nom))
    assert np.array_equal(Y1, Y2, equal_nan=True)
    assert bad.size == 0, "%d nodes finite in one field only (first: %s)" % (bad.size, bad[:5])
    assert err < bound, (label, err)
    assert st.pairs_fp32 > 0, "no pair went through the far tier"
    return st


def far_sources_per_block(st, n, npt):
    """The mean number of far sources a block staged, from the kernel's own counter (it counts 64 x NPT pairs per staged far source and block)."""
    blocks = ((n + 7) // 8) ** 2 * ((n + npt - 1) // npt)
    return st.pairs_fp32 / (64.0 * npt * blocks)


@pytest.mark.parametrize("r", [0, 1, 2, 3, 5])
def test_every_remainder_of_the_far_list(shm, oracle_c, r):
    """64 k + r sources at NPT = 2: per-cluster far counts of every remainder, empty clusters between occupied ones."""
    S = 64 * 3 + r
    d, ref, zone = _reference(oracle_c, ("ellipsoid", 32, S), lambda: ellipsoid_sources(32, S))
    _check(shm, d, ref, zone, "remainder r=%d" % r, expect_npt=2)


def test_flushes_with_a_carry_pending(shm, oracle_c):
    """3000 sources on a sphere 40 cells across in a 48^3 grid.  The kernel's counter must show a MEAN of at least 2 x 256 far sources per block: then at least one
    block (in fact most blocks near the sphere) flushed its packed-fp32 sums twice, each time behind a drain of whatever its clusters -- of uneven far counts --
    had carried up to there."""
    d, ref, zone = _reference(oracle_c, ("sphere", 48, 3000), lambda: ellipsoid_sources(48, 3000, radii=(0.425, 0.425, 0.425)))
    st = _check(shm, d, ref, zone, "flush with a carry", expect_npt=2)
    mean_far = far_sources_per_block(st, 48, 2)
    print("flush case: %.0f far sources per block on average (a flush every %d)" % (mean_far, TIER_FLUSH))
    assert mean_far >= 2 * TIER_FLUSH, mean_far


def cancelling_sheets(n, sep_cells=0.1, seed=20259):
    """Two sheets of sources `sep_cells` of a cell apart with the same (x, y) positions, the same areas and opposite normals, one source per cell over the middle 0.62
    of the grid, lambda * cell = 1, gently undulating (flat sheets would make Y = (0, 0, +-1) whatever the arithmetic).  Every pair's terms cancel to about
    lambda * sep of their size: over the nodes of the 48^3 grid (numpy) |X| is 4e-2 of the sum of |terms| in the median and 8e-6 of it at worst.  Where the far
    tier's share of that sum exceeds 1e-2 |X| the a-posteriori test (eps_far L1_far <= budget |X|) fails and the block runs again.
    The separation is a tenth of a cell and no less on purpose: every tier's relative error is amplified by sum|terms| / |X|, the fp64 near body's included, and
    measured on an MI355X max|dY| against the oracle is 2e-14 / min(|X| / sum|terms|) -- 1.5e-10 at half a cell (no block runs again there), 4.5e-8 at a hundredth
    of a cell (beyond the budget, in pure fp64 arithmetic as well), 2.4e-9 expected here."""
    rng = np.random.default_rng(seed)
    cell = 2.0 ** -5
    bbox_min = np.full(3, -np.floor((n - 1) / 2) * cell)
    ext = (n - 1) * cell
    g = np.arange(int(0.62 * n)) * cell
    g = g - g.mean() + 0.37 * cell
    X, Yg = np.meshgrid(g, g, indexing="ij")
    X = X + (rng.random(X.shape) - 0.5) * 0.3 * cell
    Yg = Yg + (rng.random(X.shape) - 0.5) * 0.3 * cell
    mid = bbox_min + 0.5 * ext
    kx, ky = 5.0 / ext, 4.0 / ext
    z = 0.03 * ext * np.sin(kx * X) * np.cos(ky * Yg) + 0.123 * cell
    nv = np.stack([-0.03 * ext * kx * np.cos(kx * X) * np.cos(ky * Yg), 0.03 * ext * ky * np.sin(kx * X) * np.sin(ky * Yg), np.ones(X.shape)], -1)
    nv /= np.linalg.norm(nv, axis=-1, keepdims=True)
    lo = np.stack([X, Yg, z], -1).reshape(-1, 3) + mid
    hi = lo + np.array([0.0, 0.0, sep_cells * cell])
    area1 = (cell * cell * (0.8 + 0.4 * rng.random(len(lo))))
    pos = np.vstack([lo, hi])
    nrm = np.vstack([-nv.reshape(-1, 3), nv.reshape(-1, 3)])
    area = np.concatenate([area1, area1])
    return dict(pos=pos, wnormal=nrm * area[:, None], area=area, lam=1.0 / cell, n=n, bbox_min=bbox_min, cell=cell)


def test_second_pass_with_a_carry_pending(shm, oracle_c):
    """Two cancelling sheets a tenth of a cell apart: blocks fail the a-posteriori test -- run behind the end-of-pass drain of a pending carry -- and evaluate
    every source again in fp64, from cleared sums and an empty far list."""
    d, ref, zone = _reference(oracle_c, ("sheets", 48), lambda: cancelling_sheets(48))
    st = _check(shm, d, ref, zone, "second pass (sheets)", expect_npt=2)
    assert st.pairs_redone > 0, st.pairs_redone


def test_block_shape_npt4(shm, oracle_c):
    """The smallest side at which the solver picks NPT = 4 (97 on an MI355X): four squared z offsets per far list entry, 64 k + 5 sources."""
    n = _smallest_npt4_side()
    S = 64 * 3 + 5
    d, ref, zone = _reference(oracle_c, ("ellipsoid", n, S), lambda: ellipsoid_sources(n, S, lam_cell=0.5))
    _check(shm, d, ref, zone, "NPT = 4", expect_npt=4)


def test_cut_blocks(shm, oracle_c):
    """A side of 37 = 4 x 8 + 5 = 18 x 2 + 1: partial blocks in x, y and z run the same lists (their lanes past the grid evaluate and do not store)."""
    S = 64 * 3 + 2
    d, ref, zone = _reference(oracle_c, ("ellipsoid", 37, S), lambda: ellipsoid_sources(37, S))
    _check(shm, d, ref, zone, "cut blocks", expect_npt=2)


def test_fp32_handle(shm, oracle_c):
    """The fp32 solve: every kept source in the packed-fp32 body, no flushes, one drain at the end of the pass."""
    S = 64 * 3 + 3
    d, ref, zone = _reference(oracle_c, ("ellipsoid", 32, S), lambda: ellipsoid_sources(32, S))
    st = _check(shm, d, ref, zone, "fp32 handle", precision=32)
    assert st.pairs_fp32 > st.pairs_fp64
