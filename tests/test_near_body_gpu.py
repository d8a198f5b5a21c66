"""The near tier's body (yukawa_near / yukawa_near_batch, csrc/shm_conv_tiered.hip.h) after the Newton step was folded into the exponent scale: Step 1 alone
(shm_grid_run_conv) with step1_arith = EXACT_F64, so that every (node, source) pair runs the near body, against the C oracle on ALL planes -- a handful of sources, so
the oracle takes well under a second -- at the smallest side at which the solver picks the NPT = 4 kernel and at an NPT = 2 side with partial x and y blocks.
Inputs (seeded): 40 sources on an ellipsoid, lambda * cell = 0.3, and the three places where the one new rounding (of cc = |c| (1 + e), inside the exponent) or the
1 / |c| pre-scaling of the staged weights is largest:
  lam10    lambda x 10 (lambda * cell = 3): exponents reach hundreds of octaves across the grid, just inside the 2^-990 span the host allows the kernel;
  close    one more source 1e-3 cell from a node and one exactly on a node (non-finite there, like the oracle);
  weights  weights spanning 1e6 : 1.
The rule of tests/test_step1_edges.py throughout: the non-finite nodes are the oracle's, and nodes with lambda r_min >= 335 (where the reference's own normalisation
has lost its bits: test_gpu_parity.py::test_tier_budget_on_adversarial_inputs) are left out -- none on these inputs, and at most 5 % is asserted.

Tolerance: twice what the PARENT commit (the 12-instruction body) reads on the same inputs on an MI355X, never above the Step-1 budget of 1e-8.  The parent's max|dY|
against the C oracle, measured with this file run against the parent's library (PARENT_MAX_DY below; the new body's figures beside them):
                      base                  lam10                 close                 weights
    n = 97 (NPT 4)    4.052e-13 (4.051e-13) 1.250e-12 (1.289e-12) 1.120e-12 (1.121e-12) 1.031e-12 (1.030e-12)
    n = 27 (NPT 2)    4.407e-12 (4.411e-12) 1.874e-13 (1.878e-13) 5.212e-13 (5.221e-13) 8.964e-13 (8.969e-13)
and the parent's tiered default at n = 97 evaluates 24 114 176 pairs in fp64 and 19 149 824 in packed fp32, none twice (PARENT_PAIRS); max|dY| 1.19e-10 either way."""
import numpy as np
import pytest

from conftest import c_
from test_gpu_parity import make_solver
from test_step1_edges import LAMBDA_R_ZONE, _step1_npt

pytestmark = pytest.mark.gpu

STEP1_BUDGET = 1e-8
N_NPT2 = 27                      # NPT = 2; 27 = 3 x 8 + 3 = 13 x 2 + 1: partial blocks in x, y and z
VARIANTS = ("base", "lam10", "close", "weights")
# max|dY| of the PARENT commit on these inputs (MI355X, EXACT_F64, against the C oracle)
PARENT_MAX_DY = {("npt4", "base"): 4.052e-13, ("npt4", "lam10"): 1.250e-12, ("npt4", "close"): 1.120e-12, ("npt4", "weights"): 1.031e-12,
                 ("npt2", "base"): 4.407e-12, ("npt2", "lam10"): 1.874e-13, ("npt2", "close"): 5.212e-13, ("npt2", "weights"): 8.964e-13}
# (pairs_fp64, pairs_fp32) of the PARENT commit's tiered default on the NPT = 4 shape, "base" sources
PARENT_PAIRS = (24114176.0, 19149824.0)


def _smallest_npt4_side():
    """The smallest grid side at which launch_conv picks NPT = 4 on this device (4 workgroups per CU: 97 on the 256 CUs of an MI355X)."""
    n = 8
    while _step1_npt(n, n) != 4:
        n += 1
    return n


def near_body_sources(n, variant):
    """set_problem arguments: cell a power of two and bbox_min a multiple of it (node coordinates exact), 40 sources on an ellipsoid around the grid's centre."""
    rng = np.random.default_rng(20251)
    cell = 2.0 ** -6 if n > 64 else 2.0 ** -4
    bbox_min = np.full(3, -np.floor((n - 1) / 2) * cell)
    ext = (n - 1) * cell
    S = 40
    v = rng.normal(size=(S, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    ax3 = np.array([0.36, 0.31, 0.27]) * ext
    mid = bbox_min + 0.5 * ext + np.array([0.013, -0.021, 0.017]) * ext
    pos = mid + v * ax3
    nrm = v / ax3
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    area = 4 * np.pi * (0.3 * ext) ** 2 / S * (0.5 + rng.random(S))
    lam = 0.3 / cell
    on_node = None
    if variant == "lam10":
        lam *= 10.0
    elif variant == "weights":
        area = area * 10.0 ** (-6.0 * np.linspace(0.0, 1.0, S)[rng.permutation(S)])
    elif variant == "close":
        ijk = np.array([[n // 3, n // 2, n // 4], [2 * n // 3, n // 3 + 1, n // 2 + 2]])
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        extra = bbox_min + ijk * cell
        extra[0] += 1e-3 * cell * d
        u = rng.normal(size=(2, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        pos = np.vstack([pos, extra])
        nrm = np.vstack([nrm, u])
        area = np.concatenate([area, np.full(2, float(area.mean()))])
        on_node = ijk[1]
    elif variant != "base":
        raise ValueError(variant)
    d = dict(pos=pos, wnormal=nrm * area[:, None], area=area, lam=float(lam), n=n, bbox_min=bbox_min, cell=cell)
    return d, on_node


def oracle_field(oracle_c, d):
    n = int(d["n"])
    ref = np.zeros(3 * n ** 3)
    oracle_c.shmo_conv_normalize(n, c_(d["bbox_min"]), float(d["cell"]), len(d["area"]), c_(d["pos"]).reshape(-1), c_(d["wnormal"]).reshape(-1), float(d["lam"]), 0, n, ref)
    return ref.reshape(-1, 3)


def accurate_zone(d):
    """Nodes with lambda r_min < 335, r_min the distance to the nearest source (exact: a handful of sources)."""
    from scipy.spatial import cKDTree
    n = int(d["n"])
    ijk = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 3)[:, ::-1]   # (x fastest)
    r_min, _ = cKDTree(d["pos"]).query(d["bbox_min"] + ijk * d["cell"])
    return d["lam"] * r_min < LAMBDA_R_ZONE


_REF = {}


def _reference(oracle_c, n, variant):
    """(inputs, the on-node source's node, the oracle's Y, the zone): computed once per (n, variant), shared, never written to."""
    key = (n, variant)
    if key not in _REF:
        d, on_node = near_body_sources(n, variant)
        ref = oracle_field(oracle_c, d)
        ref.setflags(write=False)
        _REF[key] = (d, on_node, ref, accurate_zone(d))
    return _REF[key]


def _field(s):
    return np.stack([s.get_field(f) for f in (0, 1, 2)], axis=1)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", ["npt4", "npt2"])
def test_near_body_matches_the_oracle(shm, oracle_c, shape, variant):
    """Every pair through the near body (EXACT_F64): Y within twice the parent's own error against the C oracle, never above the Step-1 budget; the same non-finite nodes."""
    n = _smallest_npt4_side() if shape == "npt4" else N_NPT2
    assert _step1_npt(n, n) == (4 if shape == "npt4" else 2)
    d, on_node, ref, zone = _reference(oracle_c, n, variant)
    S = len(d["area"])
    s = make_solver(shm, d)
    s.run_conv(step1="exact_f64")
    Y = _field(s)
    fin = np.isfinite(ref).all(axis=1)
    bad = np.flatnonzero(np.isfinite(Y).all(axis=1) != fin)
    assert bad.size == 0, "%d nodes finite in one field only (first: %s)" % (bad.size, bad[:5])
    if on_node is not None:
        flat = (on_node[2] * n + on_node[1]) * n + on_node[0]
        assert not fin[flat] and int((~fin).sum()) == 1          # NaN under the source on a node, and nowhere else
    else:
        assert fin.all()
    assert 1.0 - zone.mean() <= 0.05, zone.mean()
    ok = fin & zone
    err = float(np.abs(Y[ok] - ref[ok]).max())
    # the kernel that ran, from the counters of a solve with the same arithmetic: the tiered kernel counts every source of non-zero weight against every
    # 8 x 8 x NPT block, padded (the all-fp64 kernel of rounds 1-4 pads to 8 x 8 x 8 / 16 tiles)
    pairs = None
    if variant == "base":
        npt = 4 if shape == "npt4" else 2
        st = s.solve(step1="exact_f64", max_iters=2, allow_noconv=True)
        pairs = (st.pairs_fp64, st.pairs_fp32)
    s.close()
    parent = PARENT_MAX_DY.get((shape, variant))
    print("\nnear body %s (n=%d) %-7s: max|dY| vs C oracle %.3e (parent %s), excluded %.4f, non-finite %d, pairs %s" % (
        shape, n, variant, err, "%.3e" % parent if parent else "not recorded", 1.0 - zone.mean(), int((~fin).sum()), pairs))
    if pairs is not None:
        blocks = ((n + 7) // 8) ** 2 * ((n + npt - 1) // npt)
        assert pairs == (float(blocks * 64 * npt * S), 0.0), (pairs, blocks * 64 * npt * S)
    assert parent is not None
    assert err <= min(2.0 * parent, STEP1_BUDGET), (err, parent)


def test_tiered_default_classifies_as_the_parent_did(shm, oracle_c):
    """The shipped tiered mode at the NPT = 4 shape: the pairs evaluated in fp64 and in packed fp32 equal the parent commit's counts exactly (the near body's scale is
    no business of the classification), two runs of the same build give bit-identical Y, and Y stays within the budget of the oracle."""
    n = _smallest_npt4_side()
    d, _, ref, zone = _reference(oracle_c, n, "base")
    s = make_solver(shm, d)
    s.run_conv()
    Y1 = _field(s)
    s.run_conv()
    Y2 = _field(s)
    st = s.solve(max_iters=2, allow_noconv=True)
    s.close()
    err = float(np.abs(Y1[zone] - ref[zone]).max())
    print("\ntiered default n=%d: pairs fp64 %.0f packed fp32 %.0f redone %.0f (parent %s), max|dY| vs C oracle %.3e" % (
        n, st.pairs_fp64, st.pairs_fp32, st.pairs_redone, PARENT_PAIRS, err))
    assert np.array_equal(Y1, Y2, equal_nan=True)
    assert err < STEP1_BUDGET, err
    assert st.pairs_fp32 > 0
    assert PARENT_PAIRS is not None
    assert (st.pairs_fp64, st.pairs_fp32) == PARENT_PAIRS, ((st.pairs_fp64, st.pairs_fp32), PARENT_PAIRS)
