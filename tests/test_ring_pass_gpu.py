"""Step 1 of the fp64 solve with a RING PASS behind a failed a-posteriori test (conv_tiered_kernel, csrc/shm_conv_tiered.hip.h; the pass plan is csrc/shm_tier_passes.h):
a block whose packed-fp32 tier fails eps_far L1_far <= budget |X| at some node is walked again from cleared sums with the far threshold G + ring -- in the classification
and in the test's price -- and only when that pass fails too is every source evaluated in fp64.  Every case runs Step 1 alone (shm_grid_run_conv) on a small grid and
holds Y to the C oracle on ALL planes within the Step-1 budget, with the rule of tests/test_far_carry_gpu.py (the oracle's non-finite nodes; at most 5 % of the nodes
outside the accurate zone -- none here), and asserts two runs bit-equal.  G and the ring are pinned by the knobs SHM_CONV_TIER_LOG / SHM_CONV_TIER_RING (read per handle at
set_problem; tests/conftest.py switches the knobs on), so that the cases mean the same whatever setting ships.

Inputs:
  settles      two cancelling sheets SEP_SETTLES of a cell apart at 48^3 (NPT 2).  On the CPU, block by block with the kernel's box rule (ring_pass_blocks): some block's far
               tier carries more than the test's ratio of |X| at a node with the threshold G and less than it at every node with G + ring -- that block is walked again
               and settled by the ring pass.  pairs_redone > 0, and smaller than with the ring at 0;
  fails too    the sheets a tenth of a cell apart (the second-pass input of test_far_carry_gpu.py): every block that runs again fails on what it dropped and goes straight
               to the all-fp64 pass;
  three passes the sphere with a wider double shell and a ring of 0.5: the far tier fails at G and at G + ring, the block makes all three passes -- pairs_redone ABOVE the
               ring-off run's;
  carry/flush  the 3000-source sphere of test_flushes_with_a_carry_pending with a cancelling double shell inside it: the blocks between the shells run again, and their
               ring passes stage the sphere's far sources -- >= 256 per re-run block on average, from the counters: a flush inside the ring pass, carries before it;
  shapes       NPT 4 at the smallest side that picks it, a side of 37 (cut blocks), NPT 2 at 32 -- each with a double shell inside, so that blocks run again and are settled;
  untouched    EXACT_F64 (no packed-fp32 pair, nothing evaluated again) and an fp32 handle (one pass)."""
import numpy as np
import pytest

from test_far_carry_gpu import cancelling_sheets, ellipsoid_sources
from test_gpu_parity import Y_BUDGET, Y_BUDGET_F32, make_solver
from test_near_body_gpu import _smallest_npt4_side, accurate_zone, oracle_field
from test_step1_edges import _step1_npt

pytestmark = pytest.mark.gpu

G = 8.0                 # far threshold of the cases (nats): SHM_CONV_TIER_LOG
RING = 2.0              # ring width of the cases: SHM_CONV_TIER_RING
RING_NARROW = 0.5       # ... of the three-pass case: narrow enough that the far tier still fails behind the ring pass
TIER_FLUSH = 256        # kTierFlush
EPS_FAR, U0, BUDGET, DROP_EPS = 1.0e-6, 24.0, 1.0e-8, 2.0e-9   # kTierEpsFar, kTierU0, kTierBudget, the fp64 solve's drop budget
SEP_SETTLES = 0.12      # separation (cells) of the sheets of the "settles" case: picked with ring_pass_blocks below (see the test's docstring for the figures)
LOG2E = 1.4426950408889634


def ring_pass_blocks(d, npt, g, ring, planes=None):
    """The a-posteriori test's far term, block by block (8 x 8 x npt nodes) with the kernel's box rule -- the rule of every grid with fewer than 64 layers of blocks --:
        far(s)  <=>  lambda (dist(s, box) - r_hi) > g + ln(|w_s| / |w_*|)  and  dist(s, box) >= r_hi
    (s* the source nearest the block's centre, r_hi the block's farthest corner from it), L1_far(x) = sum_far |w_s|_1 e^{-lambda r} / r against
    ratio(u) |X(x)|, ratio(u) = budget / (eps_far max(1, u / 24)), u = (lambda d0 + g) log2 e, d0 = max(0, |c - s*| - block radius).  Sources further than 60 e-folds from
    the block are left out (the drop rule and the fp32 exponent range take them out of the tier; their terms are below e^-60).  Returns, per block, the largest
    L1_far / (ratio |X|) over its nodes at the threshold g and at g + ring: above 1 the block's test fails on the far tier alone.  `planes`: only these planes of nodes are
    evaluated (blocks elsewhere report 0) -- a few planes through the region of interest keep the large inputs to a few seconds."""
    n, cell, lam = int(d["n"]), float(d["cell"]), float(d["lam"])
    pos, w = d["pos"], d["wnormal"]
    w2, w1 = np.linalg.norm(w, axis=1), np.abs(w).sum(axis=1)
    h = np.array([3.5, 3.5, 0.5 * (npt - 1)]) * cell
    rt = float(np.linalg.norm(h))
    nb, nbz = (n + 7) // 8, (n + npt - 1) // npt
    bi, bj, bk = np.meshgrid(np.arange(nb), np.arange(nb), np.arange(nbz), indexing="ij")
    org = np.stack([bi * 8, bj * 8, bk * npt], -1).reshape(-1, 3)
    cen = d["bbox_min"] + org * cell + h
    B = len(cen)
    far0, far1 = np.zeros((B, len(w2)), bool), np.zeros((B, len(w2)), bool)
    ratio0, ratio1 = np.zeros(B), np.zeros(B)
    for b in range(B):
        dc = np.linalg.norm(pos - cen[b], axis=1)
        star = int(np.argmin(dc))
        r_hi = float(np.linalg.norm(np.abs(cen[b] - pos[star]) + h))
        dist = np.linalg.norm(np.maximum(np.abs(pos - cen[b]) - h, 0.0), axis=1)
        marg = lam * (dist - r_hi) - np.log(w2 / w2[star])
        ok = (dist >= r_hi) & (lam * dist < 60.0)
        far0[b], far1[b] = ok & (marg > g), ok & (marg > g + ring)
        coff = lam * LOG2E * max(0.0, dc[star] - rt)
        ratio0[b] = BUDGET / EPS_FAR * min(1.0, U0 / (coff + g * LOG2E))
        ratio1[b] = BUDGET / EPS_FAR * min(1.0, U0 / (coff + (g + ring) * LOG2E))
    share0, share1 = np.zeros(B), np.zeros(B)
    p2 = (pos * pos).sum(axis=1)
    for k in (range(n) if planes is None else planes):   # a plane of nodes at a time: r^2 by one matrix product
        i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
        x = d["bbox_min"] + np.stack([i.ravel(), j.ravel(), np.full(n * n, k)], -1) * cell
        r = np.sqrt(np.maximum((x * x).sum(axis=1)[:, None] + p2[None, :] - 2.0 * (x @ pos.T), 1e-300))
        gk = np.exp(-lam * r) / r
        X = np.linalg.norm(gk @ w, axis=1)
        blk = ((i.ravel() // 8) * nb + (j.ravel() // 8)) * nbz + k // npt
        gw = gk * w1[None, :]
        np.maximum.at(share0, blk, (gw * far0[blk]).sum(axis=1) / (ratio0[blk] * X))
        np.maximum.at(share1, blk, (gw * far1[blk]).sum(axis=1) / (ratio1[blk] * X))
    return share0, share1


def double_shell(n, S_outer, S_inner=600, sep_cells=0.1, seed=20261, r_inner=0.16, lam_cell=1.0, radii=(0.425, 0.425, 0.425)):
    """The ellipsoid / sphere of test_far_carry_gpu.py with a cancelling double shell inside it: S_inner sources on a small sphere and the same sources `sep_cells` further
    out with the opposite normals -- between and around the two shells |X| is a fraction lambda * sep of the sum of |terms|, so the blocks there fail the a-posteriori
    test, and what their packed-fp32 tier holds is the OUTER surface."""
    d = ellipsoid_sources(n, S_outer, lam_cell=lam_cell, radii=radii)
    rng = np.random.default_rng(seed)
    ext = (n - 1) * d["cell"]
    mid = d["bbox_min"] + 0.5 * ext + np.array([0.013, -0.021, 0.017]) * ext
    v = rng.normal(size=(S_inner, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    r0 = r_inner * ext
    area = 4 * np.pi * r0 ** 2 / S_inner * (0.5 + rng.random(S_inner))
    pos = np.vstack([d["pos"], mid + v * r0, mid + v * (r0 + sep_cells * d["cell"])])
    wn = np.vstack([d["wnormal"], v * area[:, None], -v * area[:, None]])
    return dict(pos=pos, wnormal=wn, area=np.concatenate([d["area"], area, area]), lam=d["lam"], n=n, bbox_min=d["bbox_min"], cell=d["cell"])


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


def _run(shm, monkeypatch, d, ref, zone, label, ring=RING, precision=64, expect_npt=None, g=G, step1=None):
    """Two runs of Step 1 on a fresh handle with the knobs set: the same bits, the oracle's non-finite nodes, max|dY| inside the bound; returns the counters of a solve with
    the same arithmetic."""
    n = int(d["n"])
    if expect_npt is not None:
        assert _step1_npt(n, n) == expect_npt, (n, expect_npt)
    monkeypatch.setenv("SHM_CONV_TIER_LOG", repr(g))
    monkeypatch.setenv("SHM_CONV_TIER_RING", repr(ring))
    kw = {} if step1 is None else {"step1": step1}
    s = make_solver(shm, d, precision=precision)
    s.run_conv(**kw)
    Y1 = _field(s)
    s.run_conv(**kw)
    Y2 = _field(s)
    st = s.solve(max_iters=2, allow_noconv=True, **kw)
    s.close()
    fin = np.isfinite(ref).all(axis=1)
    bad = np.flatnonzero(np.isfinite(Y1).all(axis=1) != fin)
    assert 1.0 - zone.mean() <= 0.05, zone.mean()
    ok = fin & zone
    err = float(np.abs(Y1[ok] - ref[ok]).max())
    bound = Y_BUDGET if precision == 64 else Y_BUDGET_F32
    nom = float(n) ** 3 * len(d["area"])
    print("\nring pass %-30s n=%d S=%d fp%d G=%g ring=%g: max|dY| vs C oracle %.3e (bound %.0e, margin %.1fx); pairs fp64 %.0f packed fp32 %.0f redone %.0f (of nominal: %.3f %.3f %.4f)" % (
        label, n, len(d["area"]), precision, g, ring, err, bound, bound / max(err, 1e-300), st.pairs_fp64, st.pairs_fp32, st.pairs_redone,
        st.pairs_fp64 / nom, st.pairs_fp32 / nom, st.pairs_redone / nom))
    assert np.array_equal(Y1, Y2, equal_nan=True)
    assert bad.size == 0, "%d nodes finite in one field only (first: %s)" % (bad.size, bad[:5])
    assert err < bound, (label, err)
    return st


def test_ring_pass_settles_a_block(shm, oracle_c, monkeypatch):
    """Sheets SEP_SETTLES of a cell apart at 48^3.  CPU (ring_pass_blocks): at some node of some block the far tier's L1 sum exceeds the test's ratio of |X| with the
    threshold G and falls under it with G + ring -- one block of the 864 at 0.12 cell: 2.41 times the ratio at G = 8, 0.44 times at G + 2 (none at 0.14 cell and beyond, where
    the largest share is 0.55; the share grows as 1 / separation).  With the ring that block evaluates its near list of G + ring again, not every source: pairs_redone > 0
    and below the ring-off run's.  Measured on an MI355X: four blocks run again, pairs_redone 861 184 with the ring off and 731 904 with it -- three of the four fail on
    what they DROPPED (the sheets' far edge), which no ring can settle, and go straight to the all-fp64 pass; max|dY| 1.44e-9 either way."""
    d, ref, zone = _reference(oracle_c, ("sheets", 48, SEP_SETTLES), lambda: cancelling_sheets(48, sep_cells=SEP_SETTLES))
    assert 0.1 < SEP_SETTLES < 0.5
    share_g, share_ring = ring_pass_blocks(d, 2, G, RING)
    settled = (share_g > 1.01) & (share_ring < 0.99)
    print("\nsheets %.2f cell apart: the far tier's L1 / (ratio |X|) exceeds 1 in %d of %d blocks at G = %g (largest %.3g), %d of them fall under 1 at G + %g (that block: %.3g)" % (
        SEP_SETTLES, (share_g > 1.01).sum(), share_g.size, G, share_g.max(), settled.sum(), RING, share_ring[np.argmax(share_g)]))
    assert settled.any()
    on = _run(shm, monkeypatch, d, ref, zone, "settles (sheets %.2f)" % SEP_SETTLES, expect_npt=2)
    off = _run(shm, monkeypatch, d, ref, zone, "settles, ring off", ring=0.0)
    assert on.pairs_redone > 0, on.pairs_redone
    assert on.pairs_redone < off.pairs_redone, (on.pairs_redone, off.pairs_redone)


def test_ring_pass_fails_too(shm, oracle_c, monkeypatch):
    """Sheets a tenth of a cell apart: Y within the budget, and every block that fails ends all-fp64 -- nothing of the ring-off run's second passes is lost.  (Measured on an
    MI355X: three blocks run again, all three on what they dropped: pairs_redone 645 888 with the ring and without, max|dY| 3.70e-9.)"""
    d, ref, zone = _reference(oracle_c, ("sheets", 48, 0.1), lambda: cancelling_sheets(48))
    on = _run(shm, monkeypatch, d, ref, zone, "fails too (sheets 0.1)", expect_npt=2)
    off = _run(shm, monkeypatch, d, ref, zone, "fails too, ring off", ring=0.0)
    assert off.pairs_redone > 0, off.pairs_redone
    assert on.pairs_redone >= off.pairs_redone, (on.pairs_redone, off.pairs_redone)


def test_three_passes(shm, oracle_c, monkeypatch):
    """The ring pass runs, fails, and the block ends all-fp64: the 3000-source sphere with a double shell 0.25 of the grid's extent across inside it, the ring pinned at
    RING_NARROW = 0.5 nats.  CPU (ring_pass_blocks on four planes through the shell's equator): a block whose far tier carries 1.9 times the ratio at G = 8 and still 1.18
    times at G + 0.5 -- its test fails on the far tier in both tiered passes.  So pairs_redone EXCEEDS the ring-off run's: the ring pass's near pairs on top of every
    all-fp64 pair (18 blocks run again on an MI355X: 9.68e6 pairs with the ring off, 9.87e6 with it; the same input with a ring of 2: 7.44e6).  The sums, the L1 sums, the
    far list's carry and the pending count are cleared twice on that path; Y within the budget, two runs bit-equal."""
    d, ref, zone = _reference(oracle_c, ("shell", 48, 3000, 0.25), lambda: double_shell(48, 3000, r_inner=0.25))
    share_g, share_ring = ring_pass_blocks(d, 2, G, RING_NARROW, planes=range(22, 26))
    both = (share_g > 1.01) & (share_ring > 1.01)
    print("\nshell 0.25: %d block(s) of the four planes above the ratio at G = %g and at G + %g (largest %.3g -> %.3g)" % (both.sum(), G, RING_NARROW, share_g.max(), share_ring[np.argmax(share_g)]))
    assert both.any()
    on = _run(shm, monkeypatch, d, ref, zone, "three passes (ring %.1f)" % RING_NARROW, ring=RING_NARROW, expect_npt=2)
    off = _run(shm, monkeypatch, d, ref, zone, "three passes, ring off", ring=0.0)
    assert off.pairs_redone > 0, off.pairs_redone
    assert on.pairs_redone > off.pairs_redone, (on.pairs_redone, off.pairs_redone)
    assert on.pairs_fp32 > off.pairs_fp32, (on.pairs_fp32, off.pairs_fp32)


def _rerun_blocks_and_far(on, off, npt, S):
    """From the counters of a ring-on and a ring-off run of one input: the blocks that ran again -- ring off, each of them evaluates every one of the S sources once more
    (nothing lies beyond the exponent span on these grids), so pairs_redone / (64 npt S) is their number -- and the far sources the ring passes staged (what pairs_fp32
    gained: pass 0 is the same in both runs)."""
    per = 64.0 * npt
    return off.pairs_redone / (per * S), (on.pairs_fp32 - off.pairs_fp32) / per


def test_carry_and_flush_inside_the_ring_pass(shm, oracle_c, monkeypatch):
    """The 3000-source sphere 40 cells across in a 48^3 grid (test_flushes_with_a_carry_pending) with a cancelling double shell (2 x 600 sources, a tenth of a cell apart)
    15 cells across inside it.  Blocks at the shells fail pass 0 on their far tier; their ring passes stage the sphere's far sources, cluster by cluster with uneven far
    counts: at least 256 per re-run block on average, so a flush of the packed-fp32 sums (every 256) behind a drain inside the ring pass, and carries of every remainder
    before it.  (Two blocks ran again on an MI355X, as ring_pass_blocks finds on the CPU, and both were settled by the ring pass.)"""
    d, ref, zone = _reference(oracle_c, ("shell", 48, 3000), lambda: double_shell(48, 3000))
    on = _run(shm, monkeypatch, d, ref, zone, "carry + flush in the ring pass", expect_npt=2)
    off = _run(shm, monkeypatch, d, ref, zone, "carry + flush, ring off", ring=0.0)
    assert off.pairs_redone > 0 and on.pairs_redone > 0, (off.pairs_redone, on.pairs_redone)
    blocks, far_ring = _rerun_blocks_and_far(on, off, 2, len(d["area"]))
    mean_far = far_ring / blocks
    print("carry + flush: %.1f blocks ran again, their ring passes staged %.0f far sources: %.0f per block on average (a flush every %d)" % (blocks, far_ring, mean_far, TIER_FLUSH))
    assert mean_far >= TIER_FLUSH, mean_far


@pytest.mark.parametrize("shape", ["npt4", "cut37", "npt2_32"])
def test_block_shapes(shm, oracle_c, monkeypatch, shape):
    """Blocks that run again and are settled by the ring pass in every shape: pairs_redone > 0 and below the ring-off run's.
      npt4     the smallest side that picks NPT 4 (four squared z offsets per far list entry), lambda * cell = 0.5, 64 k + 5 sources on the ellipsoid around a double shell of
               2 x 150: 70 blocks run again, pairs_redone 4.45e6 -> 3.58e6 (MI355X);
      cut37    a side of 37 (partial blocks in x, y and z: the test's and the short cut's live_xy / kk_end gating, a drain on cut blocks), 64 k + 2 sources on the sphere
               around a double shell 0.22 of the extent across, a twentieth of a cell apart: 10 blocks, 4.15e6 -> 2.21e6;
      npt2_32  NPT 2 at 32, 64 k + 3 sources, the same shell: 10 blocks, 4.16e6 -> 3.42e6."""
    if shape == "npt4":
        n, S = _smallest_npt4_side(), 64 * 3 + 5
        make = lambda: double_shell(n, S, S_inner=150, lam_cell=0.5, radii=(0.36, 0.31, 0.27))
    else:
        n, S = (37, 64 * 46 + 2) if shape == "cut37" else (32, 64 * 46 + 3)
        make = lambda: double_shell(n, S, S_inner=150, r_inner=0.22, sep_cells=0.05)
    d, ref, zone = _reference(oracle_c, ("shell", n, S), make)
    on = _run(shm, monkeypatch, d, ref, zone, "shape " + shape, expect_npt=4 if shape == "npt4" else 2)
    off = _run(shm, monkeypatch, d, ref, zone, "shape " + shape + ", ring off", ring=0.0)
    assert on.pairs_fp32 > off.pairs_fp32 > 0, (on.pairs_fp32, off.pairs_fp32)
    assert 0 < on.pairs_redone < off.pairs_redone, (on.pairs_redone, off.pairs_redone)


def test_exact_f64_is_untouched(shm, oracle_c, monkeypatch):
    """An exact_f64 solve: no packed-fp32 pair, nothing evaluated again, whatever the ring."""
    d, ref, zone = _reference(oracle_c, ("sheets", 48, 0.1), lambda: cancelling_sheets(48))
    st = _run(shm, monkeypatch, d, ref, zone, "exact_f64", step1="exact_f64")
    assert st.pairs_fp32 == 0 and st.pairs_redone == 0, (st.pairs_fp32, st.pairs_redone)


def test_fp32_handle_is_untouched(shm, oracle_c, monkeypatch):
    """An fp32 handle makes one pass: nothing evaluated again, Y within the fp32 bound."""
    S = 64 * 3 + 3
    d, ref, zone = _reference(oracle_c, ("ellipsoid", 32, S), lambda: ellipsoid_sources(32, S))
    st = _run(shm, monkeypatch, d, ref, zone, "fp32 handle", precision=32)
    assert st.pairs_redone == 0 and st.pairs_fp32 > st.pairs_fp64, (st.pairs_redone, st.pairs_fp32, st.pairs_fp64)
