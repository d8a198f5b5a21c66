"""Step 1 (conv_tiered_kernel, csrc/shm_conv_tiered.hip.h) at the edges the other parity tests do not reach, against the C oracle (the reference's serial
loops), never against the library's own all-fp64 mode -- that mode shares the kernel's classification front end (fp32 copies of the weights, the `valid` mask):
  A. blocks cut off by the grid's sides and by slab boundaries (grid sides that are not multiples of the 8 x 8 x NPT block, 1 / 3 / 5 slabs, the weighted slab plan);
  B. sources of tiny weight pinned 1e-10 ... 1e-9 cells from a node, the inputs on which the hard fallback of the drop rule used to drop a term 100 x the budget;
  C. sources exactly on nodes, cell faces and edges, and one ulp inside the top faces (powers of two make the node coordinates exact).
One rule throughout: the non-finite nodes are the oracle's, and where the oracle is finite and lambda r < 335 (the zone where the reference's own
normalisation is accurate: test_gpu_parity.py::test_tier_budget_on_adversarial_inputs) max|dY| stays under Y_BUDGET (fp64 default), 1e-10 (exact_f64) or
Y_BUDGET_F32 (fp32 handle; A only: the fp32 solve evaluates every kept pair in packed fp32 by design, where a source 1e-10 cells from a node or on it has
the node's own fp32 coordinates -- its non-finite nodes there are not the reference's, and B and C hold the fp64 handle).  Every test prints its worst error and
its margin."""
import os

import numpy as np
import pytest

from conftest import ROOT, c_, load_golden
from test_gpu_parity import Y_BUDGET, Y_BUDGET_F32, make_solver

pytestmark = pytest.mark.gpu

EXACT_BOUND = 1e-10
LAMBDA_R_ZONE = 335.0
BOUND = {"fp64": Y_BUDGET, "exact_f64": EXACT_BOUND, "fp32": Y_BUDGET_F32}
ORACLE_THREADS = min(16, os.cpu_count() or 1)


def _oracle_planes(oracle_c, d, ks):
    """The oracle's Y on z-planes ks (dict k -> (n * n, 3)), on at most 16 threads."""
    n = int(d["n"])
    out = {}
    oracle_c.shmo_set_threads(ORACLE_THREADS)
    try:
        for k in ks:
            Yp = np.zeros(3 * n * n)
            oracle_c.shmo_conv_normalize_planes(n, c_(d["bbox_min"]), float(d["cell"]), len(d["area"]), c_(d["pos"]).reshape(-1),
                                                c_(d["wnormal"]).reshape(-1), float(d["lam"]), int(k), int(k) + 1, Yp)
            out[k] = Yp.reshape(-1, 3)
    finally:
        oracle_c.shmo_set_threads(min(8, os.cpu_count() or 1))
    return out


def _zone(d, k):
    """Nodes of plane k nearer than lambda r = 335 to the sources (r bounded below by the distance to the sources' bounding box)."""
    n, cell = int(d["n"]), float(d["cell"])
    j, i = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")     # (x fastest, like the field)
    xyz = np.stack([i.ravel(), j.ravel(), np.full(n * n, k)], -1) * cell + np.asarray(d["bbox_min"])
    lo, hi = d["pos"].min(axis=0), d["pos"].max(axis=0)
    r_lb = np.linalg.norm(np.maximum(0.0, np.maximum(lo - xyz, xyz - hi)), axis=1)
    return float(d["lam"]) * r_lb < LAMBDA_R_ZONE


def _compare(Y, ref, zone, what):
    """The rule of this file on one plane: equal non-finite sets, then the largest |dY| on the finite nodes inside the zone."""
    fin = np.isfinite(ref).all(axis=1)
    bad = np.flatnonzero(np.isfinite(Y).all(axis=1) != fin)
    assert bad.size == 0, "%s: %d nodes finite in one field only (first: %s)" % (what, bad.size, bad[:5])
    ok = fin & zone
    return float(np.abs(Y[ok] - ref[ok]).max()) if ok.any() else 0.0


def _step1_npt(n, planes):
    """Nodes per lane of the fp64 tiered kernel on a slab of `planes` planes (launch_conv, shm_solver.hip.h: 4 when the grid still yields a full wave of
    workgroups -- conv_grid_cap = 4 workgroups per CU -- else 2)."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = (n + 7) // 8
    return 4 if tiles * tiles * ((planes + 15) // 16) >= 4 * cus else 2


def _slab_bounds(shm, d, slabs, weighted, precision):
    n = int(d["n"])
    if slabs == 1:
        return [(0, n)]
    if not weighted:
        return [shm.plan_slab(n, slabs, r) for r in range(slabs)]
    w = shm.step1_plane_weights(d["pos"], d["wnormal"], d["lam"], n, d["bbox_min"], d["cell"], precision)
    return [shm.plan_slab_weighted(n, slabs, r, w, 4 if precision == 64 else 8) for r in range(slabs)]


def _edge_planes(n, bounds, npt):
    """0, n - 1, the centre plane (every plane of a grid whose side is not a multiple of 8 runs through partial x / y block columns), and per slab the planes
    k0 - 1, k0, k0 + 1, k1 - 1 and those of its last (partial) z-block."""
    ks = {0, n - 1, n // 2}
    for k0, k1 in bounds:
        ks |= {k0 - 1, k0, k0 + 1, k1 - 1}
        ks |= set(range(k0 + ((k1 - k0 - 1) // npt) * npt, k1))
    return sorted(k for k in ks if 0 <= k < n)


def _run_layout(shm, oracle_c, d, slabs, weighted, label):
    """Step 1 of an fp64 handle (default and exact_f64) and an fp32 handle on one slab layout; every slab read on its owned range by get_field_planes."""
    n = int(d["n"])
    worst = {}
    ref_cache = {}
    for precision, ariths in ((64, ("fp64", "exact_f64")), (32, ("fp32",))):
        bounds = _slab_bounds(shm, d, slabs, weighted, precision)
        npts = sorted({_step1_npt(n, k1 - k0) for k0, k1 in bounds})
        ks = _edge_planes(n, bounds, max(npts))
        need = [k for k in ks if k not in ref_cache]
        ref_cache.update(_oracle_planes(oracle_c, d, need))
        s = make_solver(shm, d, precision=precision, local_slabs=slabs, slab_plan=1 if weighted else 0)
        for arith in ariths:
            s.run_conv(step1="exact_f64" if arith == "exact_f64" else "auto")
            e = 0.0
            for k0, k1 in bounds:
                Ys = np.stack([s.get_field_planes(f, k0, k1) for f in (0, 1, 2)], axis=1).reshape(k1 - k0, n * n, 3)
                for k in ks:
                    if k0 <= k < k1:
                        e = max(e, _compare(Ys[k - k0], ref_cache[k], _zone(d, k), "%s %s plane %d" % (label, arith, k)))
            worst[arith] = e
        s.close()
    print("\nStep 1 edges %s: npt %s, planes %s; max|dY| vs C oracle %s" % (
        label, npts, ks, ", ".join("%s %.2e (margin %.0fx)" % (a, e, BOUND[a] / max(e, 1e-300)) for a, e in worst.items())))
    for a, e in worst.items():
        assert e < BOUND[a], (label, a, e)
    return npts


# ---- A. Partial blocks and slab edges ----------------------------------------------------------------------------------------------------------------------
LAYOUTS = {"1": (1, False), "3": (3, False), "5": (5, False), "w3": (3, True)}


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("n", [11, 33, 45, 90])
def test_step1_partial_blocks_and_slab_edges(shm, oracle_c, n, layout):
    """The 16^3 bunny fixture with the cell rescaled to n - 1 intervals (as test_matches_c_oracle_odd_sizes): none of these sides is a multiple of the 8 x 8 block,
    so every plane holds partial x / y blocks; the slabs start z-blocks at planes that are not multiples of NPT.  All of these sizes run with NPT = 2 (asserted
    for 45: a side of NPT 4 is the real input below)."""
    g = load_golden("bunny_small_n16")
    d = dict(pos=g["pos"], wnormal=g["wnormal"], area=g["area"], lam=float(g["lam"]), n=n, bbox_min=g["bbox_min"], cell=float(g["cell"]) * 15 / (n - 1))
    slabs, weighted = LAYOUTS[layout]
    npts = _run_layout(shm, oracle_c, d, slabs, weighted, "bunny_small_n16 at n=%d, slabs %s" % (n, layout))
    if n == 45 and slabs == 1:
        assert npts == [2]


@pytest.mark.parametrize("layout", ["1", "w3"])
def test_step1_real_input_at_a_non_power_of_two_side(shm, oracle_c, layout):
    """bunny_small.obj at hCoef 3.5 through HostSolver.preprocess: n = 181 (= 22 x 8 + 5 and = 45 x 4 + 1: partial blocks on every side), NPT 4 on one slab."""
    from signed_heat_3d_amd.host_abi import HostSolver
    pre = HostSolver(os.path.join(ROOT, "data", "bunny_small.obj")).preprocess(hCoef=3.5)
    assert pre["n"] == 181
    d = dict(pos=pre["pos"], wnormal=pre["wnormal"], area=pre["area"], lam=pre["lam"], n=pre["n"], bbox_min=pre["bbox_min"], cell=pre["cell"])
    slabs, weighted = LAYOUTS[layout]
    npts = _run_layout(shm, oracle_c, d, slabs, weighted, "bunny_small.obj hCoef 3.5 (n=181), slabs %s" % layout)
    if slabs == 1:
        assert npts == [4]


# ---- B. Tiny sources pinned next to nodes ------------------------------------------------------------------------------------------------------------------
def _x_at(d, x):
    """X(x) = sum_s w_s e^{-lambda r} / r in fp64 (the reference's sum) at the points x (m, 3)."""
    r = np.linalg.norm(x[:, None, :] - d["pos"][None, :, :], axis=2)
    g = np.exp(-d["lam"] * r) / r
    return g @ d["wnormal"]


def _pinned_sources(variant, seed):
    """A closed surface (3000 sources on an ellipsoid, areas over one decade, lambda * cell = 0.45) on a 128^3 grid with bbox_min and cell powers of two, plus
    pinned sources of weight two powers of two under the hard threshold of their block (at most 1e-15 |w_max|), delta * cell (delta in {1e-10, 1e-9}) from a
    corner node of an 8 x 8 x NPT block the surface passes near (so an ordinary source nearer to the block's centre than the corner stays its reference source s*):
      inside:  32 sources, each inside its block (distance 0 from the block's box);
      outside: 32 sources, each just outside its block (0 < distance < r_hi);
      packed:  64 sources at one corner node inside one block (consecutive in Morton order: one or two clusters of their own -- whole-cluster tests in the blocks
               beyond r_hi, which need gap > 0 and are sound; in their own block the source-level scan sees them, like `inside`).
    Their normals are perpendicular to X at their node, where each one's term is far above 100 x Y_BUDGET of |X| (asserted by the test).
    Returns (set_problem arguments, pinned source indices, their nodes (m, 3) as indices, NPT)."""
    rng = np.random.default_rng(seed)
    n, cell = 128, 2.0 ** -6
    bbox_min = np.array([-1.0, -1.0, -1.0])
    S0 = 3000
    v = rng.normal(size=(S0, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    ax3 = np.array([0.6, 0.5, 0.4])
    pos = v * ax3 + np.array([-0.02, 0.01, -0.03])
    nrm = v / ax3
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    area = 4 * np.pi * 0.5 ** 2 / S0 * 10.0 ** (-rng.random(S0))
    base = dict(pos=pos, wnormal=nrm * area[:, None], area=area, lam=0.45 / cell, n=n, bbox_min=bbox_min, cell=cell)
    npt = _step1_npt(n, n)
    # blocks whose centre lies within 3 cells of a source, away from the grid's faces
    bx = np.arange(1, n // 8 - 1)
    bz = np.arange(1, n // npt - 1)
    B = np.stack(np.meshgrid(bx, bx, bz, indexing="ij"), -1).reshape(-1, 3)
    centre = bbox_min + (B * np.array([8, 8, npt]) + np.array([3.5, 3.5, 0.5 * (npt - 1)])) * cell
    from scipy.spatial import cKDTree
    dmin, _ = cKDTree(pos).query(centre)
    B = B[dmin < 3.0 * cell]
    # below the grid's centre on every axis: there a source's offset of 1e-10 cells from its node survives the library's shift to grid-centred coordinates
    # (Solver::set_problem) exactly -- above it the shift can round the offset by an ulp of the coordinate, ~1e-5 of it, which the reference does not do
    B = B[(B * np.array([8, 8, npt]) + np.array([7, 7, npt - 1]) < (n - 1) / 2).all(axis=1)]
    count = 1 if variant == "packed" else 32
    blocks = B[rng.choice(len(B), size=count, replace=False)]
    m = 64 if variant == "packed" else 32
    # the corner with the smallest |X|: the one farthest from the surface
    corners = np.array([[a, b, c] for a in (0, 1) for b in (0, 1) for c in (0, 1)])
    cand = blocks[:, None, :] * np.array([8, 8, npt]) + corners[None, :, :] * np.array([7, 7, npt - 1])
    xabs = np.linalg.norm(_x_at(base, bbox_min + cand.reshape(-1, 3) * cell), axis=1).reshape(count, 8)
    corner = corners[np.argmin(xabs, axis=1)]
    node = np.repeat(blocks * np.array([8, 8, npt]) + corner * np.array([7, 7, npt - 1]), m // count, axis=0)
    inward = np.repeat(1.0 - 2.0 * corner, m // count, axis=0)                           # towards the block's inside along each axis
    dirs = inward * (0.5 + rng.random((m, 3)))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    xn = bbox_min + node * cell
    # normals perpendicular to X at the node: what the term adds to X turns Y by its whole size
    X = _x_at(base, xn)
    t = np.cross(X, rng.normal(size=(m, 3)))
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    # weights two powers of two below the hard threshold of their block (lb = log2 tau_hard - 2), at most 1e-15 |w_max|
    wstar, r_hi = _block_star(base, node, npt)
    ltau_hard = np.log2(0.125 * 2e-9 / (S0 + m))
    wmax = np.linalg.norm(base["wnormal"], axis=1).max()
    w = np.minimum(1e-15 * wmax, wstar * 2.0 ** (ltau_hard - 2.0 - base["lam"] * np.log2(np.e) * r_hi))
    # 1e-9 cells from the node where that makes the term > 1e-5 |X| there, else 1e-10
    delta = np.where(w / (1e-9 * cell) > 1e-5 * np.linalg.norm(X, axis=1), 1e-9, 1e-10)
    p = xn + (delta * cell)[:, None] * (dirs if variant != "outside" else -dirs)
    d = dict(base)
    d["pos"] = np.vstack([pos, p])
    d["wnormal"] = np.vstack([base["wnormal"], t * w[:, None]])
    d["area"] = np.concatenate([area, w])
    return d, np.arange(S0, S0 + m), node, npt


def _block_star(d, node, npt):
    """|w_s*| and r_hi of the blocks of the nodes: s* the source nearest to the block's centre, r_hi the distance from it to the block's farthest corner."""
    cell = float(d["cell"])
    half = np.array([3.5, 3.5, 0.5 * (npt - 1)]) * cell
    centre = d["bbox_min"] + ((node // np.array([8, 8, npt])) * np.array([8, 8, npt]) + half / cell) * cell
    r = np.linalg.norm(d["pos"][None, :, :] - centre[:, None, :], axis=2)
    star = np.argmin(r, axis=1)
    return np.linalg.norm(d["wnormal"][star], axis=1), np.linalg.norm(np.abs(d["pos"][star] - centre) + half, axis=1)


def _hard_drop_regime(d, pinned, node, npt):
    """What the kernel's hard fallback reads for every pinned source, recomputed on the host (shm_conv_tiered.hip.h, in fp64): the block's reference source s*
    (nearest to its centre), r_hi (the block's farthest corner from s*), lb = log2(|w_s| / |w_s*|) + lambda log2(e) (r_hi - d_s) with d_s the source's distance
    from the block's box, against log2(tau_hard), tau_hard = (conv_drop_eps64 / 8) / S (Solver::launch_conv); and the pinned term at its node against |X|."""
    cell, lam, S = float(d["cell"]), float(d["lam"]), len(d["area"])
    half = np.array([3.5, 3.5, 0.5 * (npt - 1)]) * cell
    centre = d["bbox_min"] + ((node // np.array([8, 8, npt])) * np.array([8, 8, npt]) + half / cell) * cell
    wstar, r_hi = _block_star(d, node, npt)
    wabs = np.linalg.norm(d["wnormal"], axis=1)
    dist = np.linalg.norm(np.maximum(0.0, np.abs(d["pos"][pinned] - centre) - half), axis=1)
    lb = np.log2(wabs[pinned] / wstar) + lam * np.log2(np.e) * (r_hi - dist)
    ltau_hard = np.log2(0.125 * 2e-9 / S)
    xn = d["bbox_min"] + node * cell
    rs = np.linalg.norm(xn - d["pos"][pinned], axis=1)
    term = wabs[pinned] * np.exp(-lam * rs) / rs
    xabs = np.linalg.norm(_x_at(d, xn), axis=1)
    return lb, ltau_hard, dist, r_hi, term / xabs


@pytest.mark.parametrize("variant", ["inside", "outside", "packed"])
def test_step1_tiny_sources_pinned_next_to_nodes(shm, oracle_c, variant):
    """The hard fallback of the drop rule (a source with lb <= log2 tau_hard dropped whatever the running sum; lb leaves out the factor r_hi / d_s of its bound) must not
    drop a source nearer to the block than r_hi: such a source's term at its node here is 4e-6 ... 1e-4 of |X|, and before the fix it was dropped with tau_hard booked
    for it -- the a-posteriori test never saw it.  The inputs are checked to be in that regime on the host first, with the kernel's own thresholds."""
    worst = {}
    for seed in (1, 2):
        d, pinned, node, npt = _pinned_sources(variant, seed)
        lb, ltau_hard, dist, r_hi, rel_term = _hard_drop_regime(d, pinned, node, npt)
        assert (lb <= ltau_hard - 0.5).all(), (lb.max(), ltau_hard)                     # every pinned source is a hard-drop candidate of its block
        assert (rel_term > 100 * Y_BUDGET).all(), rel_term.min()                       # ... whose term at its node is far over the budget
        assert ((dist == 0) if variant != "outside" else ((dist > 0) & (dist < r_hi))).all(), (dist.min(), dist.max())
        ks = sorted(set(int(k) for k in node[:, 2]))
        ref = _oracle_planes(oracle_c, d, ks)
        n = int(d["n"])
        s = make_solver(shm, d)
        for arith in ("fp64", "exact_f64"):
            s.run_conv(step1="exact_f64" if arith == "exact_f64" else "auto")
            e, e_pin = 0.0, 0.0
            for k in ks:
                Y = np.stack([s.get_field_planes(f, k, k + 1) for f in (0, 1, 2)], axis=1)
                e = max(e, _compare(Y, ref[k], _zone(d, k), "%s seed %d %s plane %d" % (variant, seed, arith, k)))
                at = node[node[:, 2] == k]
                idx = at[:, 1] * n + at[:, 0]
                e_pin = max(e_pin, float(np.abs(Y[idx] - ref[k][idx]).max()))
            worst[arith] = max(worst.get(arith, 0.0), e)
            worst[arith + " at the pinned nodes"] = max(worst.get(arith + " at the pinned nodes", 0.0), e_pin)
        s.close()
    print("\npinned tiny sources (%s): term / |X| at the node >= %.1e, lb - log2 tau_hard <= %.1f; max|dY| vs C oracle %s" % (
        variant, rel_term.min(), (lb - ltau_hard).max(), ", ".join("%s %.2e (margin %.0fx)" % (a, e, BOUND[a.split()[0]] / max(e, 1e-300)) for a, e in worst.items())))
    for a, e in worst.items():
        assert e < BOUND[a.split()[0]], (variant, a, e)


# ---- C. Sources exactly on nodes and cell faces ------------------------------------------------------------------------------------------------------------
def _on_grid_sources(seed):
    """64^3, bbox_min = -1, cell = 2^-5: every node coordinate is exact.  An ellipsoid of 1500 sources plus sources exactly on interior nodes, on cell faces
    (one coordinate on a node plane) and edges (two), one ulp inside each top face, and one of weight 1e-30 |w_max| -- below the point where its fp32 square
    underflows -- exactly on a node.  Returns (set_problem arguments, indices of the sources on nodes)."""
    rng = np.random.default_rng(seed)
    n, cell = 64, 2.0 ** -5
    bbox_min = np.array([-1.0, -1.0, -1.0])
    S0 = 1500
    v = rng.normal(size=(S0, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    ax3 = np.array([0.6, 0.5, 0.45])
    pos = [v * ax3]
    nrm = v / ax3
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = [nrm]
    area = [np.full(S0, 4 * np.pi * 0.5 ** 2 / S0) * (0.5 + rng.random(S0))]
    a0 = float(area[0].mean())
    node_pts = bbox_min + rng.integers(8, n - 8, size=(6, 3)) * cell                               # on interior nodes
    face = bbox_min + (rng.integers(8, n - 8, size=(4, 3)) + np.array([0.0, 0.37, 0.61])) * cell   # on a face x = const
    edge = bbox_min + (rng.integers(8, n - 8, size=(4, 3)) + np.array([0.0, 0.0, 0.45])) * cell    # on an edge (x, y) = const
    top = bbox_min + (n - 1) * cell
    ulp_in = []
    for a in range(3):                                                    # the top face's coordinate, stepped down by ulps until the ABI's cell test (x - bbox_min) / cell < n - 1 holds
        q = bbox_min + np.array([20.3, 30.7, 40.1]) * cell
        q[a] = np.nextafter(top[a], -np.inf)
        while not np.floor((q[a] - bbox_min[a]) / cell) + 1.0 <= n - 1:
            q[a] = np.nextafter(q[a], -np.inf)
        ulp_in.append(q)
    tiny = bbox_min + np.array([[33, 21, 30]]) * cell                                               # tiny weight exactly on a node
    extra = np.vstack([node_pts, face, edge, np.array(ulp_in), tiny])
    u = rng.normal(size=extra.shape)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    pos.append(extra)
    nrm.append(u)
    area.append(np.concatenate([np.full(len(extra) - 1, a0), [1e-30 * float(area[0].max())]]))
    pos, nrm, area = np.vstack(pos), np.vstack(nrm), np.concatenate(area)
    d = dict(pos=pos, wnormal=nrm * area[:, None], area=area, lam=0.45 / cell, n=n, bbox_min=bbox_min, cell=cell)
    on_nodes = np.concatenate([np.arange(S0, S0 + 6), [len(pos) - 1]])
    return d, on_nodes


def _sources_in_cells(n, cells, t, seed, cell=2.0 ** -3, bbox_min=(-1.0, -1.0, -1.0), lam_cells=0.45):
    """One source per chosen cell: cells (m, 3) integer (i, j, k) in [0, n - 2], distinct, and local coordinates t (m, 3) in [0, 1) -- set_problem admits no
    source on the top faces, so a node of index n - 1 is reached as t = 1 - 2^-30 in cell n - 2.  bbox_min and cell are powers of two (or sums of few), and t is
    expected to have few bits, so that bbox_min + (cells + t) * cell is exact and the library's locate_source gives back exactly (cells, t): every row, fold and
    weight of a test is then the one the test chose.  Random unit normals, areas within a factor 3, lambda = lam_cells / cell.  Returns set_problem arguments."""
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    t = np.asarray(t, dtype=np.float64).reshape(-1, 3)
    m = cells.shape[0]
    assert t.shape[0] == m and cells.min() >= 0 and cells.max() <= n - 2 and t.min() >= 0.0 and t.max() < 1.0
    assert len({tuple(c) for c in cells.tolist()}) == m, "one source per cell: the cells must be distinct"
    bbox_min = np.asarray(bbox_min, dtype=np.float64)
    pos = bbox_min + (cells + t) * cell
    back = np.floor((pos - bbox_min) / cell)                                           # locate_source, shm_constraints.h
    assert np.array_equal(back, cells) and np.array_equal((pos - (back * cell + bbox_min)) / cell, t), "the positions do not give back the chosen cells and t exactly"
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(m, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    area = cell * cell * (0.5 + rng.random(m))
    return dict(pos=pos, wnormal=u * area[:, None], area=area, lam=lam_cells / cell, n=int(n), bbox_min=bbox_min, cell=float(cell))


def test_step1_sources_exactly_on_nodes_and_faces(shm, oracle_c):
    """Y: the nodes under a source come out non-finite exactly where the oracle's do (w e^0 / 0), including under a source whose weight's fp32 square underflows
    (the kernel's `valid` mask used to read that source as padding and leave its node finite); the rest within the bounds.  Constraint rows bit-exact against
    shmo_constraint_rows; phi (mesh overload, scrub on) within 1e-7 of shmo_compute_distance."""
    d, on_nodes = _on_grid_sources(3)
    n, S = int(d["n"]), len(d["area"])
    ijk = np.rint((d["pos"][on_nodes] - d["bbox_min"]) / d["cell"]).astype(np.int64)
    assert np.array_equal(d["bbox_min"] + ijk * d["cell"], d["pos"][on_nodes])                  # exactly on nodes
    ref = np.zeros(3 * n ** 3)
    oracle_c.shmo_set_threads(ORACLE_THREADS)
    oracle_c.shmo_conv_normalize(n, c_(d["bbox_min"]), d["cell"], S, c_(d["pos"]).reshape(-1), c_(d["wnormal"]).reshape(-1), d["lam"], 0, n, ref)
    ref = ref.reshape(-1, 3)
    flat = ijk[:, 2] * n * n + ijk[:, 1] * n + ijk[:, 0]
    assert not np.isfinite(ref[flat]).all(axis=1).any()                                             # the reference's arithmetic: NaN under every source on a node
    zone = np.concatenate([_zone(d, k) for k in range(n)])
    worst = {}
    s = make_solver(shm, d)
    for arith in ("fp64", "exact_f64"):
        s.run_conv(step1="exact_f64" if arith == "exact_f64" else "auto")
        Y = np.stack([s.get_field(f) for f in (0, 1, 2)], axis=1)
        worst[arith] = _compare(Y, ref, zone, "on-grid sources %s" % arith)
    nodes, coeffs = s.get_constraints()
    rn, rc = np.zeros(8 * S, dtype=np.int64), np.zeros(8 * S)
    m = oracle_c.shmo_constraint_rows(n, c_(d["bbox_min"]), d["cell"], S, c_(d["pos"]).reshape(-1), rn, rc)
    assert nodes.shape[0] == m
    assert np.array_equal(nodes, rn[:8 * m].reshape(-1, 8))
    assert np.array_equal(coeffs, rc[:8 * m].reshape(-1, 8))
    s.solve(tol=1e-10, scrub=True)
    phi, _ = s.get_phi()
    phi_ref, st = np.zeros(n ** 3), np.zeros(5)
    rc_ = oracle_c.shmo_compute_distance(n, c_(d["bbox_min"]), d["cell"], S, c_(d["pos"]).reshape(-1), c_(d["wnormal"]).reshape(-1), c_(d["area"]),
                                         d["lam"], 1, 0, 1e-12, 100000, phi_ref, st)
    assert rc_ == 0
    worst["phi"] = float(np.abs(phi - phi_ref).max())
    s.close()
    oracle_c.shmo_set_threads(min(8, os.cpu_count() or 1))
    bound = dict(BOUND, phi=1e-7)
    print("\nsources on nodes / faces / edges / one ulp inside the top faces: %d NaN nodes as the oracle's; max|d| vs C oracle %s" % (
        int((~np.isfinite(ref).all(axis=1)).sum()), ", ".join("%s %.2e (margin %.0fx)" % (a, e, bound[a] / max(e, 1e-300)) for a, e in worst.items())))
    for a, e in worst.items():
        assert e < bound[a], (a, e)
