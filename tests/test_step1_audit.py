"""The device audit of Step 1 (shm_grid_audit_step1, csrc/shm_audit.hip.h), its node sampler (shm_audit_sample_nodes) and SHM_STEP1_REFERENCE_F64.

The yardstick is never the library: the C oracle (the reference's serial loops) or, where sums must be exact, fp64 terms added with math.fsum.  How far two correct
evaluations of Y at a node may lie apart is DERIVED, not measured -- the "price" of a node:

    price_i = 2 * 2^-53 * sum_s |w_s|_1 g_s (lambda r_s + C) / |X_i|,      g_s = exp(-lambda r_s) / r_s.

A term w g carries a relative error of at most (lambda r + 8) u, u = 2^-53: the rounding of r (three differences, three squares, two sums, one square root: <= 4 u)
is amplified by lambda r in the exponential and by 1 in the division, exp and the division add one rounding each (<= 1.5 u with a 1-ulp exp), the product one more
-- lambda r u + 8 u with room.  A plain sum of S such terms adds at most S u sum |terms| (C = S + 8: the C oracle, whatever its order); an exact sum adds nothing
(C = 8: math.fsum, and the audit's double-double sums to first order).  |w|_1 bounds the three components at once.  An error dX of X turns Y = X / |X| by at most
|dX| / |X|; the factor 2 pays for both sides of a comparison."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, c_, load_golden

U = 2.0 ** -53
ZONE = 335.0
CLI = os.environ.get("SHM_CLI") or os.path.join(ROOT, "signed-heat-3d_amd", "bin", "shm_grid_cli")
ORACLE_THREADS = min(16, os.cpu_count() or 1)


# ---- the numpy restatement ------------------------------------------------------------------------------------------------------------------------------------
def _ijk(n, nodes):
    nodes = np.asarray(nodes, dtype=np.int64)
    return np.stack([nodes % n, (nodes // n) % n, nodes // (n * n)], axis=-1)


def _yardstick(d, nodes, exact=False):
    """At the nodes (flat indices): dict of Y (Q, 3) by plain fp64 sums (exact=False) or math.fsum of the fp64 terms (exact=True), the price with C = S + 8 / 8,
    |X| / L1, what two evaluations of L1 may differ by, lambda r_min and the finite mask.  Node positions as the reference forms them: i * cell + bbox_min, two roundings."""
    n, lam, S = int(d["n"]), float(d["lam"]), len(d["area"])
    pos, w = np.asarray(d["pos"], dtype=np.float64), np.asarray(d["wnormal"], dtype=np.float64)
    xyz = _ijk(n, nodes) * float(d["cell"]) + np.asarray(d["bbox_min"], dtype=np.float64)
    w1 = np.abs(w).sum(axis=1)
    Cc = 8.0 if exact else S + 8.0
    Q = len(xyz)
    X, L1, Lp, rmin = np.zeros((Q, 3)), np.zeros(Q), np.zeros(Q), np.zeros(Q)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        step = max(16, 2000000 // S)                                                  # (chunks of ~2e6 pairs: 50 MB of temporaries)
        for a in range(0, Q, step):
            dd = xyz[a:a + step, None, :] - pos[None, :, :]
            r = np.sqrt(dd[..., 0] * dd[..., 0] + dd[..., 1] * dd[..., 1] + dd[..., 2] * dd[..., 2])
            g = np.exp(-lam * r) / r
            if exact:
                t = g[:, :, None] * w[None, :, :]
                X[a:a + step] = [[math.fsum(t[q, :, p]) if np.isfinite(t[q, :, p]).all() else np.nan for p in range(3)] for q in range(t.shape[0])]
            else:
                X[a:a + step] = (g[:, :, None] * w[None, :, :]).sum(axis=1)
            L1[a:a + step] = (g * w1).sum(axis=1)
            Lp[a:a + step] = (g * w1 * (lam * r + Cc)).sum(axis=1)
            rmin[a:a + step] = r.min(axis=1)
        nrm = np.sqrt((X * X).sum(axis=1))
        Y = X / nrm[:, None]
        # l1_rel: the same allowance for the plain sum L1 itself, relative to it (two plain sums of it are 2 u sum |w|_1 g (lambda r + C) apart at most)
        return dict(Y=Y, price=2.0 * U * Lp / nrm, ratio=nrm / L1, l1_rel=2.0 * U * Lp / L1, lam_rmin=lam * rmin, finite=np.isfinite(Y).all(axis=1))


def _oracle_at(oracle_c, d, nodes):
    """The C oracle's Y at the nodes, from its planes (shmo_conv_normalize_planes on every plane the list touches)."""
    n = int(d["n"])
    ijk = _ijk(n, nodes)
    out = np.zeros((len(ijk), 3))
    oracle_c.shmo_set_threads(ORACLE_THREADS)
    try:
        for k in np.unique(ijk[:, 2]):
            Yp = np.zeros(3 * n * n)
            oracle_c.shmo_conv_normalize_planes(n, c_(d["bbox_min"]), float(d["cell"]), len(d["area"]), c_(d["pos"]).reshape(-1), c_(d["wnormal"]).reshape(-1),
                                                float(d["lam"]), int(k), int(k) + 1, Yp)
            sel = ijk[:, 2] == k
            out[sel] = Yp.reshape(-1, 3)[ijk[sel, 1] * n + ijk[sel, 0]]
    finally:
        oracle_c.shmo_set_threads(min(8, os.cpu_count() or 1))
    return out


def _from_file(name, hcoef):
    from signed_heat_3d_amd.host_abi import HostSolver
    pre = HostSolver(os.path.join(ROOT, "data", name)).preprocess(hCoef=hcoef)
    return dict(pos=pre["pos"], wnormal=pre["wnormal"], area=pre["area"], lam=pre["lam"], n=pre["n"], bbox_min=pre["bbox_min"], cell=pre["cell"])


def _golden(name):
    g = load_golden(name)
    return dict(pos=g["pos"], wnormal=g["wnormal"], area=g["area"], lam=float(g["lam"]), n=int(g["n"]), bbox_min=g["bbox_min"], cell=float(g["cell"]))


def _solver(shm, d, **kw):
    s = shm.GridSolver(**kw)
    s.set_problem(d["pos"], d["wnormal"], d["area"], float(d["lam"]), int(d["n"]), d["bbox_min"], float(d["cell"]))
    return s


def _device_Y(s, nodes):
    """The resident Y at the nodes, through get_field_planes (every slab's planes, read range by range)."""
    n = s.n
    ijk = _ijk(n, nodes)
    k0, k1 = s.owned_planes()
    Y = np.stack([s.get_field_planes(f, k0, k1) for f in (0, 1, 2)], axis=1)
    return Y[(ijk[:, 2] - k0) * n * n + ijk[:, 1] * n + ijk[:, 0]]


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_audit_entry_points_and_struct_layout(shm):
    """Both symbols are exported and declared, the ctypes mirror of shm_step1_audit follows the header field by field, and the ABI version did not move."""
    lib = shm.load_library()
    from signed_heat_3d_amd.grid_abi import ShmStep1Audit
    header = open(os.path.join(ROOT, "include", "shm_grid.h")).read()
    for name in ("shm_grid_audit_step1", "shm_audit_sample_nodes"):
        assert hasattr(lib, name) and (name + "(") in header, name
    body = header[header.index("typedef struct {\n    int64_t n_audited"):header.index("} shm_step1_audit;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}
    decl = [(nm.strip(), ctype[t]) for t, names in re.findall(r"\b(int32_t|int64_t|double)\s+([\w, ]+);", body) for nm in names.split(",")]
    assert decl == list(ShmStep1Audit._fields_)
    assert C.sizeof(ShmStep1Audit) == 96
    assert lib.shm_grid_abi_version() == 5
    assert shm.GridSolver.STEP1["reference_f64"] == 2 and "SHM_STEP1_REFERENCE_F64 = 2" in header


def _strata_counts(n, k_begin, k_end, nodes):
    """Per layer of four planes counted from k_begin: (nodes taken, capacity), and per 8 x 8 x 4 block of every layer the same."""
    ijk = _ijk(n, nodes)
    layers = (k_end - k_begin + 3) // 4
    tiles = (n + 7) // 8
    lay = (ijk[:, 2] - k_begin) // 4
    per_layer = np.bincount(lay, minlength=layers)
    nz = np.array([min(k_end, k_begin + 4 * l + 4) - (k_begin + 4 * l) for l in range(layers)])
    side = np.array([min(8, n - 8 * b) for b in range(tiles)])
    bcap = side[None, :, None] * side[None, None, :] * nz[:, None, None]
    per_block = np.zeros((layers, tiles, tiles), dtype=np.int64)
    np.add.at(per_block, (lay, ijk[:, 1] // 8, ijk[:, 0] // 8), 1)
    return per_layer, nz * n * n, per_block, bcap


def _even_up_to_capacity(taken, cap):
    """Strata that are not taken whole differ by at most one, and none of them holds fewer than a stratum that is."""
    assert (taken <= cap).all()
    open_ = taken[taken < cap]
    if open_.size:
        assert open_.max() - open_.min() <= 1, (open_.min(), open_.max())
        if (taken == cap).any():
            assert taken[taken == cap].max() <= open_.min()


@pytest.mark.parametrize("n,k_begin,k_end", [(16, 0, 16), (24, 0, 24), (33, 0, 33), (64, 0, 64), (33, 5, 22), (64, 13, 43), (24, 3, 5), (16, 7, 8)])
def test_sampler_is_stratified_deterministic_and_seeded(shm, n, k_begin, k_end):
    """shm_audit_sample_nodes: min(count, nodes in range) ascending distinct nodes of the planes asked for, a function of its arguments alone; the counts per
    four-plane layer, and per 8 x 8 x 4 block within a layer, differ by at most one (a stratum smaller than its share is taken whole); seeds matter."""
    in_range = (k_end - k_begin) * n * n
    for count in (1, 7, 4096, in_range + 1000):
        a = shm.audit_sample_nodes(n, k_begin, k_end, count, seed=1)
        assert a.dtype == np.int64 and len(a) == min(count, in_range)
        assert (np.diff(a) > 0).all()
        assert a.min() >= k_begin * n * n and a.max() < k_end * n * n
        assert np.array_equal(a, shm.audit_sample_nodes(n, k_begin, k_end, count, seed=1))
        per_layer, lcap, per_block, bcap = _strata_counts(n, k_begin, k_end, a)
        _even_up_to_capacity(per_layer, lcap)
        for l in range(len(per_layer)):
            _even_up_to_capacity(per_block[l].ravel(), bcap[l].ravel())
        b = shm.audit_sample_nodes(n, k_begin, k_end, count, seed=2)
        if count < in_range // 4:
            assert not np.array_equal(a, b)
        else:
            assert len(b) == len(a)
    # the raw entry point: nothing written for an empty range or count <= 0
    lib = shm.load_library()
    buf = np.full(4, -7, dtype=np.int64)
    assert lib.shm_audit_sample_nodes(n, k_end, k_begin, 4, 0, buf.ctypes.data) == 0 and lib.shm_audit_sample_nodes(n, k_begin, k_end, 0, 0, buf.ctypes.data) == 0
    assert (buf == -7).all()


def test_cli_lists_the_audit_flags_and_refuses_both_step1_modes():
    p = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert p.returncode == 0 and "--audit <count>" in p.stdout and "--reference-step1" in p.stdout
    # refused while the arguments are read: no mesh is loaded, no device is touched (a path that does not exist would otherwise be the error)
    p = subprocess.run([CLI, "no_such_mesh.obj", "--exact-step1", "--reference-step1"], capture_output=True, text=True)
    assert p.returncode != 0 and "exclude each other" in p.stderr and "no_such_mesh" not in p.stderr


def test_numpy_restatement_is_held_to_the_c_oracle(shm, oracle_c):
    """What the GPU tests use as their price and as their class rule is itself checked: the plain-sum Y of _yardstick at 2048 seeded nodes of bunny_small_n32
    agrees with shmo_conv_normalize_planes and with the fixture's Y, per node, within the price (C = S + 8); no node is out of zone or non-finite.
    (Measured when this was written: max |dY| against the oracle 2.2e-16, largest price 4.0e-12, worst node at 0.0002 of its price, max lambda r_min 44.5.)"""
    g = load_golden("bunny_small_n32")
    d = _golden("bunny_small_n32")
    nodes = np.sort(np.random.default_rng(11).choice(int(d["n"]) ** 3, size=2048, replace=False))
    y = _yardstick(d, nodes)
    assert y["finite"].all() and (y["lam_rmin"] < ZONE).all()
    Yo = _oracle_at(oracle_c, d, nodes)
    e_oracle = np.abs(y["Y"] - Yo).max(axis=1)
    e_fixture = np.abs(y["Y"] - g["Y"][nodes]).max(axis=1)
    print("\nnumpy restatement vs C oracle: max |dY| %.2e, largest price %.2e, worst node at %.4f of its price; max lambda r_min %.1f"
          % (e_oracle.max(), y["price"].max(), (e_oracle / y["price"]).max(), y["lam_rmin"].max()))
    assert (e_oracle <= y["price"]).all() and (e_fixture <= y["price"]).all()
    ye = _yardstick(d, nodes[:64], exact=True)                                       # the exact-sum form: inside the plain form's price, and a smaller price
    assert (np.abs(ye["Y"] - y["Y"][:64]).max(axis=1) <= y["price"][:64]).all() and (ye["price"] < y["price"][:64]).all()


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------------------------
def _audit_against_oracle(s, oracle_c, d, count=4096, seed=0, extra=0.0):
    """Audit a `count`-node sample with per-node output and hold every node to the oracle: |dy_audit - |Y_device - Y_oracle||_inf <= price (+ extra), with the
    yardstick's precondition (no out-of-zone, no non-finite node) and max / argmax consistency.  Returns (audit dict, yardstick dict, dy by the oracle)."""
    a = s.audit_step1(count=count, seed=seed, per_node=True)
    nodes = a["nodes"]
    assert len(nodes) == count
    y = _yardstick(d, nodes)
    assert y["finite"].all() and (y["lam_rmin"] < ZONE).all()                        # precondition: nothing can be excluded
    dy_oracle = np.abs(_device_Y(s, nodes) - _oracle_at(oracle_c, d, nodes)).max(axis=1)
    gap = np.abs(a["dy"] - dy_oracle)
    print("\naudit vs oracle: n=%d S=%d max_dy %.3e (oracle's %.3e), worst gap / price %.3e, min ratio %.3e, audit %.3f ms"
          % (d["n"], len(d["area"]), a["max_dy"], dy_oracle.max(), (gap / (y["price"] + extra)).max(), a["min_ratio"], a["ms"]))
    assert (gap <= y["price"] + extra).all(), float((gap / (y["price"] + extra)).max())
    assert a["n_audited"] == count and a["n_not_owned"] == a["n_nonfinite"] == a["n_out_of_zone"] == a["n_finite_mismatch"] == 0
    assert a["max_dy"] == a["dy"].max() and a["worst_node"] == nodes[int(np.argmax(a["dy"]))]
    assert a["worst_ratio"] == a["ratio"][int(np.argmax(a["dy"]))] and a["min_ratio"] == a["ratio"].min()
    assert (np.abs(a["ratio"] / y["ratio"] - 1.0) <= y["price"] + y["l1_rel"]).all()            # |X| to within the price, L1 to within its own
    return a, y, dy_oracle


@pytest.mark.gpu
@pytest.mark.parametrize("name,hcoef,n", [("bunny_small.obj", 2.0, 64), ("bunny_small.obj", 3.0, 128), ("knot.obj", 2.0, 64), ("bunny.pc", 2.0, 64)])
def test_audit_agrees_with_the_oracle_and_default_step1_is_within_budget(shm, oracle_c, name, hcoef, n):
    d = _from_file(name, hcoef)
    assert d["n"] == n
    s = _solver(shm, d)
    s.solve(tol=1e-8, scrub=not name.endswith(".pc"))
    a, _, _ = _audit_against_oracle(s, oracle_c, d)
    s.close()
    assert a["step1_arith"] == 0 and a["budget"] == 1e-8
    assert a["max_dy"] <= 1e-8 and a["within_budget"] == 1


@pytest.mark.gpu
def test_audit_follows_the_budget_of_the_solve(shm, oracle_c):
    d = _from_file("bunny_small.obj", 3.0)
    s = _solver(shm, d)
    s.solve(tol=1e-8)
    default = s.audit_step1()
    s.solve(tol=1e-8, step1_budget=1e-4)
    a, _, _ = _audit_against_oracle(s, oracle_c, d)
    s.close()
    print("\nbudget 1e-4: max_dy %.3e within_budget %d (default budget: max_dy %.3e)" % (a["max_dy"], a["within_budget"], default["max_dy"]))
    assert a["budget"] == 1e-4 and default["budget"] == 1e-8
    assert a["within_budget"] == (1 if a["max_dy"] <= 1e-4 else 0)


def _cancelling_sheets(seed):
    """Two parallel sheets of 16 x 16 sources 1/512 of a cell apart, the upper one's weights the negated lower one's (normals tilted a little off z, areas over
    half a decade), between two node planes of a 32^3 grid: everywhere the sheets' terms cancel to ~ (lambda + 1 / r) * separation of their size."""
    rng = np.random.default_rng(seed)
    n, cell = 32, 2.0 / 31
    bbox_min = np.array([-1.0, -1.0, -1.0])
    gx, gy = np.meshgrid(np.linspace(-0.5, 0.5, 16), np.linspace(-0.5, 0.5, 16), indexing="ij")
    p = np.stack([gx.ravel(), gy.ravel(), np.full(256, -1.0 + 15.37 * cell)], axis=1) + rng.normal(scale=0.1 * cell, size=(256, 3)) * np.array([1, 1, 0])
    nrm = np.array([0.0, 0.0, 1.0]) + rng.normal(scale=0.05, size=(256, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    area = (1.0 / 256) * 10.0 ** (-0.5 * rng.random(256))
    sep = cell / 512
    pos = np.vstack([p + [0, 0, 0.5 * sep], p - [0, 0, 0.5 * sep]])
    wn = np.vstack([nrm * area[:, None], -nrm * area[:, None]])
    return dict(pos=pos, wnormal=wn, area=np.concatenate([area, area]), lam=0.45 / cell, n=n, bbox_min=bbox_min, cell=cell)


@pytest.mark.gpu
def test_audit_in_deep_cancellation(shm):
    """Where |X| is a thousandth and less of its terms the audit's compensated sums are what keeps it a reference: against fp64 terms summed exactly (math.fsum)
    it agrees at the price with C = 8, and its min_ratio is the yardstick's to 1e-6 (|X| itself is known to u (lambda r + 8) / ratio: ratio >= 1e-8 asserted)."""
    d = _cancelling_sheets(5)
    n = d["n"]
    k, j, i = np.meshgrid(np.arange(11, 21), np.arange(6, 26, 2), np.arange(6, 26, 2), indexing="ij")
    nodes = np.sort((i + j * n + k * n * n).ravel()).astype(np.int64)
    y = _yardstick(d, nodes, exact=True)
    assert y["finite"].all() and (y["lam_rmin"] < ZONE).all()
    assert 1e-8 <= y["ratio"].min() <= 1e-3, y["ratio"].min()
    s = _solver(shm, d)
    s.run_conv()
    a = s.audit_step1(nodes=nodes, per_node=True)
    dy_exact = np.abs(_device_Y(s, nodes) - y["Y"]).max(axis=1)
    s.close()
    gap = np.abs(a["dy"] - dy_exact)
    print("\ncancelling sheets: %d nodes, |X| / L1 from %.2e to %.2e; max_dy %.3e, worst gap / price %.3e (largest price %.2e)"
          % (len(nodes), y["ratio"].min(), y["ratio"].max(), a["max_dy"], (gap / y["price"]).max(), y["price"].max()))
    assert a["n_audited"] == len(nodes)
    assert (gap <= y["price"]).all(), float((gap / y["price"]).max())
    assert abs(a["min_ratio"] / y["ratio"].min() - 1.0) < 1e-6
    assert np.abs(a["ratio"] / y["ratio"] - 1.0).max() < 1e-6


@pytest.mark.gpu
def test_reference_f64_mode(shm, oracle_c):
    """SHM_STEP1_REFERENCE_F64: Y within the price of the C oracle at every sampled node (the cubic body's own 1.1e-16 lambda r per term sits inside the price's
    lambda r u), the audit agrees, the mode has no budget, no pair goes through fp32, and phi is EXACT_F64's to the 1e-9 the header states."""
    d = _from_file("bunny_small.obj", 2.0)
    s = _solver(shm, d)
    s.run_conv("reference_f64")
    a, y, dy_oracle = _audit_against_oracle(s, oracle_c, d)
    print("\nreference_f64: worst |Y - Y_oracle| / price %.3e; audit max_dy %.3e, largest price %.3e" % ((dy_oracle / y["price"]).max(), a["max_dy"], y["price"].max()))
    assert (dy_oracle <= y["price"]).all()
    assert a["max_dy"] <= y["price"].max()
    assert a["budget"] == 0.0 and a["within_budget"] == -1 and a["step1_arith"] == 2
    st = s.solve(tol=1e-10, step1="reference_f64")
    phi_ref = s.get_phi()[0]
    assert st.pairs_fp32 == 0 and st.pairs_fp64 >= float(d["n"]) ** 3 * int((np.abs(d["wnormal"]).sum(axis=1) > 0).sum())
    assert s.audit_step1()["step1_arith"] == 2
    s.solve(tol=1e-10, step1="exact_f64")
    phi_exact = s.get_phi()[0]
    e = s.audit_step1()
    s.close()
    print("reference_f64 vs exact_f64: max |dphi| %.3e" % np.abs(phi_ref - phi_exact).max())
    assert e["step1_arith"] == 1 and e["budget"] == 0.0 and e["within_budget"] == -1
    assert np.abs(phi_ref - phi_exact).max() < 1e-9


def _on_grid_sources(seed):
    """64^3, bbox_min = -1, cell = 2^-5 (every node coordinate exact): an ellipsoid of 1500 sources plus six sources exactly on interior nodes and one of weight
    1e-30 |w_max| exactly on a node (the sources-on-nodes input of test_step1_edges.py, restated).  Returns (set_problem arguments, flat indices of those nodes)."""
    rng = np.random.default_rng(seed)
    n, cell = 64, 2.0 ** -5
    bbox_min = np.array([-1.0, -1.0, -1.0])
    S0 = 1500
    v = rng.normal(size=(S0, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    ax3 = np.array([0.6, 0.5, 0.45])
    nrm = v / ax3
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    area = np.full(S0, 4 * np.pi * 0.5 ** 2 / S0) * (0.5 + rng.random(S0))
    on = np.vstack([rng.integers(8, n - 8, size=(6, 3)), [[33, 21, 30]]])
    assert len(np.unique(on, axis=0)) == 7
    u = rng.normal(size=(7, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    a_on = np.concatenate([np.full(6, float(area.mean())), [1e-30 * float(area.max())]])
    d = dict(pos=np.vstack([v * ax3, bbox_min + on * cell]), wnormal=np.vstack([nrm * area[:, None], u * a_on[:, None]]), area=np.concatenate([area, a_on]),
             lam=0.45 / cell, n=n, bbox_min=bbox_min, cell=cell)
    return d, on[:, 0] + on[:, 1] * n + on[:, 2] * n * n


@pytest.mark.gpu
def test_audit_classes(shm, oracle_c):
    """Non-finite: the nodes under a source are the oracle's non-finite nodes and the device's, none is a mismatch (whole grid audited).  Out of zone: a coarse
    grid whose corners lie beyond lambda r_min = 335 -- the count is numpy's, and those nodes are excluded from max_dy."""
    d, under = _on_grid_sources(3)
    n = d["n"]
    ref = np.zeros(3 * n ** 3)
    oracle_c.shmo_set_threads(ORACLE_THREADS)
    oracle_c.shmo_conv_normalize(n, c_(d["bbox_min"]), d["cell"], len(d["area"]), c_(d["pos"]).reshape(-1), c_(d["wnormal"]).reshape(-1), d["lam"], 0, n, ref)
    oracle_c.shmo_set_threads(min(8, os.cpu_count() or 1))
    bad = np.flatnonzero(~np.isfinite(ref.reshape(-1, 3)).all(axis=1))
    assert np.array_equal(bad, np.sort(under))
    s = _solver(shm, d)
    s.run_conv()
    a = s.audit_step1(nodes=np.arange(n ** 3, dtype=np.int64), per_node=True)
    s.close()
    print("\nsources on nodes: %d non-finite, %d mismatches, %d out of zone, max_dy %.3e over %d nodes in %.2f ms"
          % (a["n_nonfinite"], a["n_finite_mismatch"], a["n_out_of_zone"], a["max_dy"], a["n_audited"], a["ms"]))
    assert a["n_nonfinite"] == len(bad) and a["n_finite_mismatch"] == 0 and a["n_out_of_zone"] == 0 and a["n_audited"] == n ** 3 - len(bad)
    assert np.array_equal(np.flatnonzero(np.isnan(a["dy"])), bad)

    d = _golden("bunny_small_n16")
    nodes = np.arange(16 ** 3, dtype=np.int64)
    d["lam"] = 1.0
    d["lam"] = 400.0 / float(_yardstick(d, nodes)["lam_rmin"].max())                  # the farthest corner at lambda r_min = 400
    lam_rmin = _yardstick(d, nodes)["lam_rmin"]
    out_of_zone = lam_rmin >= ZONE
    assert 0 < out_of_zone.sum() < len(nodes) // 2
    s = _solver(shm, d)
    s.run_conv()
    a = s.audit_step1(nodes=nodes, per_node=True)
    s.close()
    print("coarse grid: %d of %d nodes out of zone (numpy: %d), %d audited, %d non-finite, %d mismatches"
          % (a["n_out_of_zone"], len(nodes), out_of_zone.sum(), a["n_audited"], a["n_nonfinite"], a["n_finite_mismatch"]))
    assert a["n_out_of_zone"] == int(out_of_zone.sum())
    assert a["n_audited"] + a["n_nonfinite"] + a["n_finite_mismatch"] == int((~out_of_zone).sum())
    assert a["max_dy"] == np.nanmax(np.where(out_of_zone, np.nan, a["dy"]))


def _slab_bounds(shm, d, slabs, weighted):
    n = int(d["n"])
    if not weighted:
        return [shm.plan_slab(n, slabs, r) for r in range(slabs)]
    w = shm.step1_plane_weights(d["pos"], d["wnormal"], d["lam"], n, d["bbox_min"], d["cell"], 64)
    return [shm.plan_slab_weighted(n, slabs, r, w, 4) for r in range(slabs)]


@pytest.mark.gpu
@pytest.mark.parametrize("slabs,weighted", [(2, False), (3, False), (3, True)])
def test_audit_on_several_slabs(shm, slabs, weighted):
    """Nodes on the first and last plane of every slab.  |X| / L1 does not see Y: bit-identical to the single-slab handle's under every arithmetic.  dy sees Y: with
    REFERENCE_F64 -- where a node's Y does not depend on the block it falls in, which the slab plan moves -- dy is bit-identical as well; with AUTO the classes agree
    and dy is the handle's own |Y - Y_ref| (exact sums, C = 8)."""
    d = _golden("bunny_small_n32")
    n = d["n"]
    rng = np.random.default_rng(7)
    bounds = _slab_bounds(shm, d, slabs, weighted)
    planes = sorted({k for k0, k1 in bounds for k in (k0, k1 - 1)})
    nodes = np.sort(np.concatenate([k * n * n + rng.choice(n * n, size=48, replace=False) for k in planes])).astype(np.int64)
    one, many = _solver(shm, d), _solver(shm, d, local_slabs=slabs, slab_plan=1 if weighted else 0)
    assert many.owned_planes() == (0, n)
    y = _yardstick(d, nodes[:96], exact=True)
    for arith in ("reference_f64", "auto"):
        one.run_conv(arith)
        many.run_conv(arith)
        a1, am = one.audit_step1(nodes=nodes, per_node=True), many.audit_step1(nodes=nodes, per_node=True)
        assert np.array_equal(a1["ratio"], am["ratio"]) and a1["min_ratio"] == am["min_ratio"]
        for key in ("n_audited", "n_not_owned", "n_nonfinite", "n_out_of_zone", "n_finite_mismatch", "step1_arith", "budget"):
            assert a1[key] == am[key] and a1["n_audited"] == len(nodes), key
        if arith == "reference_f64":
            assert np.array_equal(a1["dy"], am["dy"]) and a1["max_dy"] == am["max_dy"] and a1["worst_node"] == am["worst_node"]
        gap = np.abs(am["dy"][:96] - np.abs(_device_Y(many, nodes[:96]) - y["Y"]).max(axis=1))
        assert (gap <= y["price"]).all(), (arith, float((gap / y["price"]).max()))
    one.close()
    many.close()


@pytest.mark.gpu
def test_audit_state_arguments_and_purity(shm, oracle_c):
    d = _golden("bunny_small_n32")
    n = d["n"]
    lib = shm.load_library()
    from signed_heat_3d_amd.grid_abi import ShmStep1Audit
    s = _solver(shm, d)
    with pytest.raises(shm.ShmError) as e:
        s.audit_step1(count=16)
    assert e.value.status == 7                                                          # SHM_ERR_STATE before any Step 1
    s.solve(tol=1e-10)
    phi0, Y0 = s.get_phi()[0], np.stack([s.get_field(f) for f in (0, 1, 2)])
    out, nodes = ShmStep1Audit(), np.array([0, 5, n ** 3 - 1], dtype=np.int64)
    assert lib.shm_grid_audit_step1(s._h, -1, nodes.ctypes.data, None, None, C.byref(out)) == 1
    assert lib.shm_grid_audit_step1(s._h, 3, None, None, None, C.byref(out)) == 1
    assert lib.shm_grid_audit_step1(s._h, 3, nodes.ctypes.data, None, None, None) == 1
    for bad in (-1, n ** 3):
        assert lib.shm_grid_audit_step1(s._h, 3, np.array([0, bad, 1], dtype=np.int64).ctypes.data, None, None, C.byref(out)) == 1
    assert lib.shm_grid_audit_step1(s._h, 3, nodes.ctypes.data, None, None, C.byref(out)) == 0 and out.n_audited == 3
    assert lib.shm_grid_audit_step1(s._h, 0, None, None, None, C.byref(out)) == 0 and out.n_audited == 0 and out.worst_node == -1
    a, b = s.audit_step1(per_node=True, seed=3), s.audit_step1(per_node=True, seed=3)
    for key in a:
        if key != "ms":
            assert np.array_equal(a[key], b[key]), key
    assert np.array_equal(phi0, s.get_phi()[0]) and np.array_equal(Y0, np.stack([s.get_field(f) for f in (0, 1, 2)]))
    s.run_divergence()                                                                  # the state flags are as they were: the stages after Step 1 still run
    s.close()
    # fp32 handle: the audit reads the stored fp32 Y.  Both sides of the comparison read the same stored values, so the price alone would do; the storage
    # rounding of a component (|Y_p| <= 1: at most 2^-24) is the derived allowance the comparison is granted on top
    s = _solver(shm, d, precision=32)
    s.run_conv("reference_f64")                                                          # ignored by an fp32 handle, as EXACT_F64 is
    a, _, dy_oracle = _audit_against_oracle(s, oracle_c, d, extra=2.0 ** -24)
    s.close()
    print("\nfp32 handle: max_dy %.3e" % a["max_dy"])
    assert a["budget"] == 0.0 and a["within_budget"] == -1 and a["step1_arith"] == 0


@pytest.mark.gpu
def test_cli_audit_line_matches_the_python_path(shm):
    from signed_heat_3d_amd.host_abi import HostSolver
    p = subprocess.run([CLI, os.path.join(ROOT, "data", "bunny_small.obj"), "--h", "2", "--audit", "4096"], capture_output=True, text=True, timeout=300)
    print("\n" + p.stderr.strip())
    assert p.returncode == 0, p.stderr
    lines = p.stderr.splitlines()
    at = [i for i, l in enumerate(lines) if l.startswith("step1 audit:")]
    assert len(at) == 1 and lines[at[0] - 1].startswith("min:")
    m = re.match(r"step1 audit: max_dy (\S+) budget (\S+) within budget worst_node (\d+) worst_ratio (\S+) min_ratio (\S+) audited 4096 out_of_zone 0 nonfinite 0 "
                 r"mismatch 0 not_owned 0 ms (\S+)$", lines[at[0]])
    assert m, lines[at[0]]
    h = HostSolver(os.path.join(ROOT, "data", "bunny_small.obj"))
    h.compute_distance(hCoef=2.0)
    a = h.audit_step1(4096)
    assert m.group(1) == "%.3e" % a["max_dy"] and int(m.group(3)) == a["worst_node"] and m.group(5) == "%.3e" % a["min_ratio"]
    assert a["within_budget"] == 1 and float(m.group(2)) == 1e-8
    r = HostSolver(os.path.join(ROOT, "data", "bunny_small.obj"), step1="reference_f64")
    _, st = r.compute_distance(hCoef=2.0)
    assert st.pairs_fp32 == 0 and r.audit_step1(256)["step1_arith"] == 2
