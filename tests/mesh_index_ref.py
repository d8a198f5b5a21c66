"""A numpy restatement of the attached mesh's index (csrc/shm_mesh_index.h; include/shm_grid.h states the contract under shm_grid_attach_mesh_device): the box
on the order-preserving integer image, the automatic c and its halving, the per-axis cell ranges from two floors, the big list (slivers and ranges of more than
64 cells), the far rule, and a walk under the culls of csrc/shm_closest_index.h with the index's own (c + 1, lo, cell) and eps = max(2^-16 cell, 2^-44 M).

`build` files the triangles and returns the (cell, triangle) pairs in (triangle, k, j, i) order: tests/native/test_mesh_index.cpp writes the same list.
`answers` evaluates queries against a built index.  Its walk takes the occupied cells shell by shell, in the device's order of shells, under the device's
culls (the whole-grid gap, the shell bound, the grown-box gap of a cell against lim = min(running d^2, max_dist^2) (1 + 2^-18)), but lowers lim between shells
and not inside one: inside a shell it tests a superset of what the device tests, which cannot change a minimum with a smallest-id tie rule.
`brute` is the contract itself: closest_point_ref.brute_force over the triangles with three finite corners, ids mapped back.
`build(..., shrink_upper=True)` seeds a defect (every range loses its last cell per axis) for the test that shows the inputs reach the rule."""
import numpy as np

import closest_point_ref as cpr
import mesh_smooth_ref as msr

MAX_CELLS, BIG_CELLS, MAX_BIG, FAR_CELLS = 512, 64, 4096, 4096.0
SLACK = 1.0 + 2.0 ** -18


class Refused(Exception):
    pass


def auto_cells(nt):
    c = 1
    while c < MAX_CELLS and 8 * c * c < nt:
        c += 1
    return c


def box(V):
    """(lo, hi, any) over the finite vertices, on the integer image."""
    V = np.asarray(V, dtype=np.float64).reshape(-1, 3)
    fin = np.isfinite(V).all(axis=1)
    if not fin.any():
        return np.zeros(3), np.zeros(3), False
    k = msr.key(V[fin])
    return msr.unkey(k.min(axis=0)), msr.unkey(k.max(axis=0)), True


def grid(c, lo, hi, any_):
    """dict(n, lo, cell, eps) of mi_grid."""
    E = float(np.max(hi - lo)) if any_ else 0.0
    M = float(max(np.abs(lo).max(), np.abs(hi).max())) if any_ else 0.0
    if not np.isfinite(E):
        raise Refused("extent")
    cell = E / c if E > 0 else 1.0
    if not cell > 0:
        raise Refused("extent")
    return dict(n=c + 1, lo=np.asarray(lo if any_ else np.zeros(3), dtype=np.float64), cell=cell, eps=max(cell * 2.0 ** -16, M * 2.0 ** -44))


def _cell_axis(x, b, cell, n):
    with np.errstate(over="ignore", invalid="ignore"):
        f = np.floor((x - b) / cell)
    return np.where(f < 0, 0, np.where(f > n - 2, n - 2, f)).astype(np.int64)


def classify(G, V, F, shrink_upper=False):
    """(cls [nt] in {0 skip, 1 filed, 2 big}, r0 [nt, 3], r1 [nt, 3])."""
    X = V[F]
    nt = len(F)
    fin = np.isfinite(X).all(axis=(1, 2)) if nt else np.zeros(0, bool)
    Xs = np.where(fin[:, None, None], X, 0.0)
    thin = cpr.slivers(np.where(np.isfinite(V), V, 0.0), F, G["cell"]) if nt else np.zeros(0, bool)
    r0 = np.stack([_cell_axis(Xs[:, :, a].min(axis=1), G["lo"][a], G["cell"], G["n"]) for a in range(3)], axis=1) if nt else np.zeros((0, 3), np.int64)
    r1 = np.stack([_cell_axis(Xs[:, :, a].max(axis=1), G["lo"][a], G["cell"], G["n"]) for a in range(3)], axis=1) if nt else np.zeros((0, 3), np.int64)
    cells = (r1 - r0 + 1).prod(axis=1)
    cls = np.where(~fin, 0, np.where(thin | (cells > BIG_CELLS), 2, 1))
    if shrink_upper:
        r1 = np.maximum(r1 - 1, r0)
    return cls, r0, r1


def build(V, F, cells=0, shrink_upper=False):
    """The index of mesh (V [nv, 3], F [nt, 3]) as a dict: c, G, big [ids], pair_cell / pair_tri (the filed pairs in (triangle, k, j, i) order), occ [nocc, 3]
    (i, j, k of the occupied cells), runs (list of id arrays, one per occupied cell), cand [ids of the triangles with finite corners]."""
    V = np.asarray(V, dtype=np.float64).reshape(-1, 3)
    F = np.asarray(F, dtype=np.int64).reshape(-1, 3)
    if not 0 <= cells <= MAX_CELLS:
        raise Refused("cells")
    if len(F) and (F.min() < 0 or F.max() >= len(V)):
        raise Refused("index")
    lo, hi, any_ = box(V)
    c = cells or auto_cells(len(F))
    while True:
        G = grid(c, lo, hi, any_)
        cls, r0, r1 = classify(G, V, F, shrink_upper)
        big = np.nonzero(cls == 2)[0]
        if len(big) <= MAX_BIG:
            break
        if cells or c == 1:
            raise Refused("big")
        c //= 2
    n = G["n"]
    pc, pt = [], []
    for t in np.nonzero(cls == 1)[0]:
        k, j, i = np.meshgrid(np.arange(r0[t, 2], r1[t, 2] + 1), np.arange(r0[t, 1], r1[t, 1] + 1), np.arange(r0[t, 0], r1[t, 0] + 1), indexing="ij")
        g = (i + n * (j + n * k)).reshape(-1)
        pc.append(g)
        pt.append(np.full(len(g), t, dtype=np.int64))
    pair_cell = np.concatenate(pc) if pc else np.zeros(0, np.int64)
    pair_tri = np.concatenate(pt) if pt else np.zeros(0, np.int64)
    order = np.argsort(pair_cell, kind="stable")
    gs, first = np.unique(pair_cell[order], return_index=True)
    runs = np.split(pair_tri[order], first[1:]) if len(gs) else []
    occ = np.stack([gs % n, (gs // n) % n, gs // (n * n)], axis=1) if len(gs) else np.zeros((0, 3), np.int64)
    return dict(c=c, G=G, V=V, F=F, big=big, pair_cell=pair_cell, pair_tri=pair_tri, occ=occ, runs=runs, cand=np.nonzero(cls != 0)[0])


def _gap(x, i, b, cell, eps):
    lo, hi = i * cell + b, (i + 1) * cell + b
    g = np.maximum(lo - x, x - hi) - eps
    return np.where(g > 0, g, 0.0)


def _far(G, q):
    hi = (G["n"] - 1) * G["cell"] + G["lo"]
    g = np.maximum(G["lo"] - q, q - hi)
    g2 = 0.0
    for a in range(3):
        if g[a] > 0:
            g2 += g[a] * g[a]
    f = FAR_CELLS * G["cell"]
    return g2 > f * f


def answers(X, pts, max_dist):
    """closest_point_ref's result dict (dist, cp, tri, answered, n_answered, d2, tri_all) of the queries against the index X."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    G, V, F = X["G"], X["V"], X["F"]
    n, b, cell, eps = G["n"], G["lo"], G["cell"], G["eps"]
    Q = len(pts)
    out_d2, out_tri = np.full(Q, np.inf), np.full(Q, -1, dtype=np.int64)
    max2 = max_dist * max_dist
    TX = V[F] if len(F) else np.zeros((0, 3, 3))
    occ, runs = X["occ"], X["runs"]

    def offer(q, ids, best, bt):
        if not len(ids):
            return best, bt
        rel = TX[ids] - q
        d2, _ = cpr.tri_closest(rel[:, 0], rel[:, 1], rel[:, 2])
        m = d2.min()
        t = int(ids[d2 == m].min())
        if m < best or (m == best and t < bt):
            return float(m), t
        return best, bt

    for qi, q in enumerate(pts):
        if not np.isfinite(q).all() or not len(X["cand"]):
            continue
        best, bt = np.inf, -1
        if _far(G, q):
            best, bt = offer(q, X["cand"], best, bt)
            out_d2[qi], out_tri[qi] = best, bt
            continue
        best, bt = offer(q, X["big"], best, bt)
        lim = min(best, max2) * SLACK
        c0 = np.array([int(_cell_axis(q[a], b[a], cell, n)) for a in range(3)])
        g0 = sum(float(_gap(q[a], c0[a], b[a], cell, eps)) ** 2 for a in range(3))
        if not g0 > lim and len(occ):
            s_of = np.abs(occ - c0).max(axis=1)
            gx, gy, gz = (_gap(q[a], occ[:, a], b[a], cell, eps) for a in range(3))
            g2 = (gz * gz + gy * gy) + gx * gx
            for s in np.unique(s_of):
                if s > 0:
                    g = (s - 1) * cell - eps
                    if g > 0 and g * g > lim:
                        break
                sel = np.nonzero((s_of == s) & ~(g2 > lim))[0]
                if len(sel):
                    best, bt = offer(q, np.unique(np.concatenate([runs[o] for o in sel])), best, bt)
                    lim = min(best, max2) * SLACK
        out_d2[qi], out_tri[qi] = best, bt
    return cpr._finish(pts, V, F, out_d2, out_tri, np.full(Q, np.inf), max_dist)


def brute(V, F, pts, max_dist):
    """The contract with no index: closest_point_ref.brute_force over the triangles whose corners are finite; tri are ids of F."""
    V = np.asarray(V, dtype=np.float64).reshape(-1, 3)
    F = np.asarray(F, dtype=np.int64).reshape(-1, 3)
    keep = np.nonzero(np.isfinite(V[F]).all(axis=(1, 2)))[0] if len(F) else np.zeros(0, np.int64)
    r = cpr.brute_force(V, F[keep], pts, max_dist)
    for k in ("tri", "tri_all"):
        r[k] = np.where(r[k] >= 0, keep[np.maximum(r[k], 0)] if len(keep) else -1, -1).astype(np.int64)
    return r


def families(V, F, X, seed=7, Q=256):
    """closest_point_ref.families over the index's own grid, plus: points 10^3 box sides away; points exactly on vertices and on edge midpoints."""
    G = X["G"]
    V = np.asarray(V, dtype=np.float64).reshape(-1, 3)
    fam = cpr.families(V[np.isfinite(V).all(axis=1)], np.zeros((0, 3), np.int64), G["n"], G["lo"], G["cell"], seed=seed, Q=Q)
    rng = np.random.default_rng(seed + 1)
    side = (G["n"] - 1) * G["cell"]
    u = rng.standard_normal((min(Q, 64), 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    fam["far"] = G["lo"] + 0.5 * side + 1e3 * side * u
    cand = X["cand"]
    if len(cand):
        T = V[F[cand[rng.permutation(len(cand))[:Q]]]]
        fam["centroids"] = T.mean(axis=1)
        fam["on_vertices"] = T[:, 0]
        fam["edge_midpoints"] = 0.5 * (T[:, 0] + T[:, 1])
    if "vertices" in fam:
        fam["vertices"] = fam["vertices"][:: max(1, len(fam["vertices"]) // Q)]
    return fam


def deviation(Xidx, pts):
    """(max, mean) of the distance of pts to the indexed mesh, max_dist = inf."""
    r = answers(Xidx, pts, np.inf)
    d = r["dist"][np.isfinite(r["dist"])]
    return float(d.max()), float(d.mean())
