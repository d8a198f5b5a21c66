"""Plain-numpy restatement of the connected components of an indexed mesh and of their records (shm_grid_label_mesh_device, shm_grid_isosurface_components,
shm_grid_isosurface_keep_components; include/shm_grid.h states the contract).  Test infrastructure: nothing here is shared with csrc/shm_iso_components.hip.h.

roots():     labels by min-propagation to the fixed point -- every vertex, and the vertex its label names, takes the smallest label among the corners of its
             triangles, and then the label of its label.  A label of v is always an id of v's component that is <= v, so at the fixed point root[v] is the
             smallest vertex id of v's component, as a function of the triangle list alone.
records():   one record per component from a fetched mesh, with the header's fixed-point formulas: float64, one rounding per operation (numpy fuses nothing).
keep_mesh(): the numpy filter the device's compaction is held to."""
from fractions import Fraction

import numpy as np

DTYPE = np.dtype([("first_vertex", "<i8"), ("n_vertices", "<i8"), ("n_triangles", "<i8"), ("area", "<f8"), ("volume", "<f8"),
                  ("lo", "<f8", (3,)), ("hi", "<f8", (3,)), ("touches_box", "<i4"), ("reserved", "<i4")])


def roots(nv, F):
    F = np.asarray(F, dtype=np.int64).reshape(-1, 3)
    r = np.arange(nv, dtype=np.int64)
    while True:
        before = r.copy()
        if len(F):
            L = r[F]
            m = np.repeat(L.min(axis=1), 3)
            np.minimum.at(r, F.reshape(-1), m)   # a vertex takes the smallest label among the corners of its triangles ...
            np.minimum.at(r, L.reshape(-1), m)   # ... and so does the vertex its label names (without this a permuted strip needs one round per triangle)
        while True:                              # the label of the label, to its own fixed point
            j = r[r]
            if np.array_equal(j, r):
                break
            r = j
        if np.array_equal(r, before):
            return r


def roots_bfs(nv, F):
    """The same labels by a breadth-first search over an adjacency list: independent of roots()."""
    adj = [[] for _ in range(nv)]
    for a, b, c in np.asarray(F, dtype=np.int64).reshape(-1, 3):
        adj[a] += [b, c]
        adj[b] += [a, c]
        adj[c] += [a, b]
    r = np.full(nv, -1, dtype=np.int64)
    for s in range(nv):
        if r[s] >= 0:
            continue
        r[s] = s
        front = [s]
        while front:
            nxt = []
            for u in front:
                for w in adj[u]:
                    if r[w] < 0:
                        r[w] = s
                        nxt.append(int(w))
            front = nxt
    return r


def quanta(n, cell):
    return cell * cell * 2.0 ** -32, cell * cell * cell * 2.0 ** -20


def _cross(u, w):
    return np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], axis=1)


def triangle_quanta(V, F, cell, origin):
    """(llrint(A_t / qA), llrint(V_t / qV)) per triangle as int64, V_t taken about `origin`."""
    qA, qV = quanta(0, cell)
    a, b, c = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    nrm = _cross(b - a, c - a)
    At = 0.5 * np.sqrt((nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2])
    o = np.asarray(origin, dtype=np.float64).reshape(-1, 3)
    p, q, r = a - o, b - o, c - o
    m = _cross(q, r)
    Vt = ((p[:, 0] * m[:, 0] + p[:, 1] * m[:, 1]) + p[:, 2] * m[:, 2]) / 6.0
    return np.rint(At / qA).astype(np.int64), np.rint(Vt / qV).astype(np.int64)


def records(V, F, n, bbox_min, cell):
    """(records [nc] of DTYPE ascending in first_vertex, tri_component [nt], vertex_component [nv], area quanta [nc] int64, volume quanta [nc] int64)."""
    V = np.asarray(V, dtype=np.float64).reshape(-1, 3)
    F = np.asarray(F, dtype=np.int64).reshape(-1, 3)
    bbox_min = np.asarray(bbox_min, dtype=np.float64)
    nv = len(V)
    r = roots(nv, F)
    first = np.flatnonzero(r == np.arange(nv))
    vcomp = np.searchsorted(first, r)
    tcomp = vcomp[F[:, 0]] if len(F) else np.zeros(0, dtype=np.int64)
    nc = len(first)
    rec = np.zeros(nc, dtype=DTYPE)
    rec["first_vertex"] = first
    rec["n_vertices"] = np.bincount(vcomp, minlength=nc)
    rec["n_triangles"] = np.bincount(tcomp, minlength=nc)
    qA, qV = quanta(n, cell)
    ia, iv = triangle_quanta(V, F, cell, bbox_min) if len(F) else (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
    sa = np.zeros(nc, dtype=np.int64)
    sv = np.zeros(nc, dtype=np.int64)
    np.add.at(sa, tcomp, ia)
    np.add.at(sv, tcomp, iv)
    rec["area"] = qA * sa.astype(np.float64)
    rec["volume"] = qV * sv.astype(np.float64)
    hi_plane = np.array([(n - 1) * cell + bbox_min[a] for a in range(3)])
    hi_fused = np.array([float(Fraction(n - 1) * Fraction(float(cell)) + Fraction(float(bbox_min[a]))) for a in range(3)])   # the same in one rounding
    touch = ((V == bbox_min[None, :]) | (V == hi_plane[None, :]) | (V == hi_fused[None, :])).any(axis=1)
    for c in range(nc):
        sel = vcomp == c
        rec["lo"][c] = V[sel].min(axis=0)
        rec["hi"][c] = V[sel].max(axis=0)
        rec["touches_box"][c] = int(touch[sel].any())
    return rec, tcomp, vcomp, sa, sv


def keep_mesh(V, F, vcomp, tcomp, mask):
    """The mesh restricted to the components with mask != 0: vertices and triangles in their order, indices renumbered."""
    mask = np.asarray(mask) != 0
    kv = mask[vcomp] if len(vcomp) else np.zeros(0, dtype=bool)
    kt = mask[tcomp] if len(tcomp) else np.zeros(0, dtype=bool)
    newid = np.cumsum(kv) - 1
    return V[kv], newid[F[kt]].astype(np.int64).reshape(-1, 3)


def boundary_edges(F):
    if not len(F):
        return 0
    e = np.sort(np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]]), axis=1)
    _, cnt = np.unique(e, axis=0, return_counts=True)
    return int((cnt == 1).sum())


def largest_mask(rec, keep_largest=None, min_triangles=None):
    """keep_largest components by n_triangles (ties: the smaller first_vertex) among those with at least min_triangles triangles."""
    nc = len(rec)
    mask = np.ones(nc, dtype=bool)
    if min_triangles is not None:
        mask &= rec["n_triangles"] >= min_triangles
    if keep_largest is not None:
        order = sorted(range(nc), key=lambda c: (-int(rec["n_triangles"][c]), int(rec["first_vertex"][c])))
        top = np.zeros(nc, dtype=bool)
        top[order[:keep_largest]] = True
        mask &= top
    return mask
