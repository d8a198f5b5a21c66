"""A numpy restatement of shm_grid_redistance_exact (include/shm_grid.h): the pair distance of csrc/shm_tri_dist.h over a triangle mesh, the minimum per node,
the rounding to the handle's precision, the band and the sign.  It knows nothing of cells, waves or atomics.

Layout: phi is [n^3] in the node order of get_phi (x fastest), viewed as [k, j, i].  X is the mesh as corner positions [nt, 3, 3] (triangle, corner, xyz): of
iso_ref.marching_cubes (`mesh`), or of the device's own fetched mesh (V[F]).  dtype is the precision u is stored in: the arithmetic is float64 (or, for the
audit of the formula itself, any dtype handed to `tri_dist2`), u is rounded to it once.

Culling (`exact_distance`).  Brute force over all triangles (`brute_force`) is what the contract says; `exact_distance` evaluates fewer pairs, by a rule that keeps
every pair that can decide a node's result.  Write D(p, t) for the distance of node p to the axis-aligned bounding box of triangle t, and d(p, t) >= D(p, t)
for its distance to the triangle itself (the triangle lies in its box).  Let ub(p) be the distance of p to the nearest mesh VERTEX: ub(p) >= min_t d(p, t),
since every vertex lies on a triangle.  A pair (p, t) is evaluated iff
    D(p, t) <= lim(p) (1 + 1e-6),     lim(p) = min(ub(p), band).
Proof that this is a superset.  (a) Let t* attain the minimum d* = min_t d(p, t).  Then D(p, t*) <= d* <= ub(p).  If d* <= band the pair (p, t*) is
evaluated and the minimum over the evaluated pairs is d*.  (b) If d* > band (1 + 1e-6) nothing below band (1 + 1e-6) can come out of any pair, so whichever
pairs are evaluated, u = T(sqrt(.)) >= band even after rounding to fp32 (2^-24 relative) and the node is not reached -- the same as by brute force.
(c) For band < d* <= band (1 + 1e-6) the pair (p, t*) has D <= d* <= band (1 + 1e-6) = lim (1 + 1e-6) and is evaluated, as in (a).  The factor 1 + 1e-6 also
covers the rounding of D, ub and the computed d themselves (relative 1e-13 at these grids).  A node with no evaluated pair keeps +inf and is not reached."""
import numpy as np

import iso_ref

SLACK = 1.0 + 1e-6


def _round(a, dtype):
    return np.asarray(a, dtype=np.float64).astype(dtype).astype(np.float64)


def _dot(u, w):
    return (u[..., 0] * w[..., 0] + u[..., 1] * w[..., 1]) + u[..., 2] * w[..., 2]


def _cross(u, w):
    return np.stack([u[..., 1] * w[..., 2] - u[..., 2] * w[..., 1], u[..., 2] * w[..., 0] - u[..., 0] * w[..., 2], u[..., 0] * w[..., 1] - u[..., 1] * w[..., 0]], axis=-1)


def seg_dist2(P, Q):
    e = Q - P
    ee = _dot(e, e)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.where(ee > 0, np.clip(-_dot(P, e) / np.where(ee > 0, ee, 1), 0, 1), 0)
    c = P + t[..., None] * e
    return _dot(c, c)


def tri_dist2(A, B, C):
    """Squared distance from the origin to the triangles (A, B, C), each [..., 3], in the dtype of the inputs: the formula of csrc/shm_tri_dist.h."""
    d2 = np.minimum(np.minimum(seg_dist2(A, B), seg_dist2(B, C)), seg_dist2(C, A))
    N = _cross(B - A, C - A)
    nn = _dot(N, N)
    s = _dot(A, N)
    ok = nn > 0
    nn1 = np.where(ok, nn, 1)
    q = (s / nn1)[..., None] * N
    a, b, c = A - q, B - q, C - q
    ok = ok & (_dot(_cross(b, c), N) >= 0) & (_dot(_cross(c, a), N) >= 0) & (_dot(_cross(a, b), N) >= 0)
    return np.where(ok, np.minimum(d2, s * s / nn1), d2)


def node_positions(n, bbox_min, cell):
    """[3][n]: idx*cell + bbox_min per axis, the isosurface kernels' expression."""
    idx = np.arange(n, dtype=np.float64)
    return [idx * cell + float(bbox_min[a]) for a in range(3)]


def mesh(phi, n, bbox_min, cell, iso):
    """X [nt, 3, 3] of iso_ref.marching_cubes in its own order, under its rule for non-finite nodes: no triangle from a cell with a non-finite corner."""
    P = np.asarray(phi, dtype=np.float64).reshape(-1)
    pts, tris = iso_ref.marching_cubes(P, n, bbox_min, cell, iso, drop_nonfinite=True)
    if not tris:
        return np.zeros((0, 3, 3))
    return np.array([[pts[e] for e in t] for t in tris], dtype=np.float64).reshape(-1, 3, 3)


def _finish(d2, phi, n, iso, band, dtype):
    P = np.asarray(phi, dtype=np.float64).reshape(-1)
    u = _round(np.sqrt(d2), dtype)
    reached = np.isfinite(P) & (u < band)
    s = np.where(P < iso, -1.0, 1.0)
    psi = _round(s * np.where(reached, u, band), dtype)
    psi[~np.isfinite(P)] = np.nan
    info = dict(n_reached=int(reached.sum()), max_abs=float(u[reached].max()) if reached.any() else 0.0, reached=reached, u=u)
    return psi, info


def brute_force_d2(X, n, bbox_min, cell, work=np.float64, chunk=64, nodes=None):
    """min over ALL triangles of d^2 for every node (or for the flat node indices `nodes`), in the arithmetic `work` (np.float64: the contract; np.longdouble:
    the audit of the formula)."""
    px, py, pz = node_positions(n, bbox_min, cell)
    pos = np.stack(np.meshgrid(pz, py, px, indexing="ij")[::-1], axis=-1).reshape(-1, 3)
    if nodes is not None:
        pos = pos[nodes]
    pos = pos.astype(work)
    d2 = np.full(len(pos), np.inf, dtype=work)
    Xw = np.asarray(X, dtype=work)
    for a in range(0, len(Xw), chunk):
        rel = Xw[None, a:a + chunk, :, :] - pos[:, None, None, :]
        d2 = np.minimum(d2, tri_dist2(rel[:, :, 0], rel[:, :, 1], rel[:, :, 2]).min(axis=1))
    return d2


def brute_force(X, phi, n, bbox_min, cell, iso, band, dtype=np.float64, d2=None):
    """Every node against every triangle: (psi, info) of the contract with no cull at all.  d2: a brute_force_d2 of the same mesh, to share between bands."""
    if d2 is None:
        d2 = brute_force_d2(X, n, bbox_min, cell)
    return _finish(np.asarray(d2, dtype=np.float64), phi, n, iso, band, dtype)


def nearest_vertex(X, pos_axes, chunk=256):
    """ub [n, n, n]: the distance of every node to the nearest corner of the mesh (+inf for an empty mesh)."""
    pz, py, px = pos_axes[2], pos_axes[1], pos_axes[0]
    n = len(px)
    ub2 = np.full((n, n, n), np.inf)
    V = np.unique(np.asarray(X, dtype=np.float64).reshape(-1, 3), axis=0)
    for a in range(0, len(V), chunk):
        v = V[a:a + chunk]
        dx2 = (px[None, :] - v[:, 0:1]) ** 2
        dy2 = (py[None, :] - v[:, 1:2]) ** 2
        dz2 = (pz[None, :] - v[:, 2:3]) ** 2
        ub2 = np.minimum(ub2, (dz2[:, :, None, None] + dy2[:, None, :, None] + dx2[:, None, None, :]).min(axis=0))
    return np.sqrt(ub2)


def exact_distance(X, phi, n, bbox_min, cell, iso, band, dtype=np.float64):
    """(psi [n^3] float64 holding dtype values, info): the contract of shm_grid_redistance_exact over the mesh X, with the cull the module docstring proves."""
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3, 3)
    axes = node_positions(n, bbox_min, cell)
    d2 = np.full((n, n, n), np.inf)
    if len(X):
        lim = np.minimum(nearest_vertex(X, axes), band) * SLACK
        lim2 = lim * lim
        lo, hi = X.min(axis=1), X.max(axis=1)
        reach = band * SLACK
        for t in range(len(X)):
            sl, gap2 = [], []
            for a in range(3):
                p = axes[a]
                i0 = int(np.searchsorted(p, lo[t, a] - reach, side="left"))
                i1 = int(np.searchsorted(p, hi[t, a] + reach, side="right"))
                sl.append(slice(i0, i1))
                g = np.maximum(np.maximum(lo[t, a] - p[i0:i1], p[i0:i1] - hi[t, a]), 0.0)
                gap2.append(g * g)
            box = (sl[2], sl[1], sl[0])
            D2 = gap2[2][:, None, None] + gap2[1][None, :, None] + gap2[0][None, None, :]
            kk, jj, ii = np.nonzero(D2 <= lim2[box])
            if not len(kk):
                continue
            kk, jj, ii = kk + sl[2].start, jj + sl[1].start, ii + sl[0].start
            p = np.stack([axes[0][ii], axes[1][jj], axes[2][kk]], axis=-1)
            v = tri_dist2(X[t, 0] - p, X[t, 1] - p, X[t, 2] - p)
            d2[kk, jj, ii] = np.minimum(d2[kk, jj, ii], v)
    psi, info = _finish(d2.reshape(-1), phi, n, iso, band, dtype)
    info["n_triangles"] = len(X)
    return psi, info


def candidate_pairs(phi, n, cell, iso, band):
    """n_candidate_pairs of the header: over the cells that carry a triangle (none with a non-finite corner does), the nodes whose distance to the cell's box,
    in index space, has (gx^2 + gy^2 + gz^2) cell^2 < band^2 (1 + 2^-18)."""
    table, _ = iso_ref._mc_table()
    P = np.asarray(phi, dtype=np.float64).reshape(n, n, n)
    ntri = np.array([len(t) for t in table])[iso_ref.cell_cases(P, iso)] * iso_ref.finite_cells(P)
    ck, cj, ci = np.nonzero(ntri > 0)
    if not len(ck):
        return 0
    cull2 = band * band * (1.0 + 2.0 ** -18) / (cell * cell)
    G = int(np.ceil(band / cell)) + 2
    g = np.arange(G)
    M = ((g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2).astype(np.float64) < cull2).astype(np.int64)
    idx = np.arange(n)

    def hist(c):
        gap = np.maximum(np.maximum(c[:, None] - idx[None, :], idx[None, :] - (c[:, None] + 1)), 0)
        return np.stack([(gap == v).sum(axis=1) for v in range(G)], axis=1).astype(np.int64)   # nodes of the axis per gap value

    return int(np.einsum("cx,cy,cz,xyz->", hist(ci), hist(cj), hist(ck), M))
