"""The numpy restatement of shm_grid_mesh_raycast's contract (include/shm_grid.h; the rule is csrc/shm_ray_tri.h): brute force over all triangles, float64, one
operation per numpy call so that nothing is contracted, sums of three terms taken (x + y) + z.  Test infrastructure, no device code.

    cast(V, F, origins, dirs, t_min, t_max)   the answer for arbitrary rays: t, tri, bary, count, hit
    axis_cast(V, F, coords, axis, sense)      the same answer for the rays from every node of a grid along +-axis, t in [0, inf): for such rays Sx = Sy = 0,
                                              the sheared corner is P[kx] - o[kx] exactly and the edge functions do not depend on where along its grid line
                                              the origin sits, so they are evaluated once per line.  The same operations on the same values as cast -- which
                                              tests/test_mesh_raycast.py asserts on a sample -- n times cheaper.
    sphere / two_spheres                      closed-form fields whose contour is closed inside the box and that put no node on the isovalue 0
"""
import numpy as np


def _sign_adjusted(e, Px, Py, Qx, Qy):
    """The adjusted sign of the edge function e of the directed edge P -> Q: sign(e), else sign(Qy - Py), else sign(Px - Qx), else 0."""
    s = np.sign(e)
    s = np.where(s == 0, np.sign(Qy - Py), s)
    return np.where(s == 0, np.sign(Px - Qx), s)


def setup(d):
    """kx, ky, kz [Q] and Sx, Sy, Sz [Q] of directions d [Q, 3] (finite, not zero)."""
    a = np.abs(d)
    kz = np.zeros(len(d), dtype=np.int64)
    m = a[:, 0].copy()
    up = a[:, 1] > m
    kz[up], m[up] = 1, a[up, 1]
    kz[a[:, 2] > m] = 2
    kx, ky = (kz + 1) % 3, (kz + 2) % 3
    rows = np.arange(len(d))
    dz = d[rows, kz]
    neg = dz < 0
    kx, ky = np.where(neg, ky, kx), np.where(neg, kx, ky)
    return kx, ky, kz, d[rows, kx] / dz, d[rows, ky] / dz, 1.0 / dz


def valid(o, d, t_min, t_max):
    return np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1) & (d != 0).any(axis=1) & bool(t_min <= t_max)


def pairs(V, F, o, d, t_min, t_max):
    """The rule for every (ray, triangle) pair: (hit [Q, T] bool, t, u, v, det [Q, T]); o, d valid."""
    kx, ky, kz, Sx, Sy, Sz = setup(d)
    perm = np.stack([kx, ky, kz], axis=1)[:, None, :]
    sh = []
    for c in range(3):
        P = V[F[:, c]][None, :, :] - o[:, None, :]
        P = np.take_along_axis(P, perm, axis=2)
        pz = P[:, :, 2]
        sx = Sx[:, None] * pz
        sy = Sy[:, None] * pz
        sh.append((P[:, :, 0] - sx, P[:, :, 1] - sy, Sz[:, None] * pz))
    (Ax, Ay, Az), (Bx, By, Bz), (Cx, Cy, Cz) = sh
    with np.errstate(all="ignore"):
        U = Cx * By - Cy * Bx
        Vv = Ax * Cy - Ay * Cx
        W = Bx * Ay - By * Ax
        su, sv, sw = _sign_adjusted(U, Bx, By, Cx, Cy), _sign_adjusted(Vv, Cx, Cy, Ax, Ay), _sign_adjusted(W, Ax, Ay, Bx, By)
        det = (U + Vv) + W
        t = ((U * Az + Vv * Bz) + W * Cz) / det
        hit = (su != 0) & (su == sv) & (su == sw) & (det != 0) & (t >= t_min) & (t <= t_max)
        return hit, t, Vv / det, W / det, det


def cast(V, F, origins, dirs, t_min=0.0, t_max=np.inf, budget=1 << 21):
    """The answer, brute force: dict of t [Q] (NaN for a miss), tri [Q] int64 (-1), bary [Q, 2] (NaN), count [Q] int32, hit [Q] bool, n_hits."""
    V, F = np.asarray(V, dtype=np.float64), np.asarray(F, dtype=np.int64).reshape(-1, 3)
    o, d = np.asarray(origins, dtype=np.float64).reshape(-1, 3), np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    Q, T = len(o), len(F)
    out = dict(t=np.full(Q, np.nan), tri=np.full(Q, -1, dtype=np.int64), bary=np.full((Q, 2), np.nan), count=np.zeros(Q, dtype=np.int32))
    ok = np.flatnonzero(valid(o, d, t_min, t_max)) if T else np.zeros(0, dtype=np.int64)
    step = max(1, budget // max(T, 1))
    for a in range(0, len(ok), step):
        q = ok[a:a + step]
        hit, t, u, v, _ = pairs(V, F, o[q], d[q], t_min, t_max)
        tt = np.where(hit, t, np.inf)
        best = tt.argmin(axis=1)                       # the first, that is the smallest id, among equal minima
        rows = np.arange(len(q))
        any_hit = hit.any(axis=1)
        out["count"][q] = hit.sum(axis=1)
        out["t"][q] = np.where(any_hit, tt[rows, best], np.nan)
        out["tri"][q] = np.where(any_hit, best, -1)
        out["bary"][q, 0] = np.where(any_hit, u[rows, best], np.nan)
        out["bary"][q, 1] = np.where(any_hit, v[rows, best], np.nan)
    out["hit"] = out["tri"] >= 0
    out["n_hits"] = int(out["hit"].sum())
    return out


def node_coords(n, bbox_min, cell):
    """[3][n]: the node coordinates i cell + bbox_min, as every test builds its node origins."""
    return [np.arange(n, dtype=np.float64) * cell + float(bbox_min[a]) for a in range(3)]


def node_rays(coords, axis, sense):
    """(origins [n^3, 3] in get_phi's node order, dirs [n^3, 3]) of the rays axis_cast answers."""
    z, y, x = np.meshgrid(coords[2], coords[1], coords[0], indexing="ij")
    o = np.stack([x, y, z], axis=-1).reshape(-1, 3)
    d = np.zeros_like(o)
    d[:, axis] = float(sense)
    return o, d


def axis_cast(V, F, coords, axis, sense, budget=1 << 21):
    """cast() for node_rays(coords, axis, sense) with t in [0, inf): dict of t, tri, bary, count in get_phi's node order (x fastest)."""
    V, F = np.asarray(V, dtype=np.float64), np.asarray(F, dtype=np.int64).reshape(-1, 3)
    n = len(coords[0])
    kz = axis
    kx, ky = ((kz + 1) % 3, (kz + 2) % 3) if sense > 0 else ((kz + 2) % 3, (kz + 1) % 3)
    Sz = 1.0 / float(sense)
    ox, oy = np.meshgrid(coords[kx], coords[ky], indexing="ij")        # one line of origins per (index along kx, index along ky)
    ox, oy = ox.reshape(-1), oy.reshape(-1)
    lx, ly = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    lx, ly = lx.reshape(-1), ly.reshape(-1)
    T = len(F)
    t_best = np.full((n * n, n), np.inf)
    tri_best = np.full((n * n, n), np.iinfo(np.int64).max, dtype=np.int64)
    u_best, v_best = np.full((n * n, n), np.nan), np.full((n * n, n), np.nan)
    count = np.zeros((n * n, n), dtype=np.int32)
    step = max(1, budget // max(T, 1))
    for a in range(0, n * n if T else 0, step):
        L = slice(a, a + step)
        c = [(V[F[:, k], kx][None, :] - ox[L, None], V[F[:, k], ky][None, :] - oy[L, None]) for k in range(3)]
        (Ax, Ay), (Bx, By), (Cx, Cy) = c
        U = Cx * By - Cy * Bx
        Vv = Ax * Cy - Ay * Cx
        W = Bx * Ay - By * Ax
        su, sv, sw = _sign_adjusted(U, Bx, By, Cx, Cy), _sign_adjusted(Vv, Cx, Cy, Ax, Ay), _sign_adjusted(W, Ax, Ay, Bx, By)
        det = (U + Vv) + W
        line, tri = np.nonzero((su != 0) & (su == sv) & (su == sw) & (det != 0))      # ascending (line, tri)
        if not len(line):
            continue
        U, Vv, W, det = U[line, tri], Vv[line, tri], W[line, tri], det[line, tri]
        line = line + a
        z = [Sz * (V[F[tri, k], kz][:, None] - coords[kz][None, :]) for k in range(3)]     # [pairs, n]: the corners' levels seen from every origin of the line
        t = ((U[:, None] * z[0] + Vv[:, None] * z[1]) + W[:, None] * z[2]) / det[:, None]
        hit = t >= 0.0
        for m in range(n):
            h = hit[:, m]
            np.add.at(count[:, m], line[h], 1)
            np.minimum.at(t_best[:, m], line[h], t[h, m])
        for m in range(n):
            h = hit[:, m] & (t[:, m] == t_best[line, m])
            np.minimum.at(tri_best[:, m], line[h], tri[h])
            first = h & (tri == tri_best[line, m])
            u_best[line[first], m] = (Vv / det)[first]
            v_best[line[first], m] = (W / det)[first]
    # from (line, index along the axis) to get_phi's order
    idx = [None, None, None]
    idx[kx], idx[ky], idx[kz] = lx[:, None], ly[:, None], np.arange(n)[None, :]
    g = (idx[0] + n * (idx[1] + n * idx[2])).reshape(-1)
    hitn = np.isfinite(t_best).reshape(-1)
    out = dict(t=np.empty(n ** 3), tri=np.empty(n ** 3, dtype=np.int64), bary=np.empty((n ** 3, 2)), count=np.empty(n ** 3, dtype=np.int32))
    out["t"][g] = np.where(hitn, t_best.reshape(-1), np.nan)
    out["tri"][g] = np.where(hitn, tri_best.reshape(-1), -1)
    out["bary"][g, 0], out["bary"][g, 1] = u_best.reshape(-1), v_best.reshape(-1)
    out["count"][g] = count.reshape(-1)
    out["hit"] = out["tri"] >= 0
    out["n_hits"] = int(out["hit"].sum())
    return out


# ---- fields -----------------------------------------------------------------------------------------------------------------------------------------------------------
def _grid(n):
    k, j, i = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    return i, j, k


def sphere(n, centre=None, radius=None):
    """|u - centre| - radius in index space, n^3 values in get_phi's order.  The default centre is off every grid plane and symmetry plane by irrational-looking
    amounts and the radius leaves two cells to the box, so the contour at 0 is one closed surface; tests assert that no node equals 0."""
    c = centre if centre is not None else (0.5 * (n - 1) + 0.137, 0.5 * (n - 1) - 0.291, 0.5 * (n - 1) + 0.0731)
    r = radius if radius is not None else 0.5 * (n - 1) - 2.317
    i, j, k = _grid(n)
    return (np.sqrt((i - c[0]) ** 2 + (j - c[1]) ** 2 + (k - c[2]) ** 2) - r).reshape(-1)


def two_spheres(n):
    """The union of two disjoint spheres (min of the two fields): two closed components, rays along x and the diagonal axes cross up to four sheets."""
    m = 0.5 * (n - 1)
    r = 0.21 * (n - 1)
    a = sphere(n, (m - 0.24 * (n - 1) + 0.137, m - 0.291, m + 0.0731), r)
    b = sphere(n, (m + 0.25 * (n - 1) + 0.061, m + 0.173, m - 0.219), r * 0.93)
    return np.minimum(a, b)


def indexed_mesh(phi, n, bbox_min, cell, iso=0.0):
    """(V [nv, 3], F [nt, 3]) of tests/iso_ref.py's marching cubes, welded by edge key."""
    import iso_ref
    pts, tris = iso_ref.marching_cubes(np.asarray(phi, dtype=np.float64), n, np.asarray(bbox_min, dtype=np.float64), cell, iso)
    keys = sorted(pts)
    index = {k: a for a, k in enumerate(keys)}
    V = np.array([pts[k] for k in keys], dtype=np.float64).reshape(-1, 3)
    F = np.array([[index[k] for k in t] for t in tris], dtype=np.int64).reshape(-1, 3)
    return V, F


def inside_nodes(phi, iso=0.0):
    return np.asarray(phi) < iso


# ---- seeded ray families ----------------------------------------------------------------------------------------------------------------------------------------------
def families(V, F, n, bbox_min, cell, seed=7, Q=96):
    """dict name -> (origins [q, 3], dirs [q, 3]), a function of its arguments alone: rays from inside the box and from around it, from 10^3 and 10^6 box sides
    away, with d far from unit length, with one and two zero components (origins in general position and on grid planes / lines), aimed at the mesh's own
    vertices and edge midpoints, and along the box diagonals through nodes."""
    rng = np.random.default_rng(seed)
    bb = np.asarray(bbox_min, dtype=np.float64)
    side = (n - 1) * cell
    inside = lambda q: bb + rng.random((q, 3)) * side       # noqa: E731
    unit = lambda q: (lambda g: g / np.sqrt((g * g).sum(axis=1))[:, None])(rng.normal(size=(q, 3)))     # noqa: E731
    fam = {}
    fam["inside"] = (inside(Q), unit(Q))
    tgt = inside(Q)
    org = bb + (rng.random((Q, 3)) * 3.0 - 1.0) * side
    fam["around"] = (org, tgt - org)
    for name, far in (("far_1e3", 1e3), ("far_1e6", 1e6)):
        tgt, u = inside(Q), unit(Q)
        fam[name] = (tgt - u * (far * side), u * rng.choice([1.0, 0.37, 12.5], size=(Q, 1)))
    o, u = inside(Q), unit(Q)
    fam["unnormalised"] = (o, u * rng.choice([1e-3, 1e3, 3.7e-7, 2.9e5], size=(Q, 1)))
    o, u = inside(Q), unit(Q)
    u[np.arange(Q), rng.integers(0, 3, Q)] = 0.0
    fam["one_zero"] = (o, u)
    o = inside(Q)
    u = np.zeros((Q, 3))
    u[np.arange(Q), rng.integers(0, 3, Q)] = rng.choice([1.0, -1.0, 0.25, -3.0], size=Q)
    fam["two_zeros"] = (o, u)
    # on grid planes and grid lines, direction inside them
    nodes = bb + rng.integers(0, n, (Q, 3)) * cell
    o, u = inside(Q), unit(Q)
    a = rng.integers(0, 3, Q)
    o[np.arange(Q), a] = nodes[np.arange(Q), a]
    u[np.arange(Q), a] = 0.0
    fam["in_grid_plane"] = (o, u)
    u = np.zeros((Q, 3))
    u[np.arange(Q), a] = rng.choice([1.0, -1.0], size=Q)
    o = nodes.copy()
    o[np.arange(Q), a] = inside(Q)[np.arange(Q), a]
    fam["along_grid_line"] = (o, u)
    fam["node_diagonals"] = (nodes, rng.choice([1.0, -1.0], size=(Q, 3)))
    if len(F):
        t = rng.integers(0, len(F), Q)
        o = inside(Q)
        fam["at_vertices"] = (o, V[F[t, rng.integers(0, 3, Q)]] - o)
        o = inside(Q)
        fam["at_edge_midpoints"] = (o, 0.5 * (V[F[t, 0]] + V[F[t, 1]]) - o)
        o = inside(Q)
        fam["at_centroids"] = (o, (V[F[t, 0]] + V[F[t, 1]] + V[F[t, 2]]) / 3.0 - o)
    return fam


def join(fam):
    return np.concatenate([v[0] for v in fam.values()]), np.concatenate([v[1] for v in fam.values()])
