"""A numpy restatement of shm_grid_closest_point (include/shm_grid.h): for every query the minimum over ALL triangles of the pair distance of csrc/shm_tri_dist.h
(redistance_exact_ref.tri_dist2), the smallest triangle id attaining it, the candidate point of a numpy tri_closest, and the rule answered iff dist < max_dist.
It knows nothing of cells, masks, shells or atomics.  It is fed the device's own fetched mesh (V [nv, 3], F [nt, 3]) and the queries as given.

`brute_force` is the contract as written: every query against every triangle.  `closest` evaluates fewer pairs, by the rule of redistance_exact_ref.exact_distance
moved from nodes to queries: with D(q, t) the distance of q to the axis-aligned bounding box of triangle t (d(q, t) >= D(q, t): the triangle lies in its box) and
ub(q) the distance of q to the nearest corner of the mesh (ub(q) >= min_t d(q, t)), a pair is evaluated iff
    D(q, t) <= min(ub(q), max_dist) (1 + 1e-6) + PAD,    PAD = 1e-9 cell.
It keeps every pair that can decide an answer -- the proof is in redistance_exact_ref's docstring, (a) to (c), word for word -- and the absolute PAD keeps every
triangle within 1e-9 cell of the minimum as well, a thousand times the tolerance 4 TOL under which two triangles count as tied, so the runner-up it reports is the
true one wherever that matters.  tests/test_closest_point.py holds `closest` to `brute_force` bit for bit on the 16^3 goldens without a GPU.

Slivers.  d(q, t) >= D(q, t) is geometry, and tri_dist2 honours it only while its face candidate is refused for a foot outside the triangle.  For a triangle
thinner than 2^-22 cell (`slivers`; csrc/shm_closest_index.h derives the threshold) the inside test is rounding noise and the formula can return the distance to the
triangle's plane from cells away: vertices that coincide up to an ulp, as the device's own arithmetic leaves them where a node sits on the isovalue, do exactly
that.  The contract is the minimum of the formula, whatever it returns, so `closest` (and `shell_walk`) offer every sliver to every query.
tests/golden/closest_on_iso_n20_mesh.npz is such a mesh as the device built it (phi_fields.on_iso at n = 20: 1138 triangles, 284 of them slivers).

`shell_walk` is a third evaluation, written from the rules of csrc/shm_closest_index.h (cell key, Chebyshev shells, grown-box gap, lower bound, limit): a scalar
loop, for the self-check that those rules lose nothing."""
import numpy as np

import redistance_exact_ref as rx

SLACK = 1.0 + 1e-6


def tri_closest(A, B, C):
    """(d2 [...], c [..., 3]): tri_dist2 of the triangles (A, B, C), each [..., 3], and the candidate that attained it -- c = P + t e of the first segment
    among AB, BC, CA with the smallest candidate, or the face's foot where the face candidate is strictly smaller: shm::tri_closest."""
    def seg(P, Q):
        e = Q - P
        ee = rx._dot(e, e)
        with np.errstate(invalid="ignore", divide="ignore"):
            t = np.where(ee > 0, np.clip(-rx._dot(P, e) / np.where(ee > 0, ee, 1), 0, 1), 0)
        c = P + t[..., None] * e
        return rx._dot(c, c), c

    d2, c = seg(A, B)
    for P, Q in ((B, C), (C, A)):
        d, cc = seg(P, Q)
        take = d < d2
        d2 = np.where(take, d, d2)
        c = np.where(take[..., None], cc, c)
    N = rx._cross(B - A, C - A)
    nn = rx._dot(N, N)
    s = rx._dot(A, N)
    ok = nn > 0
    nn1 = np.where(ok, nn, 1)
    q = (s / nn1)[..., None] * N
    a, b, cc = A - q, B - q, C - q
    ok = ok & (rx._dot(rx._cross(b, cc), N) >= 0) & (rx._dot(rx._cross(cc, a), N) >= 0) & (rx._dot(rx._cross(a, b), N) >= 0)
    f = s * s / nn1
    take = ok & (f < d2)
    return np.where(take, f, d2), np.where(take[..., None], q, c)


def slivers(V, F, cell):
    """[nt] bool: 0 < nn < (2^-22 cell)^2 longest edge^2, cp_is_sliver of csrc/shm_closest_index.h."""
    X = V[F]
    ab, ac, bc = X[:, 1] - X[:, 0], X[:, 2] - X[:, 0], X[:, 2] - X[:, 1]
    N = rx._cross(ab, ac)
    nn = rx._dot(N, N)
    emax = np.maximum(np.maximum(rx._dot(ab, ab), rx._dot(ac, ac)), rx._dot(bc, bc))
    hmin = cell * 2.0 ** -22
    return (nn > 0) & (nn < hmin * hmin * emax)


def pair(V, F, pts, tri):
    """(d2 [Q], c [Q, 3]) of query q against the one triangle tri[q]."""
    X = V[F[tri]] - pts[:, None, :]
    return tri_closest(X[:, 0], X[:, 1], X[:, 2])


def _finish(pts, V, F, d2, tri, second, max_dist):
    Q = len(pts)
    dist = np.sqrt(d2)
    finite = np.isfinite(pts).all(axis=1)
    ans = finite & (tri >= 0) & (dist < max_dist)
    cp = np.full((Q, 3), np.nan)
    if ans.any():
        _, c = pair(V, F, pts[ans], tri[ans])
        cp[ans] = pts[ans] + c
    out = dict(d2=d2, dist_all=dist, tri_all=tri, second=np.sqrt(second), answered=ans, n_answered=int(ans.sum()))
    out["dist"] = np.where(ans, dist, np.nan)
    out["tri"] = np.where(ans, tri, -1).astype(np.int64)
    out["cp"] = cp
    return out


def restrict(r, V, F, pts, max_dist):
    """The answers at a smaller max_dist from those at a larger one: the minimum and its triangle do not depend on max_dist, only what counts as answered
    does.  (`closest` evaluated every pair that can decide an answer below its own max_dist, so below the smaller one as well.)"""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    return _finish(pts, V, F, r["d2"], r["tri_all"], r["second"] ** 2, max_dist)


def brute_force(V, F, pts, max_dist, pairs_per_chunk=1 << 18):
    """The contract with no cull: dict(dist, cp, tri, answered, n_answered; d2 and dist_all before the max_dist rule; second: the smallest distance among the
    OTHER triangles).  Queries with a non-finite coordinate are unanswered."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    Q, nt = len(pts), len(F)
    d2 = np.full(Q, np.inf)
    tri = np.full(Q, -1, dtype=np.int64)
    second = np.full(Q, np.inf)
    finite = np.isfinite(pts).all(axis=1)
    if nt:
        X = V[F]
        step = max(1, pairs_per_chunk // nt)
        idx = np.nonzero(finite)[0]
        for a in range(0, len(idx), step):
            sel = idx[a:a + step]
            rel = X[None, :, :, :] - pts[sel][:, None, None, :]
            m = rx.tri_dist2(rel[:, :, 0], rel[:, :, 1], rel[:, :, 2])
            t = m.argmin(axis=1)               # the first, so the smallest id, among equal minima
            d2[sel] = m[np.arange(len(sel)), t]
            tri[sel] = t
            if nt > 1:
                m[np.arange(len(sel)), t] = np.inf
                second[sel] = m.min(axis=1)
    return _finish(pts, V, F, d2, tri, second, max_dist)


def closest(V, F, pts, max_dist, cell, q_chunk=128):
    """brute_force's answers from fewer pairs (module docstring).  `second` is exact wherever it lies within 1e-9 cell of the minimum, else a lower bound of +inf's kind:
    the smallest distance among the other EVALUATED triangles."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    Q, nt = len(pts), len(F)
    d2 = np.full(Q, np.inf)
    tri = np.full(Q, -1, dtype=np.int64)
    second = np.full(Q, np.inf)
    finite = np.isfinite(pts).all(axis=1)
    if nt:
        X = V[F]
        lo, hi = X.min(axis=1), X.max(axis=1)
        corners = np.unique(X.reshape(-1, 3), axis=0)
        thin = slivers(V, F, cell)
        idx = np.nonzero(finite)[0]
        for a in range(0, len(idx), q_chunk):
            sel = idx[a:a + q_chunk]
            p = pts[sel]
            ub = np.sqrt(((corners[None, :, :] - p[:, None, :]) ** 2).sum(axis=2).min(axis=1))
            lim = np.minimum(ub, max_dist) * SLACK + 1e-9 * cell
            gap = np.maximum(np.maximum(lo[None, :, :] - p[:, None, :], p[:, None, :] - hi[None, :, :]), 0.0)
            qi, ti = np.nonzero(((gap ** 2).sum(axis=2) <= (lim * lim)[:, None]) | thin[None, :])     # row-major: ti ascends within a query
            if not len(qi):
                continue
            rel = X[ti] - p[qi][:, None, :]
            v = rx.tri_dist2(rel[:, 0], rel[:, 1], rel[:, 2])
            best = np.full(len(sel), np.inf)
            np.minimum.at(best, qi, v)
            hit = v == best[qi]
            first = np.nonzero(hit)[0][np.unique(qi[hit], return_index=True)[1]]   # the first pair of each query that attains its minimum
            got = qi[first]
            d2[sel[got]] = v[first]
            tri[sel[got]] = ti[first]
            v2 = v.copy()
            v2[first] = np.inf
            sec = np.full(len(sel), np.inf)
            np.minimum.at(sec, qi, v2)
            second[sel] = sec
    return _finish(pts, V, F, d2, tri, second, max_dist)


# ---- the rules of csrc/shm_closest_index.h, as a scalar loop ------------------------------------------------------------------------------------------------------
def _cell_axis(x, b, cell, n):
    f = np.floor((x - b) / cell)
    return 0 if f < 0 else (n - 2 if f > n - 2 else int(f))


def _gap(x, i, b, cell, eps):
    lo, hi = i * cell + b, (i + 1) * cell + b
    g = max(lo - x, x - hi) - eps
    return g if g > 0 else 0.0


def shell_walk(V, F, pts, max_dist, n, bbox_min, cell):
    """(d2 [Q], tri [Q]) before the max_dist rule turns them into answers (inf / -1 where the walk met no triangle below the limit)."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    X = V[F]
    eps, slack = cell * 2.0 ** -16, 1.0 + 2.0 ** -18
    mid = 0.5 * (X.min(axis=1) + X.max(axis=1))
    thin = slivers(V, F, cell)
    loose = [int(t) for t in np.nonzero(thin)[0]]
    cells = {}
    for t in np.nonzero(~thin)[0]:
        t = int(t)
        key = tuple(_cell_axis(mid[t, a], bbox_min[a], cell, n) for a in range(3))
        cells.setdefault(key, []).append(t)
    out_d2, out_tri = np.full(len(pts), np.inf), np.full(len(pts), -1, dtype=np.int64)
    max2 = max_dist * max_dist
    for qi, q in enumerate(pts):
        if not np.isfinite(q).all() or not len(F):
            continue
        c0 = [_cell_axis(q[a], bbox_min[a], cell, n) for a in range(3)]
        best, bt, lim = np.inf, -1, max2 * slack
        if loose:
            rel = X[loose] - q
            for t, d in zip(loose, rx.tri_dist2(rel[:, 0], rel[:, 1], rel[:, 2])):
                if d < best or (d == best and t < bt):
                    best, bt = float(d), t
                    lim = min(best, max2) * slack
        out_d2[qi], out_tri[qi] = best, bt
        if sum(_gap(q[a], c0[a], bbox_min[a], cell, eps) ** 2 for a in range(3)) > lim:
            continue
        smax = max(max(c0[a], n - 2 - c0[a]) for a in range(3))
        for s in range(smax + 1):
            if s > 0:
                g = (s - 1) * cell - eps
                if g > 0 and g * g > lim:
                    break
            for k in range(max(c0[2] - s, 0), min(c0[2] + s, n - 2) + 1):
                for j in range(max(c0[1] - s, 0), min(c0[1] + s, n - 2) + 1):
                    full = max(abs(k - c0[2]), abs(j - c0[1])) == s
                    xs = range(max(c0[0] - s, 0), min(c0[0] + s, n - 2) + 1) if full else [x for x in (c0[0] - s, c0[0] + s) if 0 <= x <= n - 2]
                    for i in xs:
                        tris = cells.get((i, j, k))
                        if not tris:
                            continue
                        g2 = _gap(q[2], k, bbox_min[2], cell, eps) ** 2 + _gap(q[1], j, bbox_min[1], cell, eps) ** 2 + _gap(q[0], i, bbox_min[0], cell, eps) ** 2
                        if g2 > lim:
                            continue
                        rel = X[tris] - q
                        v = rx.tri_dist2(rel[:, 0], rel[:, 1], rel[:, 2])
                        for t, d in zip(tris, v):
                            if d < best or (d == best and t < bt):
                                best, bt = float(d), t
                                lim = min(best, max2) * slack
        out_d2[qi], out_tri[qi] = best, bt
    return out_d2, out_tri


# ---- query families ---------------------------------------------------------------------------------------------------------------------------------------------------
def families(V, F, n, bbox_min, cell, seed=7, Q=1024):
    """The query sets of tests/test_closest_point.py as a dict name -> [q, 3]; a function of the mesh, the grid and the seed."""
    rng = np.random.default_rng(seed)
    bb = np.asarray(bbox_min, dtype=np.float64)
    L = (n - 1) * cell
    out = {}
    out["uniform"] = bb + rng.random((Q, 3)) * L
    out["grown"] = bb - 3 * cell + rng.random((Q, 3)) * (L + 6 * cell)
    if len(V):
        out["vertices"] = V.copy()
    if len(F):
        ctr = V[F].mean(axis=1)
        out["centroids"] = ctr[rng.permutation(len(ctr))[:Q]]
    # points exactly on cell faces, edges and corners (1, 2 or 3 coordinates on a node plane), the upper box faces included
    idx = rng.integers(0, n, (Q, 3)).astype(np.float64)
    frac = rng.random((Q, 3))
    on = rng.integers(1, 4, Q)[:, None] > np.argsort(rng.random((Q, 3)), axis=1)      # 1, 2 or 3 axes snapped, chosen at random
    u = np.where(on, idx, np.minimum(idx + frac, n - 1.0))
    u[: Q // 8, 0] = n - 1.0                                                            # on the upper x face
    u[Q // 8: Q // 4, 2] = n - 1.0                                                      # on the upper z face
    out["lattice"] = u * cell + bb
    bad = bb + rng.random((16, 3)) * L
    bad[0, 0], bad[1, 1], bad[2, 2] = np.nan, np.inf, -np.inf
    bad[3] = np.nan
    bad[4, 0], bad[4, 2] = np.inf, np.nan
    out["nonfinite"] = bad
    return out
