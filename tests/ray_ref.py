"""A numpy restatement of shm_grid_raycast (include/shm_grid.h) that shares nothing with the kernel's traversal: no bricks, no DDA, no stepping.

Per ray: clip to the box; collect the parameter of EVERY grid plane strictly inside the clipped interval and sort; for each consecutive pair take the cell of
the midpoint, clip(floor((p - bbox_min) / cell), 0, n-2); in that cell do the corner test, form the cubic of f along the ray, split at its interior extrema
and bisect the first bracketing piece on trilinear values nested as tests/test_sample.py's eval_ref nests them.  Vectorised over (ray, interval) pairs.

Every float in it has the dtype of the `dtype` argument, so the same code runs in float64 and in x87 long double (the stability test compares the two)."""
import numpy as np


def _trilinear(V, u, dt):
    """V: [m, 8] corners in the order 000, 100, 010, 110, 001, 101, 011, 111 (x fastest); u: [m, 3] local coordinates."""
    one = dt(1)
    tx, ty, tz = u[:, 0], u[:, 1], u[:, 2]
    v00 = V[:, 0] * (one - tx) + V[:, 1] * tx
    v01 = V[:, 4] * (one - tx) + V[:, 5] * tx
    v10 = V[:, 2] * (one - tx) + V[:, 3] * tx
    v11 = V[:, 6] * (one - tx) + V[:, 7] * tx
    v0 = v00 * (one - ty) + v10 * ty
    v1 = v01 * (one - ty) + v11 * ty
    return v0 * (one - tz) + v1 * tz, (v00, v01, v10, v11, v0, v1)


def _gradient(V, u, h, dt):
    one = dt(1)
    ty, tz = u[:, 1], u[:, 2]
    _, (v00, v01, v10, v11, v0, v1) = _trilinear(V, u, dt)
    d0 = (V[:, 1] - V[:, 0]) * (one - ty) + (V[:, 3] - V[:, 2]) * ty
    d1 = (V[:, 5] - V[:, 4]) * (one - ty) + (V[:, 7] - V[:, 6]) * ty
    return np.stack([(d0 * (one - tz) + d1 * tz) / h, ((v10 - v00) * (one - tz) + (v11 - v01) * tz) / h, (v1 - v0) / h], axis=1)


def raycast_ref(phi, n, bbox_min, cell, origins, dirs, iso=0.0, t_min=0.0, t_max=np.inf, dtype=np.float64, chunk=4000):
    """Returns dict(t [Q], grad [Q, 3], cell [Q, 3] (the restatement's cell at the hit, -1 without one), gap [Q], fprime [Q]).
    gap: the smaller of the smallest |f| over the piece end points examined (up to and including the hit's cell) and |f'(t)| cell / |d| at a hit;
    +inf for a ray that examined nothing."""
    dt = np.dtype(dtype).type
    O = np.asarray(origins, dtype=np.float64).reshape(-1, 3)
    D = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    Q = len(O)
    out = dict(t=np.full(Q, np.nan, dtype=dtype), grad=np.full((Q, 3), np.nan, dtype=dtype), cell=np.full((Q, 3), -1, dtype=np.int64),
               gap=np.full(Q, np.inf, dtype=dtype), fprime=np.full(Q, np.nan, dtype=dtype))
    for q0 in range(0, Q, chunk):
        sl = slice(q0, min(Q, q0 + chunk))
        r = _raycast_chunk(np.asarray(phi, dtype=np.float64).astype(dtype).reshape(n, n, n), n, np.asarray(bbox_min, dtype=np.float64).astype(dtype), dt(cell),
                           O[sl].astype(dtype), D[sl].astype(dtype), dt(iso), dt(t_min), dt(t_max), dt)
        for k in out:
            out[k][sl] = r[k]
    return out


def _raycast_chunk(U, n, b, h, O, D, iso, t_min, t_max, dt):
    R = len(O)
    dtype = O.dtype
    res = dict(t=np.full(R, np.nan, dtype=dtype), grad=np.full((R, 3), np.nan, dtype=dtype), cell=np.full((R, 3), -1, dtype=np.int64),
               gap=np.full(R, np.inf, dtype=dtype), fprime=np.full(R, np.nan, dtype=dtype))
    if R == 0:
        return res
    hi = dt(n - 1) * h + b
    with np.errstate(all="ignore"):
        # ---- 1. clip
        ok = np.isfinite(O).all(1) & np.isfinite(D).all(1) & (D != 0).any(1) & bool(t_min <= t_max)
        t0 = np.full(R, t_min, dtype=dtype)
        t1 = np.full(R, t_max, dtype=dtype)
        for a in range(3):
            z = D[:, a] == 0
            ok &= ~z | ((O[:, a] >= b[a]) & (O[:, a] <= hi[a]))
            ta = (b[a] - O[:, a]) / D[:, a]
            tb = (hi[a] - O[:, a]) / D[:, a]
            t0 = np.where(z, t0, np.maximum(t0, np.minimum(ta, tb)))
            t1 = np.where(z, t1, np.minimum(t1, np.maximum(ta, tb)))
        ok &= (t0 <= t1) & np.isfinite(t0)
        rows = np.nonzero(ok)[0]
        if len(rows) == 0:
            return res
        O, D, t0, t1 = O[rows], D[rows], t0[rows], t1[rows]
        m = len(rows)
        # ---- 2. every grid plane strictly inside (t0, t1); the others collapse onto t1
        p = np.arange(n).astype(dtype)
        T = [t0[:, None], t1[:, None]]
        for a in range(3):
            tp = ((p[None, :] * h + b[a]) - O[:, a:a + 1]) / D[:, a:a + 1]
            inside = (tp > t0[:, None]) & (tp < t1[:, None])
            T.append(np.where(inside, tp, t1[:, None]))
        T = np.sort(np.concatenate(T, axis=1), axis=1)
        ta, tb = T[:, :-1], T[:, 1:]
        keep = tb > ta
        keep[:, 0] = True   # (a ray that only touches the box: the single interval [t0, t0])
        ri, ii = np.nonzero(keep)   # row-major: the intervals of a ray stay in order
        ta, tb = ta[ri, ii], tb[ri, ii]
        # ---- 3. the cell of the midpoint
        tm = ta + (tb - ta) / dt(2)
        pm = O[ri] + tm[:, None] * D[ri]
        idx = np.clip(np.floor((pm - b) / h), 0, n - 2).astype(np.int64)
        i, j, k = idx[:, 0], idx[:, 1], idx[:, 2]
        V = np.stack([U[k, j, i], U[k, j, i + 1], U[k, j + 1, i], U[k, j + 1, i + 1], U[k + 1, j, i], U[k + 1, j, i + 1], U[k + 1, j + 1, i], U[k + 1, j + 1, i + 1]], axis=1)
        # ---- 4. corner test: all finite and not strictly on one side
        live = np.isfinite(V).all(1) & (V.min(1) <= iso) & (V.max(1) >= iso)
        V = V - iso   # f is the trilinear interpolant of (corner - iso): the weights sum to 1, and near the surface the small differences keep their bits
        ri, ta, tb, idx, V = ri[live], ta[live], tb[live], idx[live], V[live]
        if len(ri) == 0:
            return res
        o, d = O[ri], D[ri]
        p0 = idx.astype(dtype) * h + b

        # on an axis the ray does not move along, an origin that is exactly the position of the cell's upper plane has weight 1 exactly (include/shm_grid.h:
        # eval_ref's rule for the upper faces of the box, kept for every plane -- floor() may name the cell below a node's own rounded position)
        snap = (d == 0) & (o == (idx + 1).astype(dtype) * h + b)

        rel = o - p0   # the origin relative to the cell's corner first: t then resolves the position to an ulp of the cell, not of the coordinate

        def local(t):
            return np.where(snap, dt(1), (rel + t[:, None] * d) / h)

        def f(t):
            return _trilinear(V, local(t), dt)[0]

        # the cubic of f in s = t - ta through u = A + B s; its derivative c1 + 2 c2 s + 3 c3 s^2
        A = local(ta)
        B = d / h
        kx, ky, kz = V[:, 1] - V[:, 0], V[:, 2] - V[:, 0], V[:, 4] - V[:, 0]
        kxy, kxz, kyz = (V[:, 3] - V[:, 2]) - kx, (V[:, 5] - V[:, 4]) - kx, (V[:, 6] - V[:, 4]) - ky
        kxyz = ((V[:, 7] - V[:, 6]) - (V[:, 5] - V[:, 4])) - kxy
        Ax, Ay, Az, Bx, By, Bz = A[:, 0], A[:, 1], A[:, 2], B[:, 0], B[:, 1], B[:, 2]
        c3 = kxyz * Bx * By * Bz
        c2 = kxy * Bx * By + kxz * Bx * Bz + kyz * By * Bz + kxyz * (Ax * By * Bz + Bx * Ay * Bz + Bx * By * Az)
        c1 = (kx * Bx + ky * By + kz * Bz + kxy * (Ax * By + Bx * Ay) + kxz * (Ax * Bz + Bx * Az) + kyz * (Ay * Bz + By * Az)
              + kxyz * (Ax * Ay * Bz + Ax * By * Az + Bx * Ay * Az))
        qa, qb, qc = dt(3) * c3, dt(2) * c2, c1
        disc = qb * qb - dt(4) * qa * qc
        sq = np.sqrt(np.where(disc >= 0, disc, 0))
        qq = -(qb + np.where(qb < 0, -sq, sq)) / dt(2)
        r1 = np.where((disc >= 0) & (qa != 0), qq / qa, np.inf)
        r2 = np.where((disc >= 0) & (qq != 0), qc / qq, np.inf)
        w = tb - ta
        s1 = np.where((r1 > 0) & (r1 < w), ta + r1, tb)
        s2 = np.where((r2 > 0) & (r2 < w), ta + r2, tb)
        s1 = np.minimum(np.maximum(s1, ta), tb)
        s2 = np.minimum(np.maximum(s2, ta), tb)
        P = np.stack([ta, np.minimum(s1, s2), np.maximum(s1, s2), tb], axis=1)
        F = np.stack([f(P[:, c]) for c in range(4)], axis=1)
        # first event among the pieces: an exact zero at an end point, or a strict sign change across a piece
        lo = np.full(len(ri), np.nan, dtype=dtype)
        up = np.full(len(ri), np.nan, dtype=dtype)
        found = np.zeros(len(ri), dtype=np.int64)
        for c in range(4):
            zero = (found == 0) & (F[:, c] == 0)
            found[zero] = 1
            lo[zero] = P[zero, c]
            up[zero] = P[zero, c]
            if c < 3:
                br = (found == 0) & (((F[:, c] < 0) & (F[:, c + 1] > 0)) | ((F[:, c] > 0) & (F[:, c + 1] < 0)))
                found[br] = 2
                lo[br] = P[br, c]
                up[br] = P[br, c + 1]
        neg = np.where(found == 2, f(np.where(found == 2, lo, ta)) < 0, False)
        for _ in range(80):
            act = (found == 2)
            mid = lo + (up - lo) / dt(2)
            act &= (mid > lo) & (mid < up)
            if not act.any():
                break
            fm = f(np.where(act, mid, ta))
            z = act & (fm == 0)
            same = act & ~z & ((fm < 0) == neg)
            other = act & ~z & ~same
            lo = np.where(same | z, mid, lo)
            up = np.where(other | z, mid, up)
        th = up   # a closed bracket: the upper of two neighbouring numbers; an exact zero: lo == up
        # ---- the first hit of every ray (ri ascends and the intervals of a ray are in order)
        hit_rows = np.nonzero(found > 0)[0]
        first = np.full(m, -1, dtype=np.int64)
        if len(hit_rows):
            rr, pos = np.unique(ri[hit_rows], return_index=True)
            first[rr] = hit_rows[pos]
        has = first >= 0
        e = first[has]
        tt = th[e]
        res["t"][rows[has]] = tt
        u_hit = local(th)[e]
        res["grad"][rows[has]] = _gradient(V[e], u_hit, h, dt)
        res["cell"][rows[has]] = idx[e]
        s = tt - ta[e]
        fp = c1[e] + dt(2) * c2[e] * s + dt(3) * c3[e] * s * s
        res["fprime"][rows[has]] = fp
        # ---- gap: piece end points examined up to and including the hit's interval, and |f'| cell / |d| at the hit
        order = np.arange(len(ri))
        stop = np.where(has, first, len(ri))[ri]
        exam = order <= stop
        amin = np.abs(F).min(axis=1)
        # (the end point that IS an exact-zero hit counts: such a hit is as marginal as a ray can be)
        gap = np.full(m, np.inf, dtype=dtype)
        np.minimum.at(gap, ri[exam], amin[exam])
        dn = np.sqrt((D * D).sum(1))
        gap[has] = np.minimum(gap[has], np.abs(fp) * h / dn[has])
        res["gap"][rows] = gap
    return res


def agree(t_dev, t_ref, cell, dirs, tol=1e-9):
    """The acceptance rule: both miss, or both hit with |t_dev - t_ref| <= tol * cell / |d|."""
    t_dev, t_ref = np.asarray(t_dev, dtype=np.float64), np.asarray(t_ref, dtype=np.float64)
    dn = np.sqrt((np.asarray(dirs, dtype=np.float64).reshape(-1, 3) ** 2).sum(1))
    both_miss = np.isnan(t_dev) & np.isnan(t_ref)
    with np.errstate(all="ignore"):
        close = np.abs(t_dev - t_ref) <= tol * cell / dn
    return both_miss | (np.isfinite(t_dev) & np.isfinite(t_ref) & close)
