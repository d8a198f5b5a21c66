"""A numpy restatement of the redistancing scheme of include/shm_grid.h (shm_grid_redistance): the frozen values, the Godunov update in its difference
forms, the acceptance rule t < band and the result psi = s min(u, band).  It is a vectorised Jacobi iteration run until nothing changes; it knows nothing
of blocks, colours, halos or flags.  `gauss_seidel` is the same scheme as a plain-Python sweeping in eight orders, for the order-independence test.

Layout: phi is [n^3] in the node order of get_phi (x fastest), viewed as [k, j, i].  dtype is the precision u is stored in: every stored value is rounded
to it once (t is rounded, then compared), the arithmetic itself is float64."""
import math

import numpy as np

AXES = (2, 1, 0)   # x, y, z of the [k, j, i] view: the squares of g are summed in this order


def tol(n, dtype, psi):
    """TOL = n eps_T max|psi| over the finite nodes: an update costs a few ulp and a causal chain is at most 3 n nodes long."""
    fin = np.isfinite(psi)
    return n * float(np.finfo(dtype).eps) * (float(np.abs(psi[fin]).max()) if fin.any() else 0.0)


def _nb(a, axis, d, fill):
    """The value of the neighbour at offset d (+1 / -1) along axis; `fill` where it is outside the grid."""
    out = np.full_like(a, fill)
    src = [slice(None)] * 3
    dst = [slice(None)] * 3
    if d > 0:
        src[axis], dst[axis] = slice(1, None), slice(None, -1)
    else:
        src[axis], dst[axis] = slice(None, -1), slice(1, None)
    out[tuple(dst)] = a[tuple(src)]
    return out


def _round(a, dtype):
    return np.asarray(a, dtype=np.float64).astype(dtype).astype(np.float64)


def frozen_init(f, h, dtype=np.float64):
    """(u0, frozen, wall): u0 = |f| / g rounded to dtype at the nodes with a cut edge and +inf elsewhere; wall marks the nodes whose f is not finite."""
    wall = ~np.isfinite(f)
    neg = f < 0
    cut = np.zeros(f.shape, dtype=bool)
    g2 = np.zeros(f.shape)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for axis in AXES:
            fp, fm = _nb(f, axis, +1, np.nan), _nb(f, axis, -1, np.nan)
            hp, hm = np.isfinite(fp), np.isfinite(fm)
            g = np.zeros(f.shape)
            g = np.maximum(g, np.where(hp, np.abs(fp - f) / h, 0.0))
            g = np.maximum(g, np.where(hm, np.abs(f - fm) / h, 0.0))
            g = np.maximum(g, np.where(hp & hm, np.abs(fp - fm) / (2.0 * h), 0.0))
            cut |= hp & ((fp < 0) != neg)
            cut |= hm & ((fm < 0) != neg)
            g2 = g2 + g * g
        frozen = cut & ~wall
        u0 = np.where(frozen, _round(np.abs(f) / np.sqrt(g2), dtype), np.inf)
    return u0, frozen, wall


def godunov(u, h):
    """t of every node from its six neighbours' u (+inf outside the grid and at walls)."""
    m = np.stack([np.minimum(_nb(u, axis, +1, np.inf), _nb(u, axis, -1, np.inf)) for axis in AXES])
    m.sort(axis=0)
    a, b, c = m
    with np.errstate(invalid="ignore"):
        t1 = a + h
        d1 = b - a
        t2 = ((a + b) + np.sqrt(2.0 * (h * h) - d1 * d1)) / 2.0
        d2, d3 = c - a, c - b
        t3 = ((a + b + c) + np.sqrt(3.0 * (h * h) - (d1 * d1 + d2 * d2 + d3 * d3))) / 3.0
    return np.where(t1 <= b, t1, np.where(t2 <= c, t2, t3))


def finish(u, f, wall, band, dtype):
    psi = np.where(f < 0, -1.0, 1.0) * np.minimum(u, band)
    psi[wall] = np.nan
    return _round(psi, dtype)


def redistance(phi, n, h, iso=0.0, band=np.inf, dtype=np.float64):
    """(psi [n^3] float64 holding dtype values, info): the Jacobi iteration to its fixed point."""
    f = np.asarray(phi, dtype=np.float64).reshape(n, n, n) - iso
    u, frozen, wall = frozen_init(f, h, dtype)
    fixed = frozen | wall
    its = 0
    while True:
        tr = _round(godunov(u, h), dtype)
        acc = ~fixed & (tr < band) & (tr < u)
        if not acc.any():
            break
        u = np.where(acc, tr, u)
        its += 1
        assert its <= 8 * n + 64, "the Jacobi iteration does not end"
    psi = finish(u, f, wall, band, dtype)
    reached = ~wall & (u < band)
    info = dict(n_frozen=int(frozen.sum()), n_nonfinite=int(wall.sum()), n_reached=int(reached.sum()), iterations=its,
                max_abs=float(u[reached].max()) if reached.any() else 0.0, frozen=frozen.reshape(-1), u=u.reshape(-1))
    return psi.reshape(-1), info


def _t_scalar(a, b, c, h):
    if a > b:
        a, b = b, a
    if b > c:
        b, c = c, b
    if a > b:
        a, b = b, a
    t = a + h
    if t <= b:
        return t
    d1 = b - a
    t = ((a + b) + math.sqrt(2.0 * (h * h) - d1 * d1)) / 2.0
    if t <= c:
        return t
    d2, d3 = c - a, c - b
    return ((a + b + c) + math.sqrt(3.0 * (h * h) - (d1 * d1 + d2 * d2 + d3 * d3))) / 3.0


def gauss_seidel(phi, n, h, iso=0.0, band=np.inf, dtype=np.float64):
    """The same scheme by fast sweeping: in-place updates in the eight axis orders, repeated until a whole pass changes nothing.  Plain Python on a
    padded list; shares frozen_init and finish with the Jacobi restatement, nothing else."""
    f = np.asarray(phi, dtype=np.float64).reshape(n, n, n) - iso
    u0, frozen, wall = frozen_init(f, h, dtype)
    m = n + 2
    pad = np.full((m, m, m), np.inf)
    pad[1:-1, 1:-1, 1:-1] = u0
    u = pad.reshape(-1).tolist()
    fixed = np.ones((m, m, m), dtype=bool)
    fixed[1:-1, 1:-1, 1:-1] = frozen | wall
    fixed = fixed.reshape(-1).tolist()
    rnd = (lambda x: x) if np.dtype(dtype) == np.float64 else (lambda x: float(np.float32(x)))
    sx, sy, sz = 1, m, m * m
    fwd, bwd = list(range(1, n + 1)), list(range(n, 0, -1))
    changed = True
    passes = 0
    while changed:
        changed = False
        passes += 1
        assert passes <= 4 * n, "the sweeping does not end"
        for kk in (fwd, bwd):
            for jj in (fwd, bwd):
                for ii in (fwd, bwd):
                    for k in kk:
                        for j in jj:
                            base = k * sz + j * sy
                            for i in ii:
                                g = base + i
                                if fixed[g]:
                                    continue
                                a = min(u[g - sx], u[g + sx])
                                b = min(u[g - sy], u[g + sy])
                                c = min(u[g - sz], u[g + sz])
                                if a == math.inf and b == math.inf and c == math.inf:
                                    continue
                                t = rnd(_t_scalar(a, b, c, h))
                                if t < band and t < u[g]:
                                    u[g] = t
                                    changed = True
    u = np.array(u).reshape(m, m, m)[1:-1, 1:-1, 1:-1]
    return finish(u, f, wall, band, dtype).reshape(-1)
