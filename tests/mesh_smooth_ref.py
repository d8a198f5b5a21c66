"""Plain-numpy restatement of the mesh smoothing stage (include/shm_grid.h, "Taubin smoothing and vertex normals of an indexed mesh"; the arithmetic of
csrc/shm_mesh_smooth.h): the frame and its quantum, fixed-point int64 neighbour sums, the update, the cap, and the normals.  numpy's elementwise fp64
operations are unfused and rounded to nearest, np.rint is llrint's rounding, and integer sums do not depend on the order np.add.at happens to take: the GPU
tests hold the device to this bit for bit.  float_umbrella() is the ordinary floating-point operator the fixed-point one is compared with."""
import numpy as np

FRAME_BITS, NORMAL_BITS = 40, 41


def key(x):
    """Order-preserving image of doubles in uint64 (cmp_key of csrc/shm_iso_components.hip.h)."""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.int64)
    return (b ^ ((b >> 63) & np.int64(0x7fffffffffffffff))).view(np.uint64) ^ np.uint64(0x8000000000000000)


def unkey(u):
    s = (np.asarray(u, dtype=np.uint64) ^ np.uint64(0x8000000000000000)).view(np.int64)
    return (s ^ ((s >> 63) & np.int64(0x7fffffffffffffff))).view(np.float64)


def quantum(v, bits):
    """2^(e - bits) for v = m 2^e, m in [0.5, 1); 1 for v = 0."""
    if not v > 0.0:
        return 1.0
    e = int(np.frexp(v)[1]) - bits
    return float(np.ldexp(1.0, max(e, -1074)))


def frame(V):
    """(lo [3], q) of the input positions."""
    fin = np.isfinite(V).all(axis=1)
    if not fin.any():
        return np.zeros(3), 1.0
    k = key(V[fin])
    lo, hi = unkey(k.min(axis=0)), unkey(k.max(axis=0))
    ext = hi - lo
    assert np.isfinite(ext).all()
    return lo, quantum(float(ext.max()), FRAME_BITS)


def _round(t):
    t = np.where(np.isnan(t), 0.0, np.clip(t, -2.0 ** 62, 2.0 ** 62))
    return np.rint(t).astype(np.int64)


def quant(X, lo, q):
    with np.errstate(invalid="ignore", over="ignore"):
        return _round((X - lo) / q)


def _contributing(X, F):
    distinct = (F[:, 0] != F[:, 1]) & (F[:, 0] != F[:, 2]) & (F[:, 1] != F[:, 2])
    fin = np.isfinite(X).all(axis=1)
    return F[distinct & fin[F].all(axis=1)]


def one_pass(X, F, lo, q, f, fixed=None, X0=None, cap=0.0):
    nv = len(X)
    Fc = _contributing(X, F)
    S = np.zeros((nv, 3), dtype=np.int64)
    c = np.zeros(nv, dtype=np.int64)
    Q = quant(X, lo, q)
    for k in range(3):
        a, b, d = Fc[:, k], Fc[:, (k + 1) % 3], Fc[:, (k + 2) % 3]
        np.add.at(S, a, Q[b] + Q[d])
        np.add.at(c, a, 2)
    move = np.repeat((c > 0)[:, None], 3, axis=1)
    if fixed is not None:
        move &= ((np.asarray(fixed, dtype=np.uint8)[:, None] >> np.arange(3, dtype=np.uint8)) & 1) == 0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        mean = (S.astype(np.float64) / c.astype(np.float64)[:, None]) * q + lo
        L = mean - X
        Xn = np.where(move, X + f * L, X)
        if cap > 0.0:
            D = Xn - X0
            ln = np.sqrt((D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1]) + D[:, 2] * D[:, 2])
            s = cap / ln
            capped = (ln > cap)[:, None]
            if fixed is not None:
                capped = capped & (((np.asarray(fixed, dtype=np.uint8)[:, None] >> np.arange(3, dtype=np.uint8)) & 1) == 0)
            Xn = np.where(capped, X0 + D * s[:, None], Xn)
    return Xn


def normals_of(X, F):
    nv = len(X)
    Fc = _contributing(X, F)
    A, B, C = X[Fc[:, 0]], X[Fc[:, 1]], X[Fc[:, 2]]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        u, w = B - A, C - A
        N = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], axis=1)
        mag = np.abs(N)
        mag = mag[np.isfinite(mag)]
        qn = quantum(float(mag.max()) if mag.size else 0.0, NORMAL_BITS)
        Nq = _round(N / qn)
        S = np.zeros((nv, 3), dtype=np.int64)
        for k in range(3):
            np.add.at(S, Fc[:, k], Nq)
        s = S.astype(np.float64)
        ln = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
        out = np.where((ln > 0.0)[:, None], s / ln[:, None], 0.0)
    return out


def smooth(V, F, iterations, lam=0.5, mu=-0.53, fixed=None, max_displacement=0.0, normals=False):
    """The stage: (positions [nv, 3]) or (positions, normals)."""
    X0 = np.array(V, dtype=np.float64).reshape(-1, 3)
    F = np.asarray(F, dtype=np.int64).reshape(-1, 3)
    lo, q = frame(X0)
    X = X0.copy()
    for _ in range(iterations):
        X = one_pass(X, F, lo, q, lam, fixed, X0, max_displacement)
        if mu != 0.0:
            X = one_pass(X, F, lo, q, mu, fixed, X0, max_displacement)
    return (X, normals_of(X, F)) if normals else X


def float_umbrella(V, F, iterations, lam=0.5, mu=-0.53):
    """The same operator in ordinary floating point (sums in whatever order np.add.at takes): not reproducible under a permutation of F."""
    X = np.array(V, dtype=np.float64).reshape(-1, 3)
    F = np.asarray(F, dtype=np.int64).reshape(-1, 3)
    for _ in range(iterations):
        for f in ((lam, mu) if mu != 0.0 else (lam,)):
            Fc = _contributing(X, F)
            S = np.zeros_like(X)
            c = np.zeros(len(X))
            for k in range(3):
                np.add.at(S, Fc[:, k], X[Fc[:, (k + 1) % 3]] + X[Fc[:, (k + 2) % 3]])
                np.add.at(c, Fc[:, k], 2.0)
            m = c > 0
            Xn = X.copy()
            Xn[m] = X[m] + f * (S[m] / c[m][:, None] - X[m])
            X = Xn
    return X


def box_mask(V, n, bbox_min, cell):
    """fixed [nv] uint8 of slide_on_box: bit a where coordinate a lies in a face of the box, by touches_box's comparisons (tests/components_ref.py)."""
    from fractions import Fraction
    bbox_min = np.asarray(bbox_min, dtype=np.float64)
    hi_plane = np.array([(n - 1) * cell + bbox_min[a] for a in range(3)])
    hi_fused = np.array([float(Fraction(n - 1) * Fraction(float(cell)) + Fraction(float(bbox_min[a]))) for a in range(3)])
    on = (V == bbox_min[None, :]) | (V == hi_plane[None, :]) | (V == hi_fused[None, :])
    return (on * np.array([1, 2, 4])).sum(axis=1).astype(np.uint8)


# ---- measures of a mesh ------------------------------------------------------------------------------------------------------------------------------------------
def volume(V, F):
    o = V[np.isfinite(V).all(axis=1)].mean(axis=0)
    a, b, c = V[F[:, 0]] - o, V[F[:, 1]] - o, V[F[:, 2]] - o
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def roughness(V, F):
    """Mean angle between the unit normals of the two faces on every edge shared by exactly two faces with |N| > 1e-14."""
    N = np.cross(V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]])
    ln = np.linalg.norm(N, axis=1)
    ok = ln > 1e-14
    U = N / np.where(ok, ln, 1.0)[:, None]
    e = np.sort(np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]]), axis=1)
    t = np.tile(np.arange(len(F)), 3)
    order = np.lexsort((e[:, 1], e[:, 0]))
    e, t = e[order], t[order]
    _, first, count = np.unique(e, axis=0, return_index=True, return_counts=True)
    first = first[count == 2]
    t0, t1 = t[first], t[first + 1]
    both = ok[t0] & ok[t1]
    cosang = np.clip(np.einsum("ij,ij->i", U[t0[both]], U[t1[both]]), -1.0, 1.0)
    return float(np.arccos(cosang).mean())


OCTA_V = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)
OCTA_F = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], dtype=np.int64)
