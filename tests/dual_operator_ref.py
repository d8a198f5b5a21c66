"""References for one application of the dual solver's operator S = A K^+ A^T through the grid (tests/test_dual_operator.py), numpy and scipy only:
  - kplus(): the fast Poisson solve as a DCT chain (dctn, divide by the eigenvalue sum with the zero mode -> 0, idctn: the chain of _dct_case in
    test_stage_edges.py) in np.longdouble, np.float64 or np.float32 -- scipy's pocketfft keeps all three;
  - ConstraintRows: A and A^T from get_constraints() in a chosen precision (scipy.sparse has no long double);
  - zline_recursion() / zero_line(): numpy restatements, in float64 like the kernel, of what zsolve_sparse_kernel does on one (kx, ky) line and of
    zsolve_zero_line, and zline_chain(): the 1-D chain they are held to.
The long-double chain is the reference throughout; the same chain in the handle's precision gives the error E the device is held to a multiple of."""
import numpy as np
from scipy.fft import dct, dctn, idct, idctn

assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is no wider than float64 here: the long-double reference of the dual operator does not exist"

LD = np.longdouble
PI_LD = 4 * np.arctan(LD(1))


def eigenvalues(n, h, dtype=LD):
    """lam_k = (2 - 2 cos(pi k / n)) / h^2, k = 0 ... n - 1: the 1-D Neumann Laplacian's.  Formed in long double (float64 for a float32 chain, as _dct_case does)
    and rounded once to dtype."""
    wide = LD if np.dtype(dtype) == np.dtype(LD) else np.float64
    pi = PI_LD if wide is LD else np.pi
    return ((2 - 2 * np.cos(pi * np.arange(n, dtype=wide) / n)) / wide(h) ** 2).astype(dtype)


_INVERSE_EIGS = {}   # the last three tables: a test asks for the long-double one and the one of its handle's precision, for one (n, h), many times


def _inverse_eigs(n, h, dtype):
    """1 / (lam_i + lam_j + lam_k) on the (n, n, n) grid with the zero mode -> 0, formed in the wide type and rounded once to dtype.  Read-only, shared."""
    key = (n, float(h), np.dtype(dtype).name)
    if key in _INVERSE_EIGS:
        _INVERSE_EIGS[key] = _INVERSE_EIGS.pop(key)
        return _INVERSE_EIGS[key]
    wide = LD if np.dtype(dtype) == np.dtype(LD) else np.float64
    lam = eigenvalues(n, h, wide)
    LAM = lam[:, None, None] + lam[None, :, None] + lam[None, None, :]
    LAM[0, 0, 0] = 1
    inv = 1 / LAM
    inv[0, 0, 0] = 0
    inv = inv.astype(dtype, copy=False)
    inv.setflags(write=False)
    while len(_INVERSE_EIGS) >= 3:
        del _INVERSE_EIGS[next(iter(_INVERSE_EIGS))]
    _INVERSE_EIGS[key] = inv
    return inv


def kplus(v, n, h, dtype, planes=None, workers=None):
    """K^+ v by the DCT chain in dtype.  v: n^3 values in node order (i + n j + n^2 k), returned alike.
    planes: ascending z-planes outside which v is zero and the result is not wanted (returned as zero there).  Then only these planes are transformed along x
    and y -- a transform of zeros returns zeros, so the forward half is the full chain's bit for bit, and the inverse half merely leaves out lines nobody reads."""
    dtype = np.dtype(dtype)
    v3 = np.asarray(v, dtype=dtype).reshape(n, n, n)
    inv = _inverse_eigs(n, h, dtype)
    if planes is None:
        out = idctn(dctn(v3, type=2, norm="ortho", workers=workers) * inv, type=2, norm="ortho", workers=workers)
        assert out.dtype == dtype
        return out.reshape(-1)
    planes = np.asarray(planes)
    spec = np.zeros((n, n, n), dtype=dtype)
    spec[planes] = dctn(v3[planes], type=2, norm="ortho", axes=(1, 2), workers=workers)
    spec = dct(spec, type=2, norm="ortho", axis=0, workers=workers)
    spec *= inv
    spec = idct(spec, type=2, norm="ortho", axis=0, workers=workers)
    out = np.zeros((n, n, n), dtype=dtype)
    out[planes] = idctn(spec[planes], type=2, norm="ortho", axes=(1, 2), workers=workers)
    assert out.dtype == dtype
    return out.reshape(-1)


class ConstraintRows:
    """A (m x N, eight entries per row: get_constraints()) as index and coefficient arrays, applied in a chosen precision."""

    def __init__(self, nodes, coeffs, n):
        self.nodes, self.coeffs, self.n, self.N = np.asarray(nodes), np.asarray(coeffs, dtype=np.float64), n, n ** 3
        self.m = self.nodes.shape[0]
        self.touched = np.unique(self.nodes)                        # ascending node list: every corner counts, whatever its coefficient
        self.planes = np.unique(self.touched // (n * n))            # the active z-planes

    def scatter(self, v, dtype):
        """A^T v accumulated in dtype (N values)."""
        w = np.zeros(self.N, dtype=dtype)
        np.add.at(w, self.nodes.ravel(), (self.coeffs.astype(dtype) * np.asarray(v, dtype=dtype)[:, None]).ravel())
        return w

    def gather(self, z, dtype):
        """A z accumulated in dtype (m values)."""
        return (self.coeffs.astype(dtype) * np.asarray(z)[self.nodes].astype(dtype)).sum(axis=1)

    def schur_apply(self, v, n, h, precision, workers=None, sparse=True):
        """S v = A K^+ A^T v by the chain.  precision "ld": everything in long double (the reference).  64: everything in float64.  32: what an fp32 handle
        stores -- A^T v summed in float64 and stored once per touched node as float32, the float32 chain, the float32 result gathered in float64."""
        planes = self.planes if sparse else None
        if precision == "ld":
            return self.gather(kplus(self.scatter(v, LD), n, h, LD, planes, workers), LD)
        if precision == 64:
            return self.gather(kplus(self.scatter(v, np.float64), n, h, np.float64, planes, workers), np.float64)
        w = self.scatter(v, np.float64).astype(np.float32)
        return self.gather(kplus(w, n, h, np.float32, planes, workers), np.float64)


# ---- one (kx, ky) line of the sparse z step -------------------------------------------------------------------------------------------------------------------------
def zline_chain(f_full, d, n, h, dtype):
    """u = (d I + K_z)^-1 f for the 1-D Neumann Laplacian K_z (d > 0), or its pseudo-inverse applied to f (d = 0), by the 1-D DCT chain in dtype."""
    lam = eigenvalues(n, h, dtype) + np.asarray(d, dtype=dtype)
    inv = np.zeros(n, dtype=dtype)
    nz = lam != 0
    inv[nz] = 1 / lam[nz]
    out = idct(dct(np.asarray(f_full, dtype=dtype), type=2, norm="ortho") * inv, type=2, norm="ortho")
    assert out.dtype == np.dtype(dtype)
    return out


def zline_recursion(f, planes, n, d, a):
    """zsolve_sparse_kernel on one line, statement for statement in float64 (without the factor s_x s_y): f holds the line's values on the ascending active
    planes, d = lam_kx + lam_ky > 0, a = 1 / h^2.  Returns u on the active planes."""
    f = np.asarray(f, dtype=np.float64)
    n_act = len(planes)
    delta = d / (2. * a)
    tt = delta + np.sqrt(delta * (delta + 2.))
    r, lnr = 1. / (1. + tt), -np.log1p(tt)
    C = r / (a * (tt / (1. + tt)) * (1. + r))
    rinv = 1. + tt
    rpow = lambda e: r if e == 1 else np.exp(float(e) * lnr)
    rinvpow = lambda e: rinv if e == 1 else np.exp(-float(e) * lnr)
    # ascending: F_z, A = sum f_j r^j
    Fs = np.zeros(n_act)
    F = A = 0.
    zprev = int(planes[0])
    w = np.exp(float(zprev) * lnr)
    for t in range(n_act):
        z = int(planes[t])
        if t > 0:
            g = rpow(z - zprev)
            F *= g
            w *= g
        F += f[t]
        A += f[t] * w
        Fs[t] = F
        zprev = z
    zlast = zprev
    rn = np.exp(float(n) * lnr)
    q = 1. / (1. - rn * rn)
    v = np.exp(float(n - 1 - zlast) * lnr)
    B = F * v
    Fm, Gn = q * (A + rn * B), r * q * (B + rn * A)
    # descending: G_z, combine
    u = np.zeros(n_act)
    G = wz = fprev = 0.
    wz_on = False
    for t in range(n_act - 1, -1, -1):
        z = int(planes[t])
        if t < n_act - 1:
            gap = zprev - z
            g = rpow(gap)
            G = (G + fprev) * g
            v *= g
            if wz_on:
                wz *= rinvpow(gap)
        if not wz_on and -float(z + 1) * lnr < 700.:
            wz = np.exp(float(z + 1) * lnr)
            wz_on = True
        u[t] = C * (Fs[t] + G + Fm * wz + Gn * v)
        fprev = f[t]
        zprev = z
    return u


def zero_line(f, planes, n, a):
    """zsolve_zero_line in float64 (without the factor s_x s_y): the pseudo-inverse of K_z on the (0, 0) line by mean removal and two prefix sums (np.cumsum
    where the kernel scans per thread and across the block).  Returns u on the active planes."""
    fz = np.zeros(n)
    fz[np.asarray(planes)] = np.asarray(f, dtype=np.float64)
    ft = fz - fz.sum() / n
    g = -np.cumsum(ft)                                   # g_z = -sum_{j<=z} f~_j
    u = np.concatenate(([0.], np.cumsum(g)[:-1])) / a    # u_z = (1/a) sum_{j<z} g_j
    u -= u.sum() / n
    return u[np.asarray(planes)]
