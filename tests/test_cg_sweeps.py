"""The fused sweeps of the projected stencil CG (csrc/shm_cg_fused.hip.h), ONE STEP AT A TIME and at every launch shape fused_cfg can choose below n = 514:
cg_fused_kernel<T, VEC, RY, WX, WY, DIR | RES> through GridSolver.cg_sweeps (shm_grid_cg_sweeps) and cg_x_update2_kernel<T, VEC> through GridSolver.cg_x_update
(shm_grid_cg_x_update).  Both entries issue the solve's own launches (run_dir, finalize_pq, run_res, launch_x_update2, halo_exchange), so what is tested is the
loop's code and not a copy of it.  A converged solve held to 1e-7 cannot see a wrong dot product (CG converges anyway, a few iterations later) nor a stencil
that is wrong in one halo row; one step held to a counted rounding bound sees both.

Same discipline as tests/test_stage_edges.py.  THE REFERENCE IS FED THE DEVICE'S OWN INPUT and every stage is isolated from the one before it:
    p'        from the inputs z, p and the scalars                       (all rounded to the handle's precision first: exact input for the reference)
    rho_new   from red0, uw
    alpha     from the device's rho_new and the DEVICE'S p' as read back (K p' and the dot product restated on it)
    r'        from r, the DEVICE'S alpha and K of the device's p'
    ||r'||^2  from the DEVICE'S r' as read back
in numpy long double for fp64 handles and float64 for fp32 handles (the bounds carry the reference's own roundings, u_ref, as _div_check carries U[64]).
K = -L in the Neumann convention: an out-of-grid neighbour is the node itself.

Bounds: per node, counted beside each constant below and never fitted to what the device returns.  gamma(k, u) = k u / (1 - k u) is the standard bound of k
successive roundings.  A contracted multiply-add only removes roundings.  Every test prints its worst error, its bound and its margin.

One assumption is made and thereby tested: the DIR sweep forms p'.K p' from the p' in its registers, where the rows and planes bordering a workgroup are
recomputed by the same expression from the same inputs as the values the neighbouring workgroup stores -- so they are taken to be the stored p' bit for bit,
and alpha (DIR's registers) and r' (RES, from the stored p') are held to one and the same restated K p'.

Out of scope here:
  - WX = 8 with VEC > 1: needs n >= 514 in fp64 or n >= 1028 in fp32, too large for a test of seconds.  Its WY = 2, 16-wave body is the code n = 258 runs with WY = 4.
  - the 16-wave shapes forced onto small rows by SHM_FUSED_WAVES;
  - the classic four-kernel loop, and the SHM_ERR_INVALID of both entries where the fused sweeps do not serve the grid (SHM_CG_CLASSIC is read once per process);
  - the multi-process halo over RCCL (both entries are single-process)."""
import os

import numpy as np
import pytest

try:
    import torch  # noqa: F401  (as tests/test_stage_edges.py: torch first, one HIP runtime)
except ImportError:
    torch = None

from conftest import ROOT
from test_gpu_parity import make_solver
from test_stage_edges import TINY, U, _bunny, _line, _round_to

gpu = pytest.mark.gpu
SHM_ERR_INVALID, SHM_ERR_STATE = 1, 7


def gamma(k, u):
    return k * u / (1.0 - k * u)


# ---- the reference ------------------------------------------------------------------------------------------------------------------------------------------------
def K_restated(p3, ih2, absolute=False):
    """K p = -L p on a field p3[z, y, x], K p = (6 c - sum of the six neighbours) / h^2 with an out-of-grid neighbour replaced by the node itself.
    absolute: (sum |neighbours| + 6 |c|) / h^2, the T of the bounds."""
    a = np.pad(p3, 1, mode="edge")
    if absolute:
        a = np.abs(a)
    nb = a[1:-1, 1:-1, 2:] + a[1:-1, 2:, 1:-1] + a[2:, 1:-1, 1:-1] + a[1:-1, 1:-1, :-2] + a[1:-1, :-2, 1:-1] + a[:-2, 1:-1, 1:-1]
    c = a[1:-1, 1:-1, 1:-1]
    return (nb + 6 * c) * ih2 if absolute else -((nb - 6 * c) * ih2)


class StepRef:
    """One CG step restated, with the bound of each device quantity.  F: the reference's float type; u: unit roundoff of the handle's format; u_ref: of F;
    c32: 1 on fp32 handles, where the conversion of a double scalar (beta, alpha, 1 / h^2) to T rounds, 0 on fp64 handles, where it is exact."""

    def __init__(self, n, cell, precision):
        self.n, self.precision = n, precision
        self.F = np.longdouble if precision == 64 else np.float64
        self.u, self.u_ref, self.c32 = U[precision], float(np.finfo(self.F).eps) / 2, 1 if precision == 32 else 0
        self.tiny = TINY[precision]
        self.ih2 = self.F(1) / (self.F(cell) * self.F(cell))

    def f3(self, v):
        return np.asarray(v, dtype=self.F).reshape(self.n, self.n, self.n)

    def direction(self, z, p, rho_old, red0, uw, use_uw, init):
        """(rho_new, beta, p', bound of p').  Device: rho_new = red0 - uw in double (1 rounding of 2^-53), beta = rho_new / rho_old in double (1), its
        conversion to T (c32), the product beta p (1 of u), the addition (1 of u): a term beta p passes 2 + c32 roundings of u and carries 2 of 2^-53 in beta; z
        passes the addition alone and is given the same 2 + c32.  The reference: subtraction, division, product, addition, 4 of u_ref."""
        F = self.F
        rho_new = F(red0) - (F(uw) if use_uw else F(0))
        beta = F(0) if (init or rho_old == 0.) else rho_new / F(rho_old)
        z, p = self.f3(z), self.f3(p)
        bp = beta * p
        T = np.abs(z) + np.abs(bp)
        bound = (gamma(2 + self.c32, self.u) + 4 * self.u_ref) * T + 2 * U[64] * np.abs(bp) + self.tiny
        return rho_new, beta, -z + bp, bound

    def operator(self, p1):
        """(K p', B_q: the bound of the device's K p' per node).  cg_fused_kernel: s = (xp + up + nxt + xm + dn + prv) - 6 c; qv = -s * ih2.  The first neighbour
        passes five additions (5), the subtraction (1) and the product with ih2 (1): 7 roundings of u; 6 c is rounded once and passes two of those.  ih2 is
        1 / (cell * cell) formed in double on the host (2 of 2^-53) and converted to T (c32).  So |q_dev - q| <= (gamma(7 + c32, u) + 2 * 2^-53) T with
        T = (sum |neighbours| + 6 |c|) / h^2.  The reference: nine operations, 9 u_ref."""
        p1 = self.f3(p1)
        q = K_restated(p1, self.ih2)
        T = K_restated(p1, self.ih2, absolute=True)
        return q, (gamma(7 + self.c32, self.u) + 2 * U[64] + 9 * self.u_ref) * T + self.tiny

    def residual(self, r, alpha, q, Bq):
        """(r', bound).  Device: alpha converted to T (c32), the product alpha qv (1), the addition (1): alpha q passes 2 + c32 roundings of u, r one; plus
        |alpha| B_q for the device's own q.  The reference: product and addition, 2 u_ref (3 taken)."""
        r, a = self.f3(r), self.F(alpha)
        aq = a * q
        T = np.abs(r) + np.abs(aq)
        return r + aq, abs(a) * Bq + (gamma(2 + self.c32, self.u) + 3 * self.u_ref) * T + self.tiny

    def alpha(self, rho_new, p1, q, Bq, k):
        """(alpha, bound, p'.Kp').  The device sums (double) c * (double) qv in double: the product is exact on fp32 handles and rounded once on fp64 ones
        (counted always: k + 1), then at most k additions on the longest chain of the reduction.  |pq_dev - pq| <= dpq = sum |c| B_q + gamma(k + 1, 2^-53)
        sum |c q|, plus the reference's pairwise sum (40 u_ref covers log2 of 2^25 terms and the products).  alpha = rho / pq by one division in double; the
        first term is the exact effect of dpq on a quotient, no linearisation."""
        p1 = self.f3(p1)
        pq = (p1 * q).sum()
        S = (np.abs(p1) * np.abs(q)).sum()
        dpq = (np.abs(p1) * Bq).sum() + (gamma(k + 1, U[64]) + 40 * self.u_ref) * S
        rho = self.F(rho_new)
        if rho == 0:
            return self.F(0), 0., pq
        assert dpq < abs(pq), "p'.Kp' is not resolved by the bound of its own rounding: the input is degenerate"
        a = rho / pq
        return a, float(abs(rho) * dpq / (abs(pq) * (abs(pq) - dpq)) + (2 * U[64] + 2 * self.u_ref) * abs(a) + TINY[64]), pq

    def norm2(self, r1, k):
        """(||r'||^2 of the device's own r', bound): the square in double (exact on fp32 handles, one rounding on fp64 ones: k + 1) and at most k additions,
        plus the reference's pairwise sum."""
        r1 = self.f3(r1)
        rr = (r1 * r1).sum()
        return rr, float((gamma(k + 1, U[64]) + 40 * self.u_ref) * rr + TINY[64])

    def x_update(self, x, pa, pb, alpha_a, alpha_b, use_a, use_b):
        """(x', bound).  cg_x_update2_kernel: each alpha converted to T (c32), xv += a0 * av, xv += a1 * bv: alpha_a p_a passes its product and both additions
        (3 + c32 roundings of u), every other term fewer.  The reference: two products, two additions, 3 per term."""
        F = self.F
        x = np.asarray(x, dtype=F)
        ta = F(alpha_a) * np.asarray(pa, dtype=F) if use_a else np.zeros_like(x)
        tb = F(alpha_b) * np.asarray(pb, dtype=F) if use_b else np.zeros_like(x)
        T = np.abs(x) + np.abs(ta) + np.abs(tb)
        return x + ta + tb, (gamma(3 + self.c32, self.u) + 3 * self.u_ref) * T + self.tiny


def chain_lengths(shape, slabs):
    """(k of p'.Kp', k of ||r'||^2): additions on the longest chain of each reduction, from the launch shape the device reported.
      lane accumulator: RY * VEC * zc terms;  wave_sum: 6;  the workgroup's sum over its NW = WX * WY waves: NW;
      the sum over the np = yblocks * zchunks block partials:
        p'.Kp', one slab  -- inside the RES sweep (NW * 64 threads): ceil(np / (64 NW)) + 6 + NW
        p'.Kp', several   -- finalize_sum_kernel (256 threads): ceil(np / 256) + 6 + 4, then sum_slabs_kernel: one addition per slab
        ||r'||^2          -- finalize_sum_kernel, then sum_slabs_kernel on several slabs."""
    nw = shape["wx"] * shape["wy"]
    np_ = shape["yblocks"] * shape["zchunks"]
    block = shape["ry"] * shape["vec"] * shape["zc"] + 6 + nw
    fin = -(-np_ // 256) + 6 + 4 + (slabs if slabs > 1 else 0)
    k_pq = block + (-(-np_ // (64 * nw)) + 6 + nw if slabs == 1 else fin)
    return k_pq, block + fin


def _vec(n, precision):
    w = 2 if precision == 64 else 4
    return w if n % w == 0 else 1


def _inputs(n, precision, seed, count=3):
    rng = np.random.default_rng(seed)
    return [_round_to(rng.standard_normal(n ** 3), precision) for _ in range(count)]


# ---- CPU: the reference itself ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 11, 16])
def test_restated_K_matches_the_oracle(oracle_c, n):
    """K_restated = -shmo_laplacian_apply in float64: the oracle forms 1 / (h * h) (2 roundings), adds six times and multiplies (7); the restatement as many in
    another order: 2 * 9 * 2^-53 T, per node."""
    rng = np.random.default_rng(300 + n)
    u = rng.standard_normal(n ** 3)
    cell = float(rng.uniform(0.05, 0.5))
    ref = np.empty_like(u)
    oracle_c.shmo_laplacian_apply(n, cell, u, ref)
    u3 = u.reshape(n, n, n)
    got = K_restated(u3, 1.0 / (cell * cell)).reshape(-1)
    T = K_restated(u3, 1.0 / (cell * cell), absolute=True).reshape(-1)
    r = float((np.abs(got + ref) / (18 * U[64] * T)).max())
    _line("restated K n=%d vs -shmo_laplacian_apply" % n, ["worst error / bound %.3f" % r])
    assert r <= 1.0
    lo = K_restated(np.asarray(u3, dtype=np.longdouble), np.longdouble(1) / (np.longdouble(cell) * np.longdouble(cell)))
    assert float((np.abs(lo.reshape(-1) - got) / (9 * U[64] * T)).max()) <= 1.0      # ... and the long-double instance agrees with the float64 one


def test_api_symbols_header_and_wrappers(shm):
    """Both entries are exported, declared in include/shm_grid.h with their documentation, listed in ABI_SYMBOLS and wrapped by GridSolver; the ABI stays 5."""
    from signed_heat_3d_amd.grid_abi import ABI_SYMBOLS
    lib = shm.load_library()
    header = open(os.path.join(ROOT, "include", "shm_grid.h")).read()
    for name in ("shm_grid_cg_sweeps", "shm_grid_cg_x_update"):
        assert name in ABI_SYMBOLS and hasattr(lib, name) and ("shm_status %s(" % name) in header and ("  %s: " % name) in header, name
    assert lib.shm_grid_abi_version() == 5 and "#define SHM_GRID_ABI_VERSION 5" in header
    assert callable(shm.GridSolver.cg_sweeps) and callable(shm.GridSolver.cg_x_update)
    assert shm.GridSolver.CG_SHAPE == ("vec", "ry", "wx", "wy", "zc", "zchunks", "yblocks", "overlap")
    assert chain_lengths(dict(vec=1, ry=4, wx=2, wy=4, zc=8, zchunks=9, yblocks=5), 1) == (32 + 6 + 8 + 1 + 6 + 8, 32 + 6 + 8 + 1 + 6 + 4)


# fp64 bounds: a defect must exceed its bound by 10^6.  An fp32 bound is 2^29 = 5e8 times the fp64 one on the same input, and a defect of relative size d exceeds a
# bound of relative size ~ 10 u by d / (10 u): the one-row defect (d = 1 / n^2 = 1.7e-3 at n = 24) by some 3e3 in fp32.  There: two orders of magnitude.
SENSITIVITY = {64: 1e6, 32: 1e2}


@pytest.mark.parametrize("precision", [64, 32])
def test_the_bounds_see_five_seeded_defects(precision):
    """On the reference alone (its own outputs, rounded to the precision, stand in for the device's): each defect a kernel of this shape can have moves its
    quantity by at least SENSITIVITY times that quantity's bound.  n = 24 as three slabs of eight planes, chunks of eight planes, row blocks of 16 rows."""
    n, cell = 24, 0.07
    z, p, r = _inputs(n, precision, 77)
    ref = StepRef(n, cell, precision)
    shape = dict(vec=1, ry=4, wx=1, wy=4, zc=8, zchunks=3, yblocks=2)
    k_pq, k_rr = chain_lengths(shape, 1)
    rho_new, beta, p1, bp = ref.direction(z, p, 1.0, 0.4, 0., False, False)
    p1d = _round_to(np.asarray(p1, dtype=np.float64), precision)                  # "the device's p'"
    q, Bq = ref.operator(p1d)
    a, ba, pq = ref.alpha(float(rho_new), p1d, q, Bq, k_pq)
    r1, br = ref.residual(r, float(a), q, Bq)
    r1d = _round_to(np.asarray(r1, dtype=np.float64), precision)
    rr, brr = ref.norm2(r1d, k_rr)
    p1_3, z3, p3 = ref.f3(p1d), ref.f3(z), ref.f3(p)
    found = {}
    # 1. a periodic wrap instead of the clamp on the face x = 0
    pad = np.pad(p1_3, 1, mode="edge")
    pad[1:-1, 1:-1, 0] = p1_3[:, :, -1]
    nb = pad[1:-1, 1:-1, 2:] + pad[1:-1, 2:, 1:-1] + pad[2:, 1:-1, 1:-1] + pad[1:-1, 1:-1, :-2] + pad[1:-1, :-2, 1:-1] + pad[:-2, 1:-1, 1:-1]
    q1 = -((nb - 6 * p1_3) * ref.ih2)
    found["1 wrap on a face -> r'"] = float((np.abs(ref.f3(r) + a * q1 - r1) / br).max())
    # 2. one row at a row-block border (plane 3, row 16) left out of p'.Kp'
    a2 = rho_new / (pq - (p1_3[3, 16] * q[3, 16]).sum())
    found["2 a border row missing from p'.Kp' -> alpha"] = float(abs(a2 - a) / ba)
    # 3. a ghost plane taken from the wrong side: the second slab's top plane 15 reads its lower ghost (plane 7) where plane 16 belongs
    q3 = q.copy()
    q3[15] += (p1_3[16] - p1_3[7]) * ref.ih2
    found["3 ghost plane of the wrong side -> r'"] = float((np.abs(a * (q3 - q)) / br).max())
    # 4. beta applied to the halo of p but not to its interior
    found["4 beta missing in the interior -> p'"] = float((np.abs((-z3 + p3) - p1) / bp)[1:-1, 1:-1, 1:-1].max())
    # 5. the partial of one 8-plane chunk counted twice
    found["5 a chunk counted twice -> ||r'||^2"] = float(abs((ref.f3(r1d)[8:16] ** 2).sum()) / brr)
    a5 = rho_new / (pq + (p1_3[8:16] * q[8:16]).sum())
    found["5 a chunk counted twice -> alpha"] = float(abs(a5 - a) / ba)
    _line("sensitivity fp%d (defect / bound, at least %.0e)" % (precision, SENSITIVITY[precision]), ["%s: %.2e" % kv for kv in sorted(found.items())])
    for what, factor in found.items():
        assert factor >= SENSITIVITY[precision], (what, factor)


# ---- GPU: one step ---------------------------------------------------------------------------------------------------------------------------------------------------
def _ratio(err, bound):
    r = np.asarray(err / bound, dtype=np.float64)
    i = int(np.argmax(r))
    return float(r.reshape(-1)[i]), i


def _seam_planes(shm, n, slabs):
    ks = set()
    for s in range(1, slabs):
        k0 = shm.plan_slab(n, slabs, s)[0]
        ks |= {k0 - 1, k0}
    return sorted(ks)


def run_step(shm, s, n, cell, precision, slabs, want, seed, it=0, use_uw=False, init=False, rho_old=1.0, red0=0.4, uw=0.137, p_fill=None, what=""):
    """One call of cg_sweeps on handle s held to the reference at every node.  Returns (p', r', scalars, shape, printed items)."""
    z, p, r = _inputs(n, precision, seed)
    if p_fill is not None:
        p = np.full(n ** 3, p_fill)
    if use_uw:
        red0 = red0 + uw                       # beta stays ~ 0.4
    p1d, r1d, (rho_d, alpha_d, rr_d), shape = s.cg_sweeps(z, p, r, rho_old, red0, uw, use_uw=use_uw, init=init, it=it)
    for key, val in want.items():              # a case that promises an instance fails, not skips, if the device chose otherwise
        assert shape[key] == val, "%s: the device ran %s, the case promises %s = %d" % (what, shape, key, val)
    ref = StepRef(n, cell, precision)
    k_pq, k_rr = chain_lengths(shape, slabs)
    items = ["shape %s" % " ".join("%s=%d" % (k, shape[k]) for k in shm.GridSolver.CG_SHAPE)]

    def held(name, err, bound, seams=True):
        ratio, at = _ratio(err, bound)
        txt = "%s max err %.3e, worst err/bound %.3f (bound there %.3e, margin %s)" % (
            name, float(np.max(err)), ratio, float(np.reshape(bound, -1)[at]) if np.ndim(bound) else float(bound), "%.1fx" % (1 / ratio) if ratio > 0 else "inf")
        if seams and slabs > 1 and np.ndim(err) == 3:
            ks = _seam_planes(shm, n, slabs)
            txt += " [seam planes %s: %.3f]" % (ks, _ratio(err[ks], bound[ks])[0])
        items.append(txt)
        assert ratio <= 1.0, "%s: %s" % (what, txt)        # (NaN fails: not <= 1)

    rho_new, beta, p1, bp = ref.direction(z, p if p_fill is None else np.zeros(n ** 3), rho_old, red0, uw, use_uw, init)
    held("rho_new", abs(ref.F(rho_d) - rho_new), (U[64] + ref.u_ref) * abs(float(rho_new)) + TINY[64])       # one subtraction in double
    if init or rho_old == 0.:
        assert np.array_equal(p1d, -z), "%s: p' is not -z bit for bit" % what
        items.append("p' == -z bit for bit")
    else:
        held("p'", np.abs(ref.f3(p1d) - p1), bp)
    q, Bq = ref.operator(p1d)
    a, ba, _ = ref.alpha(rho_d, p1d, q, Bq, k_pq)
    if rho_d == 0.:
        assert alpha_d == 0. and np.array_equal(r1d, r), "%s: rho = 0 must leave alpha = 0 and r untouched" % what
        items.append("alpha == 0, r' == r bit for bit")
    else:
        held("alpha", abs(ref.F(alpha_d) - a), ba)
        r1, br = ref.residual(r, alpha_d, q, Bq)
        held("r'", np.abs(ref.f3(r1d) - r1), br)
    rr, brr = ref.norm2(r1d, k_rr)
    held("||r'||^2", abs(ref.F(rr_d) - rr), brr)
    _line("cg_sweeps %s" % what, items)
    return p1d, r1d, (rho_d, alpha_d, rr_d), shape


def _case(shm, n, precision, slabs, want, **kw):
    d = _bunny(n)
    s = make_solver(shm, d, precision=precision, local_slabs=slabs)
    what = "n=%d fp%d slabs %d %s" % (n, precision, slabs, " ".join("%s=%s" % kv for kv in sorted(kw.items())))
    try:
        return run_step(shm, s, n, float(d["cell"]), precision, slabs, want, seed=1000 * n + precision + slabs, what=what, **kw)
    finally:
        s.close()


# (n, precision) -> the instance fused_cfg must choose on 256 CUs, one slab
VEC1 = dict(vec=1, ry=4)
ONE_SLAB = [
    (11, 64, dict(VEC1, wx=1, wy=8)), (11, 32, dict(VEC1, wx=1, wy=8)),                          # the fixtures' shapes: the entry's own baseline
    (16, 64, dict(vec=2, ry=2, wx=1, wy=8)), (16, 32, dict(vec=4, ry=2, wx=1, wy=8)),
    (65, 64, dict(VEC1, wx=2, wy=4, zc=8, zchunks=9)), (65, 32, dict(VEC1, wx=2, wy=4, zc=8, zchunks=9)),       # second wave: one live lane; last chunk: one plane
    (129, 64, dict(VEC1, wx=4, wy=2, zc=8, zchunks=17)), (129, 32, dict(VEC1, wx=4, wy=2, zc=8, zchunks=17)),   # a wave with one live lane and a wholly idle wave
    (130, 64, dict(vec=2, ry=2, wx=2, wy=4)),
    (130, 32, dict(VEC1, wx=4, wy=2)),                                                           # VEC 1 on an even side (130 % 4 != 0)
    (128, 64, dict(vec=2, ry=2, wx=1, wy=8)), (256, 32, dict(vec=4, ry=2, wx=1, wy=8)),          # exactly 64 full lanes: lane == 63 && wx == WX - 1, no idle lane
    (256, 64, dict(vec=2, ry=2, wx=2, wy=4)),                                                    # both waves exactly full
    (257, 64, dict(VEC1, wx=8, wy=1)), (257, 32, dict(VEC1, wx=8, wy=1)),                        # WX 8, WY 1: both halo rows per wave, three idle waves
    (258, 64, dict(vec=2, ry=2, wx=4, wy=4)),                                                    # 16 waves
    (260, 32, dict(vec=4, ry=2, wx=2, wy=4)),
]


@gpu
@pytest.mark.parametrize("n,precision,want", ONE_SLAB, ids=["n%d-fp%d" % (n, pr) for n, pr, _ in ONE_SLAB])
def test_one_step_at_every_launch_shape(shm, n, precision, want):
    """DIR of iteration 0 and RES of iteration 1 on one slab, every output against the reference at every node, on the instance the case names."""
    _case(shm, n, precision, 1, dict(want, overlap=0))


SLABS = [(65, 3, dict(VEC1, wx=2, wy=4, zc=8, zchunks=3, overlap=1)),        # planes 22 / 22 / 21: three chunks each, INTERIOR is a single chunk
         (129, 3, dict(VEC1, wx=4, wy=2, overlap=1)), (129, 5, dict(VEC1, wx=4, wy=2, overlap=1)),
         (33, 3, dict(VEC1, wx=1, wy=8, zchunks=2, overlap=0))]              # fewer than three chunks: halo exchange, then one FUSED_ALL sweep


@gpu
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("n,slabs,want", SLABS, ids=["n%d-slabs%d" % (n, sl) for n, sl, _ in SLABS])
def test_one_step_on_several_slabs(shm, n, slabs, want, precision):
    """The INTERIOR / BOUNDARY launches beside the halo exchange (or the exchange first), finalize_sum_kernel and the sum over the slabs.  The entry uploads z with
    NaN in its ghost planes: p' of a slab's ghost planes, and with it r' on both sides of every seam, is finite only if the exchange ran before the BOUNDARY
    chunks.  The seam planes' own worst ratio is printed beside the whole grid's."""
    _case(shm, n, precision, slabs, want)


@gpu
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("use_uw", [0, 1])
@pytest.mark.parametrize("it", [0, 1])
def test_parities_and_uw(shm, it, use_uw, precision):
    """n = 65: both parities of the iteration (direction buffers, rho and alpha slots swapped) with rho_new = red0 and red0 - u.w."""
    _case(shm, 65, precision, 1, dict(VEC1, wx=2, wy=4), it=it, use_uw=bool(use_uw))


@gpu
@pytest.mark.parametrize("precision", [64, 32])
def test_scalar_edges_and_repeatability(shm, precision):
    """n = 65, one handle.  init with p full of NaN: p' = -z bit for bit (p is not read), for both values of `it`.  rho_old = 0: beta = 0, p' = -z bit for bit.
    rho_new = 0: alpha = 0 and r' = r bit for bit.  The same input twice: the same bits in p', r' and the three scalars."""
    n = 65
    d = _bunny(n)
    cell = float(d["cell"])
    want = dict(VEC1, wx=2, wy=4)
    s = make_solver(shm, d, precision=precision)
    try:
        for it in (0, 1):
            run_step(shm, s, n, cell, precision, 1, want, seed=5, it=it, init=True, p_fill=np.nan, what="n=65 fp%d init it=%d, p = NaN" % (precision, it))
        run_step(shm, s, n, cell, precision, 1, want, seed=6, rho_old=0., what="n=65 fp%d rho_old = 0" % precision)
        run_step(shm, s, n, cell, precision, 1, want, seed=7, red0=0., what="n=65 fp%d rho_new = 0" % precision)
        first = run_step(shm, s, n, cell, precision, 1, want, seed=8, it=1, what="n=65 fp%d first of two" % precision)
        run_step(shm, s, n, cell, precision, 1, want, seed=9, what="n=65 fp%d another input between" % precision)
        again = run_step(shm, s, n, cell, precision, 1, want, seed=8, it=1, what="n=65 fp%d second of two" % precision)
    finally:
        s.close()
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]) and first[2] == again[2] and first[3] == again[3]


# ---- GPU: x update -------------------------------------------------------------------------------------------------------------------------------------------------
def _x_case(shm, s, n, precision, slabs, half, use_a, use_b, seed):
    x, pa, pb = _inputs(n, precision, seed)
    aa, ab = 0.731, -1.37
    pa_in = pa if use_a else np.full(n ** 3, np.nan)          # a switched-off direction must not reach x
    pb_in = pb if use_b else np.full(n ** 3, np.nan)
    got = s.cg_x_update(x, pa_in, pb_in, aa, ab, use_a=use_a, use_b=use_b, half=half)
    ref = StepRef(n, 1.0, precision)
    want, bound = ref.x_update(x, pa, pb, aa, ab, use_a, use_b)
    N, vec = n ** 3, _vec(n, precision)
    nlow = (N // vec // 2) * vec                              # the halves split at a vector boundary
    lo, hi = {-1: (0, N), 0: (0, nlow), 1: (nlow, N)}[half]
    outside = np.ones(N, dtype=bool)
    outside[lo:hi] = False
    assert np.array_equal(got[outside], x[outside]), "n=%d fp%d half %d: nodes outside the half moved" % (n, precision, half)
    ratio, _ = _ratio(np.abs(got[lo:hi] - want[lo:hi]), bound[lo:hi])
    assert ratio <= 1.0, (n, precision, slabs, half, use_a, use_b, ratio)
    if use_a or use_b:
        assert not np.array_equal(got[lo:hi], x[lo:hi])
    return ratio


@gpu
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("n", [11, 65, 130])
def test_x_update_halves_and_switches(shm, n, precision):
    """All nine combinations of half in {-1, 0, 1} with (use_a, use_b) in {(1, 1), (1, 0), (0, 1)}: per node inside the bound, nodes outside the half
    bit-identical to x, the split at floor(N / vec / 2) * vec, a switched-off direction (full of NaN) not read."""
    s = make_solver(shm, _bunny(n), precision=precision)
    items = []
    try:
        for half in (-1, 0, 1):
            for use_a, use_b in ((1, 1), (1, 0), (0, 1)):
                r = _x_case(shm, s, n, precision, 1, half, use_a, use_b, seed=n + 10 * half + use_a + 2 * use_b)
                items.append("half %d use (%d, %d): %.3f" % (half, use_a, use_b, r))
    finally:
        s.close()
    _line("cg_x_update n=%d fp%d vec %d, worst err/bound" % (n, precision, _vec(n, precision)), items)


@gpu
@pytest.mark.parametrize("precision", [64, 32])
def test_x_update_on_several_slabs(shm, precision):
    """n = 65 on three slabs: half = -1 updates every slab; the halves are refused there, as is any other value of half on one slab."""
    n = 65
    s = make_solver(shm, _bunny(n), precision=precision, local_slabs=3)
    try:
        r = _x_case(shm, s, n, precision, 3, -1, 1, 1, seed=3)
        v = np.zeros(n ** 3)
        for half in (0, 1):
            with pytest.raises(shm.ShmError) as e:
                s.cg_x_update(v, v, v, 1., 1., half=half)
            assert e.value.status == SHM_ERR_INVALID and str(e.value)
    finally:
        s.close()
    _line("cg_x_update n=65 fp%d three slabs" % precision, ["half -1: worst err/bound %.3f" % r])


# ---- GPU: state ------------------------------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("precision", [64, 32])
def test_state_after_the_entries(shm, precision):
    """After either entry get_phi and get_field(DIV) say SHM_ERR_STATE, and a following solve returns phi bit-identical to a fresh handle's."""
    n = 16
    d = _bunny(n)
    tol = 1e-10 if precision == 64 else 1e-5
    fresh = make_solver(shm, d, precision=precision)
    fresh.solve(tol=tol, solver="primal", precond="none")
    phi = fresh.get_phi()[0]
    fresh.close()
    z, p, r = _inputs(n, precision, 11)
    s = make_solver(shm, d, precision=precision)
    try:
        for entry in (lambda: s.cg_sweeps(z, p, r, 1.0, 0.4), lambda: s.cg_x_update(z, p, r, 0.5, 0.25)):
            s.solve(tol=tol, solver="primal", precond="none")
            assert np.array_equal(s.get_phi()[0], phi)
            entry()
            for call in (s.get_phi, lambda: s.get_field(s.FIELD_DIV), lambda: s.get_field(s.FIELD_PHI)):
                with pytest.raises(shm.ShmError) as e:
                    call()
                assert e.value.status == SHM_ERR_STATE
        s.solve(tol=tol, solver="primal", precond="none")
        assert np.array_equal(s.get_phi()[0], phi)
    finally:
        s.close()


@gpu
def test_refusals(shm):
    """SHM_ERR_STATE before set_problem; SHM_ERR_INVALID for every NULL argument and for a half outside {-1, 0, 1}."""
    n = 11
    v, out = np.zeros(n ** 3), np.zeros(n ** 3)
    sc, shape = np.zeros(3), np.zeros(8, dtype=np.int32)
    s = shm.GridSolver()
    lib = s._lib
    P = lambda a: a.ctypes.data                                                                      # noqa: E731
    assert lib.shm_grid_cg_sweeps(s._h, P(v), P(v), P(v), 1.0, 0.4, 0.0, 0, 0, 0, P(out), P(out), P(sc), P(shape)) == SHM_ERR_STATE
    assert lib.shm_grid_cg_x_update(s._h, P(v), P(v), P(v), 1.0, 1.0, 1, 1, -1, P(out)) == SHM_ERR_STATE
    s.close()
    s = make_solver(shm, _bunny(n))
    try:
        ok = [P(v), P(v), P(v), 1.0, 0.4, 0.0, 0, 0, 0, P(out), P(out), P(sc), P(shape)]
        for i in (0, 1, 2, 9, 10, 11, 12):
            args = list(ok)
            args[i] = None
            assert lib.shm_grid_cg_sweeps(s._h, *args) == SHM_ERR_INVALID, i
        assert lib.shm_grid_cg_sweeps(s._h, *ok) == 0
        ok = [P(v), P(v), P(v), 1.0, 1.0, 1, 1, -1, P(out)]
        for i in (0, 1, 2, 8):
            args = list(ok)
            args[i] = None
            assert lib.shm_grid_cg_x_update(s._h, *args) == SHM_ERR_INVALID, i
        for half in (-2, 2):
            args = list(ok)
            args[7] = half
            assert lib.shm_grid_cg_x_update(s._h, *args) == SHM_ERR_INVALID and lib.shm_grid_last_error(s._h)
        assert lib.shm_grid_cg_x_update(s._h, *ok) == 0
        with pytest.raises(ValueError):
            s.cg_sweeps(np.zeros(8), v, v, 1.0, 0.4)
    finally:
        s.close()
