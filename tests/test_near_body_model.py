"""The near tier's e^{-lambda r} / r (yukawa_near, csrc/shm_conv_tiered.hip.h) modelled on the host in exact rational arithmetic: the 12-instruction chain of rounds 5-6
and the 11-instruction chain that folds the Newton step into the exponent scale, every fma / mul / add rounded correctly to double (float(Fraction) does that), v_rsq_f64
as 1 / sqrt(x) with a relative error of up to 2^-24 (both signs, the extremes included), the reference 2^(r c / 2048) / r from `decimal` at 50 digits.
What the new chain adds is ONE rounding, of cc = |c| (1 + e), inside the exponent: at most 2^-53 |r c| ln 2 / 2048 relative in the term -- 7.7e-14 at the edge of the
2^-990 span the host allows a block (Solver::tier_exponent_span_ok) -- and the 1 / |c| pre-scaling of the staged weights two more of 2^-53 (1 / |c| itself, w / |c|).
So: max relative error of the new chain <= that of the old chain on the same sample + 7.7e-14 + 2^-52, over the whole sample and bin by bin in |r c|.
(It comes out no larger at all: the old chain's r = fma(t, e, t) carried the rounding that cc carries now.  Measured: 2.000e-11 old, 1.994e-11 new over the sample,
both the Newton residual 1.5 (2^-24)^2 times the exponent.)  7.7e-14 is the formula at |r c| = 990 * 2048, the widest span of a block, but the sample -- r up to 1e3
cells at lambda * cell up to 4 -- holds exponents |r c| of up to 5770 octaves, where one rounding is 4.4e-13: a bin that reaches beyond 990 octaves is held to the
formula at its own largest exponent, every bin below and the whole sample to the constant.
The second half holds the compiler's near loop to its instruction count (tools/step1_isa_check.py; no GPU)."""
import decimal
import os
import random
from fractions import Fraction as F

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

A1 = 3.384507729693224e-04           # kNearA1
A2 = 5.727446245172041e-08           # (ln2/2048)^2 / 2
BIG = 6755399441055744.0             # 1.5 * 2^52
BOUND_EXTRA = 7.7e-14 + 2.0 ** -52
N_SAMPLES = 20000
BIN_EDGES = [0.0, 1.0, 10.0, 30.0, 70.0, 150.0, 350.0, 990.0, 2500.0, float("inf")]     # |r c| / 2048: octaves of the term's exponent

decimal.getcontext().prec = 50
D = decimal.Decimal
LN2 = D(2).ln()


def fma(a, b, c):
    """a b + c exactly (doubles are ratios of integers), rounded once: float(Fraction) rounds correctly."""
    (an, ad), (bn, bd), (cn, cd) = a.as_integer_ratio(), b.as_integer_ratio(), c.as_integer_ratio()
    return float(F(an * bn * cd + cn * ad * bd, ad * bd * cd))


def mul(a, b):
    (an, ad), (bn, bd) = a.as_integer_ratio(), b.as_integer_ratio()
    return float(F(an * bn, ad * bd))


def _table():
    return [float((D(j) / 2048 * LN2).exp()) for j in range(2048)]


def _low_word(tm):
    """The low 32 bits of tm's mantissa as a signed integer (tm in [2^52, 2^53): ulp 1)."""
    ki = int(tm) & 0xffffffff
    return ki - (1 << 32) if ki >= 1 << 31 else ki


def old_chain(x, y0, c, k0, tab):
    """Rounds 5-6.  Returns (mantissa of the term before the table's power of two, that power, f, ki, exact r c)."""
    m1 = BIG - 2048.0 * k0
    t = mul(x, y0)
    h = 0.5 * y0
    e = fma(-t, h, 0.5)
    r = fma(t, e, t)
    rinv = fma(y0, e, y0)
    tm = fma(r, c, m1)
    kf = tm - m1
    ki = _low_word(tm)
    f = fma(r, c, -kf)
    p = fma(fma(A2, f, A1), f, 1.0)
    j = ki & 2047
    g = mul(tab[j], mul(p, rinv))
    return F(g), (ki - j) >> 11, f, ki, F(r) * F(c)


def new_chain(x, y0, c, k0, tab, w):
    """Round 7: returns the term ON THE OLD SCALE -- |c| g times the staged weight w' = rn(w rn(1 / |c|)), over w."""
    m1 = BIG - 2048.0 * k0
    c1, c2 = -c, -0.5 * c
    t = mul(x, y0)
    e2 = fma(-t, y0, 1.0)
    cc = fma(e2, c2, c1)
    tm = fma(-t, cc, m1)
    kf = tm - m1
    ki = _low_word(tm)
    f = fma(-t, cc, -kf)
    q = mul(y0, cc)
    p = fma(fma(A2, f, A1), f, 1.0)
    j = ki & 2047
    g = mul(tab[j], mul(p, q))
    cinv = float(1 / F(c1))
    ws = mul(w, cinv)
    return F(g) * F(ws) / F(w), (ki - j) >> 11, f, ki, -F(t) * F(cc)


def _round_half_even(q):
    return round(q)     # Fraction.__round__: to the nearest integer, ties to even


def _samples():
    rng = random.Random(7)
    out = []
    for i in range(N_SAMPLES):
        r = 10.0 ** rng.uniform(-3.0, 3.0)                   # cells (the cell is the unit of length)
        lam = 0.15 * (4.0 / 0.15) ** rng.random()            # lambda * cell
        if i % 50 == 0:
            r, lam = 10.0 ** rng.uniform(2.5, 3.0), rng.uniform(2.0, 4.0)      # the far corner of the ranges: thousands of octaves
        x = r * r
        c = -lam * 2954.639443740597
        octaves = abs(r * c) / 2048.0
        # the block's exponent: 2^k0 ~ e^{-lambda d0} with d0 <= r, the term up to 990 octaves below it
        u = (0.0, 1.0, rng.random(), rng.random())[i % 4] * min(990.0, octaves)
        k0 = min(0, int(-(octaves - u) // 1))
        if -octaves - k0 < -990.0:
            k0 -= 1
        delta = (F(1, 1 << 24), F(-1, 1 << 24), F(rng.randrange(-(1 << 30), (1 << 30) + 1), 1 << 54), F(0))[(i // 4) % 4]
        w = 1.0 + rng.random()
        out.append((x, c, k0, delta, w))
    return out


@pytest.fixture(scope="module")
def model_errors():
    """Per sample: (octaves of |r c|, relative error of the old chain, of the new chain, f and ki - round(product) + 2048 k0 of both, distance of ki from the true r c)."""
    tab = _table()
    rows = []
    for x, c, k0, delta, w in _samples():
        rt = D(x).sqrt()
        y0 = float(F(1 / rt) * (1 + delta))
        E = rt * D(c) / 2048
        res = []
        for chain in (old_chain(x, y0, c, k0, tab), new_chain(x, y0, c, k0, tab, w)):
            g, kk, f, ki, prod = chain
            ref = ((E - k0 - kk) * LN2).exp() / rt              # 2^(r c / 2048 - k0) / r with the chain's power of two taken off
            err = abs(D(g.numerator) / D(g.denominator) / ref - 1)
            res.append((float(err), f, ki - (_round_half_even(prod) - 2048 * k0), abs(D(ki + 2048 * k0) - rt * D(c))))
        rows.append((float(abs(E)), res[0], res[1]))
    return rows


def test_new_chain_is_within_the_derived_bound_of_the_old(model_errors):
    worst_old = max(r[1][0] for r in model_errors)
    worst_new = max(r[2][0] for r in model_errors)
    print("\nnear body model, %d samples: max relative error old chain %.3e, new chain %.3e (bound: old + %.2e)" % (len(model_errors), worst_old, worst_new, BOUND_EXTRA))
    assert worst_new <= worst_old + BOUND_EXTRA
    for lo, hi in zip(BIN_EDGES[:-1], BIN_EDGES[1:]):
        rows = [r for r in model_errors if lo <= r[0] < hi]
        assert len(rows) >= 100, (lo, hi, len(rows))
        o, n = max(r[1][0] for r in rows), max(r[2][0] for r in rows)
        # 7.7e-14 is 2^-53 |r c| ln 2 / 2048 at |r c| = 990 * 2048, the widest SPAN of a block; the sample (r up to 1e3 cells at lambda * cell up to 4) holds
        # exponents |r c| of up to 5770 octaves, and there the same formula is what one rounding can add
        top = max(r[0] for r in rows)
        extra = max(BOUND_EXTRA, 2.0 ** -53 * top * 0.6931471805599453 + 2.0 ** -52)
        print("  |r c| / 2048 in [%6g, %6g): %5d samples, old %.3e new %.3e (new - old %+.2e, bound %.2e)" % (lo, hi, len(rows), o, n, n - o, extra))
        assert n <= o + extra, (lo, hi, o, n)


def test_remainder_and_exponent_word(model_errors):
    """f -- the rounding error of the fma that forms tm -- stays within [-1/2, 1/2], the low word of tm is round(r c) - 2048 k0 (r c: the chain's own product, exact),
    and it is the integer nearest to the TRUE r c - 2048 k0 up to the chain's error in r c."""
    for _, old, new in model_errors:
        for err, f, dki, off in (old, new):
            assert -0.5 <= f <= 0.5, f
            assert dki == 0, dki
            assert off <= D("0.5") + D("1e-6"), off


def test_near_loop_instruction_count():
    """The compiler's near loop (one source against a lane's four nodes) of both instantiations: 100 instructions where rounds 5-6 had 104, still four v_rsq_f64 and
    at most two s_nop; the far loops as tests/test_abi_and_host.py holds them."""
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    import importlib.util
    spec = importlib.util.spec_from_file_location("step1_isa_check", os.path.join(ROOT, "tools", "step1_isa_check.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    r = mod.loops()      # (a loop is found BY its four v_rsq_f64_e32)
    for name in ("fp64 solve near loop", "fp32 solve near loop"):
        assert name in r, r
        assert r[name]["instructions"] <= 100 and r[name]["s_nop"] <= 2, (name, r[name])
    assert r["fp64 solve far loop"]["instructions"] <= 128 and r["fp32 solve far loop"]["instructions"] <= 120, r
