"""Steps 1-2 at arbitrary points (shm_grid_field_at_points / _device, csrc/shm_field_points.hip.h): X(q) = sum_s w_s exp(-lambda r) / r and Y = X / |X| at points
of the caller's choosing, through the kernel, the C ABI, the Python bindings, the C++ host mirror and the CLI.

The yardstick is never the library: tests/field_points_ref.py restates the sum in numpy (plain fp64 sums; tests/test_field_points_host.py holds it to the
fixture's Y at every node) and derives the price of a point -- what two correct fp64 evaluations may differ by:
    price = 2 * 2^-53 * sum_s |w_s|_1 g_s (lambda r_s + S_padded + 8) / |X|.
EXACT is held to |dY|_inf <= price, AUTO to budget + price, the ratio |X| / L1 to a relative price + l1_rel (+ budget).  Every point of the seeded families is
finite and in zone (asserted), so no point is left out of any bound."""
import contextlib
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

# torch first: see tests/test_sample.py
try:
    import torch  # noqa: F401
except ImportError:
    torch = None

from conftest import ROOT, load_golden
import field_points_ref as ref

SHM_ERR_INVALID, SHM_ERR_STATE = 1, 7
CLI = os.environ.get("SHM_CLI") or os.path.join(ROOT, "signed-heat-3d_amd", "bin", "shm_grid_cli")
_CACHE = {}


def bunny():
    if "bunny" not in _CACHE:
        g = load_golden("bunny_small_n16")
        _CACHE["bunny"] = dict(pos=g["pos"], wnormal=g["wnormal"], area=g["area"], lam=float(g["lam"]), n=int(g["n"]), bbox_min=g["bbox_min"],
                               cell=float(g["cell"]), Y=g["Y"])
    return _CACHE["bunny"]


def family_ref(fam, Q=2000):
    """(points, yardstick) of a seeded family around the bunny: computed once, shared, never written to."""
    key = ("family", fam, Q)
    if key not in _CACHE:
        d = bunny()
        pts = ref.family(fam, d, Q, seed=11)
        y = ref.yardstick(d["pos"], d["wnormal"], d["lam"], pts)
        assert y["finite"].all() and (y["lam_rmin"] < ref.ZONE).all()      # the excluded share of these inputs is 0
        pts.setflags(write=False)
        _CACHE[key] = (pts, y)
    return _CACHE[key]


def solver(shm, d, **kw):
    s = shm.GridSolver(**kw)
    s.set_problem(d["pos"], d["wnormal"], d["area"], float(d["lam"]), int(d["n"]), d["bbox_min"], float(d["cell"]))
    return s


def bunny_solver(shm):
    if "bunny_solver" not in _CACHE:
        _CACHE["bunny_solver"] = solver(shm, bunny())
    return _CACHE["bunny_solver"]


def check(name, Y, r, y, budget=0.0):
    """|dY|_inf <= budget + price and the ratio within a relative budget + price + l1_rel, at every point; prints the figures first."""
    err = np.abs(Y - y["Y"]).max(axis=1)
    bound = budget + y["price"]
    print("%-28s Q %6d  max |dY| %.3e  max |dY| / bound %.3f" % (name, len(Y), err.max(), (err / bound).max()), end="")
    assert np.isfinite(Y).all()
    assert (err <= bound).all(), (name, int(np.argmax(err / bound)), float((err / bound).max()))
    if r is not None:
        rel = np.abs(r - y["ratio"]) / y["ratio"]
        rb = budget + y["price"] + y["l1_rel"]
        print("  max ratio err / bound %.3f" % (rel / rb).max(), end="")
        assert (rel <= rb).all(), (name, float((rel / rb).max()))
    print()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- 1. entry points ------------------------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_and_struct_layout(shm):
    """Both entries are exported and declared, ShmFieldStats follows the header field by field, and the ABI version did not move."""
    import re
    lib = shm.load_library()
    from signed_heat_3d_amd.grid_abi import ABI_SYMBOLS, ShmFieldStats
    header = open(os.path.join(ROOT, "include", "shm_grid.h")).read()
    for name in ("shm_grid_field_at_points", "shm_grid_field_at_points_device"):
        assert hasattr(lib, name) and (name + "(") in header and name in ABI_SYMBOLS, name
    body = header[header.index("typedef struct {\n    int64_t points, answered;"):header.index("} shm_field_stats;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}
    decl = [(nm.strip(), ctype[t]) for t, names in re.findall(r"\b(int32_t|int64_t|double)\s+([\w, ]+);", body) for nm in names.split(",")]
    assert decl == list(ShmFieldStats._fields_)
    assert C.sizeof(ShmFieldStats) == 80
    assert lib.shm_grid_abi_version() == 5


# ---- 2. EXACT against the yardstick --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("fam", ref.FAMILIES)
def test_exact_on_the_families(shm, fam):
    pts, y = family_ref(fam)
    s = bunny_solver(shm)
    Y, r, st = s.field_at_points(pts, arith="exact", ratio=True, stats=True)
    check("exact " + fam, Y, r, y)
    assert st["points"] == len(pts) and st["answered"] == len(pts) and st["out_of_zone"] == 0 and st["points_redone"] == 0
    assert st["pairs_evaluated"] == len(pts) * len(bunny()["area"]) and st["pairs_dropped"] == 0
    assert st["lambda"] == bunny()["lam"] and st["budget"] == 0.0 and st["arith"] == 1 and st["ms"] > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 63, 64, 65, 130])
def test_exact_at_the_edges_of_cluster_padding_and_wave(shm, S):
    """S at the edges of a cluster of 64 and of its padding, Q from one point to more than a workgroup's share.  (Lists this short run one point per wave;
    test_points_per_wave_at_the_edges repeats the grid with 2, 4 and 8.)"""
    d = ref.seeded_sources(S, seed=100 + S)
    s = solver(shm, d)
    rng = np.random.default_rng(S)
    allp = rng.uniform(-1.5, 1.5, (257, 3))
    y = ref.yardstick(d["pos"], d["wnormal"], d["lam"], allp)
    assert y["finite"].all() and (y["lam_rmin"] < ref.ZONE).all()
    for Q in (1, 3, 4, 5, 63, 64, 65, 257):
        for arith in ("exact", "auto"):
            Y, r, st = s.field_at_points(allp[:Q], arith=arith, ratio=True, stats=True)
            check("S %d Q %d %s" % (S, Q, arith), Y, r, {k: v[:Q] for k, v in y.items()}, budget=1e-8 if arith == "auto" else 0.0)
            assert st["answered"] == Q and st["pairs_evaluated"] + st["pairs_dropped"] == (Q + st["points_redone"]) * S


# ---- 3. EXACT at the nodes against the existing pipeline ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_exact_at_the_nodes_against_step1_and_the_fixture(shm):
    d = bunny()
    pts = ref.node_positions(d)
    y = ref.yardstick(d["pos"], d["wnormal"], d["lam"], pts)
    s = solver(shm, d)
    Y = s.field_at_points(pts, arith="exact")
    s.run_conv(step1="reference_f64")
    grid = np.stack([s.get_field(f) for f in (0, 1, 2)], axis=1)
    for name, other in (("Step 1 (reference_f64)", grid), ("the fixture", d["Y"]), ("the restatement", y["Y"])):
        err = np.abs(Y - other).max(axis=1)
        print("nodes against %-24s max |dY| %.3e  max |dY| / price %.3f" % (name, err.max(), (err / y["price"]).max()))
        assert (err <= y["price"]).all(), name


# ---- 4. AUTO ------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("fam", ref.FAMILIES)
def test_auto_on_the_families(shm, fam):
    pts, y = family_ref(fam)
    s = bunny_solver(shm)
    Y, r, st = s.field_at_points(pts, arith="auto", ratio=True, stats=True)
    check("auto " + fam, Y, r, y, budget=1e-8)
    S = len(bunny()["area"])
    print("   pairs dropped %.0f of %.0f, points redone %d" % (st["pairs_dropped"], len(pts) * S, st["points_redone"]))
    assert st["budget"] == 1e-8 and st["arith"] == 0 and st["answered"] == len(pts)
    assert st["pairs_evaluated"] + st["pairs_dropped"] == (len(pts) + st["points_redone"]) * S


def _two_blobs():
    if "blobs" not in _CACHE:
        d = ref.two_blobs()
        pts = 0.2 * np.random.default_rng(1).standard_normal((300, 3))
        y = ref.yardstick(d["pos"], d["wnormal"], d["lam"], pts)
        assert y["finite"].all() and (y["lam_rmin"] < ref.ZONE).all()
        _CACHE["blobs"] = (d, pts, y)
    return _CACHE["blobs"]


@pytest.mark.gpu
def test_auto_drops_the_far_blob_and_counts_its_pairs(shm):
    """Two blobs of 65 sources 3.0 apart, lambda 20: the second moves Y by 1e-17 and its whole cluster is dropped; the pair counts add up.  Budgets 1e-6, 1e-8
    and 1e-10: each within its own budget + price, and a tighter budget never drops more."""
    d, pts, y = _two_blobs()
    s = solver(shm, d)
    S, Q = len(d["area"]), len(pts)
    dropped = []
    for budget in (1e-6, 1e-8, 1e-10):
        Y, r, st = s.field_at_points(pts, arith="auto", budget=budget, ratio=True, stats=True)
        check("two blobs, budget %.0e" % budget, Y, r, y, budget=budget)
        print("   pairs dropped %.0f, points redone %d" % (st["pairs_dropped"], st["points_redone"]))
        assert st["budget"] == budget
        assert st["pairs_dropped"] > 0
        assert st["pairs_evaluated"] + st["pairs_dropped"] == Q * S + st["points_redone"] * S
        dropped.append(st["pairs_dropped"])
    assert dropped[0] >= dropped[1] >= dropped[2], dropped
    assert s.field_at_points(pts, arith="auto", budget=0.0, stats=True)[1]["budget"] == 1e-8


@pytest.mark.gpu
def test_auto_on_cancelling_sheets_needs_the_a_posteriori_test(shm):
    """Two 16 x 16 sheets of opposite weight at z = +-0.05, points just above the mid-plane (|X| / L1 ~ 1e-3), a blob of 64 sources at x = D.  At D = 1.4 the
    blob is worth a few 1e-10 of L1 -- inside a drop allowance taken against the largest term -- yet leaving it out moves Y by up to 2.7e-7: only the test of
    the dropped bound against |X_kept| keeps the budget.  Held at every D; somewhere among them the test must have fired."""
    pts = ref.sheet_points(300)
    redone = 0
    for D in (1.2, 1.4, 1.6):
        d = ref.cancelling_sheets(D)
        y = ref.yardstick(d["pos"], d["wnormal"], d["lam"], pts)
        assert y["finite"].all() and (y["lam_rmin"] < ref.ZONE).all() and y["ratio"].max() < 3e-3 and y["price"].max() < 2e-10
        s = solver(shm, d)
        Y, r, st = s.field_at_points(pts, arith="auto", ratio=True, stats=True)
        check("sheets, D %.1f" % D, Y, r, y, budget=1e-8)
        print("   pairs dropped %.0f, points redone %d" % (st["pairs_dropped"], st["points_redone"]))
        assert st["pairs_evaluated"] + st["pairs_dropped"] == (len(pts) + st["points_redone"]) * len(d["area"])
        redone += st["points_redone"]
    assert redone > 0


# ---- 5. per-point purity ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("arith", ["exact", "auto"])
def test_a_row_depends_on_its_point_alone(shm, arith):
    """The same points shuffled, a subset of them and a repeat call give bit-identical rows; the device entry gives the host entry's bits."""
    if torch is None or not torch.cuda.is_available():
        pytest.fail("torch with a HIP device is needed for the device entry point")
    pts, _ = family_ref("box")
    s = bunny_solver(shm)
    Y, r = s.field_at_points(pts, arith=arith, ratio=True)
    perm = np.random.default_rng(2).permutation(len(pts))
    Yp, rp = s.field_at_points(pts[perm], arith=arith, ratio=True)
    assert same_bits(Yp, Y[perm]) and same_bits(rp, r[perm])
    sub = np.sort(np.random.default_rng(3).choice(len(pts), 333, replace=False))
    Ys, rs = s.field_at_points(pts[sub], arith=arith, ratio=True)
    assert same_bits(Ys, Y[sub]) and same_bits(rs, r[sub])
    for q in (0, 1, 7, 1999):
        assert same_bits(s.field_at_points(pts[q:q + 1], arith=arith), Y[q:q + 1])
    Y2, r2 = s.field_at_points(pts, arith=arith, ratio=True)
    assert same_bits(Y2, Y) and same_bits(r2, r)
    t = torch.from_numpy(np.array(pts)).to("cuda:0")
    Yd, rd, st = s.field_at_points_device(t, arith=arith, ratio=True, stats=True)
    assert same_bits(Yd.cpu().numpy(), Y) and same_bits(rd.cpu().numpy(), r) and st["answered"] == len(pts)
    Yd1 = s.field_at_points_device(t[5:6].contiguous(), arith=arith)
    assert same_bits(Yd1.cpu().numpy(), Y[5:6])


@pytest.mark.gpu
def test_chunks_of_the_host_entry_do_not_show(shm):
    """Q = 2^20 + 3 with S = 65 (6.8e7 pairs): the rows on both sides of the chunk boundary equal the same points evaluated alone, 4096 seeded rows are within
    price, and the counts cover every point."""
    d = ref.seeded_sources(65, seed=7)
    s = solver(shm, d)
    Q = (1 << 20) + 3
    pts = np.random.default_rng(8).uniform(-1.5, 1.5, (Q, 3))
    Y, r, st = s.field_at_points(pts, arith="exact", ratio=True, stats=True)
    assert st["points"] == Q and st["answered"] == Q and st["pairs_evaluated"] == Q * 65.0
    edge = np.arange((1 << 20) - 2, (1 << 20) + 3)
    Ye, re_ = s.field_at_points(pts[edge], arith="exact", ratio=True)
    assert same_bits(Ye, Y[edge]) and same_bits(re_, r[edge])
    rows = np.random.default_rng(9).choice(Q, 4096, replace=False)
    y = ref.yardstick(d["pos"], d["wnormal"], d["lam"], pts[rows])
    assert y["finite"].all() and (y["lam_rmin"] < ref.ZONE).all()
    check("2^20 + 3, 4096 rows", Y[rows], r[rows], y)
    Ya = s.field_at_points(pts, arith="auto")
    assert same_bits(s.field_at_points(pts[edge], arith="auto"), Ya[edge])


@pytest.mark.gpu
def test_two_local_slabs_give_the_bits_of_one(shm):
    pts, _ = family_ref("box")
    one = bunny_solver(shm)
    two = solver(shm, bunny(), local_slabs=2)
    for arith in ("exact", "auto"):
        assert same_bits(two.field_at_points(pts, arith=arith), one.field_at_points(pts, arith=arith))


# ---- 5b. points per wave ----------------------------------------------------------------------------------------------------------------------------------------------
# A list shorter than 8192 points runs one point per wave on a 256-CU device (Solver::field_points_per_wave), so everything above except the 2^20-point call
# exercises P = 1 only.  SHM_FIELD_P (an experiment knob, read on every call) fixes P: with 2, 4 and 8 the points of a wave share the loaded clusters, keep
# different ones, a short last group repeats its last point, and lane p finishes point p.  None of it may show: rows bit-identical to the P = 1 rows, within
# the derived bound, and the same counts.
@contextlib.contextmanager
def points_per_wave(P):
    old = os.environ.get("SHM_FIELD_P")
    os.environ["SHM_FIELD_P"] = str(P)
    try:
        yield
    finally:
        if old is None:
            del os.environ["SHM_FIELD_P"]
        else:
            os.environ["SHM_FIELD_P"] = old


STAT_KEYS = ("points", "answered", "out_of_zone", "points_redone", "pairs_evaluated", "pairs_dropped")


def same_counts(a, b):
    return all(a[k] == b[k] for k in STAT_KEYS)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 63, 64, 65, 130])
def test_points_per_wave_at_the_edges(shm, S):
    """The S x Q grid of test_exact_at_the_edges_of_cluster_padding_and_wave with 2, 4 and 8 points per wave: Q = 1, 3, 5, 63, 65, 257 leave a short last group
    for every P, 4 and 64 fill whole groups of 2 and 4."""
    d = ref.seeded_sources(S, seed=100 + S)
    s = solver(shm, d)
    allp = np.random.default_rng(S).uniform(-1.5, 1.5, (257, 3))
    y = ref.yardstick(d["pos"], d["wnormal"], d["lam"], allp)
    assert y["finite"].all() and (y["lam_rmin"] < ref.ZONE).all()
    for arith in ("exact", "auto"):
        with points_per_wave(1):
            Y1, r1, st1 = s.field_at_points(allp, arith=arith, ratio=True, stats=True)
        check("S %d P 1 %s" % (S, arith), Y1, r1, y, budget=1e-8 if arith == "auto" else 0.0)
        for P in (2, 4, 8):
            with points_per_wave(P):
                for Q in (1, 3, 4, 5, 63, 64, 65, 257):
                    Y, r, st = s.field_at_points(allp[:Q], arith=arith, ratio=True, stats=True)
                    assert same_bits(Y, Y1[:Q]) and same_bits(r, r1[:Q]), (S, P, Q, arith)
                    assert st["points"] == Q and st["answered"] == Q and st["out_of_zone"] == 0
                    assert st["pairs_evaluated"] + st["pairs_dropped"] == (Q + st["points_redone"]) * S
                    if Q == 257:
                        assert same_counts(st, st1), (S, P, arith, st, st1)


@pytest.mark.gpu
@pytest.mark.parametrize("P", [2, 4, 8])
def test_points_per_wave_on_the_bunny_and_the_sheets(shm, P):
    """Wave neighbours that keep different clusters of a real source set.  Bunny (45 clusters), 1999 points of the near and box families interleaved -- odd, so
    the last group is short for every P -- in order, shuffled and as a subset; the cancelling sheets at D = 1.4, 299 points, where 136 points are summed
    again: rows and counts of P = 1, and the bounds."""
    near, yn = family_ref("near")
    box, yb = family_ref("box")
    pts = np.empty((1999, 3))
    pts[0::2], pts[1::2] = near[:1000], box[:999]
    y = {k: np.empty((1999,) + yn[k].shape[1:], dtype=yn[k].dtype) for k in yn}
    for k in y:
        y[k][0::2], y[k][1::2] = yn[k][:1000], yb[k][:999]
    s = bunny_solver(shm)
    S = len(bunny()["area"])
    for arith, budget in (("exact", 0.0), ("auto", 1e-8)):
        with points_per_wave(1):
            Y1, r1, st1 = s.field_at_points(pts, arith=arith, ratio=True, stats=True)
        with points_per_wave(P):
            Y, r, st = s.field_at_points(pts, arith=arith, ratio=True, stats=True)
            check("bunny P %d %s" % (P, arith), Y, r, y, budget=budget)
            assert same_bits(Y, Y1) and same_bits(r, r1) and same_counts(st, st1), (st, st1)
            assert st["pairs_evaluated"] + st["pairs_dropped"] == (1999 + st["points_redone"]) * S
            if arith == "auto":
                assert st["pairs_dropped"] > 0
            perm = np.random.default_rng(40 + P).permutation(1999)
            Yp, rp, stp = s.field_at_points(pts[perm], arith=arith, ratio=True, stats=True)
            assert same_bits(Yp, Y1[perm]) and same_bits(rp, r1[perm]) and same_counts(stp, st1)
            sub = np.sort(np.random.default_rng(50 + P).choice(1999, 333, replace=False))
            Ys, rs = s.field_at_points(pts[sub], arith=arith, ratio=True)
            assert same_bits(Ys, Y1[sub]) and same_bits(rs, r1[sub])
    d = ref.cancelling_sheets(1.4)
    sp = ref.sheet_points(300)[:299]
    ys = ref.yardstick(d["pos"], d["wnormal"], d["lam"], sp)
    ss = solver(shm, d)
    with points_per_wave(1):
        Y1, r1, st1 = ss.field_at_points(sp, arith="auto", ratio=True, stats=True)
    with points_per_wave(P):
        Y, r, st = ss.field_at_points(sp, arith="auto", ratio=True, stats=True)
    check("sheets P %d" % P, Y, r, ys, budget=1e-8)
    print("   pairs dropped %.0f, points redone %d" % (st["pairs_dropped"], st["points_redone"]))
    assert same_bits(Y, Y1) and same_bits(r, r1) and same_counts(st, st1), (st, st1)
    assert st["points_redone"] > 0 and st["pairs_dropped"] > 0
    assert st["pairs_evaluated"] + st["pairs_dropped"] == (299 + st["points_redone"]) * len(d["area"])


@pytest.mark.gpu
@pytest.mark.parametrize("P", [2, 4, 8])
def test_points_per_wave_nan_rules_and_fp32_device_entry(shm, P):
    """The planted NaN / inf / on-a-source rows of test_nan_rules among 301 good points (308 rows, the planted ones at group edges and inside groups), and the
    fp32 handle's device entry on 1999 float points: rows and counts of P = 1, in both modes."""
    if torch is None or not torch.cuda.is_available():
        pytest.fail("torch with a HIP device is needed for the device entry point")
    d = bunny()
    good, _ = family_ref("box")
    good = good[:301]
    bad = np.array([[np.nan, 0.1, 0.2], [0.1, np.inf, 0.2], [0.1, 0.2, -np.inf], [np.nan, np.nan, np.nan], d["pos"][0], d["pos"][1234], d["pos"][-1]])
    where = np.array([0, 3, 64, 65, 130, 255, 307])
    pts = np.empty((len(good) + len(bad), 3))
    mask = np.zeros(len(pts), dtype=bool)
    mask[where] = True
    pts[mask] = bad
    pts[~mask] = good
    s = bunny_solver(shm)
    s32 = solver(shm, d, precision=32)
    p32 = np.ascontiguousarray(family_ref("near")[0][:1999], dtype=np.float32)
    y32 = ref.yardstick(d["pos"], d["wnormal"], d["lam"], p32.astype(np.float64))
    assert y32["finite"].all() and (y32["lam_rmin"] < ref.ZONE).all()
    t = torch.from_numpy(p32).to("cuda:0")
    for arith, budget in (("exact", 0.0), ("auto", 1e-8)):
        with points_per_wave(1):
            Y0, r0 = s.field_at_points(good, arith=arith, ratio=True)
            Yd1, rd1, std1 = s32.field_at_points_device(t, arith=arith, ratio=True, stats=True)
        with points_per_wave(P):
            Y, r, st = s.field_at_points(pts, arith=arith, ratio=True, stats=True)
            Yd, rd, std = s32.field_at_points_device(t, arith=arith, ratio=True, stats=True)
        assert np.isnan(Y[mask]).all() and np.isnan(r[mask]).all()
        assert same_bits(Y[~mask], Y0) and same_bits(r[~mask], r0)
        assert st["points"] == len(pts) and st["answered"] == len(good) and st["out_of_zone"] == 0
        assert Yd.dtype == torch.float32 and torch.equal(Yd, Yd1) and torch.equal(rd, rd1) and same_counts(std, std1), (std, std1)
        err = np.abs(Yd.cpu().numpy().astype(np.float64) - y32["Y"]).max(axis=1)
        assert (err <= budget + y32["price"] + 2.0 ** -24).all()
        if arith == "auto":
            assert std["pairs_dropped"] > 0


# ---- 6. lambda ------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_lambda_argument(shm):
    """lam=0 is the problem's lambda bit for bit; lambda / 2 and 2 lambda are each within the price computed for that lambda."""
    d = bunny()
    pts, _ = family_ref("box")
    pts = pts[:500]
    s = bunny_solver(shm)
    for arith in ("exact", "auto"):
        assert same_bits(s.field_at_points(pts, lam=0.0, arith=arith), s.field_at_points(pts, lam=d["lam"], arith=arith))
    for f in (0.5, 2.0):
        y = ref.yardstick(d["pos"], d["wnormal"], f * d["lam"], pts)
        assert y["finite"].all() and (y["lam_rmin"] < ref.ZONE).all()
        Y, r, st = s.field_at_points(pts, lam=f * d["lam"], arith="exact", ratio=True, stats=True)
        check("lambda x %.1f exact" % f, Y, r, y)
        assert st["lambda"] == f * d["lam"]
        Y, r = s.field_at_points(pts, lam=f * d["lam"], arith="auto", ratio=True)
        check("lambda x %.1f auto" % f, Y, r, y, budget=1e-8)


# ---- 7. NaN rules -----------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("arith", ["exact", "auto"])
def test_nan_rules(shm, arith):
    """NaN and infinite coordinates and copies of source positions among good points: exactly those rows are NaN (Y and ratio), answered is Q minus their
    number, and every other row is bit-identical to the run without them."""
    d = bunny()
    good, _ = family_ref("box")
    good = good[:301]
    s = bunny_solver(shm)
    Y0, r0 = s.field_at_points(good, arith=arith, ratio=True)
    bad = np.array([[np.nan, 0.1, 0.2], [0.1, np.inf, 0.2], [0.1, 0.2, -np.inf], [np.nan, np.nan, np.nan], d["pos"][0], d["pos"][1234], d["pos"][-1]])
    where = np.array([0, 3, 64, 65, 130, 255, 307])      # positions of the planted rows in the combined array (first, last, wave and workgroup edges)
    pts = np.empty((len(good) + len(bad), 3))
    mask = np.zeros(len(pts), dtype=bool)
    mask[where] = True
    pts[mask] = bad
    pts[~mask] = good
    Y, r, st = s.field_at_points(pts, arith=arith, ratio=True, stats=True)
    assert np.isnan(Y[mask]).all() and np.isnan(r[mask]).all()
    assert same_bits(Y[~mask], Y0) and same_bits(r[~mask], r0)
    assert st["points"] == len(pts) and st["answered"] == len(good) and st["out_of_zone"] == 0


# ---- 8. state and purity of the handle -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_state_and_argument_checks(shm):
    if torch is None or not torch.cuda.is_available():
        pytest.fail("torch with a HIP device is needed for the device entry point")
    d = bunny()
    pts, y = family_ref("box")
    pts = pts[:200]
    s = shm.GridSolver()
    with pytest.raises(shm.ShmError) as e:
        s.field_at_points(pts)
    assert e.value.status == SHM_ERR_STATE
    s.set_problem(d["pos"], d["wnormal"], d["area"], d["lam"], d["n"], d["bbox_min"], d["cell"])
    Y = s.field_at_points(pts, arith="exact")                     # after set_problem alone: no solve, no run_conv
    check("after set_problem alone", Y, None, {k: v[:200] for k, v in y.items()})
    with pytest.raises(shm.ShmError) as e:
        s.get_field(0)                                            # ... and it did not pretend a Step 1 had run
    assert e.value.status == SHM_ERR_STATE
    assert s.field_at_points(np.zeros((0, 3)), stats=True)[1]["points"] == 0      # Q = 0 is fine

    lib, h = s._lib, s._h
    st = shm.ShmFieldStats()
    out = np.empty((200, 3))
    p = np.array(pts)

    def refused(rc, word):
        msg = lib.shm_grid_last_error(h).decode()
        assert rc == SHM_ERR_INVALID and word in msg, (rc, msg)

    refused(lib.shm_grid_field_at_points(h, -1, p.ctypes.data, 0.0, 0, 0.0, out.ctypes.data, None, C.byref(st)), "Q < 0")
    refused(lib.shm_grid_field_at_points(h, 200, None, 0.0, 0, 0.0, out.ctypes.data, None, C.byref(st)), "null")
    refused(lib.shm_grid_field_at_points(h, 200, p.ctypes.data, 0.0, 0, 0.0, None, None, C.byref(st)), "null")
    refused(lib.shm_grid_field_at_points(h, 200, p.ctypes.data, -1.0, 0, 0.0, out.ctypes.data, None, C.byref(st)), "lambda")
    refused(lib.shm_grid_field_at_points(h, 200, p.ctypes.data, float("nan"), 0, 0.0, out.ctypes.data, None, C.byref(st)), "lambda")
    refused(lib.shm_grid_field_at_points(h, 200, p.ctypes.data, float("inf"), 0, 0.0, out.ctypes.data, None, C.byref(st)), "lambda")
    refused(lib.shm_grid_field_at_points(h, 200, p.ctypes.data, 0.0, 0, 1e-13, out.ctypes.data, None, C.byref(st)), "budget")
    refused(lib.shm_grid_field_at_points(h, 200, p.ctypes.data, 0.0, 0, 1e-2, out.ctypes.data, None, C.byref(st)), "budget")
    refused(lib.shm_grid_field_at_points(h, 200, p.ctypes.data, 0.0, 7, 0.0, out.ctypes.data, None, C.byref(st)), "arith")
    assert lib.shm_grid_field_at_points(h, 200, p.ctypes.data, 0.0, 1, 1e-2, out.ctypes.data, None, None) == 0    # exact mode ignores the budget; stats may be NULL
    t = torch.from_numpy(p).to("cuda:0")
    o = torch.empty((200, 3), dtype=torch.float64, device="cuda:0")
    refused(lib.shm_grid_field_at_points_device(h, 200, p.ctypes.data, 0.0, 0, 0.0, o.data_ptr(), None, C.byref(st)), "device memory")
    refused(lib.shm_grid_field_at_points_device(h, 1 << 40, t.data_ptr(), 0.0, 0, 0.0, o.data_ptr(), None, C.byref(st)), "fewer")
    refused(lib.shm_grid_field_at_points_device(h, 200, t.data_ptr(), 0.0, 0, 0.0, None, None, C.byref(st)), "null")
    assert same_bits(s.field_at_points(pts, arith="exact"), Y)    # the handle works on after the refusals


@pytest.mark.gpu
def test_resident_fields_are_untouched(shm):
    """After a full solve, phi and Y read the same bits before and after the call, in both modes and through both entries."""
    if torch is None or not torch.cuda.is_available():
        pytest.fail("torch with a HIP device is needed for the device entry point")
    d = bunny()
    s = solver(shm, d)
    s.solve(tol=1e-8)
    before = [s.get_phi()[0]] + [s.get_field(f) for f in (0, 1, 2)]
    pts, _ = family_ref("near")
    s.field_at_points(pts, arith="exact", ratio=True)
    s.field_at_points(pts, arith="auto", lam=2.0 * d["lam"])
    s.field_at_points_device(torch.from_numpy(np.array(pts)).to("cuda:0"), arith="auto")
    after = [s.get_phi()[0]] + [s.get_field(f) for f in (0, 1, 2)]
    for a, b in zip(before, after):
        assert same_bits(a, b)


# ---- 9. fp32 handle -------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_fp32_handle(shm):
    """The arithmetic is fp64 in an fp32 handle: the host entry gives the fp64 handle's bits, the device entry takes float tensors and its results are the
    fp64 results at the float-rounded points rounded once -- within price + 2^-24 of the yardstick there."""
    if torch is None or not torch.cuda.is_available():
        pytest.fail("torch with a HIP device is needed for the device entry point")
    d = bunny()
    pts, _ = family_ref("box")
    s32 = solver(shm, d, precision=32)
    for arith in ("exact", "auto"):
        assert same_bits(s32.field_at_points(pts, arith=arith), bunny_solver(shm).field_at_points(pts, arith=arith))
    p32 = np.ascontiguousarray(pts, dtype=np.float32)
    y = ref.yardstick(d["pos"], d["wnormal"], d["lam"], p32.astype(np.float64))
    assert y["finite"].all() and (y["lam_rmin"] < ref.ZONE).all()
    t = torch.from_numpy(p32).to("cuda:0")
    for arith, budget in (("exact", 0.0), ("auto", 1e-8)):
        Y, r, st = s32.field_at_points_device(t, arith=arith, ratio=True, stats=True)
        assert Y.dtype == torch.float32 and r.dtype == torch.float32 and st["answered"] == len(pts)
        err = np.abs(Y.cpu().numpy().astype(np.float64) - y["Y"]).max(axis=1)
        bound = budget + y["price"] + 2.0 ** -24
        print("fp32 handle, device entry, %s: max |dY| %.3e, max |dY| / bound %.3f" % (arith, err.max(), (err / bound).max()))
        assert (err <= bound).all()
        rel = np.abs(r.cpu().numpy().astype(np.float64) - y["ratio"]) / y["ratio"]
        assert (rel <= budget + y["price"] + y["l1_rel"] + 2.0 ** -24).all()
    with pytest.raises(ValueError):
        s32.field_at_points_device(torch.from_numpy(np.array(pts)).to("cuda:0"))


# ---- 10. CLI and mirror -------------------------------------------------------------------------------------------------------------------------------------------------
def test_cli_help_lists_the_field_flags():
    p = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert p.returncode == 0
    for flag in ("--field-at <file>", "--field-out <file>", "--field-lambda <L>", "--field-arith <auto|exact>", "--field-budget <B>"):
        assert flag in p.stdout, flag


@pytest.mark.gpu
def test_cli_and_mirror_reproduce_the_python_path(shm, tmp_path):
    """shm_grid_cli data/bunny_small.obj --g --h 0 --field-at F --field-out G, the C++ mirror's vectorFieldAt and GridSolver.field_at_points on the same
    sources: bit for bit the same Y, and the CLI's line carries the stats."""
    from signed_heat_3d_amd.host_abi import HostSolver
    mesh = os.path.join(ROOT, "data", "bunny_small.obj")
    host = HostSolver(mesh, tol=1e-8)
    pre = host.preprocess(hCoef=0.0)
    d = dict(pos=pre["pos"], wnormal=pre["wnormal"], area=pre["area"], lam=pre["lam"], n=pre["n"], bbox_min=pre["bbox_min"], cell=pre["cell"])
    pts = np.concatenate([ref.family("box3", d, 700, seed=21), ref.family("near", d, 300, seed=22)])
    s = solver(shm, d)
    host.compute_distance(hCoef=0.0)
    for arith, extra in (("auto", []), ("exact", ["--field-arith", "exact"]), ("auto", ["--field-budget", "1e-6", "--field-lambda", "7.5"])):
        kw = dict(arith=arith)
        if extra and extra[0] == "--field-budget":
            kw.update(budget=1e-6, lam=7.5)
        Y, st = s.field_at_points(pts, stats=True, **kw)
        Ym, rm, stm = host.vector_field_at(pts, ratio=True, stats=True, **kw)
        assert same_bits(Ym, Y) and stm["pairs_dropped"] == st["pairs_dropped"] and stm["answered"] == len(pts)
        assert same_bits(rm, s.field_at_points(pts, ratio=True, **kw)[1])
        pts.astype("<f8").tofile(tmp_path / "q.f64")
        p = subprocess.run([CLI, mesh, "--g", "--h", "0", "--field-at", str(tmp_path / "q.f64"), "--field-out", str(tmp_path / "y.f64")] + extra,
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        assert same_bits(np.fromfile(tmp_path / "y.f64", dtype="<f8").reshape(-1, 3), Y)
        line = [l for l in p.stderr.splitlines() if l.startswith("field at points:")]
        assert len(line) == 1, p.stderr
        for word in ("points %d" % len(pts), "answered %d" % len(pts), "out_of_zone 0", "points_redone %d" % st["points_redone"],
                     "pairs_evaluated %.0f" % st["pairs_evaluated"], "pairs_dropped %.0f" % st["pairs_dropped"], "budget", "arith %d" % st["arith"], " ms "):
            assert word in line[0], (word, line[0])
