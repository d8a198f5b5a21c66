"""The inverse of G = A A^T in every form the device has, on constraint sets built to order.  Which form runs depends only on the number of rows m and on where the
source cells lie (csrc/shm_solver.hip.h: enqueue_gj_invert, build_two_level), and rows are "one per distinct cell, in source order": one source per chosen cell
(ginv_ref.fill) gives exactly the m, the boxes and the separator wanted.  The sets (ginv_ref.SETS):
  dense_4032 ... dense_6144   63 pivot blocks (the last size of the one-launch-per-pivot-block form) and 64, 65, 66, 68, 96: the outer form with outer blocks of four
                              pivot blocks -- padded and not, tails of one, two and no pivot block;
  default_box                 6145 random cells: the two-level split at its default box of 16 cells, no knob;
  shapes                      boxes of exactly 1, 63, 64, 65, 129 and 2048 rows at the default box, boxes with no, 64 and 65 separator columns, a separator row that
                              no box borders, a colour without a box, 63 padded separator rows;
  fallback                    a box of 2049 rows: the library drops to boxes of 8;
  sheet                       6400 rows, none interior: the partition does not fit and the dense inverse runs at 100 pivot blocks;
  small_boxes                 boxes of one and of two pivot blocks in one batch (SHM_TL_MIN_M=32, SHM_TL_BOX=8).
Without a GPU: every set has the shape it was built for (a drifting set fails here and does not silently test less); the fp64 numpy block elimination
(ginv_ref.two_level_solve) agrees with the refined reference, and seeded defects in it do not; the restated partition equals the library's.
On the GPU: stage C of test_stage_edges.py unchanged -- its _projector_case and _projector_errors, the random v, the v of null(A), bit-equal untouched nodes, A P v,
P P v, P A^T w -- with the refined reference passed in and THE BOUND TAKEN FROM NUMPY'S OWN ERROR ON THE SAME INPUT: 8 E + 16 * 2^-53 of max|v|, E the error of
np.linalg.inv(G) @ w (dense sets) or of two_level_solve (two-level sets) against the refined reference, pushed through A^T.  The factor 8 is the project's rule for
"the same arithmetic in another order" (stage E, test_dual_operator.py).  The bound is computed in the test, never read from the device, and never above the figures
stage C holds on the fixtures.  And shm_grid_spd_solve at the sizes that reach the outer form, against numpy refined on a long-double residual."""
import contextlib
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import ginv_ref
from ginv_ref import DENSE_M, SETS, TWO_LEVEL, HostProjector, partition, problem, rows_of, two_level_solve
from test_ldl_solve_gpu import CONDS, SIZES, _system
from test_stage_edges import PROJ_FP64, PROJ_TWO_LEVEL, U, _projector_case, _round_to

gpu = pytest.mark.gpu
FACTOR = 8                      # device error <= FACTOR * (numpy's error on the same input) + FLOOR * 2^-53 max|v|
FLOOR = 16


# ---- shared references ----------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(name):
    """(problem, cells, HostProjector from the restated rows, partition or None) of a set, built once."""
    d, cells = problem(name)
    c2, nodes, coeffs = rows_of(d)
    assert np.array_equal(c2, cells)
    box = SETS[name][1]
    return d, cells, HostProjector(nodes, coeffs, int(d["n"]) ** 3), (partition(cells, box) if box else None)


def _random_v(N, precision):
    """The first vector _projector_case draws (default_rng(1)), rounded to the handle's precision as it rounds it."""
    return _round_to(np.random.default_rng(1).standard_normal(N), precision)


def _pushed(P, mu, mu_ref, v):
    """An error of the multipliers as the projector shows it: max|A^T (mu - mu_ref)| / max|v|."""
    return float(np.abs(P.A.T @ (mu - mu_ref)).max() / np.abs(v).max())


# ---- without a GPU: the sets -------------------------------------------------------------------------------------------------------------------------------------------
# What each two-level set was built to be, read off partition(): a changed seed or fill has to change these lines too.
EXPECTED = {
    "default_box": dict(m=6145, n=33, fits=True, box=16, P=8, nS=1066, nI=5079, maxs=658, maxc=197, colours={c: 1 for c in range(8)}),
    "shapes": dict(m=6200, n=49, fits=True, box=16, P=26, nS=1089, nI=5111, maxs=2048, maxc=65, colours={0: 8, 1: 4, 2: 4, 3: 2, 4: 4, 5: 2, 6: 2}),
    "fallback": dict(m=6249, n=33, fits=True, box=8, P=64, nS=1778, nI=4471, maxs=222, maxc=131, colours={c: 8 for c in range(8)}),
    "sheet": dict(m=6400, n=81, fits=False, box=16, P=0, nS=6400),
    "small_boxes": dict(m=1442, n=33, fits=True, box=8, P=16, nS=330, nI=1112, maxs=128, maxc=14, colours={0: 8, 4: 8}),
}


def _colours(part):
    out = {}
    for bx in part["boxes"]:
        out[bx["colour"]] = out.get(bx["colour"], 0) + 1
    return out


@pytest.mark.parametrize("m", DENSE_M)
def test_dense_sets_have_the_pivot_blocks_they_were_built_for(m):
    """m distinct cells of the 33^3 grid, at most 6144 of them (the dense form is planned), and the pivot-block counts of the table: 63 is the last stepped size,
    64 the first outer one; 65 and 66 leave a tail outer block of one and two pivot blocks, 68 and 96 none; 4033, 4097 and 4300 are padded, 4224 and 6144 not."""
    d, cells, P, part = _reference("dense_%d" % m)
    assert part is None and int(d["n"]) == 33 and P.G.shape[0] == m == len(np.unique(cells, axis=0)) and m <= 6144
    nb = (m + 63) // 64
    assert nb == {4032: 63, 4033: 64, 4097: 65, 4224: 66, 4300: 68, 6144: 96}[m]
    assert (nb < 64) == (m == 4032) and nb % 4 == {63: 3, 64: 0, 65: 1, 66: 2, 68: 0, 96: 0}[nb] and (64 * nb - m) == {4032: 0, 4033: 63, 4097: 63, 4224: 0, 4300: 52, 6144: 0}[m]


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_two_level_sets_have_the_shape_they_were_built_for(name):
    d, cells, P, part = _reference(name)
    want = EXPECTED[name]
    assert len(cells) == want["m"] > (6144 if name != "small_boxes" else 32) and int(d["n"]) == want["n"]
    for key in ("fits", "box", "P", "nS"):
        assert part[key] == want[key], (key, part[key])
    if not part["fits"]:
        return
    for key in ("nI", "maxs", "maxc"):
        assert part[key] == want[key], (key, part[key])
    assert _colours(part) == want["colours"]
    assert part["nI"] + part["nS"] == want["m"] and part["nSp"] % 64 == 0 and 0 <= part["nSp"] - part["nS"] < 64
    s_c = {bx["key"]: (len(bx["rows"]), len(bx["cols"])) for bx in part["boxes"]}
    if name == "shapes":
        for key, s in ginv_ref.SHAPE_ROWS.items():
            assert s_c[key][0] == s, (key, s_c[key])
        for key, c in ginv_ref.SHAPE_COLS.items():
            assert s_c[key][1] == c, (key, s_c[key])
        assert ginv_ref.SHAPE_EMPTY not in s_c and 7 not in _colours(part)             # the colour without a box
        assert max(_colours(part).values()) >= 4                                        # several boxes in one Schur pass
        assert part["nS"] % 64 == 1                                                     # 63 padded separator rows
        bordered = {c for bx in part["boxes"] for c in bx["cols"]}
        lone = int(np.flatnonzero((cells[part["sep"]] == ginv_ref.SHAPE_LONE_SEP).all(axis=1))[0])
        assert lone not in bordered and len(bordered) < part["nS"]                      # a separator row that no box borders
        assert {(s + 63) // 64 for s, _ in s_c.values()} >= {1, 2, 3, 32}               # boxes of different pivot-block counts in one batch
        assert {(c + 63) // 64 for _, c in s_c.values()} >= {0, 1, 2}                   # no, one and two 64-column chunks
    if name == "small_boxes":
        assert sorted(s for s, _ in s_c.values()) == sorted(ginv_ref.SMALL_ROWS)
        assert sum(s <= 64 for s, _ in s_c.values()) >= 4 and sum(65 <= s <= 128 for s, _ in s_c.values()) >= 4
    if name == "fallback":
        inside = cells[(cells % 16 != 0).all(axis=1)] // 16
        assert max(np.bincount(np.ravel_multi_index(inside.T, (2, 2, 2)))) == 2049      # one row more than a box of 16 may hold: hence the boxes of 8


# ---- without a GPU: the yardstick of the two-level sets --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _two_level_case(name):
    d, cells, P, part = _reference(name)
    v = _random_v(int(d["n"]) ** 3, 64)
    w = P.A @ v
    return P, part, v, w, P.solve(w), P.cond()


@pytest.mark.parametrize("name", TWO_LEVEL)
def test_two_level_solve_agrees_with_the_refined_reference(name):
    """The fp64 block elimination against the sparse LU refined on a long-double residual, pushed through A^T: at most 64 * 2^-53 * cond(G) of max|v|."""
    P, part, v, w, mu_ref, cond = _two_level_case(name)
    e = _pushed(P, two_level_solve(P.G, part, w), mu_ref, v)
    print("\n%s: m %d cond(G) %.2e, two_level_solve vs refined reference %.2e of max|v| (bound %.2e)" % (name, len(w), cond, e, 64 * U[64] * cond))
    assert e <= 64 * U[64] * cond


def _defects(part):
    """The seeded defects for a partition: a colour pass skipped (the colour of the box with the most separator columns), E_a^T t dropped for that box, the padded
    tail of the separator not zero."""
    a = int(np.argmax([len(bx["cols"]) for bx in part["boxes"]]))
    assert len(part["boxes"][a]["cols"]) > 0 and part["nSp"] > part["nS"]
    return [("skip_colour", part["boxes"][a]["colour"]), ("drop_Et", a), ("tail", 1.0)]


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("name", TWO_LEVEL)
def test_seeded_defects_in_the_restatement_fail_that_check(name, kind):
    """The yardstick could be wrong in the same way as the device: each defect seeded into two_level_solve misses the bound of the check above."""
    P, part, v, w, mu_ref, cond = _two_level_case(name)
    defect = _defects(part)[kind]
    e = _pushed(P, two_level_solve(P.G, part, w, defect=defect), mu_ref, v)
    print("\n%s, %s: %.2e of max|v| (bound %.2e)" % (name, defect, e, 64 * U[64] * cond))
    assert e > 64 * U[64] * cond


# ---- without a GPU: the restated partition against the library's ------------------------------------------------------------------------------------------------------
def _library_partitions(exe, d, tmp_path):
    """tests/native/test_constraints.cpp on a problem: {box request: (header dict, [per box dict(colour, rows, cols)])} from what it prints."""
    pos = np.ascontiguousarray(d["pos"], dtype=np.float64)
    head = np.concatenate([[float(d["n"]), float(len(pos)), float(d["cell"])], np.asarray(d["bbox_min"], dtype=np.float64)])
    np.concatenate([head, pos.ravel(), np.asarray(d["area"], dtype=np.float64)]).tofile(tmp_path / "in.f64")
    out = subprocess.run([exe, str(tmp_path / "in.f64"), str(tmp_path / "out"), "1"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-3000:] + out.stderr[-3000:]
    parts, cur = {}, None
    for line in out.stdout.splitlines():
        f = line.split()
        if line.startswith("partition:"):
            head = {f[i]: int(f[i + 1]) for i in range(1, len(f), 2)}
            cur = parts[head["request"]] = (head, [])
        elif line.startswith("  box "):
            cur[1].append(dict(colour=int(f[3]), s=int(f[5]), c=int(f[7])))
        elif line.startswith("    rows") or line.startswith("    cols"):
            cur[1][-1][f[0]] = [int(x) for x in f[1:]]
    return parts


@pytest.mark.parametrize("build", ["plain", "sanitizers"])
def test_restated_partition_equals_the_library(build, tmp_path):
    """two_level_partition itself (the host program of test_constraints_host.py, plain and under ASan + UBSan, stand-alone) on the small_boxes set, box requests 4
    and 8: the same box size, counts, box order, colours, rows and separator columns in the same order as partition()."""
    flags = ["-O2"] if build == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    exe = str(tmp_path / "test_constraints")
    subprocess.check_call(["g++", *flags, "-std=c++17", "-Wall", "-Wextra", os.path.join(ROOT, "tests", "native", "test_constraints.cpp"), "-o", exe])
    d, cells, _, _ = _reference("small_boxes")
    lib = _library_partitions(exe, d, tmp_path)
    assert sorted(lib) == [4, 8]
    for box, (head, boxes) in lib.items():
        part = partition(cells, box)
        assert part["fits"]
        assert head == dict(request=box, box=part["box"], P=part["P"], nI=part["nI"], nS=part["nS"], nSp=part["nSp"], maxs=part["maxs"], maxc=part["maxc"])
        assert len(boxes) == part["P"]
        for got, want in zip(boxes, part["boxes"]):
            assert got["colour"] == want["colour"] and got["rows"] == want["rows"] and got["cols"] == want["cols"] and got["s"] == len(want["rows"]) and got["c"] == len(want["cols"])


# ---- on the GPU: the projector ------------------------------------------------------------------------------------------------------------------------------------------
PLAN_LINE = re.compile(r"\[shm\] plan: .*G\^-1 (two-level|dense)")
TL_LINE = re.compile(r"\[shm\] two-level inverse of A A\^T: box (\d+), (\d+) boxes \((\d+) interior rows, largest box (\d+) rows x (\d+) separator columns\), separator (\d+) rows")
# set -> the (precision, local_slabs) of its handles; the first also holds the three properties of stage C and, on two sets, bit-equal repeats
CONFIGS = {name: [(64, 1)] for name in SETS}
CONFIGS["dense_4097"] = CONFIGS["default_box"] = [(64, 1), (32, 1), (64, 3), (32, 3)]
REPEATS = ("dense_4097", "default_box")


@contextlib.contextmanager
def _stderr_to(path):
    """The process's stderr (file descriptor 2: where a verbose handle logs) into a file."""
    sys.stderr.flush()
    saved = os.dup(2)
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o600)
    try:
        os.dup2(fd, 2)
        yield
    finally:
        sys.stderr.flush()
        os.dup2(saved, 2)
        os.close(fd)
        os.close(saved)


def _numpy_multipliers(name, P, part, w, cache):
    """What numpy gives in fp64 for (A A^T)^-1 w in the form the device uses for this set: the explicit inverse, or the block elimination."""
    if part is not None and part["fits"]:
        return two_level_solve(P.G, part, w)
    if "Ginv" not in cache:
        cache["Ginv"] = np.linalg.inv(P.G.toarray())
    return cache["Ginv"] @ w


def _run_set(shm, name):
    """Every handle of CONFIGS[name] through _projector_case with the refined reference; the bound from numpy's error on the same input.  A list of result dicts."""
    from test_gpu_parity import make_solver
    d, cells, _, part = _reference(name)
    n = int(d["n"])
    two_level = part is not None and part["fits"]
    cap = PROJ_TWO_LEVEL if two_level else PROJ_FP64
    out, cache, P = [], {}, None
    for i, (precision, slabs) in enumerate(CONFIGS[name]):
        s = make_solver(shm, d, precision=precision, local_slabs=slabs, verbose=True)
        nodes, coeffs = s.get_constraints()
        if P is None:
            assert np.array_equal(ginv_ref.cells_of_nodes(nodes, n), cells)       # the rows are the chosen cells, in the chosen order
            P = HostProjector(nodes, coeffs, n ** 3)
        v = _random_v(n ** 3, precision)
        if precision not in cache:
            w = P.A @ v
            cache[precision] = _pushed(P, _numpy_multipliers(name, P, part, w, cache), P.solve(w), v)
        E = cache[precision]
        tol = FACTOR * E + FLOOR * U[64]
        assert tol <= cap, "%s: the bound %.2e exceeds stage C's %.0e: the fill is too ill-conditioned" % (name, tol, cap)
        r = _projector_case(s, n, precision, tol, i == 0, P=P)
        if name in REPEATS:
            r["repeat_equal"] = bool(np.array_equal(s.apply_projector(v), s.apply_projector(v)))
        s.close()
        r.update(precision=precision, slabs=slabs, E=E, tol=tol)
        out.append(r)
    return out


def _check_path(name, log):
    """The plan line and the two-level line of a verbose handle's log against the set's partition.  Returns the lines seen."""
    d, cells, _, part = _reference(name)
    plans = set(PLAN_LINE.findall(log))
    lines = set(TL_LINE.findall(log))
    assert plans == {"dense" if part is None else "two-level"}, (name, plans, log[-2000:])
    if part is None or not part["fits"]:
        assert not lines, (name, lines)                     # dense sets; does not fit: planned two-level, no two-level inverse built
        return "G^-1 %s, no two-level line" % plans.pop()
    want = tuple(str(part[k]) for k in ("box", "P", "nI", "maxs", "maxc", "nS"))
    assert lines == {want}, (name, lines, want)
    return "G^-1 two-level; box %s, %s boxes (%s interior rows, largest box %s rows x %s separator columns), separator %s rows" % want


def _report(name, res, path):
    print("\n%s: %s" % (name, path))
    for r in res:
        print("  fp%d slabs %d m %d: numpy's E %.2e, bound %.2e of max|v|; random v max|d| %.2e, error / bound %.3f; null(A) v max|d| %.2e, error / bound %.3f, moved by %.2e; "
              "%d untouched nodes bit-equal%s" % (r["precision"], r["slabs"], r["m"], r["E"], r["tol"], r["e_rand"], r["r_rand"], r["e_null"], r["r_null"], r["moved"], r["untouched"],
                                                 "; repeat bit-equal: %s" % r["repeat_equal"] if "repeat_equal" in r else ""))
    for r in res:
        assert r["r_rand"] <= 1.0 and r["r_null"] <= 1.0, (name, r)
        assert r.get("repeat_equal", True), (name, "two calls on the same handle and input differ", r)


@gpu
@pytest.mark.parametrize("m", DENSE_M)
def test_projector_dense_inverse_at_the_pivot_block_edges(shm, m, tmp_path):
    """The dense inverse of G at 63 (stepped), 64, 65, 66, 68 and 96 pivot blocks (outer blocks of four, GJ_CROSS / GJ_REST, the tail outer block), held to
    8 x the error of np.linalg.inv(G) @ w on the same input plus 16 * 2^-53, of max|v|; m = 4097 also on fp32 handles and on three slabs, and two calls bit-equal."""
    name = "dense_%d" % m
    log = str(tmp_path / "log.txt")
    with _stderr_to(log):
        res = _run_set(shm, name)
    with open(log) as fh:
        path = _check_path(name, fh.read())
    _report(name, res, path)


_CHILD = r"""
import sys, json
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import shm_import
shm = shm_import.load()
import test_ginv_edges as t
json.dump(t._run_set(shm, %(name)r), open(%(out)r, "w"))
"""


@gpu
@pytest.mark.parametrize("name", ["default_box", "shapes", "fallback", "sheet", "small_boxes"])
def test_projector_two_level_inverse_on_sets_built_to_order(name, tmp_path):
    """The two-level inverse at its default box (no knob), on the shaped boxes, after the fallback to boxes of 8, where the partition does not fit (the dense inverse
    at 100 pivot blocks) and on boxes of one and two pivot blocks in one batch -- each in a child process under its own time limit (the library reads its knobs once
    per process; a verbose handle logs to the child's stderr).  The log must show the form taken with partition()'s numbers.  Bound: 8 x the error of
    two_level_solve (sheet: of np.linalg.inv) on the same input plus 16 * 2^-53, of max|v|; default_box also on fp32 handles and on three slabs, and two calls
    bit-equal."""
    out = str(tmp_path / "res.json")
    code = _CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"), name=name, out=out)
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **SETS[name][2]), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    with open(out) as fh:
        res = json.load(fh)
    _report(name, res, _check_path(name, p.stderr))


# ---- on the GPU: shm_grid_spd_solve -------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _spd_truth(m, cond):
    """(S, rhs, truth, E_inv): _system of test_ldl_solve_gpu.py, numpy's solve refined three times on a long-double residual, and the error of
    np.linalg.inv(S) @ rhs against it (max norm)."""
    S, rhs, ref = _system(m, cond)
    Sl, rl = S.astype(np.longdouble), rhs.astype(np.longdouble)
    u = ref.copy()
    for _ in range(3):
        u = u + np.linalg.solve(S, (rl - (Sl * u.astype(np.longdouble)).sum(axis=1)).astype(np.float64))   # (row by row: numpy's long-double matmul crawls at m = 4096)
    return S, rhs, u, float(np.abs(np.linalg.inv(S) @ rhs - u).max())


def _spd_case(solver, m, cond, forms):
    S, rhs, truth, e_inv = _spd_truth(m, cond)
    bound = FACTOR * e_inv + FLOOR * U[64] * float(np.abs(truth).max())
    worst = 0.
    for form in forms:
        u, flag = solver.spd_solve(S, rhs, form)
        assert flag == 0, (form, flag)
        e = float(np.abs(u - truth).max())
        print("m %d cond %.0e %s: max|u - truth| %.3e, numpy's inverse %.3e, bound %.3e, error / bound %.3f" % (m, cond, form, e, e_inv, bound, e / bound))
        worst = max(worst, e / bound)
    assert worst <= 1.0, (m, cond, worst)


@pytest.fixture(scope="module")
def spd_solver(shm):
    return shm.GridSolver()


@gpu
@pytest.mark.parametrize("cond", CONDS)
@pytest.mark.parametrize("m", [4032, 4033, 4096])
def test_spd_solve_at_the_sizes_of_the_outer_form(shm, spd_solver, m, cond):
    """63 pivot blocks (both forms) and 64 (the explicit inverse in its outer form, with the pivot kernel of the callers that refine; the factorisation must refuse
    with SHM_ERR_INVALID), padded (4033) and not (4096): each form within 8 E_inv + 16 * 2^-53 max|u| of numpy refined on a long-double residual, E_inv the error
    of np.linalg.inv(S) @ rhs against the same."""
    S, rhs, _, _ = _spd_truth(m, cond)
    if m > 4032:
        with pytest.raises(shm.ShmError) as e:
            spd_solver.spd_solve(S, rhs, "factor")
        assert e.value.status == 1   # SHM_ERR_INVALID
    _spd_case(spd_solver, m, cond, ("factor", "invert") if m == 4032 else ("invert",))


@gpu
@pytest.mark.parametrize("cond", CONDS)
@pytest.mark.parametrize("m", SIZES)
def test_spd_solve_absolute_bound_at_the_small_sizes(spd_solver, m, cond):
    """The same absolute bound at the sizes of test_ldl_solve_gpu.py, whose own assertions compare the two forms with each other."""
    _spd_case(spd_solver, m, cond, ("factor", "invert"))
