"""Host references for the inverse of G = A A^T (tests/test_ginv_edges.py), in numpy / scipy, no GPU:
  fill()            a problem with one source per chosen cell, so that the rows of A are exactly the chosen cells, in the chosen order (build_rows: "one row per
                    distinct cell, in source order");
  rows_of()         the rows of A for such a problem, restating build_rows (csrc/shm_constraints.h);
  partition()       two_level_partition's rules restated: separator, boxes in order of first appearance, their rows and separator columns, colours, the fallback of
                    the box size 16 -> 8 -> 4, "does not fit";
  two_level_solve() the block elimination of csrc/shm_twolevel.hip.h's header in fp64 numpy, in the device's order -- with three defects that can be seeded, so that a
                    test can show that the check which holds it would notice them;
  HostProjector     _HostProjector of test_stage_edges.py with a sparse LU of G and three steps of iterative refinement on a long-double residual;
  the constraint sets of the tests, each built to reach one form of the inverse (SETS)."""
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as sl

K_GJ = 64          # pivot block of the blocked Gauss-Jordan (kGJ)
TL_MAX_BOX = 2048  # rows / separator columns of a box (kTlMaxBox)
CORNERS = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)])   # the order of Row::nodes (build_rows)


# ---- problems -------------------------------------------------------------------------------------------------------------------------------------------------------
def fill(n, cells, seed):
    """One source per cell of `cells` ((m, 3) distinct cells of 0 .. n - 2, kept in order) on the unit grid of n nodes per side: trilinear parameters uniform in
    (0.15, 0.85); normals and areas arbitrary, finite and non-zero (the projector never reads them).  Cell size 1 and origin 0: the library's floor() and its
    parameters (b - c) / 1 are then exact, so rows_of() below gives the library's coefficients."""
    cells = np.asarray(cells, dtype=np.int64)
    assert cells.ndim == 2 and cells.shape[1] == 3 and cells.min() >= 0 and cells.max() <= n - 2
    assert len(np.unique(cells, axis=0)) == len(cells), "cells repeat"
    rng = np.random.default_rng(seed)
    m = len(cells)
    t = rng.uniform(0.15, 0.85, (m, 3))
    nrm = rng.standard_normal((m, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    area = rng.uniform(0.5, 1.5, m)
    return dict(pos=cells + t, wnormal=nrm * area[:, None], area=area, lam=1.0, n=n, bbox_min=np.zeros(3), cell=1.0)


def rows_of(d):
    """(cells, nodes, coeffs) of the constraint rows of a fill() problem: build_rows restated (one source per cell, so one row per source)."""
    n, h, b0 = int(d["n"]), float(d["cell"]), np.asarray(d["bbox_min"], dtype=np.float64)
    pos = np.asarray(d["pos"], dtype=np.float64)
    c = np.floor((pos - b0) / h).astype(np.int64)
    t = (pos - (c * h + b0)) / h
    nodes = np.stack([(c[:, 0] + o[0]) + n * ((c[:, 1] + o[1]) + n * (c[:, 2] + o[2])) for o in CORNERS], axis=1)
    tx, ty, tz = t[:, 0], t[:, 1], t[:, 2]
    coeffs = np.stack([(1. - tx) * (1. - ty) * (1. - tz), tx * (1. - ty) * (1. - tz), (1. - tx) * ty * (1. - tz), (1. - tx) * (1. - ty) * tz,
                       tx * ty * (1. - tz), tx * (1. - ty) * tz, (1. - tx) * ty * tz, tx * ty * tz], axis=1)
    return c, nodes, coeffs


def cells_of_nodes(nodes, n):
    """The cell of every row from its first corner (what get_constraints() of a handle returns)."""
    g = np.asarray(nodes)[:, 0]
    return np.stack([g % n, (g // n) % n, g // (n * n)], axis=1)


# ---- the partition ----------------------------------------------------------------------------------------------------------------------------------------------------
def _g_columns(cells):
    """Per row the columns of G in the library's order (assemble_G: the row's corners in Row::nodes order, per corner the rows that touch it, ascending), as a
    function row -> list."""
    row_of = {tuple(c): r for r, c in enumerate(cells.tolist())}

    def cols(r):
        i, j, k = cells[r]
        out, seen = [], set()
        for o in CORNERS.tolist():
            ni, nj, nk = i + o[0], j + o[1], k + o[2]
            touching = sorted(q for q in (row_of.get((ni - a, nj - b, nk - c)) for a in (0, 1) for b in (0, 1) for c in (0, 1)) if q is not None)
            for q in touching:
                if q not in seen:
                    seen.add(q)
                    out.append(q)
        return out
    return cols


def partition(cells, box=16):
    """two_level_partition(rows, G, box) restated from its rules.  A dict: fits, box (the size used), P, nI, nS, nSp, maxs, maxc, sep (global row of every separator
    slot), boxes (per box: key = box coordinates, colour, rows = global rows, cols = separator slots in order of first appearance along its rows)."""
    cells = np.asarray(cells, dtype=np.int64)
    m = len(cells)
    cols_of = _g_columns(cells)
    out = dict(fits=False)
    for b in (box if box > 1 else 16, 8, 4):
        is_sep = (cells % b == 0).any(axis=1)
        sep = np.flatnonzero(is_sep)
        slot = np.full(m, -1)
        slot[sep] = np.arange(len(sep))
        ids, boxes = {}, []
        for r in np.flatnonzero(~is_sep).tolist():                      # boxes in order of first appearance along the rows
            key = tuple((cells[r] // b).tolist())
            if key not in ids:
                ids[key] = len(boxes)
                boxes.append(dict(key=key, colour=(key[0] & 1) | ((key[1] & 1) << 1) | ((key[2] & 1) << 2), rows=[], cols=[]))
            boxes[ids[key]]["rows"].append(r)
        out.update(box=b, P=len(boxes), nS=len(sep), sep=sep, boxes=boxes)
        if len(boxes) == 0 or len(sep) == 0:                            # no interior row or no separator row: the dense inverse it is (no smaller box is tried)
            return out
        for bx in boxes:
            seen = set()
            for r in bx["rows"]:
                for c in cols_of(r):
                    if is_sep[c] and c not in seen:
                        seen.add(c)
                        bx["cols"].append(int(slot[c]))
        out["maxs"] = max(len(bx["rows"]) for bx in boxes)
        out["maxc"] = max(len(bx["cols"]) for bx in boxes)
        if out["maxs"] <= TL_MAX_BOX and out["maxc"] <= TL_MAX_BOX:
            break
        if b == 4:
            return out
    out["fits"] = True
    out["nI"] = sum(len(bx["rows"]) for bx in out["boxes"])
    out["nSp"] = (out["nS"] + K_GJ - 1) // K_GJ * K_GJ
    return out


# ---- the block elimination ----------------------------------------------------------------------------------------------------------------------------------------------
def two_level_solve(G, part, w, defect=None):
    """u = G^-1 w by the block elimination of shm_twolevel.hip.h, fp64 numpy, in the device's order: D_a^-1 per box (np.linalg.inv), T_a = D_a^-1 E_a, the Schur
    complement S = F - sum_a E_a^T T_a on the separator padded to whole pivot blocks (identity tail), one pass per colour, np.linalg.inv(S), then per
    application t = D^-1 w_I, v_S = w_S - sum_a E_a^T t_a, u_S = S^-1 v_S, u_I = t - T u_S.
    defect seeds one of the mistakes the device could make: ("skip_colour", c): the Schur pass of colour c is left out; ("drop_Et", a): E_a^T t_a is not taken
    off v_S for box a; ("tail", x): the padded tail of the separator is not cleared -- x stands in the padded rows of v_S and in the padding of S beside the
    separator's rows."""
    G = sp.csr_matrix(G)
    w = np.asarray(w, dtype=np.float64)
    kind, arg = defect if defect is not None else (None, None)
    sep, nS, nSp = part["sep"], part["nS"], part["nSp"]
    S = np.zeros((nSp, nSp))
    S[:nS, :nS] = G[sep][:, sep].toarray()
    S[np.arange(nS, nSp), np.arange(nS, nSp)] = 1.0
    if kind == "tail":
        S[nS:, :nS] = arg
        S[:nS, nS:] = arg
    blocks = []
    for bx in part["boxes"]:
        I, cols = np.asarray(bx["rows"]), np.asarray(bx["cols"], dtype=np.int64)
        Gi = G[I]
        Dinv = np.linalg.inv(Gi[:, I].toarray())
        E = Gi[:, sep[cols]].toarray() if len(cols) else np.zeros((len(I), 0))
        blocks.append((I, cols, Dinv, E, Dinv @ E))
    for colour in range(8):
        if kind == "skip_colour" and colour == arg:
            continue
        for (I, cols, Dinv, E, T), bx in zip(blocks, part["boxes"]):
            if bx["colour"] == colour and len(cols):
                S[np.ix_(cols, cols)] -= E.T @ T
    Sinv = np.linalg.inv(S)
    vS = np.zeros(nSp)
    vS[:nS] = w[sep]
    if kind == "tail":
        vS[nS:] = arg
    ts = []
    for a, (I, cols, Dinv, E, T) in enumerate(blocks):
        t = Dinv @ w[I]
        ts.append(t)
        if len(cols) and not (kind == "drop_Et" and a == arg):
            vS[cols] -= E.T @ t
    uS = Sinv @ vS
    u = np.zeros_like(w)
    u[sep] = uS[:nS]
    for (I, cols, Dinv, E, T), t in zip(blocks, ts):
        u[I] = t - (T @ uS[cols] if len(cols) else 0.)
    return u


# ---- the reference projector --------------------------------------------------------------------------------------------------------------------------------------------
class HostProjector:
    """P = I - A^T (A A^T)^-1 A in fp64 on the host: _HostProjector of test_stage_edges.py with a sparse LU of G (m up to about 6500 in under a second) and three
    steps of iterative refinement whose residual w - G mu is formed in long double."""

    def __init__(self, nodes, coeffs, N):
        m = nodes.shape[0]
        self.A = sp.csr_matrix((coeffs.ravel(), (np.repeat(np.arange(m), 8), nodes.ravel())), shape=(m, N))   # (duplicate entries are summed)
        G = (self.A @ self.A.T).tocsr()
        G.sum_duplicates()
        self.G = G
        self.lu = sl.splu(G.tocsc())
        self._data = G.data.astype(np.longdouble)
        self.touched = np.zeros(N, dtype=bool)
        self.touched[nodes.ravel()] = True

    def residual(self, w, mu):
        """w - G mu in long double, rounded to fp64 once (every row of G holds its diagonal, so no row is empty)."""
        prod = self._data * mu.astype(np.longdouble)[self.G.indices]
        return (w.astype(np.longdouble) - np.add.reduceat(prod, self.G.indptr[:-1])).astype(np.float64)

    def solve(self, w):
        mu = self.lu.solve(w)
        for _ in range(3):
            mu = mu + self.lu.solve(self.residual(w, mu))
        return mu

    def __call__(self, v):
        return v - self.A.T @ self.solve(self.A @ v)

    def cond(self):
        """cond_2(G) from the largest eigenvalues of G and of its inverse (Lanczos on G and on the LU solve)."""
        m = self.G.shape[0]
        lmax = sl.eigsh(self.G, 1, which="LA", return_eigenvectors=False, tol=1e-4)[0]
        imax = sl.eigsh(sl.LinearOperator((m, m), matvec=self.lu.solve, dtype=np.float64), 1, which="LA", return_eigenvectors=False, tol=1e-4)[0]
        return float(lmax * imax)


# ---- the constraint sets ----------------------------------------------------------------------------------------------------------------------------------------------
def all_cells(n):
    """Every cell of the grid, (i, j, k) with i fastest."""
    k, j, i = np.meshgrid(np.arange(n - 1), np.arange(n - 1), np.arange(n - 1), indexing="ij")
    return np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1)


def _pick(rng, cells, count):
    assert 0 <= count <= len(cells), (count, len(cells))
    return cells[rng.choice(len(cells), count, replace=False)]


def _interior(cells, box, key=None):
    """Mask of the cells strictly inside a box (of box coordinates `key`, or any)."""
    mask = (cells % box != 0).all(axis=1)
    return mask if key is None else mask & (cells // box == np.asarray(key)).all(axis=1)


def _without(cells, drop):
    """The cells not listed in `drop`."""
    if len(drop) == 0:
        return cells
    base = int(max(cells.max(), np.asarray(drop).max())) + 1
    code = lambda c: (np.asarray(c)[:, 0] * base + np.asarray(c)[:, 1]) * base + np.asarray(c)[:, 2]
    return cells[~np.isin(code(cells), code(drop))]


def dense_cells(m):
    """m random distinct cells of the 33^3 grid."""
    return 33, _pick(np.random.default_rng(4000 + m), all_cells(33), m)


def default_box_cells():
    """6145 random cells of the 33^3 grid: the first size of the two-level split, at its default box of 16 cells -- eight boxes, one per colour."""
    return 33, _pick(np.random.default_rng(6145), all_cells(33), 6145)


# Shapes at the default box, n = 49: 27 boxes of 16^3 cells, separator planes at the cell coordinates 0, 16, 32.
SHAPE_ROWS = {(2, 0, 0): 1, (2, 2, 0): 63, (0, 0, 0): 64, (0, 2, 0): 65, (0, 0, 2): 129, (2, 2, 2): 2048}   # box -> interior rows, exactly
SHAPE_COLS = {(2, 0, 0): 0, (0, 0, 0): 64, (0, 2, 0): 65}                                                    # box -> separator columns, exactly
SHAPE_EMPTY = (1, 1, 1)               # the only box of colour 7: cleared
SHAPE_LONE_SEP = (16, 16, 16)         # a separator row that no box borders: the eight interior cells at its corners are kept free
SHAPE_NS = 17 * 64 + 1                # separator rows: 63 padded rows
SHAPE_M = 6200


def shapes_cells():
    """The set of the table above, filled up at random elsewhere to 6200 rows.  The boxes (0, 0, 0) and (0, 2, 0) hold one layer of cells beside the separator plane
    i = 0 (an 8 x 8 patch, and the patch plus one cell) and the separator holds exactly the cells across it: 64 and 65 separator columns; the other separator cells
    next to those layers are kept free."""
    n, b = 49, 16
    rng = np.random.default_rng(49)
    cells = all_cells(n)
    patch = [(y, z) for z in range(4, 12) for y in range(4, 12)]
    forced_int, forced_sep, keep_free = [], [], []
    for key, yz in (((0, 0, 0), patch), ((0, 2, 0), patch + [(12, 4)])):
        oy, oz = b * key[1], b * key[2]
        forced_int += [(1, oy + y, oz + z) for y, z in yz]
        forced_sep += [(0, oy + y, oz + z) for y, z in yz]
        ring = {(y + dy, z + dz) for y, z in yz for dy in (-1, 0, 1) for dz in (-1, 0, 1)} - set(yz)
        keep_free += [(0, oy + y, oz + z) for y, z in ring]
    forced_int.append((2 * b + 8, 8, 8))                                   # the lone cell in the middle of its box: no separator column
    forced_sep.append(SHAPE_LONE_SEP)
    keep_free += [(16 + dx, 16 + dy, 16 + dz) for dx in (-1, 1) for dy in (-1, 1) for dz in (-1, 1)]
    free = _without(cells, np.array(keep_free + forced_int + forced_sep))
    parts = [np.array(forced_int), np.array(forced_sep)]
    for key, s in SHAPE_ROWS.items():                                       # the shaped boxes that are filled at random
        if key not in ((2, 0, 0), (0, 0, 0), (0, 2, 0)):
            parts.append(_pick(rng, free[_interior(free, b, key)], s))
    shaped = np.array(list(SHAPE_ROWS) + [SHAPE_EMPTY])
    plain = _interior(free, b) & ~(free[:, None, :] // b == shaped[None, :, :]).all(axis=2).any(axis=1)   # interiors of the twenty other boxes
    parts.append(_pick(rng, free[~_interior(free, b)], SHAPE_NS - len(forced_sep)))
    parts.append(_pick(rng, free[plain], SHAPE_M - SHAPE_NS - sum(SHAPE_ROWS.values())))
    out = np.concatenate(parts)
    return n, out[rng.permutation(len(out))]


def fallback_cells():
    """One box of 2049 rows at box 16 (and 4200 random cells elsewhere) on the 33^3 grid: the library must drop to boxes of 8."""
    rng = np.random.default_rng(2049)
    cells = all_cells(33)
    inside = _interior(cells, 16, (0, 0, 0))
    out = np.concatenate([_pick(rng, cells[inside], 2049), _pick(rng, cells[~inside], 4200)])
    return 33, out[rng.permutation(len(out))]


def sheet_cells():
    """Every cell of the sheet k = 16 of the 81^3 grid, m = 6400: above the dense limit, and no row is interior to a box."""
    cells = all_cells(81)
    return 81, cells[cells[:, 2] == 16]


SMALL_ROWS = [63, 64, 65, 128, 100, 1, 127, 40, 64, 65, 96, 33, 128, 2, 66, 70]   # interior rows of the sixteen populated boxes: one and two pivot blocks
SMALL_SEP = 330


def small_box_cells():
    """About 1500 rows on the 33^3 grid for boxes of 8 (forced by SHM_TL_MIN_M=32, SHM_TL_BOX=8): sixteen boxes (every box with even box coordinates in i and j)
    with the interior row counts of SMALL_ROWS -- one pivot block and two in the same batch -- and 330 random separator cells."""
    rng = np.random.default_rng(8)
    cells = all_cells(33)
    keys = [(bi, bj, bk) for bk in range(4) for bj in (0, 2) for bi in (0, 2)]
    parts = [_pick(rng, cells[_interior(cells, 8, key)], s) for key, s in zip(keys, SMALL_ROWS)]
    parts.append(_pick(rng, cells[~_interior(cells, 8)], SMALL_SEP))
    out = np.concatenate(parts)
    return 33, out[rng.permutation(len(out))]


DENSE_M = [4032, 4033, 4097, 4224, 4300, 6144]
# name -> (cells, the box size the library is asked for (None: the dense form is planned), environment of the process that runs it)
SETS = {"dense_%d" % m: (functools.partial(dense_cells, m), None, {}) for m in DENSE_M}
SETS.update({
    "default_box": (default_box_cells, 16, {}),
    "shapes": (shapes_cells, 16, {}),
    "fallback": (fallback_cells, 16, {}),
    "sheet": (sheet_cells, 16, {}),
    "small_boxes": (small_box_cells, 8, {"SHM_TL_MIN_M": "32", "SHM_TL_BOX": "8"}),
})
TWO_LEVEL = ["default_box", "shapes", "fallback", "small_boxes"]


@functools.lru_cache(maxsize=None)
def problem(name):
    """(problem dict, cells in row order) of a set: built once and shared."""
    n, cells = SETS[name][0]()
    d = fill(n, cells, seed=sum(map(ord, name)))
    cells.setflags(write=False)
    return d, cells
