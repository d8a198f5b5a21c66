"""Plain-python marching tetrahedra (Kuhn split) and marching cubes, the test-side restatements of csrc iso_kernel / iso_mc_kernel.  Test infrastructure.

Non-finite nodes (include/shm_grid.h): a cell with a non-finite corner contributes no triangle, and an edge carries a vertex only if both its ends are finite and
it is cut.  drop_nonfinite=True (the default) applies it; for a finite field it changes nothing.  drop_nonfinite=False is the plain table walk, in which a NaN
corner counts as outside and the vertices on its edges are NaN."""
import numpy as np

KUHN = [(0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7)]


def finite_cells(P):
    """[nz-1, n-1, n-1] bool: the cells of the [k, j, i] field P whose eight corners are all finite."""
    nz, n = P.shape[0], P.shape[2]
    fin = np.isfinite(P)
    good = np.ones((nz - 1, n - 1, n - 1), dtype=bool)
    for q in range(8):
        good &= fin[(q >> 2) & 1:nz - 1 + ((q >> 2) & 1), (q >> 1) & 1:n - 1 + ((q >> 1) & 1), (q & 1):n - 1 + (q & 1)]
    return good


def cut_edges(phi, n, iso, nz=None, drop_nonfinite=True):
    """Ascending keys 3 g + axis (g = i + j n + k n^2 the edge's lower node, numbered from the field's first plane) of the grid edges that carry a vertex: cut,
    and with the rule both ends finite -- whether or not a surviving cell references them."""
    nz = n if nz is None else nz
    P = np.asarray(phi, dtype=np.float64).reshape(nz, n, n)
    with np.errstate(invalid="ignore"):
        inside = P < iso
    fin = np.isfinite(P) if drop_nonfinite else np.ones_like(inside)
    g = np.arange(nz * n * n, dtype=np.int64).reshape(nz, n, n)
    cx = (inside[:, :, :-1] != inside[:, :, 1:]) & fin[:, :, :-1] & fin[:, :, 1:]
    cy = (inside[:, :-1, :] != inside[:, 1:, :]) & fin[:, :-1, :] & fin[:, 1:, :]
    cz = (inside[:-1] != inside[1:]) & fin[:-1] & fin[1:]
    return np.sort(np.concatenate([3 * g[:, :, :-1][cx], 3 * g[:, :-1, :][cy] + 1, 3 * g[:-1][cz] + 2]))


def marching_tets(phi, n, bbox_min, cell, iso, drop_nonfinite=True):
    """Returns (edge_points: dict edge_key -> xyz, triangles: list of 3 edge keys) ; edge key = (node_lo, node_hi)."""
    P = phi.reshape(n, n, n)  # [k,j,i]
    pts, tris = {}, []
    with np.errstate(invalid="ignore"):
        inside = P < iso
    cand = np.zeros((n - 1, n - 1, n - 1), dtype=np.int32)
    for q in range(8):
        cand += inside[(q >> 2) & 1:n - 1 + ((q >> 2) & 1), (q >> 1) & 1:n - 1 + ((q >> 1) & 1), (q & 1):n - 1 + (q & 1)]
    live = (cand > 0) & (cand < 8)
    if drop_nonfinite:
        live &= finite_cells(P)
    for k, j, i in zip(*np.nonzero(live)):
        node = lambda q: (i + (q & 1)) + (j + ((q >> 1) & 1)) * n + (k + ((q >> 2) & 1)) * n * n  # noqa: E731
        pos = lambda q: np.array([(i + (q & 1)) * cell + bbox_min[0], (j + ((q >> 1) & 1)) * cell + bbox_min[1],  # noqa: E731
                                  (k + ((q >> 2) & 1)) * cell + bbox_min[2]])
        val = lambda q: P[k + ((q >> 2) & 1), j + ((q >> 1) & 1), i + (q & 1)]  # noqa: E731
        for tet in KUHN:
            ins = [q for q in tet if val(q) < iso]
            outs = [q for q in tet if not val(q) < iso]
            if not ins or not outs:
                continue

            def ep(a, b):
                key = (min(node(a), node(b)), max(node(a), node(b)))
                t = (iso - val(a)) / (val(b) - val(a))
                pts[key] = pos(a) + t * (pos(b) - pos(a))
                return key
            if len(ins) == 1:
                loop = [ep(ins[0], o) for o in outs]
            elif len(ins) == 3:
                loop = [ep(a, outs[0]) for a in ins]
            else:
                loop = [ep(ins[0], outs[0]), ep(ins[0], outs[1]), ep(ins[1], outs[1]), ep(ins[1], outs[0])]
            tris.append(tuple(loop[:3]))
            if len(loop) == 4:
                tris.append((loop[0], loop[2], loop[3]))
    return pts, tris


def _mc_table():
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("gen_mc_table", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "gen_mc_table.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    return g.build_table(), g.EDGES


def cell_cases(P, iso):
    """[nz-1, n-1, n-1] int32: the marching-cubes case of every cell of the [k, j, i] field P, bit q set where corner q has P < iso (NaN: not set)."""
    nz, n = P.shape[0], P.shape[2]
    with np.errstate(invalid="ignore"):
        inside = P < iso
    case = np.zeros((nz - 1, n - 1, n - 1), dtype=np.int32)
    for q in range(8):
        case |= inside[(q >> 2) & 1:nz - 1 + ((q >> 2) & 1), (q >> 1) & 1:n - 1 + ((q >> 1) & 1), (q & 1):n - 1 + (q & 1)].astype(np.int32) << q
    return case


def marching_cubes(phi, n, bbox_min, cell, iso, nz=None, drop_nonfinite=True):
    """Same return convention as marching_tets.  The case table comes from the generator (tools/gen_mc_table.py), not from the C header: the header is checked
    against the generator in tests/test_abi_and_host.py, the kernel against this function.  nz: number of z planes when the field is not a cube."""
    table, edges = _mc_table()
    nz = n if nz is None else nz
    P = phi.reshape(nz, n, n)  # [k,j,i]
    pts, tris = {}, []
    case = cell_cases(P, iso)
    live = (case > 0) & (case < 255)
    if drop_nonfinite:
        live &= finite_cells(P)
    for k, j, i in zip(*np.nonzero(live)):
        node = lambda q: (i + (q & 1)) + (j + ((q >> 1) & 1)) * n + (k + ((q >> 2) & 1)) * n * n  # noqa: E731
        pos = lambda q: np.array([(i + (q & 1)) * cell + bbox_min[0], (j + ((q >> 1) & 1)) * cell + bbox_min[1],  # noqa: E731
                                  (k + ((q >> 2) & 1)) * cell + bbox_min[2]])
        val = lambda q: P[k + ((q >> 2) & 1), j + ((q >> 1) & 1), i + (q & 1)]  # noqa: E731
        for tri in table[case[k, j, i]]:
            keys = []
            for e in tri:
                a, b = edges[e]
                key = (node(a), node(b))
                t = (iso - val(a)) / (val(b) - val(a))
                pts[key] = pos(a) + t * (pos(b) - pos(a))
                keys.append(key)
            tris.append(tuple(keys))
    return pts, tris
