"""Seeded phi fields no solve produces, for shm_grid_set_phi (tests/test_injected_phi.py): every builder returns n^3 float64 values in get_phi's node order
(x fastest) and is a function of its arguments alone.  Test infrastructure, no device code.

The fields live in INDEX space, u = (i, j, k): a test places them in a box through u = (x - bbox_min) / cell.  The trilinear interpolant reproduces `affine`,
`on_iso` and `trilinear` exactly, so their values, gradients and ray hits are known in closed form (`affine_at`, `trilinear_at`).

Grid sizes the tests use.  n = 20: 8000 nodes are four indexed-mesh tiles of 2048 with the last one partial; 19 cells per axis leave the 8^3 ray bricks and the
8^3 redistance tiles partial on every upper face; with local_slabs = 3 the planes split 7 + 7 + 6 (seams between planes 6 | 7 and 13 | 14).  n = 12 where a
reference is brute force."""
import numpy as np


def _grid(n):
    k, j, i = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    return i, j, k


def random_sign(n, seed=1):
    """uniform(0.1, 1) times a random sign per node: every cell is a draw of the 256 marching-cubes cases; contour at isovalue 0.  At n = 20, seed 1, every case
    occurs at least 15 times (11 302 vertices, 21 846 triangles); at n = 12 every case occurs, the rarest once."""
    rng = np.random.default_rng(seed)
    mag = rng.uniform(0.1, 1.0, n ** 3)
    return mag * rng.choice([-1.0, 1.0], n ** 3)


def speck_nodes(n, seed=1, count=None):
    """[m, 3] (i, j, k) of the negative nodes of `specks`: the eight box corners' diagonal pair, nodes on box edges and faces, nodes on both sides of the two
    slab seams of local_slabs = 3, then random ones; no two closer than 3 in any norm, so every speck is a closed component (or an open one on the box)."""
    q, r = divmod(n, 3)
    s1 = q + (1 if r > 0 else 0)
    s2 = s1 + q + (1 if r > 1 else 0)          # planes [0, s1) [s1, s2) [s2, n): shm_plan_slab(n, 3, .)
    m = n // 2
    fixed = [(0, 0, 0), (n - 1, n - 1, n - 1), (m, 0, 0), (n - 1, m, n - 1), (0, n - 1, m),          # corners, edges
             (m, m, 0), (m, 3, n - 1), (0, m, m), (n - 1, 4, 4), (4, 0, m + 3), (m + 3, n - 1, 4),   # faces
             (3, 3, s1 - 1), (7, 3, s1), (3, 7, s2 - 1), (7, 7, s2), (0, n - 4, s1), (n - 1, n - 4, s2 - 1)]   # seams, two of them on a face
    rng = np.random.default_rng(seed)
    want = count if count is not None else max(len(fixed), n ** 3 // 60)
    out = []
    for p in fixed + [tuple(int(v) for v in rng.integers(0, n, 3)) for _ in range(40 * want)]:
        if len(out) >= want:
            break
        if all(max(abs(p[a] - o[a]) for a in range(3)) >= 3 for o in out):
            out.append(p)
    return np.array(out, dtype=np.int64)


def specks(n, seed=1, count=None):
    """+1 everywhere, uniform(-1, -0.1) at the isolated nodes of speck_nodes: many tiny components, bricks that are almost all skippable; isovalue 0."""
    nodes = speck_nodes(n, seed, count)
    rng = np.random.default_rng(seed + 1000)
    f = np.ones((n, n, n))
    f[nodes[:, 2], nodes[:, 1], nodes[:, 0]] = rng.uniform(-1.0, -0.1, len(nodes))
    return f.reshape(-1)


def on_iso(n, c=None):
    """The integers i + j + k - c: every node of the plane i + j + k = c equals the isovalue 0 exactly (tt = 0, coincident vertices, zero-area triangles)."""
    i, j, k = _grid(n)
    return (i + j + k - float(n if c is None else c)).reshape(-1)


# Every coefficient is a short dyadic fraction, so the node values are exact in fp32 as well: an SHM_F32 handle holds the same affine (trilinear) function and
# the closed forms are its answers too.  8 a . u is an integer and 8 c is not: no node of the generic plane equals the isovalue.
AFFINE_GENERIC = ((0.375, -0.625, 0.875), 4.3125)
AFFINE_AXIS = ((0.0, 0.0, 1.0), 7.25)         # the plane k = 7.25: psi is the exact plane distance


def affine(n, a=AFFINE_GENERIC[0], c=AFFINE_GENERIC[1]):
    """a . u - c."""
    i, j, k = _grid(n)
    return ((a[0] * i + a[1] * j) + a[2] * k - c).reshape(-1)


def affine_at(u, a=AFFINE_GENERIC[0], c=AFFINE_GENERIC[1]):
    """(value [Q], gradient with respect to u [Q, 3]) at index-space points u [Q, 3]."""
    u = np.asarray(u, dtype=np.float64).reshape(-1, 3)
    return (a[0] * u[:, 0] + a[1] * u[:, 1]) + a[2] * u[:, 2] - c, np.tile(np.asarray(a, dtype=np.float64), (len(u), 1))


TRILINEAR = (0.3125, 0.125, -0.0625, 0.046875, -0.015625, 0.0078125, 0.00390625, -0.0009765625)   # a b c d e f g h: multiples of 2^-10


def trilinear(n, coef=TRILINEAR):
    """a + b x + c y + d z + e xy + f xz + g yz + h xyz at u = (x, y, z)."""
    i, j, k = _grid(n)
    return trilinear_at(np.stack([i, j, k], axis=-1).reshape(-1, 3), coef)[0]


def trilinear_at(u, coef=TRILINEAR):
    u = np.asarray(u, dtype=np.float64).reshape(-1, 3)
    x, y, z = u[:, 0], u[:, 1], u[:, 2]
    a, b, c, d, e, f, g, h = coef
    v = a + b * x + c * y + d * z + e * x * y + f * x * z + g * y * z + h * x * y * z
    grad = np.stack([b + e * y + f * z + h * y * z, c + e * x + g * z + h * x * z, d + f * x + g * y + h * x * y], axis=1)
    return v, grad


def holed_layout(n):
    """Where `holed` puts what: centre and radius of the sphere, the NaN plane k = wall with its one finite node `hole`, and the edge whose four cells all hold a
    non-finite corner while its own ends are finite and cut (lower node `orphan`, x axis)."""
    R = 0.3 * (n - 1)
    centre = (0.5 * (n - 1), 0.5 * (n - 1), R + 0.12 * (n - 1))
    wall = int(np.ceil(centre[2] + R)) + 2           # above the sphere: beyond it phi > 0 everywhere and no edge is cut
    assert wall <= n - 2, "holed needs room behind the NaN plane"
    m = int(centre[1])
    kz = int(round(centre[2]))
    io = int(np.floor(centre[0] + np.sqrt(R * R - (m - centre[1]) ** 2 - (kz - centre[2]) ** 2)))   # (io, m, kz) inside, (io + 1, m, kz) outside
    return dict(R=R, centre=centre, wall=wall, hole=(m, m + 1, wall), orphan=(io, m, kz))


def holed(n, seed=1):
    """|u - centre| - R with non-finite nodes: NaN, +inf and -inf scattered on and off the surface, a NaN of each sign bit, two NaN beside a cut edge so that
    every cell of that edge is discarded, and a NaN plane with a one-node hole that splits the box above the sphere; isovalue 0."""
    L = holed_layout(n)
    i, j, k = _grid(n)
    cx, cy, cz = L["centre"]
    f = np.sqrt((i - cx) ** 2 + (j - cy) ** 2 + (k - cz) ** 2) - L["R"]
    rng = np.random.default_rng(seed)
    io, m, kz = L["orphan"]
    keep = np.zeros((n, n, n), dtype=bool)            # nodes the scatter must leave alone: the orphan edge's ends
    keep[kz, m, io] = keep[kz, m, io + 1] = True
    near = np.flatnonzero((np.abs(f) < 1.0).reshape(-1) & ~keep.reshape(-1) & (k.reshape(-1) < L["wall"] - 1))
    far = np.flatnonzero((np.abs(f) > 2.0).reshape(-1) & ~keep.reshape(-1) & (k.reshape(-1) < L["wall"] - 1))
    g = f.reshape(-1).copy()
    values = [np.nan, np.inf, -np.inf, np.copysign(np.nan, -1.0)]
    for t, node in enumerate(np.concatenate([rng.choice(near, 16, replace=False), rng.choice(far, 12, replace=False)])):
        g[node] = values[t % 4]
    g = g.reshape(n, n, n)
    g[kz, m + 1, io] = np.nan
    g[kz, m - 1, io] = np.copysign(np.nan, -1.0)
    g[kz, m, io], g[kz, m, io + 1] = f[kz, m, io], f[kz, m, io + 1]
    hole = g[L["wall"], L["hole"][1], L["hole"][0]]
    g[L["wall"]] = np.nan
    g[L["wall"], L["hole"][1], L["hole"][0]] = f[L["wall"], L["hole"][1], L["hole"][0]] if not np.isfinite(hole) else hole
    return g.reshape(-1)
