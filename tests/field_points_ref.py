"""numpy restatement of Steps 1-2 at arbitrary points (the yardstick of tests/test_field_points.py and tests/test_field_points_host.py; never the library):

    X(q) = sum_s w_s g_s,   g_s = exp(-lambda r_s) / r_s,   r_s = |q - b_s|,   Y = X / |X|

by plain fp64 sums, or -- exact=True -- by math.fsum of the fp64 terms, with the DERIVED price of tests/test_step1_audit.py (its docstring has the derivation):

    price = 2 * 2^-53 * sum_s |w_s|_1 g_s (lambda r_s + C) / |X|,    C = S_padded + 8 against a plain sum, C = 8 for the fsum form

(S_padded: S rounded up to whole clusters of 64 -- the device sums the zero-weight padding too), and ratio = |X| / L1 with L1 = sum_s |w_s|_1 g_s, l1_rel (what two
plain evaluations of L1 may differ by, relative to it) and lambda r_min.  Also the seeded point families and source sets the tests share."""
import math

import numpy as np

U = 2.0 ** -53
ZONE = 335.0
CLUSTER = 64


def padded(S):
    return (int(S) + CLUSTER - 1) // CLUSTER * CLUSTER


def yardstick(pos, w, lam, pts, exact=False):
    """dict of Y (Q, 3), X, price, ratio, l1_rel, lam_rmin and the finite mask at pts (Q, 3)."""
    pos, w, pts = np.asarray(pos, dtype=np.float64).reshape(-1, 3), np.asarray(w, dtype=np.float64).reshape(-1, 3), np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    S, Q, lam = len(pos), len(pts), float(lam)
    w1 = np.abs(w).sum(axis=1)
    Cc = 8.0 if exact else padded(S) + 8.0
    X, L1, Lp, rmin = np.zeros((Q, 3)), np.zeros(Q), np.zeros(Q), np.zeros(Q)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        step = max(16, 2000000 // S)                                                  # (chunks of ~2e6 pairs: 50 MB of temporaries)
        for a in range(0, Q, step):
            dd = pts[a:a + step, None, :] - pos[None, :, :]
            r = np.sqrt(dd[..., 0] * dd[..., 0] + dd[..., 1] * dd[..., 1] + dd[..., 2] * dd[..., 2])
            g = np.exp(-lam * r) / r
            t = g[:, :, None] * w[None, :, :]
            if exact:
                X[a:a + step] = [[math.fsum(t[q, :, p]) if np.isfinite(t[q, :, p]).all() else np.nan for p in range(3)] for q in range(t.shape[0])]
            else:
                X[a:a + step] = t.sum(axis=1)
            L1[a:a + step] = (g * w1).sum(axis=1)
            Lp[a:a + step] = (g * w1 * (lam * r + Cc)).sum(axis=1)
            rmin[a:a + step] = r.min(axis=1)
        nrm = np.sqrt((X * X).sum(axis=1))
        Y = X / nrm[:, None]
        return dict(Y=Y, X=X, price=2.0 * U * Lp / nrm, ratio=nrm / L1, l1_rel=2.0 * U * Lp / L1, lam_rmin=lam * rmin, finite=np.isfinite(Y).all(axis=1))


# ---- point families ---------------------------------------------------------------------------------------------------------------------------------------------------
def grid_box(d):
    lo = np.asarray(d["bbox_min"], dtype=np.float64)
    return lo, lo + (int(d["n"]) - 1) * float(d["cell"])


def family(name, d, Q, seed):
    """Seeded points around the problem d (pos, bbox_min, cell, n): "box" uniform in the grid box, "box3" uniform in the box grown threefold about its
    centre, "near" a source plus 1e-3 N(0, 1)."""
    rng = np.random.default_rng(seed)
    lo, hi = grid_box(d)
    if name == "box":
        return lo + rng.random((Q, 3)) * (hi - lo)
    if name == "box3":
        c, h = 0.5 * (lo + hi), 0.5 * (hi - lo)
        return c + (2.0 * rng.random((Q, 3)) - 1.0) * 3.0 * h
    if name == "near":
        pos = np.asarray(d["pos"], dtype=np.float64)
        return pos[rng.integers(0, len(pos), Q)] + 1e-3 * rng.standard_normal((Q, 3))
    raise ValueError(name)


FAMILIES = ("box", "box3", "near")


def node_positions(d):
    """The positions of all n^3 nodes as the reference forms them: i * cell + bbox_min, product and sum rounded separately; x fastest."""
    n = int(d["n"])
    idx = np.arange(n ** 3, dtype=np.int64)
    ijk = np.stack([idx % n, (idx // n) % n, idx // (n * n)], axis=-1)
    return ijk * float(d["cell"]) + np.asarray(d["bbox_min"], dtype=np.float64)


# ---- source sets ------------------------------------------------------------------------------------------------------------------------------------------------------
def problem(pos, w, lam, margin=0.05, n=8):
    """A problem dict around sources: the smallest n^3 grid (any small grid will do: the entry does not read it) whose cells hold every source."""
    pos, w = np.asarray(pos, dtype=np.float64).reshape(-1, 3), np.asarray(w, dtype=np.float64).reshape(-1, 3)
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    ext = float((hi - lo).max())
    pad = margin * max(ext, 1e-3) + 1e-6
    lo = lo - pad
    cell = (ext + 2.0 * pad) / (n - 1) * 1.0001
    return dict(pos=pos, wnormal=w, area=np.linalg.norm(w, axis=1), lam=float(lam), n=n, bbox_min=lo, cell=cell)


def seeded_sources(S, seed, lam=8.0):
    """S sources on a wobbly unit sphere with outward weights of uneven size."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((S, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    pos = v * (1.0 + 0.1 * rng.random((S, 1)))
    w = v * (0.01 + 0.05 * rng.random((S, 1)))
    return problem(pos, w, lam)


def two_blobs(seed=5, lam=20.0, gap=3.0, sigma=0.05, per=65):
    """Two blobs of `per` sources `gap` apart along x."""
    rng = np.random.default_rng(seed)
    a = sigma * rng.standard_normal((per, 3))
    b = sigma * rng.standard_normal((per, 3)) + np.array([gap, 0.0, 0.0])
    w = rng.standard_normal((2 * per, 3)) * 0.01 + np.array([0.0, 0.0, 0.02])
    return problem(np.concatenate([a, b]), w, lam)


def cancelling_sheets(D, lam=20.0, seed=9):
    """Two 16 x 16 sheets of opposite weight at z = +-0.05 over [-0.5, 0.5]^2, and a blob of 64 sources at x = D."""
    rng = np.random.default_rng(seed)
    u = (np.arange(16) + 0.5) / 16.0 - 0.5
    xx, yy = np.meshgrid(u, u, indexing="ij")
    top = np.stack([xx.ravel(), yy.ravel(), np.full(256, 0.05)], axis=1)
    bot = np.stack([xx.ravel(), yy.ravel(), np.full(256, -0.05)], axis=1)
    a = 1.0 / 256.0
    wt = np.tile([0.0, 0.0, a], (256, 1))
    wb = np.tile([0.0, 0.0, -a], (256, 1))
    blob = 0.02 * rng.standard_normal((64, 3)) + np.array([D, 0.0, 0.0])
    wblob = np.tile([a, 0.0, 0.0], (64, 1))
    return problem(np.concatenate([top, bot, blob]), np.concatenate([wt, wb, wblob]), lam)


def sheet_points(Q, seed=10):
    """Points just above the mid-plane of the sheets: z in (5e-5, 1e-4), x and y in the middle of the sheets."""
    rng = np.random.default_rng(seed)
    p = (rng.random((Q, 3)) - 0.5) * 0.4
    p[:, 2] = 5e-5 + 5e-5 * rng.random(Q)
    return p
