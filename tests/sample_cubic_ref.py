"""The numpy restatement of shm_grid_sample_cubic (include/shm_grid.h; csrc/shm_cubic_weights.h and shm_sample_cubic.hip.h): the Keys cubic convolution
(Catmull-Rom, a = -1/2) of the grid's nodes with Keys' ghost node folded into the weights at the faces, its gradient and its Hessian, written down
operation by operation.  numpy never fuses a multiply and an add, so with dtype float64 this is the kernel's arithmetic; with dtype np.longdouble it is the
same formula in a wider format, the reference the float64 evaluation is held to (tests/test_sample_cubic_host.py)."""
import numpy as np


def cell_t(q, lo, h, n, dtype=np.float64, t64=False):
    """One axis, coordinates inside the box: sample_kernel's cell and t.  i = floor((q - lo) / h); i > n-2 -> cell n-2 with t = 1.
    The cell is always chosen in float64, as the kernel chooses it (the Hessian jumps across a face: a reference must sit in the same cell); t is in dtype,
    or with t64 the kernel's own float64 t widened to dtype (a reference for the weights and sums alone: q - p000 cancels, so t carries an error of about
    eps |q| / h that the third derivatives of a rough field magnify)."""
    if t64 and dtype is not np.float64:
        i, t = cell_t(q, lo, h, n)
        return i, t.astype(dtype)
    q64 = np.asarray(q, dtype=np.float64)
    i = np.floor((q64 - np.float64(lo)) / np.float64(h)).astype(np.int64)
    top = i > n - 2
    i = np.where(top, n - 2, i)
    q = q64.astype(dtype)
    lo, h = dtype(lo), dtype(h)
    t = (q - (i.astype(dtype) * h + lo)) / h
    t = np.where(top, dtype(1), t)
    return i, t


def keys(t):
    """The weights on the nodes at offsets -1, 0, 1, 2 and their first and second derivatives in t: three [Q, 4] arrays, Horner forms."""
    dt = t.dtype.type
    c = lambda v: dt(v)
    w = np.stack([(((-t + c(2)) * t - c(1)) * t) / c(2), (((c(3) * t - c(5)) * t) * t + c(2)) / c(2), (((c(-3) * t + c(4)) * t + c(1)) * t) / c(2),
                  (((t - c(1)) * t) * t) / c(2)], -1)
    d1 = np.stack([((c(-3) * t + c(4)) * t - c(1)) / c(2), ((c(9) * t - c(10)) * t) / c(2), ((c(-9) * t + c(8)) * t + c(1)) / c(2),
                   ((c(3) * t - c(2)) * t) / c(2)], -1)
    d2 = np.stack([c(-3) * t + c(2), c(9) * t - c(5), c(-9) * t + c(4), c(3) * t - c(1)], -1)
    return w, d1, d2


def fold(k, i, n):
    """[Q, 4] weights on offsets -1..2 -> [Q, 4] weights on the nodes base .. base + cnt - 1 (entry 3 is 0 and unused where cnt == 3).
    Cell 0: (w0 + 3 w-1, w1 - 3 w-1, w2 + w-1).  Cell n-2: (w-1 + w2, w0 - 3 w2, w1 + 3 w2)."""
    three, zero = k.dtype.type(3), np.zeros_like(k[:, 0])
    low = np.stack([k[:, 1] + three * k[:, 0], k[:, 2] - three * k[:, 0], k[:, 3] + k[:, 0], zero], -1)
    high = np.stack([k[:, 0] + k[:, 3], k[:, 1] - three * k[:, 3], k[:, 2] + three * k[:, 3], zero], -1)
    return np.where((i <= 0)[:, None], low, np.where((i >= n - 2)[:, None], high, k))


def axis(q, lo, h, n, dtype=np.float64, t64=False):
    """base [Q], cnt [Q], (w, w', w'') each [Q, 4] for one axis."""
    i, t = cell_t(q, lo, h, n, dtype, t64)
    w, d1, d2 = keys(t)
    face = (i <= 0) | (i >= n - 2)
    base = np.where(i <= 0, 0, np.where(i >= n - 2, n - 3, i - 1))
    return base, np.where(face, 3, 4), (fold(w, i, n), fold(d1, i, n), fold(d2, i, n))


def _dot(w, f, cnt):
    """sum_a w[:, a] * f[a] from the lowest index up; the fourth term only where cnt == 4 (an absent node is neither read nor multiplied)."""
    s = w[:, 0] * f[0]
    s = s + w[:, 1] * f[1]
    s = s + w[:, 2] * f[2]
    with np.errstate(invalid="ignore"):
        return np.where(cnt == 4, s + w[:, 3] * f[3], s)


def inside_box(pts, n, bbox_min, cell):
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    b = np.asarray(bbox_min, dtype=np.float64)
    hi = (n - 1) * cell + b
    with np.errstate(invalid="ignore"):
        return np.all((pts >= b) & (pts <= hi), axis=1)


def cubic_ref(phi, n, bbox_min, cell, pts, grad=False, hess=False, dtype=np.float64, t64=False):
    """phi: n^3 values (x fastest).  Returns value [Q] and, as asked, gradient [Q, 3] and Hessian [Q, 6] (xx, yy, zz, xy, xz, yz); NaN outside the closed
    box and for NaN coordinates.  The box test is always float64 (the kernel's); everything after it is in dtype."""
    u = np.asarray(phi).astype(dtype).reshape(n, n, n)   # [k, j, i]
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    b = np.asarray(bbox_min, dtype=np.float64)
    ins = inside_box(pts, n, b, cell)
    p = pts[ins]
    Q = len(p)
    (bx, cx, (wx, wx1, wx2)), (by, cy, (wy, wy1, wy2)), (bz, cz, (wz, wz1, wz2)) = [axis(p[:, a], b[a], cell, n, dtype, t64) for a in range(3)]
    order = 2 if hess else (1 if grad else 0)
    with np.errstate(invalid="ignore", over="ignore"):
        zsum = {}
        for kz in range(4):
            k = np.minimum(bz + kz, n - 1)   # (clamped only where the plane is absent: its sums are discarded below)
            x0, x1, x2 = [], [], []
            for r in range(4):
                j = np.minimum(by + r, n - 1)
                f = [u[k, j, np.minimum(bx + a, n - 1)] for a in range(4)]
                x0.append(_dot(wx, f, cx))
                if order >= 1:
                    x1.append(_dot(wx1, f, cx))
                if order >= 2:
                    x2.append(_dot(wx2, f, cx))
            ys = {"00": _dot(wy, x0, cy)}
            if order >= 1:
                ys["10"], ys["01"] = _dot(wy, x1, cy), _dot(wy1, x0, cy)
            if order >= 2:
                ys["20"], ys["02"], ys["11"] = _dot(wy, x2, cy), _dot(wy2, x0, cy), _dot(wy1, x1, cy)
            terms = [("v", wz, "00")]
            if order >= 1:
                terms += [("gx", wz, "10"), ("gy", wz, "01"), ("gz", wz1, "00")]
            if order >= 2:
                terms += [("xx", wz, "20"), ("yy", wz, "02"), ("zz", wz2, "00"), ("xy", wz, "11"), ("xz", wz1, "10"), ("yz", wz1, "01")]
            for name, w, y in terms:
                t = w[:, kz] * ys[y]
                if kz == 0:
                    zsum[name] = t
                elif kz < 3:
                    zsum[name] = zsum[name] + t
                else:
                    zsum[name] = np.where(cz == 4, zsum[name] + t, zsum[name])
    h = dtype(cell)
    v = np.full(len(pts), np.nan, dtype=dtype)
    v[ins] = zsum["v"]
    res = [v]
    if grad:
        g = np.full((len(pts), 3), np.nan, dtype=dtype)
        if order >= 1:
            g[ins] = np.stack([zsum["gx"] / h, zsum["gy"] / h, zsum["gz"] / h], -1) if Q else np.zeros((0, 3), dtype)
        res.append(g)
    if hess:
        H = np.full((len(pts), 6), np.nan, dtype=dtype)
        with np.errstate(invalid="ignore", over="ignore"):
            H[ins] = np.stack([zsum[a] / h / h for a in ("xx", "yy", "zz", "xy", "xz", "yz")], -1) if Q else np.zeros((0, 6), dtype)
        res.append(H)
    return res[0] if len(res) == 1 else tuple(res)


def window_has(mask, n, bbox_min, cell, pts):
    """For each point: does the window of nodes the rule reads (3 or 4 per axis, the faces folded) contain a node where mask [n^3] is true?
    False outside the box."""
    m = np.asarray(mask, dtype=bool).reshape(n, n, n)
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    b = np.asarray(bbox_min, dtype=np.float64)
    ins = inside_box(pts, n, b, cell)
    p = pts[ins]
    (bx, cx, _), (by, cy, _), (bz, cz, _) = [axis(p[:, a], b[a], cell, n) for a in range(3)]
    hit = np.zeros(len(p), dtype=bool)
    for kz in range(4):
        for r in range(4):
            for a in range(4):
                ok = (kz < cz) & (r < cy) & (a < cx)
                hit |= ok & m[np.minimum(bz + kz, n - 1), np.minimum(by + r, n - 1), np.minimum(bx + a, n - 1)]
    out = np.zeros(len(pts), dtype=bool)
    out[ins] = hit
    return out


def cell_class(n, bbox_min, cell, pts):
    """0..26 per in-box point: (class_x + 3 class_y + 9 class_z) with class 0 = low face cell, 1 = interior, 2 = high face cell; -1 outside."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    b = np.asarray(bbox_min, dtype=np.float64)
    ins = inside_box(pts, n, b, cell)
    out = np.full(len(pts), -1)
    c = 0
    for a in range(3):
        i, _ = cell_t(pts[ins, a], b[a], cell, n)
        c = c + 3 ** a * np.where(i <= 0, 0, np.where(i >= n - 2, 2, 1))
    out[ins] = c
    return out
