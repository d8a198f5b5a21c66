"""A headless picture of a level set of phi: the view the demo gets from Polyscope's ray-cast isosurface (src/main.cpp:121-123), made with
shm_grid_raycast_device.  Orthographic or pinhole rays are generated on the device in 8 x 8 pixel tiles -- 64 consecutive rays, one wavefront, cover one
tile, so the rays of a wavefront walk the same bricks -- cast against phi = iso, and shaded by -d . grad / (|d| |grad|) (1: the surface faces the eye).
The image is written as a binary PPM with plain numpy.  camera_rays() is also the workload of tools/ray_bench.py.

--mesh renders the resident indexed mesh instead -- the marching-cubes mesh of phi = iso, after --keep-largest K if given, or with --offset D the offset
mesh psi = D of the exact redistance: what an export would write -- with shm_grid_mesh_raycast_device, shaded by d . N of the triangle hit and with
--components coloured by the component it belongs to.

    python tools/ray_render.py data/bunny_small.obj --h 2 --out bunny.ppm [--size 512] [--ortho] [--iso 0] [--fp32] [--azimuth 30] [--elevation 20]
                               [--mesh [--keep-largest K] [--offset D] [--components]]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import shm_import  # noqa: E402

TILE = 8


def camera_rays(torch, n, bbox_min, cell, size, ortho=False, azimuth=30.0, elevation=20.0, dtype=None, device="cuda:0", tiled=True):
    """(origins [Q, 3], dirs [Q, 3], pixel [Q]) on the device, Q = size^2 (size a multiple of 8): ray q belongs to pixel pixel[q] = y * size + x.
    tiled: ray 64 T + r is pixel r of tile T (row-major in both); otherwise rays follow the pixels row by row.  The eye sits 3 box radii from the centre of
    the box; the image plane through the centre spans 0.55 of the box's side, which holds the model (the solver's box is twice the model's radius)."""
    assert size % TILE == 0
    dt = dtype or torch.float64
    b = np.asarray(bbox_min, dtype=np.float64)
    c = b + (n - 1) * cell / 2
    R = np.sqrt(3.0) * (n - 1) * cell / 2
    az, el = np.radians(azimuth), np.radians(elevation)
    fwd = -np.array([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)])
    right = np.cross(fwd, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    eye = c - 3 * R * fwd
    W = 0.55 * (n - 1) * cell / 2   # half-width of the image plane
    q = torch.arange(size * size, device=device)
    if tiled:
        tiles_x = size // TILE
        t, r = q // (TILE * TILE), q % (TILE * TILE)
        x = (t % tiles_x) * TILE + r % TILE
        y = (t // tiles_x) * TILE + r // TILE
    else:
        x, y = q % size, q // size
    f64 = torch.float64
    u = ((x.to(f64) + 0.5) / size * 2 - 1) * W
    v = (1 - (y.to(f64) + 0.5) / size * 2) * W
    tv = lambda a: torch.tensor(a, dtype=f64, device=device)   # noqa: E731
    plane = u[:, None] * tv(right) + v[:, None] * tv(up)
    if ortho:
        O = tv(eye) + plane
        D = tv(fwd).expand(size * size, 3)
    else:
        O = tv(eye).expand(size * size, 3)
        D = 3 * R * tv(fwd) + plane   # through the image plane at the centre of the box; not normalised
    return O.to(dt).contiguous(), D.to(dt).contiguous(), y * size + x


def shade(torch, D, t, g, pixel, size):
    """uint8 image [size, size, 3]: background dark blue, hits grey by -d . grad / (|d| |grad|), leaving hits (d . grad > 0) tinted red."""
    hit = torch.isfinite(t)
    cosv = -(D * g).sum(1) / (D.norm(dim=1) * g.norm(dim=1))
    img = torch.zeros(size * size, 3, dtype=torch.float64, device=t.device)
    img[:, 2] = 0.25
    lum = (0.15 + 0.85 * cosv.abs().to(torch.float64)).clamp(0, 1)
    col = torch.stack([lum, torch.where(cosv < 0, lum * 0.4, lum), torch.where(cosv < 0, lum * 0.4, lum)], dim=1)
    img[pixel[hit]] = col[hit]
    return (img.reshape(size, size, 3) * 255).round().to(torch.uint8).cpu().numpy()


PALETTE = np.array([[0.85, 0.85, 0.85], [0.9, 0.35, 0.3], [0.3, 0.7, 0.35], [0.3, 0.45, 0.9], [0.9, 0.75, 0.25], [0.7, 0.35, 0.8], [0.3, 0.8, 0.8]])


def shade_mesh(torch, D, t, tri, V, F, pixel, size, comp=None):
    """uint8 image [size, size, 3]: background dark blue; a hit is lit by |d . N| / (|d| |N|) of its triangle (V, F numpy, the mesh fetched from the handle),
    grey, or in the palette colour of its component rank (comp: numpy [nt]) ; a triangle seen from behind (d . N > 0) is darkened."""
    dev = t.device
    hit = tri >= 0
    Vt = torch.tensor(V, dtype=torch.float64, device=dev)
    Ft = torch.tensor(F, dtype=torch.int64, device=dev)
    f = Ft[tri.clamp(min=0)]
    N = torch.cross(Vt[f[:, 1]] - Vt[f[:, 0]], Vt[f[:, 2]] - Vt[f[:, 0]], dim=1)
    D = D.to(torch.float64)
    cosv = (D * N).sum(1) / (D.norm(dim=1) * N.norm(dim=1)).clamp(min=1e-300)
    lum = (0.15 + 0.85 * cosv.abs()).clamp(0, 1) * torch.where(cosv > 0, 0.5, 1.0)
    base = torch.tensor(PALETTE, dtype=torch.float64, device=dev)
    col = base[torch.tensor(comp, device=dev)[tri.clamp(min=0)] % len(PALETTE)] if comp is not None else base[0].expand(len(t), 3)
    img = torch.zeros(size * size, 3, dtype=torch.float64, device=dev)
    img[:, 2] = 0.25
    img[pixel[hit]] = (col * lum[:, None])[hit]
    return (img.reshape(size, size, 3) * 255).round().to(torch.uint8).cpu().numpy()


def write_ppm(path, img):
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img, dtype=np.uint8).tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mesh")
    ap.add_argument("--h", type=float, default=2.0)
    ap.add_argument("--out", required=True)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--ortho", action="store_true")
    ap.add_argument("--iso", type=float, default=0.0)
    ap.add_argument("--fp32", action="store_true")
    ap.add_argument("--azimuth", type=float, default=30.0)
    ap.add_argument("--elevation", type=float, default=20.0)
    ap.add_argument("--mesh", dest="cast_mesh", action="store_true", help="cast against the resident indexed mesh instead of the level set of phi")
    ap.add_argument("--keep-largest", type=int, default=None)
    ap.add_argument("--offset", type=float, default=None, help="with --mesh: the offset mesh psi = D (a length) of the exact redistance at --iso")
    ap.add_argument("--components", action="store_true", help="with --mesh: colour by component")
    a = ap.parse_args()
    import torch   # before the library is loaded (grid_abi.GridSolver.sample_device)
    shm = shm_import.load()
    from signed_heat_3d_amd.host_abi import HostSolver
    pre = HostSolver(a.mesh).preprocess(hCoef=a.h)
    s = shm.GridSolver(precision=shm.SHM_F32 if a.fp32 else shm.SHM_F64)
    s.set_problem(pre["pos"], pre["wnormal"], pre["area"], pre["lam"], pre["n"], pre["bbox_min"], pre["cell"])
    s.solve()
    O, D, pixel = camera_rays(torch, pre["n"], pre["bbox_min"], pre["cell"], a.size, a.ortho, a.azimuth, a.elevation,
                              torch.float32 if a.fp32 else torch.float64)
    if a.cast_mesh:
        if a.offset is not None:
            s.redistance_exact(a.iso, min(16.0 * pre["cell"], abs(a.offset) + 2.0 * pre["cell"]))
            V, F = s.isosurface_indexed_psi(a.offset, keep_largest=a.keep_largest)
        else:
            V, F = s.isosurface_indexed(a.iso, keep_largest=a.keep_largest)
        comp = s.isosurface_components(labels=True)[1] if a.components else None      # (labels the mesh in the slot; the mesh itself stays)
        t, tri, nh = s.mesh_raycast_device(O, D, bary=False)
        write_ppm(a.out, shade_mesh(torch, D, t, tri, V, F, pixel, a.size, comp))
        print("%d x %d rays against the indexed mesh (%d triangles) on %d^3: %d hits; written to %s" % (a.size, a.size, len(F), pre["n"], nh, a.out))
    else:
        t, g, nh = s.raycast_device(O, D, a.iso, grad=True)
        write_ppm(a.out, shade(torch, D, t, g, pixel, a.size))
        print("%d x %d rays against phi = %g on %d^3: %d hits; written to %s" % (a.size, a.size, a.iso, pre["n"], nh, a.out))
    s.close()


if __name__ == "__main__":
    main()
