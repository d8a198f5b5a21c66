"""Time of the ray casts (shm_grid_raycast_device / shm_grid_raycast) on a solved grid against what the library offered before them: fixed-step marching at
cell / 2 through sample_device with sign-change detection, on the same rays in the same process.

For each case (bunny_small 256^3 and 512^3 in fp64, rocker 512^3 in fp32; iso = 0) and each workload -- 1024^2 camera rays, pinhole and orthographic, in 8 x 8
tiles and the same rays shuffled; 2^22 random rays from inside the box -- one warm-up of every path, then --reps alternating repetitions in one process, each
timed with a host clock around calls that return synchronised; medians.  Reported: rays/s of the device entry, of the host entry (camera, tiled, pinhole
only: it is bound by the copies), of the march (on --march-rays rays of the workload: it needs 2 n gathers per ray), how many of the march's answers are
wrong (a hit further than one step from the cast's, a miss where the cast hits, a hit where it misses), and the brick build alone (a 64-ray cast right
after a solve, which builds the bricks, less the same cast repeated).  With --count-lib, a build of the library with -DSHM_RAY_COUNT
(make -C signed-heat-3d_amd/csrc OUT=../lib/variants/raycount HIPFLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -DSHM_RAY_COUNT"), a child process casts
every workload once on that build and the brick steps, cells examined and cells kept per ray are added to the record.  One JSON line per case and workload,
appended to --out (default profiles/raycast.txt).  Not part of bench.py.

    python tools/ray_bench.py [--reps 7] [--cases bunny_small:256:64,bunny_small:512:64,rocker:512:32] [--size 1024] [--random 4194304] [--march-rays 65536]

Per-kernel times: rocprofv3 --kernel-trace --stats -- python tools/ray_bench.py --reps 1 --no-march --cases bunny_small:512:64
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import shm_import  # noqa: E402
from ray_render import camera_rays  # noqa: E402


def march(torch, s, O, D, n, bbox_min, cell, iso, chunk=1 << 14):
    """Fixed-step marching at cell / 2 through sample_device: t of the first sign change of phi - iso between two samples (linear interpolation between them),
    NaN without one.  Steps are taken between the ray's entry into and exit from the box."""
    dt = O.dtype
    b = torch.tensor(np.asarray(bbox_min), dtype=torch.float64, device=O.device)
    hi = b + (n - 1) * cell
    out = torch.full((O.shape[0],), float("nan"), dtype=torch.float64, device=O.device)
    for q0 in range(0, O.shape[0], chunk):
        o, d = O[q0:q0 + chunk].to(torch.float64), D[q0:q0 + chunk].to(torch.float64)
        ta, tb = (b - o) / d, (hi - o) / d
        t0 = torch.minimum(ta, tb).nan_to_num(nan=-float("inf")).amax(1).clamp(min=0)
        t1 = torch.maximum(ta, tb).nan_to_num(nan=float("inf")).amin(1)
        step = 0.5 * cell / d.norm(dim=1)
        nsteps = int(torch.ceil(((t1 - t0) / step).clamp(min=0)).max().item()) + 1 if o.shape[0] else 0
        k = torch.arange(nsteps + 1, device=O.device, dtype=torch.float64)
        T = torch.minimum(t0[:, None] + k[None, :] * step[:, None], t1[:, None])                     # [m, K]
        P = (o[:, None, :] + T[:, :, None] * d[:, None, :]).clamp(min=b, max=hi)
        v = s.sample_device(P.reshape(-1, 3).to(dt).contiguous())[0].to(torch.float64).reshape(T.shape) - iso
        valid = (t1 >= t0)[:, None] & torch.isfinite(v)
        cross = valid[:, :-1] & valid[:, 1:] & ((v[:, :-1] == 0) | ((v[:, :-1] < 0) != (v[:, 1:] < 0)))
        any_ = cross.any(1)
        first = cross.to(torch.int8).argmax(1)
        r = torch.arange(o.shape[0], device=O.device)
        va, vb, Ta, Tb = v[r, first], v[r, first + 1], T[r, first], T[r, first + 1]
        th = Ta + (Tb - Ta) * torch.where(vb != va, va / (va - vb), torch.zeros_like(va))
        out[q0:q0 + chunk] = torch.where(any_, th, torch.full_like(th, float("nan")))
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cases", default="bunny_small:256:64,bunny_small:512:64,rocker:512:32")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--random", type=int, default=1 << 22)
    ap.add_argument("--march-rays", type=int, default=1 << 16)
    ap.add_argument("--no-march", action="store_true")
    ap.add_argument("--iso", type=float, default=0.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raycast.txt"))
    ap.add_argument("--count-lib", default="", help="a -DSHM_RAY_COUNT build of libshm_grid.so: adds the visit counts per ray")
    ap.add_argument("--count-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    counts = {}
    if a.count_lib:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--count-child", "--cases", a.cases, "--size", str(a.size), "--random", str(a.random),
                            "--iso", repr(a.iso), "--out", os.devnull], env=dict(os.environ, SHM_GRID_LIB=os.path.abspath(a.count_lib)), capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-2000:]
        for key, q, bs, ce, ck in re.findall(r"ray_workload (\S+) (\d+)\nray_count brick_steps (\d+) cells_examined (\d+) cells_kept (\d+)", p.stderr):
            counts[key] = dict(brick_steps_per_ray=round(int(bs) / int(q), 2), cells_examined_per_ray=round(int(ce) / int(q), 2),
                               cells_kept_per_ray=round(int(ck) / int(q), 3))
    import torch
    shm = shm_import.load()
    from signed_heat_3d_amd.host_abi import HostSolver
    med = lambda x: float(np.median(x))   # noqa: E731
    with open(a.out, "a") as log:
        for case in a.cases.split(","):
            mesh, n_want, prec = case.split(":")
            n_want, prec = int(n_want), int(prec)
            pre = HostSolver(os.path.join(ROOT, "data", mesh + ".obj")).preprocess(hCoef=float(np.log2(n_want / 2) - 3))
            n, b, h = pre["n"], pre["bbox_min"], pre["cell"]
            assert n == n_want
            s = shm.GridSolver(precision=shm.SHM_F64 if prec == 64 else shm.SHM_F32)
            s.set_problem(pre["pos"], pre["wnormal"], pre["area"], pre["lam"], n, b, h)
            s.solve()
            dt = torch.float64 if prec == 64 else torch.float32
            g = torch.Generator(device="cuda:0")
            g.manual_seed(1)
            work = {}
            for view, ortho in (("pinhole", False), ("ortho", True)):
                O, D, _ = camera_rays(torch, n, b, h, a.size, ortho, dtype=dt)
                perm = torch.randperm(O.shape[0], device=O.device, generator=g)
                work[view + "_tiles"] = (O, D)
                work[view + "_shuffled"] = (O[perm].contiguous(), D[perm].contiguous())
            lo = torch.tensor(b, dtype=torch.float64, device="cuda:0")
            Or = (lo + torch.rand(a.random, 3, dtype=torch.float64, device="cuda:0", generator=g) * (n - 1) * h).to(dt).contiguous()
            Dr = torch.randn(a.random, 3, dtype=torch.float64, device="cuda:0", generator=g).to(dt).contiguous()
            work["random_inside"] = (Or, Dr)
            if a.count_child:
                s.raycast_device(Or[:64], Dr[:64], a.iso)
                for name, (O, D) in work.items():
                    sys.stderr.write("ray_workload %s/%s %d\n" % (case, name, O.shape[0]))
                    sys.stderr.flush()
                    s.raycast_device(O, D, a.iso)
                s.close()
                continue
            first, again = [], []
            for _ in range(a.reps):   # the first cast of a phi builds the bricks: time it against the same cast repeated
                s.solve()
                for lst in (first, again, again):
                    t0 = time.perf_counter()
                    s.raycast_device(Or[:64], Dr[:64], a.iso)
                    lst.append((time.perf_counter() - t0) * 1e3)
            bricks_ms = med(first) - med(again)
            for name, (O, D) in work.items():
                Q = O.shape[0]
                m = min(Q, a.march_rays)
                sel = torch.arange(0, Q, Q // m, device=O.device)[:m]   # an even sample of the workload, in its order
                Om, Dm = O[sel].contiguous(), D[sel].contiguous()
                host = name == "pinhole_tiles"
                if host:
                    Oh, Dh = O.cpu().numpy().astype(np.float64), D.cpu().numpy().astype(np.float64)
                paths = {"device": lambda: s.raycast_device(O, D, a.iso, grad=True)}
                if host:
                    paths["host"] = lambda: s.raycast(Oh, Dh, a.iso, grad=True)
                if not a.no_march:
                    paths["march"] = lambda: march(torch, s, Om, Dm, n, b, h, a.iso)
                outv = {p: f() for p, f in paths.items()}   # warm-up
                ms = {p: [] for p in paths}
                for _ in range(a.reps):
                    for p, f in paths.items():
                        t0 = time.perf_counter()
                        f()
                        ms[p].append((time.perf_counter() - t0) * 1e3)
                t_dev, _, nh = outv["device"]
                res = dict(mesh=mesh, n=n, precision=prec, iso=a.iso, workload=name, rays=Q, hits=nh, reps=a.reps, bricks_build_ms=round(bricks_ms, 4),
                           device_ms=round(med(ms["device"]), 3), device_rays_per_s=round(Q / (med(ms["device"]) * 1e-3)))
                if host:
                    res.update(host_ms=round(med(ms["host"]), 3), host_rays_per_s=round(Q / (med(ms["host"]) * 1e-3)))
                    assert np.array_equal(outv["host"][0].astype(np.float64 if prec == 64 else np.float32), t_dev.cpu().numpy(), equal_nan=True)
                if not a.no_march:
                    tm = outv["march"]
                    tc = t_dev[sel].to(torch.float64)
                    step = 0.5 * h / Dm.to(torch.float64).norm(dim=1)
                    wrong = (torch.isfinite(tm) != torch.isfinite(tc)) | (torch.isfinite(tm) & torch.isfinite(tc) & ((tm - tc).abs() > step))
                    res.update(march_rays=m, march_ms=round(med(ms["march"]), 3), march_rays_per_s=round(m / (med(ms["march"]) * 1e-3)),
                               march_wrong=int(wrong.sum().item()), march_missed=int((torch.isfinite(tc) & ~torch.isfinite(tm)).sum().item()),
                               speedup_over_march=round((Q / med(ms["device"])) / (m / med(ms["march"])), 1))
                res.update(counts.get(case + "/" + name, {}))
                line = json.dumps(res)
                print(line, flush=True)
                log.write(line + "\n")
                log.flush()
            s.close()


if __name__ == "__main__":
    main()
