"""Timing report of the Gaussian fill (neuma_amd/gaussian_fill.py): the density stage and the whole fill at K Gaussians and
a given resolution, and which part of the density stage dominates - the rocPRIM scan + pair sort or the kernels.  A report,
not a gate:
    python tools/fill_bench.py [--gaussians 200000] [--resolution 128] [--reps 10] [--out fill_bench.json]
Wall times are host times around synchronised calls (they include the one count read-back each stage needs); kernel times
come from the library's own event timing (nm_prof_*) in a separate pass, since the event pairs perturb the wall time."""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from neuma_amd import _lib, gaussian_fill as gf          # noqa: E402
from neuma_amd.extras import gaussian_fill as cpu        # noqa: E402


def scene(K, seed=0):
    """K anisotropic Gaussians uniform in a unit cube, scales log-uniform in [0.004, 0.012] (one to three cells at 128)."""
    rng = np.random.default_rng(seed)
    mu = rng.uniform(-0.5, 0.5, (K, 3)).astype(np.float32)
    q = rng.normal(size=(K, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    r, x, y, z = q.T
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], -1),
                  np.stack([2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)], -1),
                  np.stack([2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1)], -2)
    L = R * np.exp(rng.uniform(np.log(0.004), np.log(0.012), (K, 3)))[:, None, :]
    S = L @ L.transpose(0, 2, 1)
    cv = np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], -1).astype(np.float32)
    return mu, cv, rng.uniform(0.3, 0.95, K).astype(np.float32)


def wall_ms(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t))


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--gaussians", type=int, default=200_000)
    p.add_argument("--resolution", type=int, default=128)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--out", type=str, default=None)
    a = p.parse_args(argv)
    dev = torch.device("cuda", 0)
    mu, cv, op = scene(a.gaussians)
    origin, h, dims = cpu.fill_lattice(mu, cv, a.resolution)
    b0, b1 = cpu.gaussian_blocks(mu, cv, origin, h, dims)
    pairs = int((b1 - b0 + 1).prod(1).sum())
    tm, tc, to = (torch.from_numpy(x).to(dev) for x in (mu, cv, op))
    field, _ = gf.density_field(tm, tc, to, origin, h, dims)
    dens = wall_ms(lambda: gf.density_field(tm, tc, to, origin, h, dims), a.reps)
    cls = wall_ms(lambda: gf.classify_emit(field, origin, h, dims), a.reps)
    whole = wall_ms(lambda: gf.fill_from_gaussians(tm, tc, to, resolution=a.resolution, device=dev), a.reps)
    lib = _lib.lib()
    lib.nm_prof_reset()
    lib.nm_prof_enable(1, None)
    for _ in range(a.reps):
        gf.density_field(tm, tc, to, origin, h, dims)
    torch.cuda.synchronize()
    lib.nm_prof_enable(0, None)
    buf = C.create_string_buffer(1 << 16)
    lib.nm_prof_report(buf, len(buf))
    kern = {}
    for line in buf.value.decode().splitlines():
        name, calls, ms = line.split()
        kern[name] = float(ms) / max(int(calls), 1)
    # the device time of one density call, without the event pairs: events around the whole call
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dts = []
    for _ in range(a.reps):
        e0.record()
        gf.density_field(tm, tc, to, origin, h, dims)
        e1.record()
        torch.cuda.synchronize()
        dts.append(e0.elapsed_time(e1))
    dens_dev = float(np.median(dts))
    kernels = sum(kern.values())
    pts, kind, info = gf.fill_from_gaussians(tm, tc, to, resolution=a.resolution, device=dev)
    rec = dict(gaussians=a.gaussians, resolution=a.resolution, dims=[int(d) for d in dims], pairs=pairs, particles=int(len(pts)),
               density_wall_ms_median=dens[0], density_wall_ms_min=dens[1], classify_emit_wall_ms_median=cls[0],
               fill_wall_ms_median=whole[0], fill_wall_ms_min=whole[1], density_stream_ms_median=dens_dev, kernel_ms=kern,
               kernels_ms=kernels, scan_sort_and_gaps_ms=dens_dev - kernels,
               dominant="k_fill_density" if kern.get("k_fill_density", 0.0) > dens_dev - kernels else "scan + pair sort",
               device=torch.cuda.get_device_name(0))
    print(json.dumps(rec))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
