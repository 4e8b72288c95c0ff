#!/usr/bin/env python3
"""Surface extraction timing (neuma_amd.surface_mesh, csrc/nm_surface.hip): the sphere field 1 - |x - c| / R at level 1/2 on
128^3 and 256^3 lattices.
  count_ms    one nm_surface_count call (k_surface_count + the two rocPRIM scans) on device-resident, preallocated buffers
  emit_ms     one nm_surface_emit call (k_surface_emit), outputs preallocated
              (both: device events around --iters back-to-back calls after --warmup calls)
  extract_ms  surface_mesh.extract end to end: allocations, both calls and the host read-back of the totals, host clock around
              a synchronise
  bytes       the traffic the algorithm needs, from the shapes ("Surface meshes"): 18 B per extended sample (count: 4
              read + 2 written; scans: 2 read + 8 written; emit: 2 read) + 24 B per vertex + 12 B per triangle written
  hbm_frac    bytes / 6.3 TB/s (the achievable HBM rate) over count_ms + emit_ms: the share of the memory bound reached
  numpy_s     extras.surface_mesh.extract on the same lattice (context only; --cpu)

    python tools/exp_surface.py [--iters 20] [--warmup 3] [--cpu] [--sizes 128 256]

prints one JSON line.  Per-kernel times come from a run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -o surface -- python tools/exp_surface.py"""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
ISO = 0.5


def sphere(n):
    h = 2.0 / n
    ax = (np.arange(n, dtype=np.float64) + 0.5) * h
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    r = np.sqrt((X - 1.013) ** 2 + (Y - 0.979) ** 2 + (Z - 1.008) ** 2)
    return (1.0 - r / 1.8).astype(np.float32).reshape(-1), np.zeros(3), h, (n, n, n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    args = ap.parse_args()
    import ctypes as C
    import torch
    from neuma_amd import _lib as L, surface_mesh
    from neuma_amd.extras import surface_mesh as cpu
    assert torch.cuda.is_available(), "exp_surface.py measures on the GPU; there is no fallback"
    dev = torch.device("cuda", 0)
    lib = L.lib()
    out = {}
    for n in args.sizes:
        f_np, origin, h, dims = sphere(n)
        f = torch.from_numpy(f_np).to(dev)
        ne = (n + 2) ** 3
        d, o = (C.c_int32 * 3)(*dims), (C.c_double * 3)(*origin)
        c = surface_mesh.count(f, dims, ISO)
        V, T = c["V"], c["T"]
        ws = torch.empty(int(lib.nm_surface_workspace(d)), dtype=torch.uint8, device=dev)
        info = torch.empty(3, dtype=torch.int64, device=dev)
        verts, normals = torch.empty((V, 3), device=dev), torch.empty((V, 3), device=dev)
        tris = torch.empty((T, 3), dtype=torch.int32, device=dev)
        stream = L.stream_ptr(dev)

        def run_count():
            L.check(lib.nm_surface_count(d, f.data_ptr(), ISO, c["mask"].data_ptr(), c["tri_count"].data_ptr(), c["vert_offset"].data_ptr(),
                                         c["tri_offset"].data_ptr(), info.data_ptr(), ws.data_ptr(), ws.numel(), stream), "nm_surface_count")

        def run_emit():
            L.check(lib.nm_surface_emit(d, o, h, f.data_ptr(), ISO, 0, None, c["mask"].data_ptr(), c["tri_count"].data_ptr(),
                                        c["vert_offset"].data_ptr(), c["tri_offset"].data_ptr(), V, T, verts.data_ptr(), normals.data_ptr(),
                                        None, tris.data_ptr(), stream), "nm_surface_emit")

        ms = {}
        for name, fn in (("count", run_count), ("emit", run_emit)):
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            ms[name] = a.elapsed_time(b) / args.iters
        for _ in range(args.warmup):
            surface_mesh.extract(f, origin, h, dims, ISO)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            surface_mesh.extract(f, origin, h, dims, ISO)
        torch.cuda.synchronize()
        e2e = (time.perf_counter() - t0) / args.iters * 1e3
        nbytes = 18 * ne + 24 * V + 12 * T
        bound_ms = nbytes / HBM_BYTES_PER_S * 1e3
        out[str(n)] = dict(V=V, T=T, count_ms=round(ms["count"], 4), emit_ms=round(ms["emit"], 4), extract_ms=round(e2e, 4), bytes=nbytes,
                           hbm_bound_ms=round(bound_ms, 5), hbm_frac=round(bound_ms / (ms["count"] + ms["emit"]), 4))
        if args.cpu:
            t0 = time.perf_counter()
            cpu.extract(f_np, origin, h, dims, ISO)
            out[str(n)]["numpy_s"] = round(time.perf_counter() - t0, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
