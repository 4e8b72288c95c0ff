#!/usr/bin/env python3
"""Point-in-mesh timing (neuma_amd.mesh_inside, csrc/nm_mesh.hip): UV spheres of about 10^4, 10^5 and 10^6 triangles with
the 'volumetric' lattice at resolutions 36 and 60 (46 656 and 216 000 candidate points).
  native_ms   one nm_points_in_mesh call on device-resident inputs (CUDA events around --iters back-to-back calls)
  e2e_s       read_ply_mesh of a binary PLY of the sphere + mesh_inside.sample_mesh_points (upload, call, read-back), host clock
  read_s      read_ply_mesh alone (vectorised face block), and with --loop-reader the per-face loop it falls back to
  cpu_s       extras.mesh_sampling.sample_mesh_points (numpy), only with --cpu and only up to --cpu-max-tris triangles

    python tools/exp_mesh_inside.py [--iters 20] [--warmup 3] [--cpu] [--cpu-max-tris 12000] [--loop-reader] [--no-gpu]

prints one JSON line.  Per-kernel times come from a run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -o mesh -- python tools/exp_mesh_inside.py
(k_mi_prep, k_mi_grid, k_mi_count, rocPRIM's scan, k_mi_scatter, k_mi_query)."""
import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np  # noqa: E402

SIZES = {"1e4": (50, 100), "1e5": (158, 316), "1e6": (500, 1000)}      # (n_lat, n_lon): 2 n_lon (n_lat - 1) triangles


def uv_sphere(n_lat, n_lon):
    th = np.pi * np.arange(1, n_lat) / n_lat
    ph = 2 * np.pi * np.arange(n_lon) / n_lon
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.repeat(np.cos(th)[:, None], n_lon, 1)], -1)
    v = np.concatenate([[[0, 0, 1.0]], ring.reshape(-1, 3), [[0, 0, -1.0]]])
    idx = 1 + np.arange((n_lat - 1) * n_lon).reshape(n_lat - 1, n_lon)
    nxt = np.roll(idx, -1, axis=1)
    top = np.stack([np.zeros(n_lon, int), idx[0], nxt[0]], -1)
    bot = np.stack([np.full(n_lon, len(v) - 1), nxt[-1], idx[-1]], -1)
    a, b, c, d = idx[:-1], idx[1:], nxt[1:], nxt[:-1]
    mid = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return v, np.concatenate([top, mid, bot]).astype(np.int64)


def write_ply(path, v, t):
    hdr = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}", "property float x", "property float y",
           "property float z", f"element face {len(t)}", "property list uchar int vertex_indices", "end_header"]
    faces = np.zeros(len(t), dtype=[("k", "u1"), ("i", "<i4", (3,))])
    faces["k"], faces["i"] = 3, t
    Path(path).write_bytes(("\n".join(hdr) + "\n").encode() + np.asarray(v, "<f4").tobytes() + faces.tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--cpu-max-tris", type=int, default=12000)
    ap.add_argument("--loop-reader", action="store_true")
    ap.add_argument("--no-gpu", action="store_true")
    args = ap.parse_args()
    from neuma_amd.extras import mesh_sampling as cpu
    out = {}
    tmp = Path(tempfile.mkdtemp())
    for name, (nl, nm) in SIZES.items():
        v, t = uv_sphere(nl, nm)
        path = tmp / f"sphere_{name}.ply"
        write_ply(path, v, t)
        t0 = time.perf_counter()
        vr, tr = cpu.read_ply_mesh(path)
        out[f"read_s_{name}"] = round(time.perf_counter() - t0, 4)
        out[f"tris_{name}"] = int(len(tr))
        if args.loop_reader:
            fast = cpu._ply_faces_uniform
            cpu._ply_faces_uniform = lambda *a: None
            t0 = time.perf_counter()
            vl, tl = cpu.read_ply_mesh(path)
            out[f"read_loop_s_{name}"] = round(time.perf_counter() - t0, 3)
            cpu._ply_faces_uniform = fast
            assert np.array_equal(tl, tr) and np.array_equal(vl, vr)
        for res in (36, 60):
            key = f"{name}_r{res}"
            if not args.no_gpu:
                import torch
                from neuma_amd import mesh_inside
                dev = torch.device("cuda", 0)
                pts = cpu.ray_offset_points(cpu.mesh_candidate_points(vr, "volumetric", res), vr)
                P, V = torch.from_numpy(pts).to(dev), torch.from_numpy(vr).to(dev)
                T = torch.from_numpy(tr.astype(np.int32)).to(dev)
                for _ in range(args.warmup):
                    mesh_inside.inside_native(P, V, T)
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.iters):
                    m = mesh_inside.inside_native(P, V, T)
                b.record()
                torch.cuda.synchronize()
                out[f"native_ms_{key}"] = round(a.elapsed_time(b) / args.iters, 4)
                out[f"points_{key}"] = int(len(pts))
                out[f"inside_{key}"] = int(m.sum())
                t0 = time.perf_counter()
                s = mesh_inside.sample_mesh_points(*cpu.read_ply_mesh(path), "volumetric", res, device=dev)
                out[f"e2e_s_{key}"] = round(time.perf_counter() - t0, 4)
                assert len(s) == out[f"inside_{key}"]
            if args.cpu and len(tr) <= args.cpu_max_tris:
                t0 = time.perf_counter()
                cpu.sample_mesh_points(vr, tr, "volumetric", res)
                out[f"cpu_s_{key}"] = round(time.perf_counter() - t0, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
