#!/usr/bin/env python3
"""Driven-mesh timing (neuma_amd.mesh_drive, csrc/nm_meshdrive.hip): an icosphere of 655 362 vertices / 1 310 720 triangles
(level 8) inside a jittered lattice cloud of about 100 000 particles in the unit ball, k = 16.  --iters (>= 50) launches each of
nm_mesh_bind, nm_mesh_normals and the frame's position product (nm_bind_frame over the coefficient rows) under nm_prof_enable(1),
with nm_spmm_csr (D = 3) over the same rows in the same run as the yardstick; mean microseconds per launch.

  normals_bytes   what nm_mesh_normals has to move: positions, vptr, vcorner and triangles read once, normals written once
                  = 12 V + 4 (V + 1) + 12 T + 12 T + 12 V
  normals_copy_us that traffic at the 6.29 TB/s a float4 copy reaches on this part: the floor the kernel is set against

    python tools/exp_mesh_drive.py [--iters 60] [--level 8]

prints one JSON line."""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np  # noqa: E402

COPY_BYTES_PER_S = 6.29e12


def icosphere(level):
    """unit icosphere by vectorised midpoint subdivision: V = 10 * 4^level + 2"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
                  (-t, 0, -1), (-t, 0, 1)], dtype=np.float64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    f = np.array([(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
                  (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)], dtype=np.int64)
    for _ in range(level):
        e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
        key = e[:, 0] * len(v) + e[:, 1]
        uniq, inv = np.unique(key, return_inverse=True)
        mid = v[uniq // len(v)] + v[uniq % len(v)]
        mid /= np.linalg.norm(mid, axis=1, keepdims=True)
        m = len(v) + inv.reshape(3, -1)                    # midpoints of ab, bc, ca per face
        a, b, c = f[:, 0], f[:, 1], f[:, 2]
        f = np.concatenate([np.stack([a, m[0], m[2]], 1), np.stack([b, m[1], m[0]], 1), np.stack([c, m[2], m[1]], 1), np.stack([m[0], m[1], m[2]], 1)])
        v = np.concatenate([v, mid])
    return v, f.astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--level", type=int, default=8)
    args = ap.parse_args()
    import torch
    from neuma_amd import _lib as L
    from neuma_amd.mesh_drive import MeshDriver
    assert torch.cuda.is_available(), "exp_mesh_drive.py measures on the GPU; there is no fallback"
    assert args.iters >= 50
    dev = torch.device("cuda", 0)
    lib = L.lib()
    rng = np.random.default_rng(0)
    n = 58                                                # 58^3 cell centres of [-1, 1]^3, those in the unit ball: about 100 000
    ax = (np.arange(n) + 0.5) / n * 2 - 1
    g = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    X = (g + rng.uniform(-0.25, 0.25, g.shape) * 2 / n)[(g * g).sum(1) <= 1.0].astype(np.float32)
    sv, st = icosphere(args.level)
    d = MeshDriver((0.9 * sv).astype(np.float32), st, X, device=dev)
    x = d.rest + 0.05 * torch.sin(7.0 * d.rest)
    u = (x - d.rest).contiguous()
    pos = torch.empty(d.V, 3, device=dev)
    nrm = torch.empty(d.V, 3, device=dev)
    prod = torch.empty(d.V, 3, device=dev)
    s = L.stream_ptr(dev)

    def run():
        L.check(lib.nm_mesh_bind(d.V, d.N, d.k, d.damping, L.ptr(d.vertices), L.ptr(d.rest), d.idx.data_ptr(), d.d2.data_ptr(), L.ptr(d.col),
                                 L.ptr(d.coeff), L.ptr(d.weight), s), "nm_mesh_bind")
        L.check(lib.nm_bind_frame(d.V, L.ptr(d.rowptr), L.ptr(d.col), L.ptr(d.coeff), L.ptr(x), L.ptr(d.rest), L.ptr(d.vertices), None, None,
                                  L.ptr(pos), None, None, s), "nm_bind_frame")
        L.check(lib.nm_spmm_csr(d.V, 3, L.ptr(d.rowptr), L.ptr(d.col), L.ptr(d.coeff), L.ptr(u), L.ptr(prod), s), "nm_spmm_csr")
        L.check(lib.nm_mesh_normals(d.V, d.T, L.ptr(pos), L.ptr(d.triangles), L.ptr(d.vptr), L.ptr(d.vcorner), L.ptr(nrm), s), "nm_mesh_normals")

    for _ in range(3):
        run()
    torch.cuda.synchronize()
    lib.nm_prof_reset(); lib.nm_prof_enable(1, None)
    for _ in range(args.iters):
        run()
    torch.cuda.synchronize()
    lib.nm_prof_enable(0, None)
    buf = C.create_string_buffer(1 << 16)
    lib.nm_prof_report(buf, len(buf))
    rows = {r.split()[0]: (int(r.split()[1]), float(r.split()[2])) for r in buf.value.decode().splitlines() if r.strip()}
    nbytes = 12 * d.V + 4 * (d.V + 1) + 12 * d.T + 12 * d.T + 12 * d.V
    out = dict(V=d.V, T=d.T, N=d.N, k=d.k, iters=args.iters, describe=d.describe(), normals_bytes=nbytes,
               normals_copy_us=round(nbytes / COPY_BYTES_PER_S * 1e6, 2))
    for kern in ("k_mesh_bind", "k_mesh_normals", "k_bind_frame", "k_spmm_csr"):
        cnt, ms = rows.get(kern, (0, 0.0))
        out[kern + "_us"] = round(1e3 * ms / cnt, 2) if cnt else None
        out[kern + "_launches"] = cnt
    # valence 100: 6 500 closed fans (a hub and 100 rim vertices each, V about the same) through nm_mesh_normals alone - every
    # workgroup holds two or three hubs whose lanes add 100 products from LDS while their neighbours add two
    hubs, seg = 6500, 100
    ang = 2 * np.pi * np.arange(seg) / seg
    rim = np.stack([np.cos(ang), np.sin(ang), np.zeros(seg)], 1)
    fv = np.concatenate([np.concatenate([[[0.0, 0.0, 0.3]], rim]) + [3.0 * (h % 80), 3.0 * (h // 80), 0.0] for h in range(hubs)]).astype(np.float32)
    base = (np.arange(hubs) * (seg + 1))[:, None]
    j = np.arange(seg)[None, :]
    ft = np.stack([base + 0 * j, base + 1 + j, base + 1 + (j + 1) % seg], -1).reshape(-1, 3).astype(np.int32)
    from neuma_amd.extras import mesh_drive as md
    vptr, vcorner = md.corner_adjacency(ft, len(fv))
    tv, tt, tp, tc = (torch.from_numpy(a).to(dev) for a in (fv, ft, vptr, vcorner))
    fn = torch.empty(len(fv), 3, device=dev)
    lib.nm_prof_reset(); lib.nm_prof_enable(1, None)
    for _ in range(args.iters):
        L.check(lib.nm_mesh_normals(len(fv), len(ft), L.ptr(tv), L.ptr(tt), L.ptr(tp), L.ptr(tc), L.ptr(fn), s), "nm_mesh_normals")
    torch.cuda.synchronize()
    lib.nm_prof_enable(0, None)
    lib.nm_prof_report(buf, len(buf))
    rows = {r.split()[0]: (int(r.split()[1]), float(r.split()[2])) for r in buf.value.decode().splitlines() if r.strip()}
    cnt, ms = rows.get("k_mesh_normals", (0, 0.0))
    fbytes = 28 * len(fv) + 4 + 24 * len(ft)
    out["fans"] = dict(V=len(fv), T=len(ft), k_mesh_normals_us=round(1e3 * ms / cnt, 2) if cnt else None,
                       normals_copy_us=round(fbytes / COPY_BYTES_PER_S * 1e6, 2), hub_z=round(float(fn[0, 2]), 4))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
