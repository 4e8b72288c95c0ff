#!/usr/bin/env python3
"""Generate the Chamfer fixtures by EXECUTING THE REFERENCE'S OWN CODE: modules/tune/metrics.py is loaded by path and run as it
is (it imports only torch, numpy and scipy's cKDTree).

Run in the build container only (needs /root/reference; never runs on the GPU box):
    python tests/golden/gen_chamfer_golden.py

Inputs are not stored: tests/golden/chamfer_inputs.py rebuilds them from seeded draws.  Outputs (data only), under
tests/golden/chamfer/:
    <case>.npz for every chamfer_inputs.KDTREE_CASES entry: chamfer_distance_kdtree(p1, p2, give_id=True) on fp32 CPU
               tensors -> chamfer1, chamfer2 (fp32, (B,)), idx12 (int32, (B, N)), idx21 (int32, (B, M)), and
               chamfer_distance(p1, p2) (= chamfer1 + chamfer2) as chamfer
    naive.npz  chamfer_distance_naive(p1, p2) -> chamfer (fp32, (B,))
"""
import importlib.util
import os
import sys
from pathlib import Path

import numpy as np
import torch

REF = Path("/root/reference")
HERE = Path(__file__).resolve().parent
OUT = Path(os.environ.get("NEUMA_GOLDEN_OUT", HERE)) / "chamfer"   # (tests/test_chamfer_golden_regen.py regenerates elsewhere)
sys.path.insert(0, str(HERE))

import chamfer_inputs as CI  # noqa: E402


def load_metrics():
    spec = importlib.util.spec_from_file_location("ref_tune_metrics", REF / "modules" / "tune" / "metrics.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    torch.set_num_threads(1)
    M = load_metrics()
    OUT.mkdir(parents=True, exist_ok=True)
    for name, make in CI.KDTREE_CASES.items():
        a, b = make()
        p1, p2 = torch.from_numpy(a), torch.from_numpy(b)
        c1, c2, i12, i21 = M.chamfer_distance_kdtree(p1, p2, give_id=True)
        cd = M.chamfer_distance(p1, p2)
        np.savez_compressed(OUT / f"{name}.npz", chamfer1=c1.numpy(), chamfer2=c2.numpy(), chamfer=cd.numpy(),
                            idx12=i12.numpy().astype(np.int32), idx21=i21.numpy().astype(np.int32))
    for name, make in CI.NAIVE_CASES.items():
        a, b = make()
        cd = M.chamfer_distance_naive(torch.from_numpy(a), torch.from_numpy(b))
        np.savez_compressed(OUT / f"{name}.npz", chamfer=cd.numpy())
    print("wrote", sorted(f.name for f in OUT.glob("*.npz")))


if __name__ == "__main__":
    main()
