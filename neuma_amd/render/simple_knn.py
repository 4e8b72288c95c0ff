"""`distCUDA2` of the 3DGS scale initialisation (upstream imports it from simple_knn._C) on the native k-NN search:
for every point the mean squared distance to its 3 nearest OTHER points (nm_knn_mean_dist2, csrc/nm_nn.hip).  Parity with
simple_knn's own arithmetic is unpinned: its source is not part of the reference tree, the definition above is its documented
behaviour."""
import torch

from .. import _lib as L


def mean_knn_dist2(points: torch.Tensor, k: int = 3) -> torch.Tensor:
    """(N,) fp32: mean of the k smallest squared distances from each point of the (N, 3) GPU cloud to the other points
    (excluded by index: a coincident duplicate is a neighbour at distance 0).  Exact search, fp64 distances, rounded once."""
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"expected an (N, 3) tensor, got {tuple(getattr(points, 'shape', ()))}")
    if not points.is_cuda:
        raise L.NeumaHipError("distCUDA2 needs a tensor on the GPU (no CPU path)")
    n = int(points.shape[0])
    if n < k + 1:
        raise ValueError(f"distCUDA2 needs at least {k + 1} points, got {n}")
    lib = L.lib()
    p = points.detach().float().contiguous()
    out = torch.empty(n, dtype=torch.float32, device=p.device)
    ws = torch.empty(max(int(lib.nm_knn_mean_dist2_workspace(n)), 1), dtype=torch.uint8, device=p.device)
    L.check(lib.nm_knn_mean_dist2(n, L.ptr(p), int(k), L.ptr(out), L.ptr(ws), ws.numel(), L.stream_ptr(p.device)), "nm_knn_mean_dist2")
    return out


def distCUDA2(points: torch.Tensor) -> torch.Tensor:
    return mean_knn_dist2(points, 3)
