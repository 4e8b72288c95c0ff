"""fp64 brute-force yardstick of the k-nearest-neighbour search: distances from the fp32 coordinates, summed x, y, z in
separately rounded fp64 operations (the kernel's order), then a stable sort - ties go to the smaller index."""
import torch


def knn_brute(query: torch.Tensor, target: torch.Tensor, k: int, exclude_same_index: bool = False):
    """query (N,3), target (M,3) fp32 on the CPU -> (idx (N,k) int64, d2 (N,k) fp64); a non-finite query: indices 0, NaN."""
    q, t = query.float().double(), target.float().double()
    dx = q[:, None, 0] - t[None, :, 0]
    dy = q[:, None, 1] - t[None, :, 1]
    dz = q[:, None, 2] - t[None, :, 2]
    d2 = (dx * dx + dy * dy) + dz * dz
    key = d2.clone()
    key[torch.isnan(key)] = float("inf")                  # a non-finite target is nobody's neighbour
    if exclude_same_index:
        n = min(q.shape[0], t.shape[0])
        key[torch.arange(n), torch.arange(n)] = float("inf")
    order = torch.sort(key, dim=1, stable=True).indices[:, :k]
    out = torch.gather(d2, 1, order)
    bad = ~torch.isfinite(query.float()).all(dim=1)
    order[bad] = 0
    out[bad] = float("nan")
    return order, out
