"""Particle-accuracy metrics of modules/tune/metrics.py on the GPU, name for name: `chamfer_distance`,
`chamfer_distance_kdtree`, `chamfer_distance_naive` and `get_nearest_neighbors_indices_batch`.  The reference builds one scipy
cKDTree per batch item on the host; here every nearest-neighbour search is the exact grid search of one HIP entry point,
`nm_chamfer` / `nm_nearest_neighbors` (csrc/nm_nn.hip); `k_nearest_neighbors` is the same search for 1 <= k <= 16 (`nm_knn`).

`emd_native` / `earth_movers_distance` add the earth mover's distance between clouds of equal size (no reference counterpart):
an exact, bitwise repeatable linear assignment by one HIP entry point, `nm_emd` (csrc/nm_emd.hip; the numpy twin and CPU path
is extras/emd.py).

GPU tensors only: a CPU tensor raises NeumaHipError (there is no CPU path).  Coordinates are searched on fp32 copies, so fp64
inputs are rounded to fp32 first; the squared distances are computed in fp64 from those fp32 values, and the winner is the
lexicographic minimum of (distance^2, index), i.e. cKDTree's fp64 choice except on exact ties.  The distances returned are
the reference's gather form (points - points[idx])^2 in the input's floating dtype, so they are differentiable in both clouds;
the gradient flows through the gather, never through the (piecewise constant) indices."""
import numpy as np
import torch

from . import _lib as L


def _check_clouds(points1, points2):
    if not (isinstance(points1, torch.Tensor) and isinstance(points2, torch.Tensor)):
        raise TypeError("points1 and points2 must be tensors")
    if not (points1.is_cuda and points2.is_cuda):
        raise L.NeumaHipError("particle metrics need tensors on the GPU (no CPU path)")
    if points1.dim() != 3 or points2.dim() != 3 or points1.shape[2] != 3 or points2.shape[2] != 3:
        raise ValueError(f"expected (B, N, 3) and (B, M, 3) clouds, got {tuple(points1.shape)} and {tuple(points2.shape)}")
    if points1.shape[0] != points2.shape[0]:
        raise ValueError(f"batch sizes differ: {points1.shape[0]} and {points2.shape[0]}")
    if points1.shape[0] < 1 or points1.shape[1] < 1 or points2.shape[1] < 1:
        raise ValueError(f"empty point cloud: {tuple(points1.shape)} and {tuple(points2.shape)}")
    if not (points1.is_floating_point() and points2.is_floating_point()):
        raise TypeError("points must be floating point")
    L.same_device(points1, points2)


def chamfer_native(points1, points2):
    """One nm_chamfer call: (cd12[B], cd21[B], idx12[B, N], idx21[B, M]), the means fp64 and the indices int64 on the device.
    cd12[b] = mean over points1[b] of the fp64 squared distance to its nearest point of points2[b] (NaN where either cloud
    of item b holds a NaN / Inf coordinate).  No host synchronisation."""
    _check_clouds(points1, points2)
    lib = L.lib()
    p1 = points1.detach().float().contiguous()
    p2 = points2.detach().float().contiguous()
    b, n, m = int(p1.shape[0]), int(p1.shape[1]), int(p2.shape[1])
    dev = p1.device
    cd12 = torch.empty(b, dtype=torch.float64, device=dev)
    cd21 = torch.empty(b, dtype=torch.float64, device=dev)
    idx12 = torch.empty(b, n, dtype=torch.int64, device=dev)
    idx21 = torch.empty(b, m, dtype=torch.int64, device=dev)
    ws = torch.empty(max(int(lib.nm_chamfer_workspace(b, n, m)), 1), dtype=torch.uint8, device=dev)
    L.check(lib.nm_chamfer(b, n, m, L.ptr(p1), L.ptr(p2), cd12.data_ptr(), cd21.data_ptr(), idx12.data_ptr(), idx21.data_ptr(),
                           L.ptr(ws), ws.numel(), L.stream_ptr(dev)), "nm_chamfer")
    return cd12, cd21, idx12, idx21


def nearest_neighbors(query, target):
    """One nm_nearest_neighbors call: (idx[B, N] int64, d2[B, N] fp64) of every query point's nearest target point."""
    _check_clouds(query, target)
    lib = L.lib()
    q = query.detach().float().contiguous()
    t = target.detach().float().contiguous()
    b, n, m = int(q.shape[0]), int(q.shape[1]), int(t.shape[1])
    idx = torch.empty(b, n, dtype=torch.int64, device=q.device)
    d2 = torch.empty(b, n, dtype=torch.float64, device=q.device)
    ws = torch.empty(max(int(lib.nm_nn_workspace(b, n, m)), 1), dtype=torch.uint8, device=q.device)
    L.check(lib.nm_nearest_neighbors(b, n, m, L.ptr(q), L.ptr(t), idx.data_ptr(), d2.data_ptr(), L.ptr(ws), ws.numel(),
                                     L.stream_ptr(q.device)), "nm_nearest_neighbors")
    return idx, d2


def k_nearest_neighbors(query, target, k, exclude_same_index=False):
    """One nm_knn call: (idx[B, N, k] int64, d2[B, N, k] fp64), every query point's k nearest target points in ascending
    (distance^2, index) order, 1 <= k <= 16.  exclude_same_index (query and target are the same cloud): target i is no
    neighbour of query i, whatever its distance."""
    _check_clouds(query, target)
    lib = L.lib()
    q = query.detach().float().contiguous()
    t = target.detach().float().contiguous()
    b, n, m, k = int(q.shape[0]), int(q.shape[1]), int(t.shape[1]), int(k)
    idx = torch.empty(b, n, max(k, 0), dtype=torch.int64, device=q.device)
    d2 = torch.empty(b, n, max(k, 0), dtype=torch.float64, device=q.device)
    ws = torch.empty(max(int(lib.nm_knn_workspace(b, n, m, k)), 1), dtype=torch.uint8, device=q.device)
    L.check(lib.nm_knn(b, n, m, k, 1 if exclude_same_index else 0, L.ptr(q), L.ptr(t), idx.data_ptr(), d2.data_ptr(), L.ptr(ws),
                       ws.numel(), L.stream_ptr(q.device)), "nm_knn")
    return idx, d2


def _gather_sq(points, other, idx):
    """(points - other[idx])^2 summed over xyz: the reference's gather formula (metrics.py:69-79)."""
    nn = torch.gather(other, 1, idx.unsqueeze(-1).expand(-1, -1, 3))
    return (points - nn).pow(2).sum(2)


class _Chamfer(torch.autograd.Function):
    """(chamfer1[B], chamfer2[B]) with the indices of one native search; backward = the gather formula's gradient."""

    @staticmethod
    def forward(ctx, points1, points2, idx12, idx21):
        ctx.save_for_backward(points1, points2, idx12, idx21)
        with torch.no_grad():
            c1 = _gather_sq(points1, points2, idx12).mean(1)
            c2 = _gather_sq(points2, points1, idx21).mean(1)
        return c1, c2

    @staticmethod
    def backward(ctx, g1, g2):
        points1, points2, idx12, idx21 = ctx.saved_tensors
        n, m = points1.shape[1], points2.shape[1]
        d12 = points1 - torch.gather(points2, 1, idx12.unsqueeze(-1).expand(-1, -1, 3))        # (B, N, 3)
        d21 = points2 - torch.gather(points1, 1, idx21.unsqueeze(-1).expand(-1, -1, 3))        # (B, M, 3)
        w12 = d12 * (2.0 * g1.view(-1, 1, 1) / n)
        w21 = d21 * (2.0 * g2.view(-1, 1, 1) / m)
        grad1 = w12.clone()
        grad1.scatter_add_(1, idx21.unsqueeze(-1).expand(-1, -1, 3), -w21)
        grad2 = w21.clone()
        grad2.scatter_add_(1, idx12.unsqueeze(-1).expand(-1, -1, 3), -w12)
        return grad1, grad2, None, None


def _chamfer_terms(points1, points2):
    _, _, idx12, idx21 = chamfer_native(points1, points2)
    c1, c2 = _Chamfer.apply(points1, points2, idx12, idx21)
    return c1, c2, idx12, idx21


def chamfer_distance(points1, points2, use_kdtree=True, give_id=False):
    """metrics.py chamfer_distance: chamfer1 + chamfer2 per item, shape (B,), for (B, N, 3) and (B, M, 3) GPU clouds."""
    if use_kdtree:
        return chamfer_distance_kdtree(points1, points2, give_id=give_id)
    return chamfer_distance_naive(points1, points2)


def chamfer_distance_naive(points1, points2):
    """metrics.py chamfer_distance_naive: the reference's equal-size assertion, then the same native search (the reference
    forms the dense B x T x T distance matrix instead)."""
    assert points1.size() == points2.size()
    c1, c2, _, _ = _chamfer_terms(points1, points2)
    return c1 + c2


def chamfer_distance_kdtree(points1, points2, give_id=False):
    """metrics.py chamfer_distance_kdtree: chamfer1 + chamfer2, or (chamfer1, chamfer2, idx_nn_12, idx_nn_21) with
    give_id=True (int64 indices of shape (B, N) and (B, M) on the inputs' device)."""
    c1, c2, idx12, idx21 = _chamfer_terms(points1, points2)
    if give_id:
        return c1, c2, idx12, idx21
    return c1 + c2


def get_nearest_neighbors_indices_batch(points_src, points_tgt, k=1):
    """metrics.py get_nearest_neighbors_indices_batch on numpy batches: (indices, distances), lists of one int64 and one
    float64 array per item, the distances Euclidean (not squared) as cKDTree.query returns them.  The search runs on the
    current GPU."""
    if k != 1:
        raise NotImplementedError("get_nearest_neighbors_indices_batch: only k=1 is provided")
    dev = torch.device("cuda", torch.cuda.current_device())
    src = torch.as_tensor(np.asarray(points_src, dtype=np.float32)).to(dev)
    tgt = torch.as_tensor(np.asarray(points_tgt, dtype=np.float32)).to(dev)
    idx, d2 = nearest_neighbors(src, tgt)
    idx, d = idx.cpu().numpy(), torch.sqrt(d2).cpu().numpy()
    return [idx[i] for i in range(idx.shape[0])], [d[i] for i in range(d.shape[0])]


EMD_MAX_POINTS = 8192


def _check_emd_clouds(points1, points2):
    _check_clouds(points1, points2)
    if points1.shape[1] != points2.shape[1]:
        raise ValueError(f"EMD needs clouds of equal size, got {points1.shape[1]} and {points2.shape[1]} points: subsample the "
                         f"larger one (subsample_indices)")


def emd_native(points1, points2, power=1, max_rounds=None, give_prices=False):
    """One nm_emd call: (emd[B] fp64, idx[B, n] int64, rounds[B] int64[, prices[B, n] int64]) on the device, for (B, n, 3) clouds
    of equal size 1 <= n <= 8192 and power 1 or 2.  idx[b, i] is the point of points2[b] that point i of points1[b] is assigned
    to by the exact optimum of the quantised assignment problem (include/neuma_hip.h states it); emd[b] = mean_i c(i, idx(i))
    from the unquantised fp64 costs of the fp32 coordinates.  The reported value exceeds the true fp64 optimum by at most
    2^-k <= Cmax * 2^-23.  NaN / -1 / rounds 0 for an item with a NaN / Inf coordinate.  max_rounds: None = the default of
    extras/emd.py (1667 n); an item not finished by then raises NeumaHipError naming it.  No host synchronisation besides the
    status read-back of the call."""
    _check_emd_clouds(points1, points2)
    from .extras.emd import default_max_rounds
    lib = L.lib()
    p1 = points1.detach().float().contiguous()
    p2 = points2.detach().float().contiguous()
    b, n = int(p1.shape[0]), int(p1.shape[1])
    dev = p1.device
    emd = torch.empty(b, dtype=torch.float64, device=dev)
    idx = torch.empty(b, n, dtype=torch.int64, device=dev)
    rounds = torch.empty(b, dtype=torch.int64, device=dev)
    prices = torch.empty(b, n, dtype=torch.int64, device=dev) if give_prices else None
    ws = torch.empty(max(int(lib.nm_emd_workspace(b, n)), 1), dtype=torch.uint8, device=dev)
    L.check(lib.nm_emd(b, n, int(power), int(default_max_rounds(n) if max_rounds is None else max_rounds), L.ptr(p1), L.ptr(p2),
                       emd.data_ptr(), idx.data_ptr(), None if prices is None else prices.data_ptr(), rounds.data_ptr(), L.ptr(ws),
                       ws.numel(), L.stream_ptr(dev)), "nm_emd")
    return (emd, idx, rounds, prices) if give_prices else (emd, idx, rounds)


def earth_movers_distance(points1, points2, power=1, give_id=False):
    """mean_i |x_i - y_idx(i)|^power per item, shape (B,), in the input dtype, for (B, n, 3) GPU clouds of equal size n <= 8192,
    with idx the optimal assignment of one nm_emd call (emd_native); with give_id also idx (B, n) int64.  Computed through the
    gather, so it is differentiable in both clouds; the gradient flows through the gather, never through the (piecewise
    constant) indices.  Unequal sizes raise ValueError: subsample the larger cloud (subsample_indices).  The value exceeds the
    true optimum of the fp32 clouds by at most Cmax * 2^-23 plus the rounding of the input dtype."""
    if power not in (1, 2):
        raise ValueError(f"power must be 1 or 2, got {power}")
    _check_emd_clouds(points1, points2)
    if points1.shape[1] > EMD_MAX_POINTS:
        raise ValueError(f"EMD takes at most {EMD_MAX_POINTS} points per cloud, got {points1.shape[1]}: subsample both clouds "
                         f"(subsample_indices)")
    emd, idx, _ = emd_native(points1, points2, power=power)
    d2 = _gather_sq(points1, points2, idx.clamp_min(0))
    if power == 1:          # |x - y| with the zero subgradient at coincident points (sqrt alone has slope inf there)
        zero = d2 == 0
        d2 = torch.where(zero, torch.zeros_like(d2), torch.where(zero, torch.ones_like(d2), d2).sqrt())
    value = d2.mean(1)
    value = torch.where(torch.isnan(emd), torch.full_like(value, float("nan")), value)      # a non-finite item: idx is -1 there
    return (value, idx) if give_id else value


def subsample_indices(N, n, seed):
    """The sorted first n entries of numpy.random.default_rng(seed).permutation(N) as an int64 array; arange(N) when n >= N."""
    N, n = int(N), int(n)
    if n >= N:
        return np.arange(N, dtype=np.int64)
    return np.sort(np.random.default_rng(seed).permutation(N)[:n]).astype(np.int64)
