"""GPU: the exact k-nearest-neighbour search (nm_knn), distCUDA2 (nm_knn_mean_dist2) and GaussianModel.create_from_pcd against
an fp64 brute force.  With the lexicographic (distance^2, index) rule the indices have no tolerance, and the distances are
compared to the last bit (the yardstick sums x, y, z in the kernel's order)."""
import numpy as np
import pytest
import torch

from gpu_util import dev, measured
from knn_ref import knn_brute

pytestmark = pytest.mark.gpu


def _rand(n, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.rand(n, 3, generator=g)).float()


def _clouds():
    """name -> (query, target or None for 'the same cloud', k)"""
    c = {}
    c["n4_k3"] = (_rand(4, 1), None, 3)
    c["coincident64"] = (torch.full((64, 3), 0.25), None, 5)
    plane = _rand(200, 2); plane[:, 2] = 0.5
    c["plane200"] = (plane, None, 4)
    c["query_outside_box"] = (_rand(50, 3) + torch.tensor([3.0, -2.0, 5.0]), _rand(300, 4), 6)
    a, b = 0.002 * _rand(8, 5), 0.002 * _rand(8, 6) + torch.tensor([1.0, 0.0, 0.0])
    c["two_clusters_of_8"] = (torch.cat([a, b]), None, 10)
    # the same with a grid fine enough for the gap to be > 100 cell edges: 240 points -> 120 cells along x (y, z thinner than a
    # cell), 8 points in the first cell and 232 in the last twelve; the 8 need 3 neighbours from the far side
    far = 0.002 * _rand(232, 7); far[:, 0] = 0.9 + 0.1 * _rand(232, 8)[:, 0]
    c["cluster_across_100_empty_cells"] = (torch.cat([a, far]), None, 10)
    dup = _rand(150, 9)
    c["every_point_twice"] = (torch.cat([dup, dup]), None, 3)
    nanq = _rand(40, 10); nanq[7, 1] = float("nan")
    c["nan_query"] = (nanq, _rand(60, 11), 3)
    return c


CLOUDS = _clouds()


def _native(q, t, k, excl):
    from neuma_amd.particle_metrics import k_nearest_neighbors
    d = dev()
    qd = q.to(d)[None]
    td = qd if t is None else t.to(d)[None]
    idx, d2 = k_nearest_neighbors(qd, td, k, exclude_same_index=excl)
    return idx[0].cpu(), d2[0].cpu()


def _assert_equal(idx, d2, ridx, rd2):
    assert measured((idx != ridx).sum(), "index mismatches") <= 0
    same = (d2 == rd2) | (torch.isnan(d2) & torch.isnan(rd2))
    assert measured((~same).sum(), "distance bit mismatches") <= 0


@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_knn_equals_the_brute_force(name):
    q, t, k = CLOUDS[name]
    excl = t is None
    idx, d2 = _native(q, t, k, excl)
    ridx, rd2 = knn_brute(q, q if t is None else t, k, excl)
    _assert_equal(idx, d2, ridx, rd2)
    idx2, d22 = _native(q, t, k, excl)                                  # two calls of one input: identical bits
    assert torch.equal(idx, idx2) and torch.equal(d2.view(torch.int64), d22.view(torch.int64))


def test_too_few_eligible_targets_raise():
    from neuma_amd import NeumaHipError
    from neuma_amd.particle_metrics import k_nearest_neighbors
    p = _rand(3, 20).to(dev())[None]
    with pytest.raises(NeumaHipError):
        k_nearest_neighbors(p, p, 3, exclude_same_index=True)
    k_nearest_neighbors(p, p, 3)                                        # all three are eligible without the exclusion
    for k in (0, 17):
        with pytest.raises(NeumaHipError):
            k_nearest_neighbors(p, p, k)


_BATCH = torch.stack([_rand(5000, 30), 0.3 * _rand(5000, 31) + 0.2, _rand(5000, 32) * torch.tensor([1.0, 0.05, 2.0])])
_BATCH_REF = {}


def _batch_ref(k_max=16):
    if not _BATCH_REF:
        for b in range(3):
            _BATCH_REF[b] = knn_brute(_BATCH[b], _BATCH[b], k_max, True)
    return _BATCH_REF


@pytest.mark.parametrize("k", [1, 3, 8, 16])
def test_batched_random_clouds(k):
    from neuma_amd.particle_metrics import k_nearest_neighbors, nearest_neighbors
    d = dev()
    pts = _BATCH.to(d)
    idx, d2 = k_nearest_neighbors(pts, pts, k, exclude_same_index=True)
    ref = _batch_ref()
    for b in range(3):
        _assert_equal(idx[b].cpu(), d2[b].cpu(), ref[b][0][:, :k], ref[b][1][:, :k])
    if k == 1:                                                           # bit for bit the 1-NN entry point (no exclusion there)
        other = torch.roll(pts, 1, 0).contiguous()
        i1, s1 = nearest_neighbors(pts, other)
        ik, sk = k_nearest_neighbors(pts, other, 1)
        assert torch.equal(i1, ik[..., 0]) and torch.equal(s1.view(torch.int64), sk[..., 0].contiguous().view(torch.int64))


def _ulp_f32(x):
    x = np.abs(np.asarray(x, dtype=np.float32))
    return np.maximum(np.spacing(x), np.float32(1.4e-45)).astype(np.float64)


@pytest.mark.parametrize("name", sorted(n for n, (q, t, k) in CLOUDS.items() if t is None and q.shape[0] >= 4) + ["batch0"])
def test_distCUDA2_is_the_mean_of_the_three_nearest(name):
    """Bound: 1 ulp of fp32 - the mean is formed in fp64 from the exact fp64 distances and rounded once."""
    from neuma_amd.render.simple_knn import distCUDA2
    pts = _BATCH[0] if name == "batch0" else CLOUDS[name][0]
    out = distCUDA2(pts.to(dev())).cpu().numpy().astype(np.float64)
    _, rd2 = knn_brute(pts, pts, 3, True)
    ref = ((rd2[:, 0] + rd2[:, 1] + rd2[:, 2]) / 3.0).numpy()
    ref32 = ref.astype(np.float32)
    err = np.abs(out - ref32.astype(np.float64)) / _ulp_f32(ref32)
    assert measured(err.max(), "distCUDA2 error in fp32 ulp") <= 1.0
    assert out.shape == (pts.shape[0],)


def test_distCUDA2_rejects_small_and_cpu_inputs():
    from neuma_amd import NeumaHipError
    from neuma_amd.render.simple_knn import distCUDA2
    with pytest.raises(ValueError):
        distCUDA2(_rand(3, 40).to(dev()))
    with pytest.raises(NeumaHipError):
        distCUDA2(_rand(10, 41))


def test_create_from_pcd():
    from neuma_amd.render.gaussian_model import GaussianModel
    from neuma_amd.render.general_utils import RGB2SH, inverse_sigmoid
    pts, col = _rand(1000, 50), _rand(1000, 51)
    g = GaussianModel(2).create_from_pcd(pts.numpy(), col.numpy(), 1.7, device=dev())
    _, rd2 = knn_brute(pts, pts, 3, True)
    dist2 = ((rd2[:, 0] + rd2[:, 1] + rd2[:, 2]) / 3.0).float().clamp_min(1e-7)
    want = torch.log(torch.sqrt(dist2))[:, None].repeat(1, 3)
    # dist2 is the yardstick's to the bit (test above); sqrt and log on the device may each round differently from the host's:
    # sqrt's ulp moves the logarithm by 2^-24 at the most, log's own rounding is one ulp of a result of magnitude < 16 (the clamp
    # bounds it by |log sqrt 1e-7| = 8.06): 2^-20, and twice that for two differently rounded sides
    assert measured((g._scaling.detach().cpu() - want).abs().max(), "log-scale abs err") <= 2 * 2.0 ** -20
    assert torch.equal(g._opacity.detach().cpu(), inverse_sigmoid(0.1 * torch.ones(1000, 1)))
    # RGB2SH on the device, where create_from_pcd evaluates it: the device divides by a constant through its reciprocal, so the
    # host's quotient differs from it in the last bit
    assert torch.equal(g._features_dc.detach().cpu()[:, 0], RGB2SH(col.to(dev())).cpu())
    assert g._features_rest.shape == (1000, 8, 3) and float(g._features_rest.abs().max()) == 0
    assert torch.equal(g._rotation.detach().cpu(), torch.tensor([[1.0, 0, 0, 0]]).repeat(1000, 1))
    assert g.active_sh_degree == 0 and g.max_sh_degree == 2 and g.spatial_lr_scale == 1.7 and g.max_radii2D.shape == (1000,)
