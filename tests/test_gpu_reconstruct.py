"""GPU: the static Gaussian fit (neuma_amd.reconstruct).  The native iteration against the same iteration through autograd,
the densification statistics it feeds, and a short fit with densification against the autograd path under one schedule."""
import math

import numpy as np
import pytest
import torch

from gpu_util import dev, measured, parity, rel_max

pytestmark = pytest.mark.gpu

NAMES = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
_SCENE = {}


def _scene():
    """2000 target Gaussians inside a ball of radius 0.5 around (0.5, 0.5, 0.5), sh_degree 1, 6 ring cameras, 96 x 96; the
    targets rendered by the rasterizer.  Built once."""
    if not _SCENE:
        from neuma_amd import synth
        from neuma_amd.render import gaussian_activate, get_rasterizer, raster_forward_raw
        d = dev()
        g = torch.Generator().manual_seed(0)
        v = torch.randn(2000, 3, generator=g)
        xyz = 0.5 + 0.5 * v / v.norm(dim=1, keepdim=True) * torch.rand(2000, 1, generator=g) ** (1 / 3)
        P = dict(xyz=xyz.float(), dc=0.8 * torch.randn(2000, 1, 3, generator=g), rest=0.2 * torch.randn(2000, 3, 3, generator=g),
                 ls=torch.log(0.015 + 0.02 * torch.rand(2000, 3, generator=g)), rot=torch.randn(2000, 4, generator=g),
                 op=1.0 + torch.randn(2000, 1, generator=g))
        P = {k: t.float().contiguous().to(d) for k, t in P.items()}
        cams = synth.ring_cameras(6, 96, 96, device=d)
        bg = torch.zeros(3, device=d)
        cov, op = gaussian_activate(P["ls"], P["rot"], P["op"])
        sh = torch.cat((P["dc"], P["rest"]), 1).contiguous()
        gts = [raster_forward_raw(get_rasterizer(c, 1, False, bg)._cam, P["xyz"], sh, None, op, cov)[0].clone() for c in cams]
        _SCENE.update(P=P, cams=cams, bg=bg, gts=gts)
    return _SCENE


def _start_model(seed=1):
    """the targets, perturbed: a start both paths share"""
    from neuma_amd.reconstruct import fit_options
    from neuma_amd.render.gaussian_model import GaussianModel
    P = _scene()["P"]
    g = torch.Generator().manual_seed(seed)
    n = lambda t, s: (t + s * torch.randn(t.shape, generator=g).to(t.device)).contiguous()
    m = GaussianModel(1)
    m.set_params(n(P["xyz"], 0.01), n(P["dc"], 0.2), n(P["rest"], 0.05), n(P["ls"], 0.1), n(P["rot"], 0.1), n(P["op"], 0.3))
    m.spatial_lr_scale = 1.0
    m.training_setup(fit_options())
    return m


def test_native_step_matches_the_autograd_step():
    """20 iterations, no densification, one view order, the same Adam: bounds of tests/test_gpu_regist.py's native-vs-autograd
    loop (loss history 1e-4, parameters 1e-5, relative to the largest value)."""
    from neuma_amd.reconstruct import NativeGaussianFit, fit_step_torch
    from neuma_amd.render import flush_pending
    sc = _scene()
    a, b = _start_model(), _start_model()
    run = NativeGaussianFit(a, sc["bg"], 0.2, 20)
    hist_t, worst = [], {n: 0.0 for n in NAMES}
    for it in range(20):
        v = it % 6
        run.step(sc["cams"][v], sc["gts"][v])
        loss, _, _ = fit_step_torch(b, sc["cams"][v], sc["gts"][v], sc["bg"], 0.2)
        hist_t.append(float(loss))
        for n in NAMES:
            worst[n] = max(worst[n], float(rel_max(getattr(a, n).detach(), getattr(b, n).detach())))
    flush_pending()
    hist_n = run.losses()
    for n in NAMES:
        print("MEASURED", n, worst[n])
    print("MEASURED loss", float(rel_max(torch.tensor(hist_n), torch.tensor(hist_t))))
    parity("reconstruct step parity", "loss history", float(rel_max(torch.tensor(hist_n), torch.tensor(hist_t))), 1e-4)
    for n in NAMES:
        parity("reconstruct step parity", n, worst[n], 1e-5)
    assert hist_n[-1] < hist_n[0]


def test_densification_statistics_after_one_step():
    from neuma_amd.reconstruct import NativeGaussianFit, fit_options
    sc = _scene()
    m = _start_model()
    run = NativeGaussianFit(m, sc["bg"], 0.2, 2)
    for view in (0, 3):
        before_r, before_a, before_d = m.max_radii2D.clone(), m.xyz_gradient_accum.clone(), m.denom.clone()
        radii, dm2 = run.step(sc["cams"][view], sc["gts"][view])
        vis = radii > 0
        m.max_radii2D = torch.where(vis, torch.max(m.max_radii2D, radii.float()), m.max_radii2D)
        m.add_densification_stats(dm2, vis)
        want = before_a + torch.where(vis[:, None], dm2[:, :2].norm(dim=1, keepdim=True), torch.zeros_like(before_a))
        assert torch.equal(m.xyz_gradient_accum, want) and torch.equal(m.denom, before_d + vis[:, None].float())
        assert torch.equal(m.max_radii2D, torch.maximum(before_r, torch.where(vis, radii.float(), before_r)))
        assert 0 < int(vis.sum()) <= 2000 and float(m.xyz_gradient_accum[~vis & (before_d[:, 0] == 0)].abs().sum()) == 0


def _mean_l1(m, sc):
    from neuma_amd.render import gaussian_activate, get_rasterizer, raster_forward_raw
    cov, op = gaussian_activate(m._scaling.detach(), m._rotation.detach(), m._opacity.detach())
    sh = m.get_features.detach().contiguous()
    tot = 0.0
    for c, gt in zip(sc["cams"], sc["gts"]):
        img = raster_forward_raw(get_rasterizer(c, m.active_sh_degree, False, sc["bg"])._cam, m._xyz.detach(), sh, None, op, cov)[0]
        tot += float((img - gt).abs().mean())
    return tot / len(sc["cams"])


def test_it_fits_with_densification():
    """300 iterations from create_from_pcd on 1500 jittered target means with grey colours, densifying from iteration 100 every
    50: the mean L1 over the views ends below its start and no worse than 1.1 x what the autograd path reaches under the same
    schedule (the margin covers the two paths' differing fp32 summation orders once densification lets them diverge)."""
    from neuma_amd.reconstruct import camera_extent, fit, fit_options
    from neuma_amd.render.gaussian_model import GaussianModel
    sc = _scene()
    g = torch.Generator().manual_seed(2)
    pts = (sc["P"]["xyz"][:1500].cpu() + 0.02 * 0.5 * torch.randn(1500, 3, generator=g)).numpy()      # 2 % of the ball
    extent = camera_extent(sc["cams"])
    opt = fit_options(iterations=300, densify_from_iter=100, densification_interval=50, opacity_reset_interval=1000,
                      position_lr_max_steps=300)
    final, K = {}, {}
    for native in (True, False):
        m = GaussianModel(1).create_from_pcd(pts, np.full((1500, 3), 0.5, np.float32), extent, device=dev())
        m.training_setup(opt)
        if native:
            start = _mean_l1(m, sc)
        torch.manual_seed(7)
        fit(m, sc["cams"], sc["gts"], sc["bg"], opt, extent, seed=3, native=native)
        final[native], K[native] = _mean_l1(m, sc), m.get_xyz.shape[0]
        assert all(bool(torch.isfinite(getattr(m, n)).all()) for n in NAMES)
    print("MEASURED start", start, "native", final[True], K[True], "autograd", final[False], K[False])
    parity("reconstruct fit 300 it", f"mean L1 native (K={K[True]}) vs start", final[True], start)
    parity("reconstruct fit 300 it", f"mean L1 native vs 1.1 x autograd (K={K[False]})", final[True], 1.1 * final[False])
    assert K[True] != 1500
