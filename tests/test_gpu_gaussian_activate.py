"""GPU: nm_gaussian_activate / nm_gaussian_activate_backward against build_cov3D + sigmoid and their autograd gradients in fp64.
Bound (the project's rule): 4 x the same torch path's own fp32 error against that fp64 result, floor 1e-6, relative to the largest
value; the fp32 path's error is measured here and both numbers are published."""
import pytest
import torch

from gpu_util import dev, parity

pytestmark = pytest.mark.gpu


def _inputs(K, seed=0):
    g = torch.Generator().manual_seed(seed)
    ls = (-8.0 + 9.0 * torch.rand(K, 3, generator=g)).float()                 # log-scales in [-8, 1]
    rot = torch.randn(K, 4, generator=g).float() * (0.2 + 3.0 * torch.rand(K, 1, generator=g))      # un-normalised
    rot[::5] = torch.nn.functional.normalize(rot[::5], dim=1) * 1e-3             # norm 1e-3
    rot[1::3, 0] = -rot[1::3, 0].abs()                                           # negative w
    logit = (6.0 * torch.randn(K, 1, generator=g)).float()
    gc = torch.randn(K, 6, generator=g).float()
    go = torch.randn(K, 1, generator=g).float()
    return ls, rot, logit, gc, go


def _torch_path(ls, rot, logit, gc, go, mod, dtype):
    from neuma_amd.render import build_cov3D
    a = [t.detach().to(dtype).clone().requires_grad_(True) for t in (ls, rot, logit)]
    cov = build_cov3D(torch.exp(a[0]), a[1], mod)
    op = torch.sigmoid(a[2])
    ((cov * gc.to(dtype)).sum() + (op * go.to(dtype)).sum()).backward()
    return [cov.detach(), op.detach(), a[0].grad, a[1].grad, a[2].grad]


def _rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max() / max(float(b.abs().max()), 1e-30))


@pytest.mark.parametrize("mod", [1.0, 0.7])
@pytest.mark.parametrize("K", [1, 63, 64, 65, 5000])
def test_activate_and_adjoint_match_fp64(K, mod):
    from neuma_amd.render import gaussian_activate, gaussian_activate_backward
    d = dev()
    ls, rot, logit, gc, go = (t.to(d) for t in _inputs(K, seed=K))
    ref = _torch_path(ls, rot, logit, gc, go, mod, torch.float64)
    f32 = _torch_path(ls, rot, logit, gc, go, mod, torch.float32)
    cov, op = gaussian_activate(ls, rot, logit, mod)
    dls, drot, dlogit = gaussian_activate_backward(ls, rot, logit, mod, gc, go)
    for name, got, r64, r32 in zip(("cov6", "opacity", "dlog_scales", "drot", "dopacity_logit"), (cov, op, dls, drot, dlogit), ref, f32):
        noise = _rel(r32, r64)
        parity(f"gaussian_activate K={K} mod={mod}", name, _rel(got, r64), max(4 * noise, 1e-6), noise=noise)
    # NULL outputs are honoured, and two calls give identical bits
    c2, none = gaussian_activate(ls, rot, None, mod, want_opacity=False)
    none2, o2 = gaussian_activate(ls, rot, logit, mod, want_cov=False)
    assert none is None and none2 is None and torch.equal(c2, cov) and torch.equal(o2, op)
    a, b, c = gaussian_activate_backward(ls, rot, logit, mod, gc, None)
    assert c is None and torch.equal(a, dls) and torch.equal(b, drot)
    a, b, c = gaussian_activate_backward(ls, rot, logit, mod, None, go)
    assert a is None and b is None and torch.equal(c, dlogit)


def test_backward_overwrites():
    from neuma_amd import _lib as L
    d = dev()
    ls, rot, logit, gc, go = (t.to(d) for t in _inputs(300, seed=3))
    outs = [torch.full((300, n), 7.0, device=d) for n in (3, 4, 1)]
    for _ in range(2):
        L.check(L.lib().nm_gaussian_activate_backward(300, L.ptr(ls), L.ptr(rot), L.ptr(logit), 1.0, L.ptr(gc), L.ptr(go),
                                                      L.ptr(outs[0]), L.ptr(outs[1]), L.ptr(outs[2]), L.stream_ptr(d)))
    from neuma_amd.render import gaussian_activate_backward
    for got, want in zip(outs, gaussian_activate_backward(ls, rot, logit, 1.0, gc, go)):
        assert torch.equal(got, want)
