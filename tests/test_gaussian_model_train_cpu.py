"""CPU: the training surface of GaussianModel (optimiser plumbing, densification, opacity reset, PLY round trip) on CPU tensors."""
import math
from types import SimpleNamespace

import torch

from neuma_amd.render.gaussian_model import GaussianModel
from neuma_amd.render.general_utils import build_rotation

NAMES = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
ARGS = SimpleNamespace(percent_dense=0.01, position_lr_init=1.6e-4, position_lr_final=1.6e-6, position_lr_delay_mult=0.01,
                       position_lr_max_steps=30_000, feature_lr=2.5e-3, opacity_lr=0.05, scaling_lr=5e-3, rotation_lr=1e-3)
EXTENT = 2.0          # percent_dense * extent = 0.02: the clone / split divide


def _model(n=12, seed=0):
    g = torch.Generator().manual_seed(seed)
    scales = torch.full((n, 3), 0.005)
    scales[::3] = torch.tensor([0.05, 0.01, 0.03])             # rows 0, 3, 6, 9 are "large"
    m = GaussianModel(1)
    m.set_params(torch.randn(n, 3, generator=g), torch.randn(n, 1, 3, generator=g), torch.randn(n, 3, 3, generator=g),
                 torch.log(scales), torch.randn(n, 4, generator=g), 2.0 * torch.randn(n, 1, generator=g))
    m.spatial_lr_scale = 1.5
    m.training_setup(ARGS)
    for name in NAMES:                                         # one Adam step with hand-set gradients: non-zero state
        getattr(m, name).grad = torch.randn(getattr(m, name).shape, generator=g)
    m.optimizer.step()
    m.optimizer.zero_grad(set_to_none=True)
    m.max_radii2D = torch.arange(n, dtype=torch.float32)
    m.xyz_gradient_accum = torch.rand(n, 1, generator=g)
    m.denom = torch.ones(n, 1)
    return m


def _snapshot(m):
    out = {name: getattr(m, name).detach().clone() for name in NAMES}
    for group in m.optimizer.param_groups:
        st = m.optimizer.state[group["params"][0]]
        out["m_" + group["name"]], out["v_" + group["name"]] = st["exp_avg"].clone(), st["exp_avg_sq"].clone()
    return out


GROUP_OF = {"_xyz": "xyz", "_features_dc": "f_dc", "_features_rest": "f_rest", "_opacity": "opacity", "_scaling": "scaling",
            "_rotation": "rotation"}


def _check_groups_hold_the_attributes(m):
    for group in m.optimizer.param_groups:
        attr = [a for a, g in GROUP_OF.items() if g == group["name"]][0]
        assert group["params"][0] is getattr(m, attr) and getattr(m, attr).requires_grad


def test_prune_points_keeps_exactly_the_unmasked_rows():
    m = _model()
    m.get_covariance()
    before, radii, accum = _snapshot(m), m.max_radii2D.clone(), m.xyz_gradient_accum.clone()
    mask = torch.zeros(12, dtype=torch.bool)
    mask[[1, 4, 11]] = True
    m.prune_points(mask)
    after = _snapshot(m)
    for key in before:
        assert torch.equal(after[key], before[key][~mask]), key
    assert torch.equal(m.max_radii2D, radii[~mask]) and torch.equal(m.xyz_gradient_accum, accum[~mask]) and m.denom.shape == (9, 1)
    assert m._cov_cache == {} and m.get_covariance().shape == (9, 6)
    _check_groups_hold_the_attributes(m)


def test_densify_and_clone_appends_copies_with_zero_state():
    m = _model()
    before = _snapshot(m)
    grads = torch.zeros(12, 1)
    grads[[0, 1, 2, 5]] = 1.0                                 # row 0 is large: not cloned
    m.densify_and_clone(grads, 0.5, EXTENT)
    after = _snapshot(m)
    sel = [1, 2, 5]
    for name in NAMES:
        assert torch.equal(after[name][:12], before[name]) and torch.equal(after[name][12:], before[name][sel]), name
    for key in before:
        if key[:2] in ("m_", "v_"):
            assert torch.equal(after[key][:12], before[key]) and after[key].shape[0] == 15 and float(after[key][12:].abs().max()) == 0
    assert m.xyz_gradient_accum.shape == (15, 1) and float(m.xyz_gradient_accum.abs().max()) == 0 and m.max_radii2D.shape == (15,)
    _check_groups_hold_the_attributes(m)


def test_densify_and_split_replaces_large_rows_by_two_samples():
    m = _model()
    before = _snapshot(m)
    grads = torch.zeros(12, 1)
    grads[[0, 1, 3, 9]] = 1.0                                 # row 1 is small: not split; 0, 3, 9 are
    sel = [0, 3, 9]
    torch.manual_seed(5)
    m.densify_and_split(grads, 0.5, EXTENT, N=2)
    after = _snapshot(m)
    keep = [i for i in range(12) if i not in sel]
    assert after["_xyz"].shape[0] == 12 - 3 + 2 * 3
    for key in before:
        assert torch.equal(after[key][:9], before[key][keep]), key
    for rep in range(2):
        rows = slice(9 + 3 * rep, 12 + 3 * rep)
        assert torch.equal(after["_scaling"][rows], torch.log(torch.exp(before["_scaling"][sel]) / 1.6))
        for name in ("_rotation", "_features_dc", "_features_rest", "_opacity"):
            assert torch.equal(after[name][rows], before[name][sel]), name
        # the new means lie within 3 sigma of the parent along each of its axes (6 standard normal draws at seed 5)
        local = torch.einsum("kji,kj->ki", build_rotation(before["_rotation"][sel]), after["_xyz"][rows] - before["_xyz"][sel])
        assert bool((local.abs() <= 3.0 * torch.exp(before["_scaling"][sel])).all()) and float(local.abs().max()) > 0
        assert float(after["m_xyz"][rows].abs().max()) == 0 and float(after["v_scaling"][rows].abs().max()) == 0
    _check_groups_hold_the_attributes(m)


def test_reset_opacity_caps_at_one_percent_and_zeroes_its_state():
    m = _model()
    before = _snapshot(m)
    m.reset_opacity()
    after = _snapshot(m)
    want = torch.min(torch.sigmoid(before["_opacity"]), torch.full((12, 1), 0.01))
    assert torch.allclose(torch.sigmoid(after["_opacity"]), want, rtol=1e-5, atol=0)
    assert float(after["m_opacity"].abs().max()) == 0 and float(after["v_opacity"].abs().max()) == 0
    for key in before:
        if "opacity" not in key:
            assert torch.equal(after[key], before[key]), key
    _check_groups_hold_the_attributes(m)


def test_update_learning_rate_is_the_log_linear_closed_form():
    m = _model()
    lo, hi = 1.6e-4 * 1.5, 1.6e-6 * 1.5
    for it, want in ((0, lo), (1, math.exp(math.log(lo) * (1 - 1 / 30000) + math.log(hi) / 30000)),
                     (15000, math.sqrt(lo * hi)), (30000, hi)):
        got = m.update_learning_rate(it)
        assert abs(got - want) <= 1e-12 * want, (it, got, want)
        assert [g["lr"] for g in m.optimizer.param_groups if g["name"] == "xyz"] == [got]
    lrs = {g["name"]: g["lr"] for g in m.optimizer.param_groups}
    assert lrs["f_dc"] == 2.5e-3 and lrs["f_rest"] == 2.5e-3 / 20.0 and lrs["opacity"] == 0.05 and lrs["scaling"] == 5e-3
    assert lrs["rotation"] == 1e-3 and m.optimizer.defaults["eps"] == 1e-15


def test_save_ply_round_trip_is_bit_exact(tmp_path):
    from neuma_amd.io import load_gaussians_ply
    m = _model()
    m.save_ply(tmp_path / "kernels.ply")
    back = load_gaussians_ply(tmp_path / "kernels.ply", 1)
    for name in NAMES:
        assert torch.equal(getattr(back, name), getattr(m, name).detach()), name


def test_capture_restore_round_trip():
    m = _model()
    m.active_sh_degree = 0
    m.oneupSHdegree(); m.oneupSHdegree()
    assert m.active_sh_degree == 1
    state, snap = m.capture(), _snapshot(m)
    n = GaussianModel(1)
    n.restore(state, ARGS)
    back = _snapshot(n)
    for key in snap:
        assert torch.equal(back[key], snap[key]), key
    assert n.active_sh_degree == 1 and n.spatial_lr_scale == 1.5 and torch.equal(n.denom, m.denom)
    assert torch.equal(n.max_radii2D, m.max_radii2D) and torch.equal(n.xyz_gradient_accum, m.xyz_gradient_accum)


def test_densification_stats_and_scale_regularisation():
    m = _model()
    m.xyz_gradient_accum.zero_(); m.denom.zero_()
    grad = torch.arange(36, dtype=torch.float32).reshape(12, 3)
    vis = torch.arange(12) % 2 == 0
    m.add_densification_stats(grad, vis)
    want = torch.where(vis[:, None], grad[:, :2].norm(dim=1, keepdim=True), torch.zeros(12, 1))
    assert torch.equal(m.xyz_gradient_accum, want) and torch.equal(m.denom, vis[:, None].float())
    s = torch.exp(m._scaling.detach())
    ratio = s.max(dim=1).values / s.min(dim=1).values                 # ~5 on the four large rows, 1 elsewhere
    want = sum(max(float(r) - 3.0, 0.0) for r in ratio) / 12
    assert want > 0.5 and abs(float(m.get_scale_regularization(3.0).detach()) - want) < 1e-6
