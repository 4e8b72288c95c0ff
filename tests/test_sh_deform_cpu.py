"""CPU: one SH rotation per Gaussian (rotate_shs_per_gaussian_torch, the torch form of nm_sh_rotate_polar's formula) in fp64 -
against the single-rotation form when all rotations are equal, and against the identity that defines it,
sum_j c'_j Y_j(R d) = sum_j c_j Y_j(d).  Both bounds are fp64 round-off of sums of at most 7 terms of magnitude around 1."""
import pytest
import torch

from svd_cases import _haar


def _coeffs(K, deg, seed):
    return torch.randn(K, (deg + 1) ** 2 - 1, 3, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize("deg", [1, 2, 3])
def test_equal_rotations_give_the_single_rotation_form(deg):
    from neuma_amd.render.transform_utils import rotate_shs_per_gaussian_torch, rotate_shs_torch
    K = 50
    c = _coeffs(K, deg, 10 + deg)
    R = _haar(1, torch.Generator().manual_seed(20 + deg))[0]
    out = rotate_shs_per_gaussian_torch(c, R.expand(K, 3, 3).contiguous())
    ref = rotate_shs_torch(c, R)
    assert out.shape == c.shape and out.dtype == torch.float64
    assert float((out - ref).abs().max()) <= 1e-13


@pytest.mark.parametrize("deg", [1, 2, 3])
def test_defining_identity_holds_for_haar_rotations(deg):
    from neuma_amd.render.transform_utils import rotate_shs_per_gaussian_torch, sh_band
    g = torch.Generator().manual_seed(30 + deg)
    K = 100
    R = _haar(K, g)
    c = _coeffs(K, deg, 40 + deg)
    d = torch.randn(32, 3, generator=g, dtype=torch.float64)
    d = d / d.norm(dim=1, keepdim=True)
    out = rotate_shs_per_gaussian_torch(c, R)
    Rd = torch.einsum("gab,mb->gma", R, d)                             # (K, 32, 3)
    worst, lo = 0.0, 0
    for l in range(1, deg + 1):
        n = 2 * l + 1
        moved = torch.einsum("gmj,gjc->gmc", sh_band(l, Rd), out[:, lo:lo + n])
        rest = torch.einsum("mj,gjc->gmc", sh_band(l, d), c[:, lo:lo + n])
        worst = max(worst, float((moved - rest).abs().max()))
        lo += n
    assert worst <= 1e-12


def test_shapes_and_refusals():
    from neuma_amd import NeumaHipError
    from neuma_amd.render.transform_utils import rotate_shs_by_deformation, rotate_shs_per_gaussian_torch
    one = torch.randn(4, 1, 3)
    assert rotate_shs_per_gaussian_torch(one, torch.eye(3).expand(4, 3, 3)) is one
    with pytest.raises(ValueError):
        rotate_shs_per_gaussian_torch(torch.randn(4, 5, 3), torch.eye(3).expand(4, 3, 3))
    F = torch.eye(3).expand(4, 3, 3).contiguous()
    assert rotate_shs_by_deformation(one, F) is one
    with pytest.raises(NeumaHipError):                                   # GPU operator: no CPU path
        rotate_shs_by_deformation(torch.randn(4, 16, 3), F)
    with pytest.raises(RuntimeError, match="dependence on F is not propagated"):
        rotate_shs_by_deformation(torch.randn(4, 16, 3), F.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="dependence on F is not propagated"):
        rotate_shs_by_deformation(torch.randn(4, 16, 3).requires_grad_(True), F)
