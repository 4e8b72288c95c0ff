"""CPU, fp64: `sh_rotation_matrices` (neuma_amd/render/transform_utils.py) against the oracle's own SH evaluation
(oracle.raster.eval_sh_color).  D = diag(1, D_1, D_2, D_3) must satisfy  colour(D c, R d) = colour(c, d)  for every unit d,
be orthogonal, compose as the rotations do and be the identity at the identity; it must be differentiable in R; and the
table nm_shrot.hip holds must be the one the torch function uses (the same formula on both sides)."""
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle.raster import eval_sh_color

ROOT = Path(__file__).resolve().parent.parent
BOUND = 1e-12          # invariance, orthogonality, composition (fp64; the basis constants are O(1), the blocks at most 7x7)


def _axis_angle(axis, angle):
    a = torch.tensor(axis, dtype=torch.float64)
    a = a / a.norm()
    K = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=torch.float64)
    return torch.eye(3, dtype=torch.float64) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def _random_rotation(gen):
    q = torch.randn(4, generator=gen, dtype=torch.float64)
    from neuma_amd.regist import quat_to_rotmat
    return quat_to_rotmat(q / q.norm())


def _rotations():
    gen = torch.Generator().manual_seed(1234)
    named = [("identity", torch.eye(3, dtype=torch.float64)),
             ("pi about x", _axis_angle([1.0, 0, 0], math.pi)), ("pi about y", _axis_angle([0, 1.0, 0], math.pi)),
             ("pi about z", _axis_angle([0, 0, 1.0], math.pi)), ("1e-6 rad", _axis_angle([0.3, -0.5, 0.8], 1e-6))]
    return named + [(f"random {i}", _random_rotation(gen)) for i in range(24)]


ROTS = _rotations()


def _full(R):
    from neuma_amd.render.transform_utils import sh_rotation_matrices
    D1, D2, D3 = sh_rotation_matrices(R)
    assert D1.shape == (3, 3) and D2.shape == (5, 5) and D3.shape == (7, 7)
    return torch.block_diag(torch.ones(1, 1, dtype=R.dtype), D1, D2, D3)


@pytest.mark.parametrize("name,R", ROTS, ids=[n for n, _ in ROTS])
def test_colour_is_invariant_under_a_joint_rotation(name, R):
    gen = torch.Generator().manual_seed(7)
    K = 400
    c = 0.02 * torch.randn(K, 16, 3, generator=gen, dtype=torch.float64)      # |sum| << 0.5: the clamp at 0 never engages
    d = torch.randn(K, 3, generator=gen, dtype=torch.float64)
    d = d / d.norm(dim=1, keepdim=True)
    D = _full(R)
    zero = torch.zeros(3, dtype=torch.float64)
    for deg in (1, 2, 3):
        m = (deg + 1) ** 2
        ref, clamped = eval_sh_color(deg, c[:, :m], d, zero)
        got, _ = eval_sh_color(deg, torch.einsum("ij,kjc->kic", D[:m, :m], c[:, :m]), d @ R.T, zero)
        assert not clamped.any()
        err = float((got - ref).abs().max())
        print(f"{name} deg {deg}: invariance {err:.2e}")
        assert err <= BOUND


@pytest.mark.parametrize("name,R", ROTS, ids=[n for n, _ in ROTS])
def test_blocks_are_orthogonal(name, R):
    D = _full(R)
    err = float((D @ D.T - torch.eye(16, dtype=torch.float64)).abs().max())
    print(f"{name}: |D D^T - I| {err:.2e}")
    assert err <= BOUND


def test_blocks_compose_as_the_rotations_do():
    worst = 0.0
    for (_, R1), (_, R2) in zip(ROTS, ROTS[3:] + ROTS[:3]):
        worst = max(worst, float((_full(R1 @ R2) - _full(R1) @ _full(R2)).abs().max()))
    print(f"|D(R1 R2) - D(R1) D(R2)| {worst:.2e}")
    assert worst <= BOUND


def test_identity_gives_the_identity():
    err = float((_full(torch.eye(3, dtype=torch.float64)) - torch.eye(16, dtype=torch.float64)).abs().max())
    print(f"|D(I) - I| {err:.2e}")
    assert err <= 1e-15


def test_degree_one_block_is_R_in_the_basis_order():
    """Y_1 = C1 (-y, z, -x): D_1 = P R P^T with P the signed permutation (x, y, z) -> (-y, z, -x)."""
    from neuma_amd.render.transform_utils import sh_rotation_matrices
    P = torch.tensor([[0, -1.0, 0], [0, 0, 1.0], [-1.0, 0, 0]], dtype=torch.float64)
    for _, R in ROTS:
        assert float((sh_rotation_matrices(R)[0] - P @ R @ P.T).abs().max()) <= BOUND


def test_gradcheck_in_R():
    from neuma_amd.render.transform_utils import sh_rotation_matrices
    for _, R in ROTS[5:8]:
        assert torch.autograd.gradcheck(lambda r: sh_rotation_matrices(r), (R.clone().requires_grad_(True),), eps=1e-6, atol=1e-8)


def test_torch_rotation_is_differentiable_in_both_arguments():
    from neuma_amd.render.transform_utils import rotate_shs_torch
    gen = torch.Generator().manual_seed(3)
    c = torch.randn(5, 15, 3, generator=gen, dtype=torch.float64, requires_grad=True)
    R = ROTS[6][1].clone().requires_grad_(True)
    assert torch.autograd.gradcheck(rotate_shs_torch, (c, R), eps=1e-6, atol=1e-8)


def test_shape_rules():
    from neuma_amd._lib import NeumaHipError
    from neuma_amd.render.transform_utils import rotate_shs_torch, transform_shs_by_quat, transform_shs_by_rotmat
    R = ROTS[7][1]
    for rows in (3, 8, 15):
        c = torch.randn(6, rows, 3, dtype=torch.float64)
        out = rotate_shs_torch(c, R)
        assert out.shape == c.shape and out is not c
        with pytest.raises(NeumaHipError):                       # the kernel-backed operator has no CPU path
            transform_shs_by_rotmat(c.float(), R.float())
    for fn in (rotate_shs_torch, transform_shs_by_rotmat):
        with pytest.raises(ValueError, match="3, 8 or 15"):
            fn(torch.zeros(6, 5, 3), R.float())
        for rows in (0, 1):
            c = torch.randn(6, rows, 3)
            assert fn(c, R.float()) is c
    q = torch.tensor([1.0, 0.0, 0.0, 0.0])
    c = torch.zeros(4, 1, 3)
    assert transform_shs_by_quat(c, q) is c


def test_rotate_transform_and_quaternion_multiply_follow_regist():
    from neuma_amd import regist
    from neuma_amd.render import transform_utils as tu
    gen = torch.Generator().manual_seed(11)
    pts = torch.randn(9, 3, generator=gen, dtype=torch.float64)
    q = torch.nn.functional.normalize(torch.randn(9, 4, generator=gen, dtype=torch.float64), dim=-1)
    R = ROTS[9][1]
    p2, q2 = tu.rotate_transform(pts, q, R)
    assert torch.equal(p2, pts @ R.T)
    assert torch.equal(tu.quaternion_multiply(q, q2), regist.quaternion_multiply(q, q2))
    # the composed orientation is R times the old one
    M = regist.quat_to_rotmat(q2)
    assert float((M - R[None] @ regist.quat_to_rotmat(q)).abs().max()) <= 1e-12


def test_the_device_table_is_the_torch_functions_table():
    """nm_shrot.hip carries the directions and A_l^{-1} as literals; tools/gen_shrot_tables.py prints them from
    `sh_rotation_tables`.  The block in the source must be that output, value for value."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_shrot_tables", ROOT / "tools" / "gen_shrot_tables.py")
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    src = (ROOT / "neuma_amd" / "csrc" / "nm_shrot.hip").read_text()
    m = re.search(r"// BEGIN generated tables.*?\n(.*?)// END generated tables", src, re.S)
    assert m, "generated table block not found in nm_shrot.hip"
    assert m.group(1).strip() == gen.tables().strip()
    from neuma_amd.render.transform_utils import sh_band, sh_rotation_tables
    dirs, ainv = sh_rotation_tables()
    for l in (1, 2, 3):
        A = sh_band(l, dirs[:2 * l + 1]).T
        assert np.abs(A @ ainv[l - 1] - np.eye(2 * l + 1)).max() <= 1e-14
        assert np.linalg.cond(A) < 4.0
