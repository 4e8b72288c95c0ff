"""A torch stand-in for the subset of `pytorch3d.transforms` that the reference's se3_utils.py imports.  GENERATOR-SIDE TEST
INFRASTRUCTURE, like warp_scalar.py: it lets `tests/golden/gen_regist_golden.py` import the reference's transform_utils.py
(which imports se3_utils, which imports pytorch3d) without pytorch3d being installed.  pytorch3d's source is not part of the
reference tree, so these functions are written from pytorch3d's published documentation and conventions:

  * quaternions are (w, x, y, z); quaternion_to_matrix accepts non-unit quaternions (two_s = 2 / |q|^2);
  * matrix_to_quaternion builds the four candidates q_by_rijk / (2 max(|q_i|, 0.1)), keeps the one of the largest |q_i| and
    returns it standardised (non-negative real part);
  * rotation_6d_to_matrix: Gram-Schmidt on the two 3-vectors, which become the ROWS; matrix_to_rotation_6d: the first two rows;
  * euler_angles_to_matrix(e, "XYZ") = R_X(e0) R_Y(e1) R_Z(e2); matrix_to_euler_angles inverts it (Tait-Bryan XYZ only).

The product restates the same conventions in neuma_amd/regist.py; tests/test_regist_cpu.py holds the two against each other and
against hand-computed values.  Parity with pytorch3d itself is unpinned (no source, no package on the build machine).
The axis-angle entry points are imported by se3_utils.py but never reached by registration: they raise."""
import torch
import torch.nn.functional as F


def quaternion_to_matrix(q):
    r, i, j, k = torch.unbind(q, -1)
    two_s = 2.0 / (q * q).sum(-1)
    o = torch.stack((1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                     two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                     two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)), -1)
    return o.reshape(q.shape[:-1] + (3, 3))


def _sqrt_positive_part(x):
    ret = torch.zeros_like(x)
    pos = x > 0
    ret[pos] = torch.sqrt(x[pos])
    return ret


def standardize_quaternion(q):
    return torch.where(q[..., 0:1] < 0, -q, q)


def matrix_to_quaternion(matrix):
    batch = matrix.shape[:-2]
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = torch.unbind(matrix.reshape(batch + (9,)), -1)
    q_abs = _sqrt_positive_part(torch.stack([1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22,
                                             1.0 - m00 + m11 - m22, 1.0 - m00 - m11 + m22], -1))
    quat_by_rijk = torch.stack([
        torch.stack([q_abs[..., 0] ** 2, m21 - m12, m02 - m20, m10 - m01], -1),
        torch.stack([m21 - m12, q_abs[..., 1] ** 2, m10 + m01, m02 + m20], -1),
        torch.stack([m02 - m20, m10 + m01, q_abs[..., 2] ** 2, m12 + m21], -1),
        torch.stack([m10 - m01, m20 + m02, m21 + m12, q_abs[..., 3] ** 2], -1)], -2)
    flr = torch.tensor(0.1).to(dtype=q_abs.dtype, device=q_abs.device)
    quat_candidates = quat_by_rijk / (2.0 * q_abs[..., None].max(flr))
    out = quat_candidates[F.one_hot(q_abs.argmax(dim=-1), num_classes=4) > 0.5, :].reshape(batch + (4,))
    return standardize_quaternion(out)


def _axis_angle_rotation(axis, angle):
    cos, sin = torch.cos(angle), torch.sin(angle)
    one, zero = torch.ones_like(angle), torch.zeros_like(angle)
    if axis == "X":
        flat = (one, zero, zero, zero, cos, -sin, zero, sin, cos)
    elif axis == "Y":
        flat = (cos, zero, sin, zero, one, zero, -sin, zero, cos)
    else:
        flat = (cos, -sin, zero, sin, cos, zero, zero, zero, one)
    return torch.stack(flat, -1).reshape(angle.shape + (3, 3))


def euler_angles_to_matrix(euler_angles, convention):
    matrices = [_axis_angle_rotation(c, e) for c, e in zip(convention, torch.unbind(euler_angles, -1))]
    return torch.matmul(torch.matmul(matrices[0], matrices[1]), matrices[2])


def matrix_to_euler_angles(matrix, convention):
    if convention != "XYZ":
        raise NotImplementedError(convention)
    return torch.stack((torch.atan2(-matrix[..., 1, 2], matrix[..., 2, 2]), torch.asin(matrix[..., 0, 2]),
                        torch.atan2(-matrix[..., 0, 1], matrix[..., 0, 0])), -1)


def rotation_6d_to_matrix(d6):
    a1, a2 = d6[..., :3], d6[..., 3:]
    b1 = F.normalize(a1, dim=-1)
    b2 = a2 - (b1 * a2).sum(-1, keepdim=True) * b1
    b2 = F.normalize(b2, dim=-1)
    b3 = torch.cross(b1, b2, dim=-1)
    return torch.stack((b1, b2, b3), dim=-2)


def matrix_to_rotation_6d(matrix):
    batch_dim = matrix.size()[:-2]
    return matrix[..., :2, :].clone().reshape(batch_dim + (6,))


def _unused(*_a, **_k):
    raise NotImplementedError("axis-angle conversions are not part of the stand-in")


axis_angle_to_matrix = axis_angle_to_quaternion = quaternion_to_axis_angle = _unused


def install(modules):
    import types
    pkg = types.ModuleType("pytorch3d")
    tr = types.ModuleType("pytorch3d.transforms")
    for name, val in list(globals().items()):
        if callable(val) and not name.startswith("install"):
            setattr(tr, name, val)
    pkg.transforms = tr
    modules["pytorch3d"] = pkg
    modules["pytorch3d.transforms"] = tr
