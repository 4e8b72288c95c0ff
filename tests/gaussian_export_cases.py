"""Inputs, fp64 definition, row filter and the existing-code yardstick for nm_gaussian_deform.  A plain helper module shared by
tests/test_gaussian_export_cpu.py (numpy fp64 path, host half of the kernel body) and tests/test_gpu_gaussian_export.py (the kernel).

Inputs: the rows of svd_cases.families() as F; log-scales uniform in [log 1e-3, log 1e-1] per axis, drawn independently (anisotropy
up to 100); raw quaternions random with norm in [0.5, 2].  Everything is rounded to fp32 once and the fp64 definition
Sigma' = F L L^T F^T (extras.gaussian_export.deformed_covariance) works on the rounded values.

Row filter, from the fp64 definition alone: rows whose max|Sigma'| lies in [1e-30, 1e30] (representable in fp32 with room to
square) are compared; at least 90 % of a family must survive.  Two families do not, by their definition, and are DROPPED from the
comparison (not from the checks every row must pass: finite outputs, unit quaternion, r >= 0):
    zero        F = 0: Sigma' = 0 on every row
    scaled_out  F scaled by 2^-100 .. 2^-40 and 2^34 .. 2^60: Sigma' is below 1e-30 on half of the rows and above 1e30 on a sixth
"""
import math
from collections import OrderedDict

import numpy as np
import torch

import svd_cases as sc
from neuma_amd.extras import gaussian_export as ge
from neuma_amd.render.general_utils import build_rotation

DROPPED = ("zero", "scaled_out")
KEEP_LO, KEEP_HI, KEEP_SHARE = 1e-30, 1e30, 0.9
FLOOR = 2e-6                     # of max|Sigma'|: the fp32 ulp of a log-scale near -10 is about 1e-6, the file format imposes it
MARGIN = 4.0                     # over the yardstick: the quaternion round trip and the normalisation, a few roundings of O(1) values


def inputs(seed=0):
    """name -> (F (n,3,3), log_scales (n,3), rot (n,4)) float32 CPU tensors, in the order of svd_cases.families()"""
    fams = sc.families(seed)
    g = torch.Generator().manual_seed(1000 + seed)
    out = OrderedDict()
    for name, F in fams.items():
        n = F.shape[0]
        ls = math.log(1e-3) + (math.log(1e-1) - math.log(1e-3)) * torch.rand(n, 3, generator=g, dtype=torch.float64)
        q = torch.randn(n, 4, generator=g, dtype=torch.float64)
        q = q / q.norm(dim=1, keepdim=True) * (0.5 + 1.5 * torch.rand(n, 1, generator=g, dtype=torch.float64))
        out[name] = (F, ls.float().contiguous(), q.float().contiguous())
    return out


def sigma64(F, ls, rot, mod=1.0):
    """the definition in fp64 from the fp32-rounded inputs: (n,3,3) numpy"""
    return ge.deformed_covariance(ls.double().numpy(), rot.double().numpy(), None if F is None else F.double().numpy(), mod)


def kept(S64):
    m = np.abs(S64).max(axis=(1, 2))
    return (m >= KEEP_LO) & (m <= KEEP_HI)


def activated64(ls_out, rot_out):
    """the covariance raw parameters stand for (modifier 1), in fp64: (n,3,3) numpy"""
    return ge.covariance(np.asarray(ls_out, dtype=np.float64), np.asarray(rot_out, dtype=np.float64))


def full_from_cov6(c6):
    c = np.asarray(c6, dtype=np.float64)
    return np.stack([np.stack([c[:, 0], c[:, 1], c[:, 2]], -1), np.stack([c[:, 1], c[:, 3], c[:, 4]], -1),
                     np.stack([c[:, 2], c[:, 4], c[:, 5]], -1)], 1)


def family_error(S_got, S64, keep):
    """the largest over kept rows of max|S_got - S64| / max|S64|; inf if a kept row is not finite"""
    got, ref = np.asarray(S_got, dtype=np.float64)[keep], S64[keep]
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - ref).max(axis=(1, 2)) / np.abs(ref).max(axis=(1, 2))).max())


def yardstick_cov(F, ls, rot, svd, mod=1.0):
    """The same computation by code older than the kernel, in torch fp32 on the device of the inputs: M = F @ L, svd(M) -> (U, s, Vh)
    (nm_svd3_fwd on the GPU, oracle.material.svd3 on the CPU), log|s|, exp, square, U diag(.) U^T.  (n,3,3) fp32.  The log / exp round
    trip belongs here: the file stores log-scales."""
    Lm = build_rotation(rot) * (mod * torch.exp(ls))[:, None, :]
    M = (F @ Lm).contiguous()
    U, s, _ = svd(M)
    e = torch.exp(torch.log(s.abs()))
    return U @ torch.diag_embed(e * e) @ U.transpose(1, 2)
