"""Classical (closed-form) constitutive laws on the HIP kernels of csrc/nm_classical.hip.

Mirrors the reference's modules/nclaw/material/preset.py:30-282 - same class names, same constructor (`cfg` with `E`, `nu`,
`random`, `mode`, `sigma_y`, `friction_angle`, `cohesion`), same parameter / buffer names, so a reference `state_dict` loads:

    CorotatedElasticity, StVKElasticity, VolumeElasticity, SigmaElasticity          F -> stress      learnable: log_E
    IdentityPlasticity, SigmaPlasticity                                             F -> F           nothing learnable
    VonMisesPlasticity                                                              F -> F           log_E, sigma_y
    DruckerPragerPlasticity                                                         F -> F           log_E, friction_angle

`nu` and `cohesion` are buffers.  forward(F) is one autograd.Function around nm_classical_fwd / nm_classical_bwd; the law's
scalars travel as a 4-float device tensor {log_E, nu, p2, p3} (no host read on the call path) and the scalar gradients come
back summed in a fixed order (two calls give the same bits).  There is no eager torch path: a CPU tensor raises.

At a row whose deviatoric Hencky strain is exactly zero the forward values are the reference's (finite where the row does not
yield, NaN on the yielding side of Drucker-Prager).  The adjoint selects the gradient of the branch the row took instead of
adding zero times the other branch: a non-yielding von Mises row returns grad_out there, where the reference returns NaN.
Non-finite gradients are passed on unchanged (the simulator's boundary applies nan_to_num_, as for the neural laws).
"""
import torch
import torch.autograd as autograd
import torch.nn as nn
from torch import Tensor

from .. import _lib as L
from .meta import InvariantFullMetaElasticity, InvariantFullMetaPlasticity, _get

LAW_COROTATED, LAW_STVK, LAW_VOLUME, LAW_SIGMA, LAW_IDENTITY, LAW_SIGMA_PLASTIC, LAW_VON_MISES, LAW_DRUCKER_PRAGER = range(8)
VOLUME_MODES = {"ziran": 0, "taichi": 1}


class ClassicalFunction(autograd.Function):
    """(F, scalars[4]) -> out through nm_classical_fwd; backward through nm_classical_bwd (SVD recomputed)."""

    @staticmethod
    def forward(ctx, F: Tensor, scalars: Tensor, law: int, mode: int):
        Fc = F.detach().float().contiguous()
        sc = None if scalars is None else scalars.detach().float().contiguous()
        out = torch.empty_like(Fc)
        L.same_device(Fc, sc)
        L.check(L.lib().nm_classical_fwd(Fc.size(0), law, mode, L.ptr(sc), L.ptr(Fc), L.ptr(out), L.stream_ptr(Fc.device)),
                "nm_classical_fwd")
        ctx.save_for_backward(Fc, sc)
        ctx.law, ctx.mode = law, mode
        return out

    @staticmethod
    def backward(ctx, gout: Tensor):
        Fc, sc = ctx.saved_tensors
        n = Fc.size(0)
        g = gout.float().contiguous()
        gF = torch.empty_like(Fc)
        lib = L.lib()
        if sc is None:
            L.check(lib.nm_classical_bwd(n, ctx.law, ctx.mode, None, L.ptr(Fc), L.ptr(g), L.ptr(gF), None, None, 0,
                                         L.stream_ptr(Fc.device)), "nm_classical_bwd")
            return gF, None, None, None
        nbytes = int(lib.nm_classical_bwd_workspace(n))
        ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=Fc.device)
        g2 = torch.empty(2, dtype=torch.float32, device=Fc.device)
        L.check(lib.nm_classical_bwd(n, ctx.law, ctx.mode, L.ptr(sc), L.ptr(Fc), L.ptr(g), L.ptr(gF), L.ptr(g2), L.ptr(ws), nbytes,
                                     L.stream_ptr(Fc.device)), "nm_classical_bwd")
        gsc = torch.zeros(4, dtype=torch.float32, device=Fc.device)
        gsc[0::2] = g2                                  # {d/d log_E, 0, d/d p2, 0}
        return gF, gsc, None, None


class _Classical(nn.Module):
    LAW = None

    def __init__(self, cfg=None) -> None:
        super().__init__()
        self.dim = 3

    def _elastic_constants(self, cfg) -> None:
        self.log_E = nn.Parameter(torch.Tensor([_get(cfg, "E")]).log())
        self.register_buffer("nu", torch.Tensor([_get(cfg, "nu")]))
        if _get(cfg, "random"):
            self.log_E.data.mul_(0.8)

    def _mode(self) -> int:
        return 0

    def _scalars(self):
        """the law's {log_E, nu, p2, p3} as one device tensor (differentiable in its parameters), or None"""
        zero = self.nu.new_zeros(1)
        return torch.cat([self.log_E, self.nu, zero, zero])

    def forward(self, F: Tensor) -> Tensor:
        if F.size(0) == 0:
            return F.float()
        return ClassicalFunction.apply(F, self._scalars(), self.LAW, self._mode())


class _ClassicalElasticity(_Classical):
    def __init__(self, cfg) -> None:
        super().__init__(cfg)
        self._elastic_constants(cfg)


class CorotatedElasticity(_ClassicalElasticity):
    """preset.py:30-58: 2 mu (F - U Vh) F^T + la J (J - 1) I with J = prod(sigma)."""
    LAW = LAW_COROTATED


class StVKElasticity(_ClassicalElasticity):
    """preset.py:61-94: 2 mu F E + la J (J - 1) I, E = (F^T F - I) / 2, J from the signed singular values."""
    LAW = LAW_STVK


class VolumeElasticity(_ClassicalElasticity):
    """preset.py:97-137: pressure only, J = det F; mode 'ziran' (kappa (J - 1 / J), gamma = 2) or 'taichi' (la J (J - 1))."""
    LAW = LAW_VOLUME

    def __init__(self, cfg) -> None:
        super().__init__(cfg)
        self.mode = _get(cfg, "mode")

    def _mode(self) -> int:
        key = str(self.mode).casefold()
        if key not in VOLUME_MODES:
            raise ValueError('invalid mode for volume plasticity: {}'.format(self.mode))
        return VOLUME_MODES[key]


class SigmaElasticity(_ClassicalElasticity):
    """preset.py:140-166: Hencky, U diag(2 mu log sigma + la tr log sigma) U^T (NaN where det F < 0, as the reference)."""
    LAW = LAW_SIGMA


class IdentityPlasticity(_Classical):
    """preset.py:170-172: returns its input tensor."""
    LAW = LAW_IDENTITY

    def forward(self, F: Tensor) -> Tensor:
        return F


class SigmaPlasticity(_Classical):
    """preset.py:175-187: diag(det(F)^(1/3)) (NaN where det F < 0, as the reference)."""
    LAW = LAW_SIGMA_PLASTIC

    def _scalars(self):
        return None


class VonMisesPlasticity(_Classical):
    """preset.py:190-230: singular values clamped at 0.05, return map where |dev log sigma| > sigma_y / (2 mu), else F."""
    LAW = LAW_VON_MISES

    def __init__(self, cfg) -> None:
        super().__init__(cfg)
        self._elastic_constants(cfg)
        self.sigma_y = nn.Parameter(torch.Tensor([_get(cfg, "sigma_y")]))
        if _get(cfg, "random"):
            self.sigma_y.data.mul_(0.8)

    def _scalars(self):
        return torch.cat([self.log_E, self.nu, self.sigma_y, self.nu.new_zeros(1)])


class DruckerPragerPlasticity(_Classical):
    """preset.py:233-282: singular values clamped at 0.05; projection onto the cone where tr log sigma < 3 cohesion, else
    exp(cohesion) U Vh."""
    LAW = LAW_DRUCKER_PRAGER

    def __init__(self, cfg) -> None:
        super().__init__(cfg)
        self._elastic_constants(cfg)
        self.friction_angle = nn.Parameter(torch.Tensor([_get(cfg, "friction_angle")]))
        self.register_buffer("cohesion", torch.Tensor([_get(cfg, "cohesion")]))
        if _get(cfg, "random"):
            self.friction_angle.data.mul_(0.8)

    def _scalars(self):
        return torch.cat([self.log_E, self.nu, self.friction_angle, self.cohesion])


CLASSICAL = {c.__name__: c for c in (CorotatedElasticity, StVKElasticity, VolumeElasticity, SigmaElasticity, IdentityPlasticity,
                                     SigmaPlasticity, VonMisesPlasticity, DruckerPragerPlasticity)}
NEURAL = {c.__name__: c for c in (InvariantFullMetaElasticity, InvariantFullMetaPlasticity)}


def build(kind_cfg, default=InvariantFullMetaElasticity) -> nn.Module:
    """A constitutive module from one `constitution.elasticity` / `constitution.plasticity` block: its optional `name` key picks
    one of the eight classical laws or the two neural classes; without it the block builds `default` (a neural class), as before
    the key existed."""
    name = _get(kind_cfg, "name")
    if name is None:
        return default(kind_cfg)
    cls = CLASSICAL.get(name) or NEURAL.get(name)
    if cls is None:
        raise ValueError(f"unknown constitutive law {name!r}: expected one of {sorted(CLASSICAL) + sorted(NEURAL)}")
    return cls(kind_cfg)
