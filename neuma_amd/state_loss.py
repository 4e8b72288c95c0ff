"""Loss on particle state: position + velocity of one simulated frame against a recorded one, l1 or l2, optional row mask.

    state_loss(x, v, x_gt, v_gt=None, mask=None, kind="l2", weight_x=1.0, weight_v=1.0) -> scalar tensor

runs nm_state_loss (csrc/nm_state.hip): the loss and both gradients in one pass, differences and sums in fp64, fixed-order
reduction (two calls give the same bits).  There is no CPU path: a CPU tensor raises NeumaHipError.

    state_loss_torch(...)  the same loss composed from torch ops (F.l1_loss / F.mse_loss over the kept rows): the yardstick of
                           the tests, and what a test on a CPU tensor calls.

The reference has no counterpart: it ships its base models, not their training (see pretrain.py)."""
from typing import Optional

import torch
import torch.autograd as autograd
import torch.nn.functional as Fn
from torch import Tensor

from . import _lib as L

KINDS = {"l1": 0, "l2": 1}
# launch geometry of k_state_loss (csrc/nm_state.hip): at most MAX_WORKGROUPS workgroups of 256 threads, 4 floats per thread and
# iteration - above ROWS_PER_SWEEP rows the grid-stride loop runs more than once
MAX_WORKGROUPS, THREADS, FLOATS_PER_THREAD = 512, 256, 4
ROWS_PER_SWEEP = MAX_WORKGROUPS * THREADS * FLOATS_PER_THREAD // 3


def _kind(kind: str) -> int:
    if kind not in KINDS:
        raise ValueError(f"state loss kind must be one of {sorted(KINDS)}, not {kind!r}")
    return KINDS[kind]


def _rows(t: Tensor) -> Tensor:
    """fp32, row-contiguous, detached; a view whose rows are already dense is passed on as it is (no copy)"""
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()


def _mask_u8(mask: Optional[Tensor], n: int) -> Optional[Tensor]:
    if mask is None:
        return None
    if mask.numel() != n:
        raise ValueError(f"mask has {mask.numel()} entries for {n} rows")
    m = mask.detach().reshape(n)
    return (m if m.dtype == torch.uint8 else (m != 0).to(torch.uint8)).contiguous()


def state_loss_raw(x, v, x_gt, v_gt=None, mask=None, kind="l2", weight_x=1.0, weight_v=1.0, loss_out=None, terms_out=None,
                   dL_dx=None, dL_dv=None):
    """One nm_state_loss call on fp32 device tensors as they are (no autograd, no copies): *loss_out += the weighted loss,
    terms_out / dL_dx / dL_dv written when given.  Returns loss_out (a fresh zeroed word if None)."""
    dev = L.same_device(x, v, x_gt, v_gt, mask, loss_out, terms_out, dL_dx, dL_dv)
    if not x.is_cuda:
        raise L.NeumaHipError("neuma_amd operators need tensors on the GPU (no CPU path)")
    n = x.shape[0]
    for t in (x, x_gt, v if v_gt is not None else None, v_gt, dL_dx, dL_dv):
        if t is not None and tuple(t.shape) != (n, 3):
            raise ValueError(f"state loss operands must all be ({n}, 3); got {tuple(t.shape)}")
    if loss_out is None:
        loss_out = torch.zeros((), dtype=torch.float32, device=dev)
    lib = L.lib()
    nbytes = int(lib.nm_state_loss_workspace(n))
    ws = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=dev)
    f32 = torch.float32
    L.check(lib.nm_state_loss(n, _kind(kind), float(weight_x), float(weight_v), L.ptr(x, f32), L.ptr(v, f32) if v_gt is not None else None,
                              L.ptr(x_gt, f32), L.ptr(v_gt, f32), L.ptr(mask, torch.uint8), L.ptr(loss_out, f32), L.ptr(terms_out, f32),
                              L.ptr(dL_dx, f32), L.ptr(dL_dv, f32), ws.data_ptr(), nbytes, L.stream_ptr(dev)), "nm_state_loss")
    return loss_out


class StateLossFunction(autograd.Function):
    """(x, v) -> loss through nm_state_loss; the gradients come out of the forward launch and are scaled in backward."""

    @staticmethod
    def forward(ctx, x: Tensor, v: Optional[Tensor], x_gt: Tensor, v_gt: Optional[Tensor], mask: Optional[Tensor], kind: str,
                weight_x: float, weight_v: float):
        n = x.shape[0]
        xc, xg = _rows(x), _rows(x_gt)
        vc, vg = (_rows(v), _rows(v_gt)) if v_gt is not None else (None, None)
        need_x = ctx.needs_input_grad[0]
        need_v = v is not None and ctx.needs_input_grad[1]
        gx = torch.empty_like(xc) if need_x else None
        gv = torch.empty(n, 3, dtype=torch.float32, device=xc.device) if need_v else None
        loss = state_loss_raw(xc, vc, xg, vg, _mask_u8(mask, n), kind, weight_x, weight_v, dL_dx=gx, dL_dv=gv)
        ctx.save_for_backward(gx, gv)
        return loss

    @staticmethod
    def backward(ctx, gout: Tensor):
        gx, gv = ctx.saved_tensors
        return (gx * gout if gx is not None else None, gv * gout if gv is not None else None, None, None, None, None, None, None)


def state_loss(x: Tensor, v: Optional[Tensor], x_gt: Tensor, v_gt: Optional[Tensor] = None, mask: Optional[Tensor] = None,
               kind: str = "l2", weight_x: float = 1.0, weight_v: float = 1.0) -> Tensor:
    """weight_x * loss(x[mask], x_gt[mask]) + weight_v * loss(v[mask], v_gt[mask]) on the GPU (mean over the kept rows' 3 m
    components; 0 when the mask keeps nothing).  v_gt=None: positions only."""
    _kind(kind)
    if not (x.is_cuda and x_gt.is_cuda):
        raise L.NeumaHipError("state_loss needs tensors on the GPU (no CPU path); state_loss_torch is the torch composition")
    if v_gt is not None and v is None:
        raise ValueError("v_gt given without v")
    return StateLossFunction.apply(x, v, x_gt, v_gt, mask, kind, float(weight_x), float(weight_v))


def state_loss_torch(x: Tensor, v: Optional[Tensor], x_gt: Tensor, v_gt: Optional[Tensor] = None, mask: Optional[Tensor] = None,
                     kind: str = "l2", weight_x: float = 1.0, weight_v: float = 1.0) -> Tensor:
    """The same loss from torch ops, on any device."""
    _kind(kind)
    fn = Fn.l1_loss if kind == "l1" else Fn.mse_loss
    keep = None if mask is None else (mask.reshape(-1) != 0)

    def term(a, b):
        if keep is not None:
            a, b = a[keep], b[keep]
        if a.numel() == 0:
            return a.sum() * 0.0          # (the mean over nothing is NaN in torch; the loss is defined as 0 there)
        return fn(a, b)

    loss = weight_x * term(x, x_gt)
    if v_gt is not None:
        loss = loss + weight_v * term(v, v_gt)
    return loss
