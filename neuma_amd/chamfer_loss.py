"""Chamfer loss of the simulated particles against an unordered point cloud: the training loss for observations that are not in
the simulator's particle numbering (a scan per frame, the centres of a reconstruction, another sampling of the same body).

    chamfer_loss(x, y, mask=None, weight_xy=1.0, weight_yx=1.0) -> scalar tensor

        weight_xy * mean over kept rows i of |x_i - nearest y|^2  +  weight_yx * mean over j of |y_j - nearest kept x|^2

runs nm_chamfer_loss (csrc/nm_chamfer_loss.hip): both exact searches of nm_chamfer, the loss and its gradient in x in one call,
differences and sums in fp64, no float atomics (two calls give the same bits - particle_metrics' scatter_add_ composition does
not).  `mask` drops rows of x altogether (a surface scan: interior particles are neither queries nor candidates); weight_xy = 0
leaves "every observed point has a simulated point nearby" (a partial scan).  y gets no gradient; the gradient flows through
the assignments, never through the (piecewise constant) indices.  There is no CPU path: a CPU tensor raises NeumaHipError.
A masked call reads the kept-row count back (one stream synchronisation); an unmasked one synchronises nothing.

    chamfer_loss_torch(...)  the same loss from torch ops on any device (brute-force cdist argmin with the lowest index on ties,
                             gather / index_add_): the CPU path and a yardstick.  O(n m) memory.

The reference has no counterpart (see pretrain.py); extras/chamfer_loss.py states the definition in numpy fp64."""
from typing import Optional

import torch
import torch.autograd as autograd
from torch import Tensor

from . import _lib as L
from .state_loss import _mask_u8, _rows

LONG_ROW = 32       # kClLongRow of csrc/nm_chamfer_loss.hip: a row chosen by more observations is summed by a wave


def _check(x: Tensor, y: Tensor) -> None:
    for name, t in (("x", x), ("y", y)):
        if t.dim() != 2 or t.shape[1] != 3 or t.shape[0] < 1:
            raise ValueError(f"{name} must be (rows >= 1, 3), got {tuple(t.shape)}")


def chamfer_loss_raw(x, y, mask=None, weight_xy=1.0, weight_yx=1.0, loss_out=None, terms_out=None, dL_dx=None, idx_xy=None,
                     idx_yx=None):
    """One nm_chamfer_loss call on fp32 device tensors as they are (no autograd, no copies): *loss_out += the weighted loss;
    terms_out (2), dL_dx (n,3), idx_xy (n) int64 and idx_yx (m) int64 are written when given.  Returns loss_out (a fresh zeroed
    word if None)."""
    dev = L.same_device(x, y, mask, loss_out, terms_out, dL_dx, idx_xy, idx_yx)
    if not (x.is_cuda and y.is_cuda):
        raise L.NeumaHipError("neuma_amd operators need tensors on the GPU (no CPU path)")
    _check(x, y)
    n, m = int(x.shape[0]), int(y.shape[0])
    if dL_dx is not None and tuple(dL_dx.shape) != (n, 3):
        raise ValueError(f"dL_dx must be ({n}, 3); got {tuple(dL_dx.shape)}")
    for name, t, rows in (("idx_xy", idx_xy, n), ("idx_yx", idx_yx, m)):
        if t is not None and (t.dtype != torch.int64 or tuple(t.shape) != (rows,) or not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous int64 tensor of {rows} entries")
    if mask is not None and mask.numel() != n:
        raise ValueError(f"mask has {mask.numel()} entries for {n} rows")
    if loss_out is None:
        loss_out = torch.zeros((), dtype=torch.float32, device=dev)
    lib = L.lib()
    nbytes = int(lib.nm_chamfer_loss_workspace(n, m))
    if nbytes == 0:
        raise ValueError(f"clouds of {n} and {m} points are outside nm_chamfer_loss's range")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    f32 = torch.float32
    L.check(lib.nm_chamfer_loss(n, m, L.ptr(x, f32), L.ptr(y, f32), L.ptr(mask, torch.uint8), float(weight_xy), float(weight_yx),
                                L.ptr(loss_out, f32), L.ptr(terms_out, f32), L.ptr(dL_dx, f32),
                                None if idx_xy is None else idx_xy.data_ptr(), None if idx_yx is None else idx_yx.data_ptr(),
                                L.ptr(ws), nbytes, L.stream_ptr(dev)), "nm_chamfer_loss")
    return loss_out


class ChamferLossFunction(autograd.Function):
    """x -> loss through nm_chamfer_loss; the gradient comes out of the forward launch and is scaled in backward."""

    @staticmethod
    def forward(ctx, x: Tensor, y: Tensor, mask: Optional[Tensor], weight_xy: float, weight_yx: float):
        xc, yc = _rows(x), _rows(y)
        gx = torch.empty_like(xc) if ctx.needs_input_grad[0] else None
        loss = chamfer_loss_raw(xc, yc, _mask_u8(mask, xc.shape[0]), weight_xy, weight_yx, dL_dx=gx)
        ctx.save_for_backward(gx)
        return loss

    @staticmethod
    def backward(ctx, gout: Tensor):
        gx, = ctx.saved_tensors
        return (gx * gout if gx is not None else None, None, None, None, None)


def chamfer_loss(x: Tensor, y: Tensor, mask: Optional[Tensor] = None, weight_xy: float = 1.0, weight_yx: float = 1.0) -> Tensor:
    """The Chamfer loss on the GPU (squared distances; 0 when the mask keeps nothing).  x (n,3) may require gradients, y (m,3)
    gets none."""
    if not (x.is_cuda and y.is_cuda):
        raise L.NeumaHipError("chamfer_loss needs tensors on the GPU (no CPU path); chamfer_loss_torch is the torch composition")
    _check(x, y)
    return ChamferLossFunction.apply(x, y, mask, float(weight_xy), float(weight_yx))


def chamfer_loss_torch(x: Tensor, y: Tensor, mask: Optional[Tensor] = None, weight_xy: float = 1.0, weight_yx: float = 1.0,
                       give_id: bool = False):
    """The same loss from torch ops, on any device and in x's dtype.  give_id: (loss, idx_xy with -1 on dropped rows, idx_yx in
    x's row numbering)."""
    _check(x, y)
    n, m = x.shape[0], y.shape[0]
    y = y.detach().to(x.dtype)
    rows = torch.arange(n, device=x.device) if mask is None else torch.nonzero(mask.reshape(-1) != 0).reshape(-1)
    k = int(rows.numel())
    idx_xy = torch.full((n,), -1, dtype=torch.int64, device=x.device)
    if k == 0:
        loss = x.sum() * 0.0
        return (loss, idx_xy, torch.full((m,), -1, dtype=torch.int64, device=x.device)) if give_id else loss
    xk = x[rows]
    with torch.no_grad():
        d = torch.cdist(xk.detach(), y, compute_mode="donot_use_mm_for_euclid_dist")          # (k, m)
        # lowest index on ties: the first position of the minimum (argmin's choice among equals is not specified)
        first = lambda t, dim: (t == t.amin(dim, keepdim=True)).to(torch.uint8).argmax(dim)       # noqa: E731
        a, b = first(d, 1), first(d, 0)
    term_xy = (xk - y[a]).pow(2).sum() / k
    # the scatter half through index_add_: every kept row collects the observations that chose it
    per_row = torch.zeros(k, dtype=x.dtype, device=x.device).index_add_(0, b, (xk[b] - y).pow(2).sum(1))
    term_yx = per_row.sum() / m
    loss = weight_xy * term_xy + weight_yx * term_yx
    if give_id:
        idx_xy[rows] = a
        return loss, idx_xy, rows[b]
    return loss
