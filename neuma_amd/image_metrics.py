"""Image-quality metrics of experiments/evaluation.py on the GPU: torchmetrics' `PeakSignalNoiseRatio(data_range=1.0)` and
`structural_similarity_index_measure` (defaults), both through one HIP entry point, `nm_image_metrics` (csrc/nm_metrics.hip).

GPU tensors only: a CPU tensor raises NeumaHipError, and arguments other than the ones the reference uses raise
NotImplementedError (there is no eager fall-back).  Inputs are (B, C, H, W) with H, W >= 11, computed on fp32 copies."""
import torch

from . import _lib as L


def _check_pair(preds, target):
    if not (isinstance(preds, torch.Tensor) and isinstance(target, torch.Tensor)):
        raise TypeError("preds and target must be tensors")
    if not (preds.is_cuda and target.is_cuda):
        raise L.NeumaHipError("image metrics need tensors on the GPU (no CPU path)")
    if preds.shape != target.shape:
        raise ValueError(f"preds and target must have the same shape, got {tuple(preds.shape)} and {tuple(target.shape)}")
    if preds.dim() != 4:
        raise ValueError(f"expected (B, C, H, W) images, got shape {tuple(preds.shape)}")
    if not (preds.is_floating_point() and target.is_floating_point()):
        raise TypeError("preds and target must be floating point images")
    L.same_device(preds, target)


def _native(preds, target, range_per_image: bool, want_ssim: bool = True):
    """(sse[B], ssim[B] or None), float64 on the inputs' device: one nm_image_metrics call, no host synchronisation."""
    _check_pair(preds, target)
    lib = L.lib()
    p = preds.detach().float().contiguous()
    t = target.detach().float().contiguous()
    b, c, h, w = (int(s) for s in p.shape)
    sse = torch.empty(b, dtype=torch.float64, device=p.device)
    ssim = torch.empty(b, dtype=torch.float64, device=p.device) if want_ssim else None
    ws = torch.empty(max(int(lib.nm_image_metrics_workspace(b, c, h, w)), 1), dtype=torch.uint8, device=p.device)
    L.check(lib.nm_image_metrics(b, c, h, w, L.ptr(p), L.ptr(t), int(bool(range_per_image)), sse.data_ptr(),
                                 None if ssim is None else ssim.data_ptr(), L.ptr(ws), ws.numel(), L.stream_ptr(p.device)),
            "nm_image_metrics")
    return sse, ssim


def _psnr_from_sse(sse: torch.Tensor, n: int, data_range: float) -> torch.Tensor:
    """10 log10(dr^2 / (sse / n)); sse = 0 gives +inf, as torchmetrics."""
    return 10.0 * torch.log10((float(data_range) ** 2) / (sse / float(n)))


def image_metrics(preds, target, range_per_image: bool = True):
    """(psnr[B], ssim[B]) as float64 device tensors: per image, PeakSignalNoiseRatio(data_range=1.0) and torchmetrics' SSIM.
    range_per_image=True takes each image's data range for SSIM's c1 / c2, i.e. the values of B separate one-frame calls
    (evaluation.py); False takes the batch-wide range, as one batched torchmetrics call does."""
    sse, ssim = _native(preds, target, range_per_image)
    n = int(preds[0].numel())
    return _psnr_from_sse(sse, n, 1.0), ssim


def peak_signal_noise_ratio(preds, target, data_range=1.0, base: float = 10.0, reduction: str = "elementwise_mean",
                            dim=None):
    """torchmetrics.functional.peak_signal_noise_ratio for a float data_range: one PSNR over the whole batch (the squared
    errors of all images summed first)."""
    if isinstance(data_range, (tuple, list)) or base != 10.0 or reduction != "elementwise_mean" or dim is not None:
        raise NotImplementedError("peak_signal_noise_ratio: only a float data_range with base=10, dim=None and the default "
                                  "reduction is provided")
    sse, _ = _native(preds, target, True, want_ssim=False)
    return _psnr_from_sse(sse.sum(), preds.numel(), data_range).to(preds.dtype)


def structural_similarity_index_measure(preds, target, gaussian_kernel: bool = True, sigma=1.5, kernel_size=11,
                                        reduction: str = "elementwise_mean", data_range=None, k1: float = 0.01,
                                        k2: float = 0.03, return_full_image: bool = False,
                                        return_contrast_sensitivity: bool = False):
    """torchmetrics.functional.structural_similarity_index_measure with its defaults: data range over the whole batch, then
    the mean over the batch of each image's mean SSIM."""
    if (not gaussian_kernel or sigma != 1.5 or kernel_size != 11 or reduction != "elementwise_mean" or data_range is not None
            or k1 != 0.01 or k2 != 0.03 or return_full_image or return_contrast_sensitivity):
        raise NotImplementedError("structural_similarity_index_measure: only the defaults (gaussian window 11, sigma 1.5, "
                                  "data_range from the inputs, k1 0.01, k2 0.03, elementwise_mean) are provided")
    _, ssim = _native(preds, target, False)
    return ssim.mean().to(preds.dtype)
