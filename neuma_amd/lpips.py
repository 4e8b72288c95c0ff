"""LPIPS on the GPU: torchmetrics' `LearnedPerceptualImagePatchSimilarity(net_type='vgg', normalize=True)`, the third number of
experiments/evaluation.py, through the HIP entry point `nm_lpips` (csrc/nm_lpips.hip): VGG-16's 13 convolutions as an exact-fp32
implicit GEMM on the f32 MFMA, four max-pools and the five heads, with no host synchronisation.  The definition is stated in
`neuma_amd/extras/lpips.py` (torch fp64: the CPU path and the yardstick).

No weights are shipped or fetched.  `load_weights` reads the two public files users of the reference already have:
  * torchvision's VGG-16 state dict (`torchvision.models.vgg16(weights="IMAGENET1K_V1").state_dict()` saved with torch.save, or
    the downloaded `vgg16-397923af.pth`): keys features.{0,2,5,...,28}.{weight,bias};
  * the LPIPS heads `vgg.pth` bundled with torchmetrics (functional/image/lpips_models/vgg.pth) and with the lpips package
    (lpips/weights/v0.1/vgg.pth): keys lin{0..4}.model.1.weight of shape (1, C, 1, 1).

GPU tensors only: a CPU tensor raises NeumaHipError (there is no eager fall-back)."""
import ctypes as C

import torch

from . import _lib as L
from .extras import lpips as twin

WORKSPACE_BUDGET = 1 << 30      # bytes of scratch one nm_lpips call may take; larger batches go in chunks


def pack_conv_weight(w: torch.Tensor) -> torch.Tensor:
    """torch's (Cout, Cin, 3, 3) -> nm_conv3x3_relu's layout: (Cout, 9, 3) for Cin = 3, else (Cin/16, Cout, 9, 16)."""
    co, ci = int(w.shape[0]), int(w.shape[1])
    if ci == 3:
        return w.permute(0, 2, 3, 1).reshape(co, 9, 3).contiguous()
    if ci % 16 or co % 64:
        raise ValueError(f"conv weight of shape {tuple(w.shape)}: Cin must be 3 or a multiple of 16, Cout a multiple of 64")
    return w.reshape(co, ci // 16, 16, 9).permute(1, 0, 3, 2).contiguous()


class LpipsWeights:
    """The 13 convolutions and 5 heads: `convs` / `heads` in torch's layout on the CPU (what extras/lpips.py takes), and packed
    once on `device` for the kernels.  `files`: the (vgg16, heads) paths load_weights read them from, else None."""

    files = None

    def __init__(self, convs, heads, device):
        device = torch.device(device)
        if len(convs) != len(twin.CONV_CHANNELS) or len(heads) != len(twin.TAP_CHANNELS):
            raise ValueError(f"expected {len(twin.CONV_CHANNELS)} convolutions and {len(twin.TAP_CHANNELS)} heads, "
                             f"got {len(convs)} and {len(heads)}")
        for i, ((w, b), (ci, co)) in enumerate(zip(convs, twin.CONV_CHANNELS)):
            if tuple(w.shape) != (co, ci, 3, 3) or tuple(b.shape) != (co,):
                raise ValueError(f"convolution {i}: expected weight {(co, ci, 3, 3)} and bias {(co,)}, got {tuple(w.shape)} and "
                                 f"{tuple(b.shape)}")
        for i, (h, c) in enumerate(zip(heads, twin.TAP_CHANNELS)):
            if tuple(h.shape) != (c,):
                raise ValueError(f"head {i}: expected shape {(c,)}, got {tuple(h.shape)}")
        self.device = device
        self.convs = [(w.detach().float().cpu().contiguous(), b.detach().float().cpu().contiguous()) for w, b in convs]
        self.heads = [h.detach().float().cpu().contiguous() for h in heads]
        self.packed = None
        if device.type == "cuda":
            self.packed = [(pack_conv_weight(w).to(device), b.to(device)) for w, b in self.convs]
            self.heads_dev = [h.to(device) for h in self.heads]
            flat = [t for wb in self.packed for t in wb]
            self._wptr = (C.c_void_p * len(flat))(*[L.ptr(t, torch.float32) for t in flat])
            self._hptr = (C.c_void_p * len(self.heads_dev))(*[L.ptr(t, torch.float32) for t in self.heads_dev])

    def require_device(self, device):
        if self.packed is None:
            raise L.NeumaHipError("these LPIPS weights were loaded for the CPU: the native path needs them on the GPU")
        if torch.device(device) != self.device and not (self.device.index is None and torch.device(device).type == "cuda"):
            raise L.NeumaHipError(f"operands on different devices: weights on {self.device}, images on {device}")


def _state_dict(path):
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(sd, dict) and isinstance(sd.get("state_dict"), dict):
        sd = sd["state_dict"]
    if not isinstance(sd, dict):
        raise ValueError(f"{path}: expected a state dict, got {type(sd).__name__}")
    return sd


def _take(sd, key, shape, path):
    if key not in sd:
        raise KeyError(f"{path}: key '{key}' is missing")
    t = sd[key]
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape):
        got = tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{path}: key '{key}' has shape {got}, expected {tuple(shape)}")
    return t


def load_weights(vgg16_path, heads_path, device="cuda") -> LpipsWeights:
    """Read torchvision's VGG-16 state dict (classifier.* ignored; a dict nested under 'state_dict' accepted) and the LPIPS
    heads file; every shape is checked and an error names the offending key."""
    vgg = _state_dict(vgg16_path)
    convs = []
    for idx, (ci, co) in zip(twin.VGG_FEATURE_INDEX, twin.CONV_CHANNELS):
        convs.append((_take(vgg, f"features.{idx}.weight", (co, ci, 3, 3), vgg16_path),
                      _take(vgg, f"features.{idx}.bias", (co,), vgg16_path)))
    hd = _state_dict(heads_path)
    heads = []
    for i, c in enumerate(twin.TAP_CHANNELS):
        key = f"lin{i}.model.1.weight"
        if key not in hd and f"lin{i}.model.0.weight" in hd:
            key = f"lin{i}.model.0.weight"
        heads.append(_take(hd, key, (1, c, 1, 1), heads_path).reshape(c))
    weights = LpipsWeights(convs, heads, device)
    weights.files = (str(vgg16_path), str(heads_path))
    return weights


def _check_images(x, what):
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{what} must be a tensor")
    if not x.is_cuda:
        raise L.NeumaHipError("LPIPS needs tensors on the GPU (no CPU path here; neuma_amd.extras.lpips is the CPU one)")
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"expected (B, 3, H, W) images, got shape {tuple(x.shape)}")
    if not x.is_floating_point():
        raise TypeError(f"{what} must be a floating point image")


def lpips(a, b, weights: LpipsWeights, workspace_budget: int = WORKSPACE_BUDGET) -> torch.Tensor:
    """float64[B] on the device: LPIPS of the pairs (a[i], b[i]), images (B, 3, H, W) in [0, 1] with H, W >= 16.  One nm_lpips call
    per chunk of pairs whose scratch fits `workspace_budget` bytes (at least one pair per call); a pair's value does not depend on
    its chunk or slot."""
    _check_images(a, "a")
    _check_images(b, "b")
    if a.shape != b.shape:
        raise ValueError(f"a and b must have the same shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    L.same_device(a, b)
    weights.require_device(a.device)
    lib = L.lib()
    x = a.detach().float().contiguous()
    y = b.detach().float().contiguous()
    n, _, h, w = (int(s) for s in x.shape)
    out = torch.empty(n, dtype=torch.float64, device=x.device)
    if n == 0:
        return out
    one = int(lib.nm_lpips_workspace(1, h, w))      # 0: sizes the library refuses; the call below says why
    chunk = n if one == 0 else max(1, min(n, int(workspace_budget) // one))
    ws = torch.empty(max(int(lib.nm_lpips_workspace(chunk, h, w)), 1), dtype=torch.uint8, device=x.device)
    for i in range(0, n, chunk):
        k = min(chunk, n - i)
        L.check(lib.nm_lpips(k, h, w, L.ptr(x[i:i + k]), L.ptr(y[i:i + k]), weights._wptr, weights._hptr,
                             out[i:i + k].data_ptr(), L.ptr(ws), ws.numel(), L.stream_ptr(x.device)), "nm_lpips")
    return out


def conv3x3_relu(x_nhwc, w_packed, bias):
    """relu(conv3x3(x) + bias) of a channels-last (N, H, W, Cin) fp32 tensor with a weight from pack_conv_weight: (N, H, W, Cout)."""
    n, h, w, ci = (int(s) for s in x_nhwc.shape)
    co = int(bias.shape[0])
    y = torch.empty(n, h, w, co, dtype=torch.float32, device=x_nhwc.device)
    L.check(L.lib().nm_conv3x3_relu(n, ci, co, h, w, L.ptr(x_nhwc, torch.float32), L.ptr(w_packed, torch.float32),
                                    L.ptr(bias, torch.float32), L.ptr(y), L.stream_ptr(x_nhwc.device)), "nm_conv3x3_relu")
    return y


def maxpool2(x_nhwc):
    """2x2 / stride 2 / floor max-pool of a channels-last (N, H, W, C) fp32 tensor"""
    n, h, w, c = (int(s) for s in x_nhwc.shape)
    y = torch.empty(n, h // 2, w // 2, c, dtype=torch.float32, device=x_nhwc.device)
    L.check(L.lib().nm_maxpool2(n, c, h, w, L.ptr(x_nhwc, torch.float32), L.ptr(y), L.stream_ptr(x_nhwc.device)), "nm_maxpool2")
    return y


def head(tap_a_nhwc, tap_b_nhwc, head_w) -> torch.Tensor:
    """float64[B]: the pixel mean of sum_c w_c (a^_c - b^_c)^2 of two channels-last (B, H, W, C) fp32 taps"""
    L.same_device(tap_a_nhwc, tap_b_nhwc, head_w)
    if tap_a_nhwc.shape != tap_b_nhwc.shape:
        raise ValueError("the two taps must have the same shape")
    n, h, w, c = (int(s) for s in tap_a_nhwc.shape)
    lib = L.lib()
    out = torch.empty(n, dtype=torch.float64, device=tap_a_nhwc.device)
    ws = torch.empty(max(int(lib.nm_lpips_head_workspace(n, h, w)), 1), dtype=torch.uint8, device=out.device)
    L.check(lib.nm_lpips_head(n, c, h, w, L.ptr(tap_a_nhwc, torch.float32), L.ptr(tap_b_nhwc, torch.float32),
                              L.ptr(head_w, torch.float32), out.data_ptr(), L.ptr(ws), ws.numel(), L.stream_ptr(out.device)),
            "nm_lpips_head")
    return out


def features(x, weights: LpipsWeights):
    """The five taps (relu1_2 .. relu5_3) of x (B, 3, H, W) in [0, 1] as (B, C, h, w) fp32 views of channels-last storage, layer
    by layer through nm_conv3x3_relu / nm_maxpool2."""
    _check_images(x, "x")
    weights.require_device(x.device)
    if min(x.shape[2:]) < twin.MIN_SIDE:
        raise ValueError(f"H and W must be at least {twin.MIN_SIDE}, got {tuple(x.shape[2:])}")
    t = twin.scale_input(x.detach().float()).permute(0, 2, 3, 1).contiguous()
    taps = []
    for i, (wp, b) in enumerate(weights.packed):
        t = conv3x3_relu(t, wp, b)
        if i in twin.TAP_AFTER:
            taps.append(t.permute(0, 3, 1, 2))
        if i in twin.POOL_AFTER:
            t = maxpool2(t)
    return taps
