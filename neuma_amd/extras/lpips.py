"""LPIPS (VGG-16, normalize=True) in torch fp64: the definition `neuma_amd.lpips` computes natively, stated once more with
`F.conv2d` / `F.max_pool2d`.  It is the CPU path and the yardstick of tests/test_gpu_lpips.py.

Written from knowledge of torchmetrics' LearnedPerceptualImagePatchSimilarity(net_type='vgg', normalize=True); neither
torchmetrics, torchvision nor lpips was available to run against.  For a, b (B, 3, H, W) in [0, 1], H, W >= 16:
  1. x = (2 x - 1 - shift) / scale per channel;
  2. VGG-16's feature stack: 3x3 convolutions, zero padding 1, bias, ReLU, channel plan PLAN ('P' = 2x2 max-pool, stride 2, floor);
  3. taps after the ReLU of convolutions 2, 4, 7, 10, 13 (relu1_2 .. relu5_3);
  4. per tap and pixel t^ = t / sqrt(1e-8 + sum_c t^2), d = sum_c w_c (a^_c - b^_c)^2, then the mean of d over the tap's pixels;
  5. the value of a pair is the sum of the five means."""
import math

import torch
import torch.nn.functional as F

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
PLAN = ((3, 64), (64, 64), "P", (64, 128), (128, 128), "P", (128, 256), (256, 256), (256, 256), "P",
        (256, 512), (512, 512), (512, 512), "P", (512, 512), (512, 512), (512, 512))
CONV_CHANNELS = tuple(p for p in PLAN if p != "P")                    # (cin, cout) of the 13 convolutions
TAP_AFTER = (1, 3, 6, 9, 12)                                           # convolution index (0-based) each tap follows
POOL_AFTER = (1, 3, 6, 9)
TAP_CHANNELS = tuple(CONV_CHANNELS[i][1] for i in TAP_AFTER)           # (64, 128, 256, 512, 512)
VGG_FEATURE_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)   # torchvision's vgg16().features positions
MIN_SIDE = 16
EPS = 1e-8


def random_weights(seed: int = 7, generator=None):
    """(convs, heads) with He-scaled normal weights: per convolution in order w = randn(co, ci, 3, 3, fp64) sqrt(2 / (9 ci)) and
    b = 0.05 randn(co), both cast to fp32; then the five heads rand(C).  Stands in for the public weights where none are at hand
    (tests, tools/exp_lpips.py): the taps come out about half zeros and every tap contributes.  A `generator` is drawn from
    as it stands (and left advanced) instead of a fresh one seeded with `seed`."""
    g = generator if generator is not None else torch.Generator().manual_seed(seed)
    convs = []
    for ci, co in CONV_CHANNELS:
        w = torch.randn(co, ci, 3, 3, dtype=torch.float64, generator=g) * math.sqrt(2.0 / (9 * ci))
        b = torch.randn(co, dtype=torch.float64, generator=g) * 0.05
        convs.append((w.float(), b.float()))
    heads = [torch.rand(c, dtype=torch.float64, generator=g).float() for c in TAP_CHANNELS]
    return convs, heads


def scale_input(x: torch.Tensor) -> torch.Tensor:
    shift = torch.tensor(SHIFT, dtype=x.dtype, device=x.device).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=x.dtype, device=x.device).view(1, 3, 1, 1)
    return (2.0 * x - 1.0 - shift) / scale


def conv3x3_relu(x, w, b):
    return F.relu(F.conv2d(x, w.to(x.dtype), b.to(x.dtype), padding=1))


def maxpool2(x):
    return F.max_pool2d(x, 2, 2)


def features(x: torch.Tensor, convs, dtype=torch.float64):
    """The five taps of x (N, 3, H, W) in [0, 1], in `dtype`."""
    if x.dim() != 4 or x.shape[1] != 3 or min(x.shape[2:]) < MIN_SIDE:
        raise ValueError(f"expected (B, 3, H, W) images with H, W >= {MIN_SIDE}, got shape {tuple(x.shape)}")
    t = scale_input(x.to(dtype))
    taps = []
    for i, (w, b) in enumerate(convs):
        t = conv3x3_relu(t, w, b)
        if i in TAP_AFTER:
            taps.append(t)
        if i in POOL_AFTER:
            t = maxpool2(t)
    return taps


def head(tap_a: torch.Tensor, tap_b: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """(B,) fp64: the pixel mean of sum_c w_c (a^_c - b^_c)^2 for taps (B, C, h, w)."""
    a, b = tap_a.double(), tap_b.double()
    an = a / torch.sqrt(EPS + (a * a).sum(1, keepdim=True))
    bn = b / torch.sqrt(EPS + (b * b).sum(1, keepdim=True))
    d = ((an - bn) ** 2 * w.double().view(1, -1, 1, 1)).sum(1)
    return d.mean(dim=(1, 2))


def lpips_terms(a, b, convs, heads, dtype=torch.float64) -> torch.Tensor:
    """(5, B) fp64: each tap's contribution"""
    fa, fb = features(a, convs, dtype), features(b, convs, dtype)
    return torch.stack([head(ta, tb, w) for ta, tb, w in zip(fa, fb, heads)])


def lpips(a, b, convs, heads, dtype=torch.float64) -> torch.Tensor:
    """(B,) fp64 LPIPS of the pairs (a[i], b[i]); `dtype` is the trunk's arithmetic (the heads are always fp64)."""
    if a.shape != b.shape:
        raise ValueError(f"a and b must have the same shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    return lpips_terms(a, b, convs, heads, dtype).sum(0)
