"""Shared inputs of the LPIPS tests (tests/test_lpips_cpu.py, tests/test_gpu_lpips.py): seeded random weights in place of the
public VGG-16 / LPIPS files (nothing is downloaded, no weights are committed), image pairs, the fp64 twin's values computed once,
and hand-written numpy loops for the three building blocks."""
import functools

import numpy as np
import torch

from neuma_amd.extras import lpips as twin

SEED = 7
CHAIN_SHAPES = ((16, 16), (37, 45), (33, 70))
EPS24 = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def weights():
    """(convs, heads) of twin.random_weights(7): w = randn sqrt(2 / (9 cin)), b = 0.05 randn, heads rand(C); fp32, torch layout"""
    return twin.random_weights(SEED)


@functools.lru_cache(maxsize=None)
def images(h, w, b=2):
    """(a, b_img) fp32 (b, 3, h, w): a = rand rounded to k / 255, b_img = a + 0.1 randn, clamped and rounded; drawn from the
    weights' generator right after the weights"""
    g = torch.Generator().manual_seed(SEED)
    twin.random_weights(generator=g)
    a = torch.round(torch.rand(b, 3, h, w, generator=g) * 255) / 255
    n = torch.round(torch.clamp(a + 0.1 * torch.randn(b, 3, h, w, generator=g), 0, 1) * 255) / 255
    return a.float().contiguous(), n.float().contiguous()


@functools.lru_cache(maxsize=None)
def twin_terms(h, w, b=2):
    """(5, b) fp64: every tap's contribution for images(h, w, b) with weights(), by the fp64 twin (computed once, shared)"""
    convs, heads = weights()
    a, n = images(h, w, b)
    return twin.lpips_terms(a, n, convs, heads)


def twin_value(h, w, b=2):
    return twin_terms(h, w, b).sum(0)


def state_dicts(convs=None, heads=None):
    """the two files' contents as the public ones are laid out: torchvision's vgg16 state dict (with a classifier entry, which the
    loader must ignore) and the heads' lin{i}.model.1.weight of shape (1, C, 1, 1)"""
    if convs is None:
        convs, heads = weights()
    vgg = {}
    for idx, (w, b) in zip(twin.VGG_FEATURE_INDEX, convs):
        vgg[f"features.{idx}.weight"] = w.clone()
        vgg[f"features.{idx}.bias"] = b.clone()
    vgg["classifier.6.bias"] = torch.zeros(10)
    hd = {f"lin{i}.model.1.weight": h.clone().view(1, -1, 1, 1) for i, h in enumerate(heads)}
    return vgg, hd


def post_relu_like(shape, g):
    """signed normal values with the negative half set to 0 (what a convolution after a ReLU sees), fp32"""
    x = torch.randn(*shape, generator=g, dtype=torch.float64)
    return torch.where(x > 0, x, torch.zeros_like(x)).float()


# ------------------------------------------------------------------ numpy loops

def np_conv3x3_relu(x, w, b):
    """x (cin, h, w), w (cout, cin, 3, 3), b (cout,) -> (cout, h, w); every sum written out, in fp64"""
    x, w, b = np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(b, np.float64)
    cin, hh, ww = x.shape
    out = np.zeros((w.shape[0], hh, ww))
    for o in range(w.shape[0]):
        for y in range(hh):
            for xx in range(ww):
                s = b[o]
                for c in range(cin):
                    for ky in range(3):
                        for kx in range(3):
                            yy, xc = y + ky - 1, xx + kx - 1
                            if 0 <= yy < hh and 0 <= xc < ww:
                                s += w[o, c, ky, kx] * x[c, yy, xc]
                out[o, y, xx] = max(s, 0.0)
    return out


def np_maxpool2(x):
    """x (c, h, w) -> (c, h // 2, w // 2)"""
    x = np.asarray(x)
    c, hh, ww = x.shape
    out = np.zeros((c, hh // 2, ww // 2), x.dtype)
    for k in range(c):
        for y in range(hh // 2):
            for xx in range(ww // 2):
                out[k, y, xx] = max(x[k, 2 * y, 2 * xx], x[k, 2 * y, 2 * xx + 1], x[k, 2 * y + 1, 2 * xx], x[k, 2 * y + 1, 2 * xx + 1])
    return out


def np_head(ta, tb, w):
    """ta, tb (c, h, w), w (c,) -> the pixel mean of sum_c w_c (a^_c - b^_c)^2"""
    ta, tb, w = np.asarray(ta, np.float64), np.asarray(tb, np.float64), np.asarray(w, np.float64)
    c, hh, ww = ta.shape
    tot = 0.0
    for y in range(hh):
        for xx in range(ww):
            na = np.sqrt(1e-8 + sum(ta[k, y, xx] ** 2 for k in range(c)))
            nb = np.sqrt(1e-8 + sum(tb[k, y, xx] ** 2 for k in range(c)))
            tot += sum(w[k] * (ta[k, y, xx] / na - tb[k, y, xx] / nb) ** 2 for k in range(c))
    return tot / (hh * ww)
