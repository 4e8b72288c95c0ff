"""fp64 numpy restatement of what experiments/evaluation.py computes (test helper, not a test module):

* torchmetrics 1.x `structural_similarity_index_measure` with its defaults (functional/image/ssim.py `_ssim_update` /
  `_ssim_compute`): gaussian window int(3.5 sigma + 0.5) * 2 + 1 = 11 taps, sigma 1.5, as an outer product (121 taps);
  data_range = max(preds.max() - preds.min(), target.max() - target.min()) over the call's batch; c1 = (0.01 dr)^2,
  c2 = (0.03 dr)^2; reflect pad 5 -> 2-D convolution without padding of x, y, x^2, y^2, xy -> sigma^2 clamped at 0 (sigma_xy
  not) -> the map cropped by 5 on each side -> mean per image -> mean over the batch;
* torchmetrics `PeakSignalNoiseRatio(data_range=1.0)`: 10 log10(dr^2 / mse) over all values of the call;
* the ground-truth compositing of evaluation.py:56-59 with its truncation to uint8, the crop and ToTensor.

The moments are computed once per image pair (`moments`), so one pair can be scored with several data ranges."""
import numpy as np

SIGMA = 1.5
KSIZE = int(3.5 * SIGMA + 0.5) * 2 + 1        # 11
PAD = (KSIZE - 1) // 2                        # 5


def gaussian_1d(kernel_size: int = KSIZE, sigma: float = SIGMA) -> np.ndarray:
    """torchmetrics _gaussian in fp64"""
    dist = np.arange((1 - kernel_size) / 2, (1 + kernel_size) / 2, 1.0)
    gauss = np.exp(-((dist / sigma) ** 2) / 2)
    return gauss / gauss.sum()


def gaussian_2d() -> np.ndarray:
    """torchmetrics _gaussian_kernel_2d: matmul(g_x^T, g_y), (11, 11)"""
    g = gaussian_1d()[None, :]
    return g.T @ g


def reflect_pad(x: np.ndarray, p: int = PAD) -> np.ndarray:
    """F.pad(x, (p, p, p, p), mode="reflect") of (..., H, W) (the edge pixel is not repeated, as numpy's "reflect")"""
    return np.pad(x, [(0, 0)] * (x.ndim - 2) + [(p, p), (p, p)], mode="reflect")


def conv2d_valid(x: np.ndarray, k: np.ndarray) -> np.ndarray:
    """F.conv2d(x, k, groups=C) without padding: out[..., i, j] = sum_{u,v} k[u, v] x[..., i + u, j + v]"""
    kh, kw = k.shape
    h, w = x.shape[-2] - kh + 1, x.shape[-1] - kw + 1
    out = np.zeros(x.shape[:-2] + (h, w))
    for u in range(kh):
        for v in range(kw):
            out += k[u, v] * x[..., u:u + h, v:v + w]
    return out


def conv2d_valid_separable(x: np.ndarray) -> np.ndarray:
    """conv2d_valid with gaussian_2d() as its two 11-tap factors (rows, then columns): the same sums within fp64 rounding at a
    fifth of the cost (the GPU tests score full-size batches with it; the CPU tests hold it to the 121-tap form)"""
    g = gaussian_1d()
    h, w = x.shape[-2] - KSIZE + 1, x.shape[-1] - KSIZE + 1
    r = np.zeros(x.shape[:-1] + (w,))
    for v in range(KSIZE):
        r += g[v] * x[..., :, v:v + w]
    out = np.zeros(x.shape[:-2] + (h, w))
    for u in range(KSIZE):
        out += g[u] * r[..., u:u + h, :]
    return out


def moments(preds: np.ndarray, target: np.ndarray, padded: bool = True, separable: bool = False):
    """The five filtered moments (mu_p, mu_t, E[p^2], E[t^2], E[pt]) of (..., H, W) images over the windows that lie inside
    the image, (..., H-10, W-10) each.  padded=True: torchmetrics' sequence (reflect pad 5, convolve, crop 5);
    padded=False: the valid windows directly."""
    p = np.asarray(preds, dtype=np.float64)
    t = np.asarray(target, dtype=np.float64)
    k = gaussian_2d()
    if padded:
        p, t = reflect_pad(p), reflect_pad(t)
    conv = conv2d_valid_separable if separable else (lambda a: conv2d_valid(a, k))
    out = [conv(a) for a in (p, t, p * p, t * t, p * t)]
    if padded:
        out = [o[..., PAD:-PAD, PAD:-PAD] for o in out]
    return out


def data_range(preds: np.ndarray, target: np.ndarray) -> float:
    p = np.asarray(preds, dtype=np.float64)
    t = np.asarray(target, dtype=np.float64)
    return max(p.max() - p.min(), t.max() - t.min())


def ssim_map(mom, dr: float) -> np.ndarray:
    mu_p, mu_t, e_pp, e_tt, e_pt = mom
    c1 = (0.01 * dr) ** 2
    c2 = (0.03 * dr) ** 2
    mu_p_sq, mu_t_sq, mu_pt = mu_p ** 2, mu_t ** 2, mu_p * mu_t
    sigma_p_sq = np.maximum(e_pp - mu_p_sq, 0.0)
    sigma_t_sq = np.maximum(e_tt - mu_t_sq, 0.0)
    sigma_pt = e_pt - mu_pt
    upper = 2 * sigma_pt + c2
    lower = sigma_p_sq + sigma_t_sq + c2
    with np.errstate(invalid="ignore", divide="ignore"):
        return ((2 * mu_pt + c1) * upper) / ((mu_p_sq + mu_t_sq + c1) * lower)


def ssim_per_image(mom, dr: float) -> np.ndarray:
    """(B,) mean over each image's (C, H-10, W-10) map"""
    m = ssim_map(mom, dr)
    return m.reshape(m.shape[0], -1).mean(-1)


def structural_similarity_index_measure(preds: np.ndarray, target: np.ndarray) -> float:
    """torchmetrics' functional SSIM of a (B, C, H, W) batch: batch-wide range, mean over the batch"""
    return float(ssim_per_image(moments(preds, target), data_range(preds, target)).mean())


def sse(preds: np.ndarray, target: np.ndarray) -> np.ndarray:
    """(B,) sum of squared errors per image"""
    d = np.asarray(preds, dtype=np.float64) - np.asarray(target, dtype=np.float64)
    return (d * d).reshape(d.shape[0], -1).sum(-1)


def psnr_from_sse(s, n: int, dr: float = 1.0):
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(dr ** 2 / (np.asarray(s, dtype=np.float64) / n))


def peak_signal_noise_ratio(preds: np.ndarray, target: np.ndarray, dr: float = 1.0) -> float:
    """torchmetrics' PSNR of one call: the squared errors of the whole batch, then one value"""
    return float(psnr_from_sse(sse(preds, target).sum(), np.asarray(preds).size, dr))


def composite_on_white(rgba: np.ndarray) -> np.ndarray:
    """evaluation.py:56-59 on (H, W, 4) uint8: the float64 blend on white; `np.array(arr*255.0, dtype=np.byte)` then read as
    uint8 by the Pillow the reference ran on = arr*255 truncated toward zero."""
    n = rgba / 255.0
    arr = n[..., :3] * n[..., 3:4] + 1 * (1 - n[..., 3:4])
    return np.floor(arr * 255.0).astype(np.uint8)


def crop(img: np.ndarray) -> np.ndarray:
    return img[220:580, 220:580, :]


def to_tensor(img_u8: np.ndarray) -> np.ndarray:
    """transforms.ToTensor of an (H, W, 3) uint8 array: (3, H, W) float32 = uint8 / 255"""
    return (img_u8.astype(np.float32) / np.float32(255)).transpose(2, 0, 1).copy()
