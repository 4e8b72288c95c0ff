"""GPU: LPIPS (csrc/nm_lpips.hip, neuma_amd/lpips.py) - the convolution, the pool and the head each on their own, the whole
chain against the fp64 twin (neuma_amd/extras/lpips.py), the exact properties (bitwise), the refusals, and
`python -m neuma_amd.evaluation --lpips_vgg ... --lpips_heads ...` end to end.  All weights are seeded random ones
(tests/lpips_cases.py); the fp64 values are computed once and shared."""
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpu_util import dev, parity

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
import lpips_cases as lc  # noqa: E402

from neuma_amd.extras import lpips as twin  # noqa: E402

CHAIN_REL_BOUND = 2e-6      # not derived: ~10x what torch's own fp32 chain deviates from fp64 on these cases (1.8e-7 on a CPU)


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


_W = {}


def gpu_weights():
    from neuma_amd.lpips import LpipsWeights
    if "w" not in _W:
        convs, heads = lc.weights()
        _W["w"] = LpipsWeights(convs, heads, dev())
    return _W["w"]


# ------------------------------------------------------------------ 1. the convolution

CONV_SHAPES = [(3, 64, 37, 45), (64, 64, 37, 45), (64, 64, 1, 70), (64, 64, 65, 3), (64, 128, 18, 22), (128, 128, 18, 22),
               (256, 256, 9, 11), (256, 512, 4, 5), (512, 512, 4, 5), (512, 512, 2, 2), (512, 512, 1, 1)]


@pytest.mark.parametrize("cin,cout,h,w", CONV_SHAPES)
def test_convolution_against_fp64(cin, cout, h, w):
    """|y - y64| <= (9 cin + 2) 2^-24 (conv(|x|, |w|) + |b|) per element: the dot-product bound, whatever the summation order; it
    survives the ReLU (|relu(u) - relu(v)| <= |u - v|)."""
    from neuma_amd.lpips import conv3x3_relu, pack_conv_weight
    n = 3
    g = torch.Generator().manual_seed(1000 * cin + 10 * h + w)
    if cin == 3:
        x = (torch.randn(n, cin, h, w, generator=g, dtype=torch.float64) * 1.5).float()
    else:
        x = lc.post_relu_like((n, cin, h, w), g)
    wt = (torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64) * math.sqrt(2.0 / (9 * cin))).float()
    b = (torch.randn(cout, generator=g, dtype=torch.float64) * 0.05).float()
    y64 = F.conv2d(x.double(), wt.double(), b.double(), padding=1)
    mag = F.conv2d(x.double().abs(), wt.double().abs(), b.double().abs(), padding=1)
    bound = (9 * cin + 2) * lc.EPS24 * mag
    y = conv3x3_relu(nhwc(x).to(dev()), pack_conv_weight(wt).to(dev()), b.to(dev()))
    assert y.shape == (n, h, w, cout)
    got = y.permute(0, 3, 1, 2).double().cpu()
    assert torch.isfinite(got).all() and (got >= 0).all() and (got > 0).any() and (got == 0).any()
    ratio = float(((got - F.relu(y64)).abs() / bound).max())
    parity(f"lpips conv {cin}->{cout} {h}x{w}", "max abs(y - y64) / ((9 cin + 2) 2^-24 (conv(abs x, abs w) + abs b))", ratio, 1.0)
    # two calls agree, and the second image of the batch alone gives that image's bits
    x_dev, w_dev, b_dev = nhwc(x).to(dev()), pack_conv_weight(wt).to(dev()), b.to(dev())
    assert torch.equal(conv3x3_relu(x_dev, w_dev, b_dev), y)
    assert torch.equal(conv3x3_relu(x_dev[1:2].contiguous(), w_dev, b_dev)[0], y[1])


# ------------------------------------------------------------------ 2. the pool

@pytest.mark.parametrize("h,w", [(37, 45), (18, 22), (9, 11), (5, 4), (3, 3)])
def test_pool_is_bitwise_max_pool2d(h, w):
    from neuma_amd.lpips import maxpool2
    g = torch.Generator().manual_seed(h * 100 + w)
    x = torch.randn(3, 64, h, w, generator=g)
    x[:, ::2] = torch.relu(x[:, ::2])                 # half the channels as the chain has them: ties at 0
    want = F.max_pool2d(x, 2, 2)
    got = maxpool2(nhwc(x).to(dev())).permute(0, 3, 1, 2).cpu()
    assert got.shape == want.shape == (3, 64, h // 2, w // 2)
    assert torch.equal(got, want)


# ------------------------------------------------------------------ 3. the head

@pytest.mark.parametrize("h,w", [(37, 45), (2, 2)])
@pytest.mark.parametrize("c", [64, 128, 256, 512])
def test_head_against_fp64(c, h, w):
    """per pair (2 C + 16) 2^-24 mean_p sum_c w_c (|a^_c| + |b^_c|)^2: the relative error of norm and quotient plus an fp32
    channel sum (the kernel's fp64 sums only do better)"""
    from neuma_amd.lpips import head
    n = 3
    g = torch.Generator().manual_seed(c + h)
    ta, tb = lc.post_relu_like((n, c, h, w), g), lc.post_relu_like((n, c, h, w), g)
    ta[0, :, 0, 0] = 0                               # one vector all zero
    tb[1, :, h - 1, w - 1] = 0
    ta[2, :, 1, 1] = 0                               # both
    tb[2, :, 1, 1] = 0
    hw = torch.rand(c, generator=g)
    want = twin.head(ta, tb, hw)
    a, b = ta.double(), tb.double()
    an = a.abs() / torch.sqrt(1e-8 + (a * a).sum(1, keepdim=True))
    bn = b.abs() / torch.sqrt(1e-8 + (b * b).sum(1, keepdim=True))
    bound = (2 * c + 16) * lc.EPS24 * ((an + bn) ** 2 * hw.double().view(1, -1, 1, 1)).sum(1).mean(dim=(1, 2))
    got = head(nhwc(ta).to(dev()), nhwc(tb).to(dev()), hw.to(dev()))
    assert got.dtype == torch.float64 and got.shape == (n,)
    ratio = float(((got.cpu() - want).abs() / bound).max())
    parity(f"lpips head C={c} {h}x{w}", "max abs(d - d64) / ((2 C + 16) 2^-24 mean sum w (abs a^ + abs b^)^2)", ratio, 1.0)
    assert torch.equal(head(nhwc(tb).to(dev()), nhwc(ta).to(dev()), hw.to(dev())), got)       # symmetric, bitwise


# ------------------------------------------------------------------ 4. the chain

@pytest.mark.parametrize("h,w", lc.CHAIN_SHAPES)
def test_chain_against_the_fp64_twin(h, w):
    from neuma_amd.lpips import features, head, lpips
    a, b = lc.images(h, w)
    want = lc.twin_value(h, w)
    W = gpu_weights()
    got = lpips(a.to(dev()), b.to(dev()), W)
    assert got.dtype == torch.float64 and got.shape == (2,) and got.is_cuda
    rel = float(((got.cpu() - want).abs() / want).max())
    parity(f"lpips chain {h}x{w}", "max abs(lpips - lpips64) / lpips64", rel, CHAIN_REL_BOUND)
    # the same chain layer by layer: features() and head()
    fa, fb = features(a.to(dev()), W), features(b.to(dev()), W)
    assert [tuple(t.shape[1:]) for t in fa] == [(c, h >> i, w >> i) for i, c in enumerate(twin.TAP_CHANNELS)]
    by_layer = sum(head(nhwc(ta), nhwc(tb), hw) for ta, tb, hw in zip(fa, fb, W.heads_dev))
    rel = float(((by_layer.cpu() - want).abs() / want).max())
    parity(f"lpips chain by layer {h}x{w}", "max abs(sum of heads(features) - lpips64) / lpips64", rel, CHAIN_REL_BOUND)


# ------------------------------------------------------------------ 5. exact properties

def test_exact_properties():
    from neuma_amd import _lib as L
    from neuma_amd.lpips import lpips
    W = gpu_weights()
    a3, b3 = (t.to(dev()) for t in lc.images(37, 45, 3))
    v = lpips(a3, b3, W)
    assert torch.equal(lpips(a3, b3, W), v)                                   # two calls
    assert torch.equal(lpips(b3, a3, W), v)                                   # symmetric
    assert torch.equal(lpips(a3, a3, W), torch.zeros(3, dtype=torch.float64, device=dev()))
    for i in range(3):                                                        # slot and stride indexing
        assert torch.equal(lpips(a3[i:i + 1], b3[i:i + 1], W), v[i:i + 1]), i
    assert torch.equal(lpips(a3, b3, W, workspace_budget=1), v)               # one pair per chunk
    one = int(L.lib().nm_lpips_workspace(1, 37, 45))
    assert torch.equal(lpips(a3, b3, W, workspace_budget=2 * one + one // 2), v)      # chunks of 2 and 1
    assert float(v.min()) > 0.1


# ------------------------------------------------------------------ 6. refusals

def test_refusals():
    from neuma_amd import NeumaHipError, _lib as L
    from neuma_amd.lpips import lpips
    W = gpu_weights()
    a, b = lc.images(16, 16)
    with pytest.raises(NeumaHipError, match="at least 16"):
        lpips(a[:, :, :15].contiguous().to(dev()), b[:, :, :15].contiguous().to(dev()), W)
    with pytest.raises(NeumaHipError, match="at least 16"):
        lpips(a[:, :, :, :15].contiguous().to(dev()), b[:, :, :, :15].contiguous().to(dev()), W)
    with pytest.raises(NeumaHipError):
        lpips(a, b, W)
    with pytest.raises(NeumaHipError):
        lpips(a.to(dev()), b, W)
    lib = L.lib()
    assert lib.nm_lpips_workspace(2, 15, 16) == 0 and lib.nm_lpips_workspace(0, 16, 16) == 0
    need = int(lib.nm_lpips_workspace(2, 16, 16))
    assert need >= 2 * (2 * 2 * 16 * 16 * 64 * 4)
    x, y = a.to(dev()), b.to(dev())
    out = torch.full((2,), -1.0, dtype=torch.float64, device=dev())
    ws = torch.empty(need, dtype=torch.uint8, device=dev())
    s = L.stream_ptr(dev())
    rc = lib.nm_lpips(2, 16, 16, L.ptr(x), L.ptr(y), W._wptr, W._hptr, out.data_ptr(), L.ptr(ws), need - 256, s)
    assert rc == -1 and b"workspace too small" in lib.nm_last_error()
    rc = lib.nm_lpips(2, 16, 16, L.ptr(x), None, W._wptr, W._hptr, out.data_ptr(), L.ptr(ws), need, s)
    assert rc == -1 and b"null pointer" in lib.nm_last_error()
    hws = torch.empty(4096, dtype=torch.uint8, device=dev())
    t = torch.zeros(2, 4, 4, 64, device=dev())
    rc = lib.nm_lpips_head(2, 64, 4, 4, L.ptr(t), L.ptr(t), L.ptr(W.heads_dev[0]), out.data_ptr(), L.ptr(hws), 8, s)
    assert rc == -1 and b"workspace too small" in lib.nm_last_error()
    rc = lib.nm_conv3x3_relu(1, 24, 64, 4, 4, L.ptr(t), L.ptr(t), L.ptr(t), L.ptr(t), s)
    assert rc == -1 and b"cin" in lib.nm_last_error()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.full((2,), -1.0, dtype=torch.float64))         # refused before any device work


# ------------------------------------------------------------------ 7. the entry point

E2E_SIZE = 400          # crops [220:400]^2 = 180 x 180


def e2e_frames():
    """frames 0..1 in the construction of test_gpu_image_metrics.py's end-to-end test (RGBA ground truth of a disc with a
    translucent rim, predictions = the composited disc plus noise), the second prediction saved as RGBA"""
    import test_gpu_image_metrics as T0
    preds, gts = T0._e2e_frames(n=2, size=E2E_SIZE, seed=5)
    rng = np.random.default_rng(11)
    preds[1] = np.concatenate([preds[1], rng.integers(0, 256, (E2E_SIZE, E2E_SIZE, 1), dtype=np.uint8)], -1)
    return preds, gts


def e2e_expected(preds, gts):
    """mean over the two frames of the fp64 twin's lpips(gt, pred) on the crops the entry point scores"""
    import image_metrics_ref as R
    convs, heads = lc.weights()
    pc = np.stack([R.to_tensor(R.crop(p[..., :3])) for p in preds])
    gc = np.stack([R.to_tensor(R.crop(R.composite_on_white(g))) for g in gts])
    v = twin.lpips(torch.from_numpy(gc).float(), torch.from_numpy(pc).float(), convs, heads)
    return float(v.mean()), v


def test_entry_point_with_lpips(tmp_path):
    from PIL import Image
    preds, gts = e2e_frames()
    pred_dir, gt_dir = tmp_path / "renders" / "images_test", tmp_path / "gt"
    pred_dir.mkdir(parents=True)
    gt_dir.mkdir()
    for i, (p, g) in enumerate(zip(preds, gts)):
        Image.fromarray(p, "RGBA" if p.shape[-1] == 4 else "RGB").save(pred_dir / f"e_0_{i:03d}.png")
        Image.fromarray(g, "RGBA").save(gt_dir / f"e_0_{i:03d}.png")
    vgg, hd = lc.state_dicts()
    torch.save(vgg, tmp_path / "vgg16.pth")
    torch.save(hd, tmp_path / "heads.pth")
    mean, per_frame = e2e_expected(preds, gts)
    # the frames keep the mean clear of a %.4f rounding boundary by ten times the chain bound
    frac = mean * 1e4 - math.floor(mean * 1e4)
    assert abs(frac - 0.5) > 10 * CHAIN_REL_BOUND * mean * 1e4, (mean, frac)
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    cmd = [sys.executable, "-m", "neuma_amd.evaluation", "-p", str(pred_dir), "-g", str(gt_dir), "--view", "0", "-n", "1"]
    r = subprocess.run(cmd + ["--lpips_vgg", str(tmp_path / "vgg16.pth"), "--lpips_heads", str(tmp_path / "heads.pth")],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "LPIPS is not computed" not in r.stdout
    assert any("vgg16.pth" in ln and "heads.pth" in ln and "LPIPS" in ln for ln in r.stdout.splitlines()), r.stdout
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("pr: ")]
    assert len(lines) == 2, r.stdout
    for ln, v in zip(lines, per_frame.tolist()):
        assert ln.endswith(f" | LPIPS: {v:.2f}") and "(180, 180, 3)" in ln and " | SSIM: " in ln, (ln, v)
    text = (tmp_path / "renders" / "images_test_metrics.txt").read_text().splitlines()
    assert len(text) == 3 and text[0].startswith("PSNR: ") and text[1].startswith("SSIM: "), text
    assert text[2] == f"LPIPS: {mean:.4f}", (text, mean)
    # one flag alone fails and names the other
    r = subprocess.run(cmd + ["--lpips_vgg", str(tmp_path / "vgg16.pth")], cwd=str(tmp_path), env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode != 0 and "without --lpips_heads" in r.stderr, r.stderr
    r = subprocess.run(cmd + ["--lpips_heads", str(tmp_path / "heads.pth")], cwd=str(tmp_path), env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode != 0 and "without --lpips_vgg" in r.stderr, r.stderr
