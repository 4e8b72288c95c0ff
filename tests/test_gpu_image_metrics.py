"""GPU: image-quality metrics of experiments/evaluation.py - nm_image_metrics against the fp64 restatement of torchmetrics'
PSNR / SSIM (tests/image_metrics_ref.py) on random and structured batches, both data-range modes, bitwise reproducibility, the
torchmetrics-style functions, the edge cases, argument errors, and `python -m neuma_amd.evaluation` end to end on frames in the
reference's naming."""
import functools
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from gpu_util import dev, measured

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
import image_metrics_ref as R  # noqa: E402

SHAPES = {"360": (3, 360, 360), "800": (3, 800, 800), "11": (3, 11, 11), "257x361": (3, 257, 361)}
B = 11


def _structured(shape, b, rng):
    """a smooth coloured pattern with a flat white border region (as a render on a white background), quantised to k / 255;
    the target is the pattern shifted by a pixel plus noise, with the same white region"""
    c, h, w = shape
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    ch = np.arange(c)[:, None, None]
    pat = 0.5 + 0.35 * np.sin((5 + b) * xx + 2.0 * ch) * np.cos(4 * yy - ch) + 0.1 * np.sin(40 * xx * yy)
    r = np.hypot(yy - 0.5, xx - 0.5)
    white = r > 0.42
    p = np.where(white, 1.0, pat)
    t = np.where(white, 1.0, np.roll(pat, 1, axis=-1) + 0.03 * rng.standard_normal(shape))
    q = lambda a: (np.round(np.clip(a, 0, 1) * 255) / 255).astype(np.float32)
    return q(p), q(t)


@functools.lru_cache(maxsize=None)
def _batch(kind, tag):
    """(preds, target, fp64 moments) of a B-image batch; images differ in range so that the two range modes differ"""
    shape = SHAPES[tag]
    rng = np.random.default_rng([7, len(kind), sum(shape)])
    ps, ts = [], []
    for b in range(B):
        if kind == "random":
            base = rng.random(shape)
            p = (0.6 * base + 0.4 * rng.random(shape)).astype(np.float32)
            t = np.clip(base + 0.1 * rng.standard_normal(shape), 0, 1).astype(np.float32)
        else:
            p, t = _structured(shape, b, rng)
        s = np.float32(0.4 + 0.06 * b)
        ps.append(p * s)
        ts.append(t * s)
    p, t = np.stack(ps), np.stack(ts)
    return p, t, R.moments(p, t, padded=False, separable=True)


def _native(p, t, per_image):
    from neuma_amd.image_metrics import _native as nat
    sse, ssim = nat(torch.from_numpy(p).to(dev()), torch.from_numpy(t).to(dev()), per_image)
    return sse.cpu().numpy(), ssim.cpu().numpy()


@pytest.mark.parametrize("kind", ["random", "structured"])
@pytest.mark.parametrize("tag", list(SHAPES))
def test_image_metrics_match_the_fp64_restatement(kind, tag):
    from neuma_amd.image_metrics import image_metrics
    p, t, mom = _batch(kind, tag)
    n = p[0].size
    per_dr = [R.data_range(p[i], t[i]) for i in range(B)]
    ref_own = np.array([R.ssim_per_image([m[i:i + 1] for m in mom], per_dr[i])[0] for i in range(B)])
    ref_batch = R.ssim_per_image(mom, R.data_range(p, t))
    ref_psnr = R.psnr_from_sse(R.sse(p, t), n)
    assert np.abs(ref_own - ref_batch).max() > 1e-4            # the two modes are told apart
    psnr, ssim = image_metrics(torch.from_numpy(p).to(dev()), torch.from_numpy(t).to(dev()), range_per_image=True)
    assert psnr.dtype == torch.float64 and ssim.dtype == torch.float64 and psnr.shape == (B,) and ssim.is_cuda
    assert measured(np.abs(ssim.cpu().numpy() - ref_own).max(), "ssim per image, own range") <= 2e-6
    assert measured(np.abs(psnr.cpu().numpy() - ref_psnr).max(), "psnr dB") <= 1e-5
    sse_b, ssim_b = _native(p, t, False)
    assert measured(np.abs(ssim_b - ref_batch).max(), "ssim per image, batch range") <= 2e-6
    assert measured(np.abs(sse_b - R.sse(p, t)).max() / R.sse(p, t).max(), "sse rel") <= 1e-12
    # B = 1: the first image alone (the two modes coincide)
    psnr1, ssim1 = image_metrics(torch.from_numpy(p[:1]).to(dev()), torch.from_numpy(t[:1]).to(dev()))
    assert measured(abs(float(ssim1[0]) - ref_own[0]), "ssim B=1") <= 2e-6
    assert measured(abs(float(psnr1[0]) - ref_psnr[0]), "psnr B=1 dB") <= 1e-5


def test_two_calls_give_identical_bits():
    p, t, _ = _batch("structured", "360")
    for per_image in (True, False):
        a = _native(p, t, per_image)
        b = _native(p, t, per_image)
        assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64))
        assert np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))


def test_torchmetrics_style_functions_on_a_batch():
    from neuma_amd.image_metrics import peak_signal_noise_ratio, structural_similarity_index_measure
    p, t, mom = _batch("structured", "360")
    pt, tt = torch.from_numpy(p).to(dev()), torch.from_numpy(t).to(dev())
    v = structural_similarity_index_measure(pt, tt)
    assert v.dim() == 0 and v.dtype == torch.float32 and v.is_cuda
    ref = float(R.ssim_per_image(mom, R.data_range(p, t)).mean())
    assert measured(abs(float(v) - ref), "functional ssim, batch") <= 2e-6
    v = peak_signal_noise_ratio(pt, tt, data_range=1.0)
    ref = R.peak_signal_noise_ratio(p, t)            # batch-global mse, not the mean of per-image PSNRs
    assert measured(abs(float(v) - ref), "functional psnr dB") <= 1e-5
    assert abs(ref - float(R.psnr_from_sse(R.sse(p, t), p[0].size).mean())) > 1e-3
    v2 = peak_signal_noise_ratio(pt, tt, data_range=2.0)
    assert measured(abs(float(v2) - R.peak_signal_noise_ratio(p, t, 2.0)), "functional psnr dr=2 dB") <= 1e-5


def test_identical_and_constant_pairs():
    from neuma_amd.image_metrics import image_metrics
    p, _, _ = _batch("random", "257x361")
    x = torch.from_numpy(p[:3]).to(dev())
    psnr, ssim = image_metrics(x, x.clone())
    assert torch.isinf(psnr).all() and (psnr > 0).all()
    assert measured((ssim - 1).abs().max(), "ssim of identical images - 1") <= 1e-9
    z = torch.zeros(2, 3, 32, 40, device=dev())
    psnr, ssim = image_metrics(z, z.clone())
    assert torch.isnan(ssim).all() and torch.isinf(psnr).all()
    # one constant image in a batch: NaN for it alone
    y = x.clone()
    y[1] = 0
    _, ssim = image_metrics(y, y.clone())
    assert torch.isnan(ssim[1]) and torch.isfinite(ssim[[0, 2]]).all()


def test_argument_errors():
    from neuma_amd import _lib as L
    from neuma_amd.image_metrics import image_metrics, structural_similarity_index_measure
    a = torch.rand(2, 3, 10, 40, device=dev())
    with pytest.raises(L.NeumaHipError, match="at least 11"):
        image_metrics(a, a.clone())
    a = torch.rand(2, 3, 40, 10, device=dev())
    with pytest.raises(L.NeumaHipError, match="at least 11"):
        image_metrics(a, a.clone())
    a = torch.rand(2, 3, 20, 20, device=dev())
    with pytest.raises(L.NeumaHipError):
        image_metrics(a.cpu(), a.cpu())
    with pytest.raises(L.NeumaHipError):
        image_metrics(a, a.cpu())
    with pytest.raises(ValueError):
        image_metrics(a, torch.rand(2, 3, 20, 21, device=dev()))
    with pytest.raises(ValueError):
        image_metrics(a[0], a[0].clone())
    with pytest.raises(NotImplementedError):
        structural_similarity_index_measure(a, a, kernel_size=7)
    # the C ABI itself: a short workspace, a null input, b <= 0
    lib = L.lib()
    need = int(lib.nm_image_metrics_workspace(2, 3, 20, 20))
    assert need > 0 and lib.nm_image_metrics_workspace(2, 3, 10, 20) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev())
    out = torch.empty(4, dtype=torch.float64, device=dev())
    s = L.stream_ptr(a.device)
    assert lib.nm_image_metrics(2, 3, 20, 20, a.data_ptr(), a.data_ptr(), 1, out.data_ptr(), out[2:].data_ptr(), ws.data_ptr(),
                                need - 8, s) != 0
    assert b"workspace too small" in lib.nm_last_error()
    assert lib.nm_image_metrics(2, 3, 20, 20, None, a.data_ptr(), 1, out.data_ptr(), out[2:].data_ptr(), ws.data_ptr(), need, s) != 0
    assert lib.nm_image_metrics(0, 3, 20, 20, a.data_ptr(), a.data_ptr(), 1, out.data_ptr(), out[2:].data_ptr(), ws.data_ptr(),
                                need, s) != 0
    assert lib.nm_image_metrics(2, 3, 20, 20, a.data_ptr(), a.data_ptr(), 1, out.data_ptr(), out[2:].data_ptr(), ws.data_ptr(),
                                need, s) == 0


# ------------------------------------------------------------------ the entry point

def _e2e_frames(n=11, size=800, seed=3):
    """n predicted RGB frames (two of them saved as RGBA with a random alpha, which the reader drops) and n ground-truth RGBA
    frames of a disc with a translucent rim on a transparent background; the predictions are the composited disc plus noise"""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(size), np.arange(size), indexing="ij")
    r = np.hypot(yy - size / 2 + 0.5, xx - size / 2 + 0.5)
    alpha = np.clip((170.0 - r) / 40.0, 0, 1)          # opaque inside r = 130, translucent rim to r = 170
    preds, gts = [], []
    for i in range(n):
        ch = np.arange(3)[None, None, :]
        col = 0.5 + 0.4 * np.sin(0.02 * (xx[..., None] + 3 * i) + ch) * np.cos(0.015 * yy[..., None] - ch)
        gt_rgb = np.clip(col * 255, 0, 255).astype(np.uint8)
        gt = np.concatenate([gt_rgb, np.round(alpha * 255).astype(np.uint8)[..., None]], -1)
        a = alpha[..., None]
        shade = np.where(a > 0, a * col + (1 - a) + 0.03 * rng.standard_normal(col.shape) + 0.004 * i, 1.0)
        pred = np.clip(np.round(shade * 255), 0, 255).astype(np.uint8)
        if i in (2, 7):
            pred = np.concatenate([pred, rng.integers(0, 256, (size, size, 1), dtype=np.uint8)], -1)
        preds.append(pred)
        gts.append(gt)
    return preds, gts


def test_entry_point_end_to_end(tmp_path):
    from PIL import Image
    preds, gts = _e2e_frames()
    pred_dir, gt_dir = tmp_path / "renders" / "images_test", tmp_path / "gt"
    pred_dir.mkdir(parents=True)
    gt_dir.mkdir()
    for i, (p, g) in enumerate(zip(preds, gts)):
        Image.fromarray(p, "RGBA" if p.shape[-1] == 4 else "RGB").save(pred_dir / f"e_0_{i:03d}.png")
        Image.fromarray(g, "RGBA").save(gt_dir / f"e_0_{i:03d}.png")
    # expected: the restatement, frame by frame (psnr(gt, pred), ssim(gt, pred), each frame with its own range)
    pc = [R.crop(p[..., :3]) for p in preds]
    gc = [R.crop(R.composite_on_white(g)) for g in gts]
    P = np.stack([R.to_tensor(x) for x in pc])
    G = np.stack([R.to_tensor(x) for x in gc])
    mom = R.moments(G, P, padded=False, separable=True)
    ssim = [R.ssim_per_image([m[i:i + 1] for m in mom], R.data_range(G[i], P[i]))[0] for i in range(len(preds))]
    psnr = R.psnr_from_sse(R.sse(G, P), P[0].size)
    mp, ms = sum(psnr) / len(psnr), sum(ssim) / len(ssim)
    for v in (mp, ms):              # the inputs keep both means away from a %.2f rounding boundary
        assert abs(v * 100 - np.floor(v * 100) - 0.5) > 0.1, v
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    r = subprocess.run([sys.executable, "-m", "neuma_amd.evaluation", "-p", str(pred_dir), "-g", str(gt_dir), "--view", "0"],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "LPIPS is not computed" in r.stdout
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("pr: ")]
    assert len(lines) == 11 and "e_0_010.png" in lines[-1] and "(360, 360, 3)" in lines[0]
    text = (tmp_path / "renders" / "images_test_metrics.txt").read_text()
    assert text == f"PSNR: {mp:.2f}\nSSIM: {ms:.2f}\n", (text, mp, ms)
    for i in range(11):
        pair = np.array(Image.open(tmp_path / "results" / "debug" / f"{i}.png"))
        assert pair.shape == (364, 726, 3)
        assert np.array_equal(pair[2:362, 2:362], pc[i]) and np.array_equal(pair[2:362, 364:724], gc[i])
        assert pair[:2].max() == 0 and pair[:, 362:364].max() == 0
    # a missing frame names its path
    (pred_dir / "e_0_004.png").unlink()
    r = subprocess.run([sys.executable, "-m", "neuma_amd.evaluation", "-p", str(pred_dir), "-g", str(gt_dir), "--view", "0",
                        "-n", "5"], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "e_0_004.png" in r.stderr
