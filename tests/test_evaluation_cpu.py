"""CPU: the host side of `python -m neuma_amd.evaluation` (experiments/evaluation.py) - flags, frame indices and names, the
ground-truth compositing with its truncation, the debug-pair layout - and the fp64 restatement of torchmetrics' SSIM that the GPU
tests score against (tests/image_metrics_ref.py): its reflect-pad / convolve / crop sequence equals the mean over the windows
lying inside the image, which is why nm_image_metrics pads nothing.  None of this opens libneuma_hip.so."""
import os
import subprocess
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
import image_metrics_ref as R  # noqa: E402


def test_flags_and_defaults_match_the_reference():
    from neuma_amd.evaluation import parse_args
    a = parse_args(["--view", "0"])
    assert (a.pred_dir, a.gt_dir, a.start, a.skip, a.num, a.device, a.view) == (None, None, 0, 1, 10, "cuda", 0)
    a = parse_args(["-p", "P", "-g", "G", "-s", "3", "-k", "2", "-n", "4", "-d", "cuda:1", "--view", "7"])
    assert (a.pred_dir, a.gt_dir, a.start, a.skip, a.num, a.device, a.view) == ("P", "G", 3, 2, 4, "cuda:1", 7)
    a = parse_args(["--pred_dir", "P", "--gt_dir", "G", "--start", "1", "--skip", "5", "--num", "2", "--device", "cuda",
                    "--view", "2"])
    assert (a.pred_dir, a.gt_dir, a.start, a.skip, a.num, a.view) == ("P", "G", 1, 5, 2, 2)
    with pytest.raises(SystemExit):           # --view is required
        parse_args(["-p", "P", "-g", "G"])


def test_frame_indices():
    from neuma_amd.evaluation import frame_indices
    assert frame_indices(3, 2, 4) == [3, 5, 7, 9, 11]
    assert frame_indices(0, 1, 10) == list(range(11))          # num + 1 frames by default


def test_frame_names_and_the_missing_file_error(tmp_path):
    from neuma_amd.evaluation import frame_paths
    pred, gt = tmp_path / "pred", tmp_path / "gt"
    pred.mkdir()
    gt.mkdir()
    with pytest.raises(FileNotFoundError, match=str(pred / "e_2_007.png")):     # both missing: the prediction is named
        frame_paths(str(pred), str(gt), 2, 7)
    (pred / "e_2_007.png").write_bytes(b"")
    with pytest.raises(FileNotFoundError, match=str(gt / "e_2_007.png")):
        frame_paths(str(pred), str(gt), 2, 7)
    (gt / "e_2_007.png").write_bytes(b"")
    assert frame_paths(str(pred), str(gt), 2, 7) == (str(pred / "e_2_007.png"), str(gt / "e_2_007.png"))
    (pred / "e_0_123.png").write_bytes(b"")
    (gt / "e_0_123.png").write_bytes(b"")
    assert frame_paths(str(pred), str(gt), 0, 123)[0].endswith("e_0_123.png")


def test_metrics_path():
    from neuma_amd.evaluation import metrics_path
    assert metrics_path("out/run/images_a") == os.path.join("out/run/images_a", "..", "images_a_metrics.txt")


def _translucent_pixels():
    """(c, a) pairs whose exact c a / 255 + 255 - a (= arr * 255) has a fractional part in [0.6, 0.9]: truncation and rounding
    differ by one, and fp64 rounding cannot move the integer part"""
    out = []
    for c in range(0, 256, 7):
        for a in range(1, 255, 5):
            v = Fraction(c * a, 255) + 255 - a
            if Fraction(3, 5) <= v - int(v) <= Fraction(9, 10):
                out.append((c, a, int(v)))
    return out


def test_compositing_truncates_translucent_pixels():
    from neuma_amd.evaluation import composite_on_white
    px = _translucent_pixels()
    assert len(px) > 50
    rgba = np.zeros((1, len(px), 4), dtype=np.uint8)
    for j, (c, a, _) in enumerate(px):
        rgba[0, j] = (c, 255 - c, c // 2, a)
    got = composite_on_white(rgba)
    for j, (c, a, trunc) in enumerate(px):
        assert got[0, j, 0] == trunc, (c, a, got[0, j, 0], trunc)           # not round(): trunc + 1
    assert np.array_equal(got, R.composite_on_white(rgba))
    # the three channels are blended independently; fully transparent pixels become white
    rgba[0, :, 3] = 0
    assert (composite_on_white(rgba) == 255).all()


def test_opaque_pixels_round_trip_unchanged():
    from neuma_amd.evaluation import composite_on_white
    v = np.arange(256, dtype=np.uint8)
    rgba = np.stack([v, v[::-1], np.roll(v, 77), np.full(256, 255, np.uint8)], -1)[None]
    assert np.array_equal(composite_on_white(rgba), rgba[..., :3])


def test_crop_and_debug_pair_layout():
    from neuma_amd.evaluation import crop, debug_pair
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (800, 800, 3), dtype=np.uint8)
    c = crop(img)
    assert c.shape == (360, 360, 3) and np.array_equal(c, img[220:580, 220:580])
    p, g = c, crop(rng.integers(0, 256, (800, 800, 3), dtype=np.uint8))
    pair = debug_pair(p, g)
    assert pair.shape == (364, 726, 3) and pair.dtype == np.uint8           # make_grid(nrow=2, padding=2)
    assert np.array_equal(pair[2:362, 2:362], p) and np.array_equal(pair[2:362, 364:724], g)
    mask = np.ones(pair.shape[:2], bool)
    mask[2:362, 2:362] = False
    mask[2:362, 364:724] = False
    assert (pair[mask] == 0).all()


def test_save_image_round_trips_every_byte():
    """ToTensor (uint8 / 255 in fp32) then save_image's mul(255).add_(0.5).clamp_(0, 255).to(uint8): every byte comes back,
    so the debug pairs can be composed from the uint8 crops"""
    import torch
    v = torch.arange(256, dtype=torch.uint8)
    back = v.float().div(255).mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8)
    assert torch.equal(back, v)
    assert np.array_equal(R.to_tensor(np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, -1))[0].ravel(),
                          v.float().div(255).numpy())


def _pair(shape, seed):
    rng = np.random.default_rng(seed)
    base = rng.random(shape)
    p = (0.6 * base + 0.4 * rng.random(shape)).astype(np.float32)
    t = np.clip(base + 0.1 * rng.standard_normal(shape), 0, 1).astype(np.float32)
    t[..., :6, :9] = 1.0                      # a flat corner in both
    p[..., :6, :9] = 1.0
    return p, t


def test_reflect_pad_and_crop_equals_the_valid_windows():
    p, t = _pair((2, 3, 23, 31), 1)
    padded = R.moments(p, t, padded=True)
    valid = R.moments(p, t, padded=False)
    for a, b in zip(padded, valid):
        assert a.shape == (2, 3, 13, 21)
        assert np.abs(a - b).max() < 1e-14
    # the valid windows, one by one: weighted means of the 11 x 11 block at each window origin
    k = R.gaussian_2d()
    assert abs(k.sum() - 1) < 1e-15 and k.shape == (11, 11)
    for (b, c, i, j) in [(0, 0, 0, 0), (1, 2, 12, 20), (0, 1, 5, 7), (1, 0, 12, 0)]:
        x, y = p[b, c, i:i + 11, j:j + 11].astype(np.float64), t[b, c, i:i + 11, j:j + 11].astype(np.float64)
        direct = [(k * x).sum(), (k * y).sum(), (k * x * x).sum(), (k * y * y).sum(), (k * x * y).sum()]
        for m in range(5):
            assert abs(padded[m][b, c, i, j] - direct[m]) < 1e-14
    dr = R.data_range(p, t)
    assert np.abs(R.ssim_per_image(padded, dr) - R.ssim_per_image(valid, dr)).max() < 1e-13
    # the separable form the GPU tests use
    sep = R.moments(p, t, padded=False, separable=True)
    for a, b in zip(sep, valid):
        assert np.abs(a - b).max() < 1e-14


def test_restatement_semantics():
    p, t = _pair((3, 3, 20, 24), 2)
    # batch-wide range for the functional form; per-image values differ from it when the ranges differ
    p[1] *= 0.5
    t[1] *= 0.5
    mom = R.moments(p, t)
    per_image = np.array([R.ssim_per_image([m[i:i + 1] for m in mom], R.data_range(p[i], t[i]))[0] for i in range(3)])
    batch = R.ssim_per_image(mom, R.data_range(p, t))
    assert abs(R.structural_similarity_index_measure(p, t) - batch.mean()) < 1e-15
    assert abs(per_image[1] - batch[1]) > 1e-6
    assert abs(per_image[0] - batch[0]) < 1e-15
    # identical images: SSIM 1, PSNR inf; a constant pair: NaN
    assert abs(R.structural_similarity_index_measure(p, p) - 1.0) < 1e-12
    assert R.peak_signal_noise_ratio(p, p) == np.inf
    z = np.zeros((1, 3, 12, 12), np.float32)
    assert np.isnan(R.structural_similarity_index_measure(z, z))
    # PSNR: one value over the whole batch
    d = (p.astype(np.float64) - t) ** 2
    assert abs(R.peak_signal_noise_ratio(p, t) - 10 * np.log10(1 / d.mean())) < 1e-12


def test_entry_point_and_helpers_do_not_open_the_library(tmp_path):
    """neuma_amd.evaluation imports and its host helpers run without libneuma_hip.so (the library opens on the first GPU call);
    the torch-facing functions reject CPU tensors and unsupported arguments before touching it"""
    code = r"""
import numpy as np, torch
from neuma_amd import _lib, evaluation, image_metrics as im
a = evaluation.parse_args(["--view", "1"])
assert evaluation.frame_indices(a.start, a.skip, a.num)[-1] == 10
evaluation.debug_pair(np.zeros((12, 12, 3), np.uint8), np.zeros((12, 12, 3), np.uint8))
evaluation.composite_on_white(np.zeros((2, 2, 4), np.uint8))
x = torch.rand(1, 3, 16, 16)
for f in (im.image_metrics, im.peak_signal_noise_ratio, im.structural_similarity_index_measure):
    try:
        f(x, x)
    except _lib.NeumaHipError:
        pass
    else:
        raise SystemExit("CPU tensor accepted")
for kw in (dict(kernel_size=7), dict(sigma=2.0), dict(data_range=1.0), dict(reduction="sum")):
    try:
        im.structural_similarity_index_measure(x, x, **kw)
    except NotImplementedError:
        pass
    else:
        raise SystemExit(f"{kw} accepted")
for kw in (dict(data_range=(0.0, 1.0)), dict(base=2.0), dict(dim=1), dict(reduction="none")):
    try:
        im.peak_signal_noise_ratio(x, x, **kw)
    except NotImplementedError:
        pass
    else:
        raise SystemExit(f"{kw} accepted")
assert _lib._lib is None
print("ok")
"""
    env = dict(os.environ, PYTHONPATH=str(ROOT), NEUMA_HIP_LIB=str(tmp_path / "missing" / "libneuma_hip.so"))
    r = subprocess.run([sys.executable, "-c", code], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
