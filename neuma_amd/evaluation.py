"""Image-quality evaluation of rendered frames against the ground truth: counterpart of experiments/evaluation.py (the
fourth stage of the NeuMA pipeline, after regist / finetune / render), reachable as
`python -m neuma_amd.evaluation -p <pred_dir> -g <gt_dir> --view V [-s start] [-k skip] [-n num] [-d cuda]
[--lpips_vgg PATH --lpips_heads PATH]`.

Frames start + i * skip (i = 0..num) are read as <dir>/e_<view>_<i:03d>.png: the prediction as RGB (alpha dropped), the ground
truth as RGBA composited on white with the reference's truncation to uint8, both cropped to [220:580, 220:580].  PSNR and SSIM
per frame (torchmetrics semantics, `neuma_amd.image_metrics`; one nm_image_metrics call per chunk of up to 64 frames, each frame
with its own data range) are averaged into <pred_dir>/../<basename>_metrics.txt, and each pair is written side by side to
results/debug/<i>.png.  LPIPS (VGG-16, `neuma_amd.lpips`) is the third number when the user names the two public weight files it
needs, torchvision's VGG-16 state dict (--lpips_vgg) and the LPIPS heads vgg.pth of torchmetrics / lpips (--lpips_heads): this
package ships and fetches neither, and without the two flags LPIPS is not computed.  The pred-gt mp4 is not written (packing
frames into a video is left to external tools).

(Not to be confused with `neuma_amd/evaluate.py`, the forward roll-out + rendering of render.py's `eval`.)"""
import argparse
import os

import numpy as np

CROP = (220, 580)          # rows, then columns (evaluation.py:33-34)
CHUNK = 64                 # frames per upload / nm_image_metrics call
DEBUG_DIR = os.path.join("results", "debug")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Calculate image metrics")
    p.add_argument("--pred_dir", "-p", type=str, help="Path to the directory containing the predicted images")
    p.add_argument("--gt_dir", "-g", type=str, help="Path to the directory containing the ground truth images")
    p.add_argument("--start", "-s", type=int, default=0, help="Start index")
    p.add_argument("--skip", "-k", type=int, default=1, help="Skip index")
    p.add_argument("--num", "-n", type=int, default=10, help="Number of images to calculate")
    p.add_argument("--device", "-d", type=str, default="cuda", help="Device to use")
    p.add_argument("--view", type=int, required=True)
    p.add_argument("--lpips_vgg", type=str, default=None, help="torchvision VGG-16 state dict (.pth); with --lpips_heads: LPIPS")
    p.add_argument("--lpips_heads", type=str, default=None, help="LPIPS heads vgg.pth of torchmetrics / lpips; with --lpips_vgg")
    args = p.parse_args(argv)
    if (args.lpips_vgg is None) != (args.lpips_heads is None):
        missing = "--lpips_heads" if args.lpips_heads is None else "--lpips_vgg"
        given = "--lpips_vgg" if args.lpips_heads is None else "--lpips_heads"
        p.error(f"LPIPS needs both weight files: {given} was given without {missing}")
    return args


def frame_indices(start: int, skip: int, num: int):
    """evaluation.py:28: num + 1 frames"""
    return [start + i * skip for i in range(num + 1)]


def frame_paths(pred_dir: str, gt_dir: str, view: int, i: int):
    """(pred, gt) paths of frame i; a missing file raises with its path, the prediction checked first."""
    pred_path = os.path.join(pred_dir, f"e_{view}_{i:03d}.png")
    if not os.path.exists(pred_path):
        raise FileNotFoundError(f"File not exist for {pred_path}")
    gt_path = os.path.join(gt_dir, f"e_{view}_{i:03d}.png")
    if not os.path.exists(gt_path):
        raise FileNotFoundError(f"File not exist for {gt_path}")
    return pred_path, gt_path


def composite_on_white(rgba: np.ndarray) -> np.ndarray:
    """evaluation.py:56-59 on an (H, W, 4) uint8 array: the float64 blend on white, then `np.array(arr * 255.0, dtype=np.byte)`
    read back as uint8 - i.e. arr * 255 TRUNCATED (not rounded) to uint8.  Opaque pixels come back unchanged."""
    norm_data = rgba / 255.0
    arr = norm_data[:, :, :3] * norm_data[:, :, 3:4] + np.array([1, 1, 1]) * (1 - norm_data[:, :, 3:4])
    return np.trunc(arr * 255.0).astype(np.uint8)


def load_pred(path) -> np.ndarray:
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert("RGB"))


def load_gt(path) -> np.ndarray:
    from PIL import Image
    with Image.open(path) as im:
        return composite_on_white(np.array(im.convert("RGBA")))


def crop(img: np.ndarray) -> np.ndarray:
    return img[CROP[0]:CROP[1], CROP[0]:CROP[1], :]


def debug_pair(pred: np.ndarray, gt: np.ndarray) -> np.ndarray:
    """save_image(cat([pred, gt]), nrow=2) of two (H, W, 3) uint8 crops: a black canvas with padding 2, pred at
    [2:H+2, 2:W+2], gt at [2:H+2, W+4:2W+4] (uint8 -> /255 -> *255 + 0.5 round-trips every byte)."""
    h, w = pred.shape[:2]
    canvas = np.zeros((h + 4, 2 * w + 6, 3), dtype=np.uint8)
    canvas[2:h + 2, 2:w + 2] = pred
    canvas[2:h + 2, w + 4:2 * w + 4] = gt
    return canvas


def metrics_path(pred_dir: str) -> str:
    """evaluation.py:84"""
    return os.path.join(pred_dir, "..", f'{pred_dir.split("/")[-1]}_metrics.txt')


def _score(preds_u8, gts_u8, device, lpips=None):
    """per-frame (psnr, ssim, lpips or None) lists of a chunk of (H, W, 3) uint8 crops: ToTensor (uint8 / 255 in fp32) on the
    device, then one nm_image_metrics call with each frame's own data range and, given LpipsWeights, nm_lpips.  Called as the
    reference does, psnr(gt, pred) / ssim(gt, pred) / lpips(gt, pred)."""
    import torch
    from .image_metrics import image_metrics

    def to_tensor(frames):
        a = torch.from_numpy(np.stack(frames)).to(device)
        return a.permute(0, 3, 1, 2).float().div(255).contiguous()

    gt, pred = to_tensor(gts_u8), to_tensor(preds_u8)
    psnr, ssim = image_metrics(gt, pred, range_per_image=True)
    lp = None
    if lpips is not None:
        from .lpips import lpips as lpips_native
        lp = lpips_native(gt, pred, lpips).cpu().tolist()
    return psnr.cpu().tolist(), ssim.cpu().tolist(), lp


def calculate_synthetic_image_metrics(pred_dir, gt_dir, start, skip, num, view, device="cuda", lpips=None):
    """evaluation.py:27-97 without the video; returns (mean PSNR, mean SSIM), or (mean PSNR, mean SSIM, mean LPIPS) when `lpips`
    holds LpipsWeights (neuma_amd.lpips.load_weights, which records the two files' names for the notice)."""
    import torch
    from PIL import Image

    device = torch.device(device)
    idx = frame_indices(start, skip, num)
    os.makedirs(DEBUG_DIR, exist_ok=True)
    print(f"current pred_dir: {pred_dir}, skip: {skip}, from {start} to {start + num * skip}")
    if lpips is None:
        print("LPIPS is not computed (no VGG-16 / LPIPS weights are shipped) and the pred-gt mp4 is not written (no video "
              "encoder); the metrics file holds PSNR and SSIM only")
    else:
        vgg_file, heads_file = lpips.files or ("<weights given as tensors>",) * 2
        print(f"LPIPS from VGG-16 weights {vgg_file} and heads {heads_file}; the pred-gt mp4 is not written (no video encoder)")
    psnr_all, ssim_all, lpips_all = [], [], []
    for c0 in range(0, len(idx), CHUNK):
        chunk = idx[c0:c0 + CHUNK]
        names, preds, gts = [], [], []
        for i in chunk:
            pred_path, gt_path = frame_paths(pred_dir, gt_dir, view, i)
            preds.append(crop(load_pred(pred_path)))
            gts.append(crop(load_gt(gt_path)))
            names.append((os.path.basename(pred_path), os.path.basename(gt_path)))
        psnr, ssim, lp = _score(preds, gts, device, lpips)
        for j, (i, (pn, gn), p, g, pv, sv) in enumerate(zip(chunk, names, preds, gts, psnr, ssim)):
            tail = "" if lp is None else f" | LPIPS: {lp[j]:.2f}"
            print(f"pr: {pn} [{p.shape}] | gt: {gn} [{g.shape}] | PSNR: {pv:.2f} | SSIM: {sv:.2f}{tail}")
            Image.fromarray(debug_pair(p, g), "RGB").save(os.path.join(DEBUG_DIR, f"{i}.png"))
        psnr_all += psnr
        ssim_all += ssim
        lpips_all += lp or []
    psnr_avg = sum(psnr_all) / len(psnr_all)           # AverageMeter: plain mean, inf / nan propagate
    ssim_avg = sum(ssim_all) / len(ssim_all)
    with open(metrics_path(pred_dir), "w") as f:
        f.write(f"PSNR: {psnr_avg:.2f}\n")
        f.write(f"SSIM: {ssim_avg:.2f}\n")
        if lpips is not None:
            lpips_avg = sum(lpips_all) / len(lpips_all)
            f.write(f"LPIPS: {lpips_avg:.4f}\n")
    if lpips is not None:
        return psnr_avg, ssim_avg, lpips_avg
    return psnr_avg, ssim_avg


def main(argv=None):
    args = parse_args(argv)
    weights = None
    if args.lpips_vgg is not None:
        from .lpips import load_weights
        weights = load_weights(args.lpips_vgg, args.lpips_heads, args.device)
    calculate_synthetic_image_metrics(args.pred_dir, args.gt_dir, args.start, args.skip, args.num, args.view, args.device,
                                      lpips=weights)


if __name__ == "__main__":
    main()
