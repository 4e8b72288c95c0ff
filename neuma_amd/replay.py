"""`python -m neuma_amd.replay -s GAUSSIANS_DIR -c cfg.yaml -dv view [view ...] [-o OUT_DIR] [--sh_degree D] [--white_background]`:
render a saved sequence of Gaussian frames (`NNN.ply`, written by `render --save_gaussians` / `inference --save_gaussians`, or any
3DGS .ply) from the cameras of a config's dataset, through the ordinary static path - load_gaussians_ply, then
diff_rasterization(g.get_xyz, None, g, cam, background).  No simulator, no checkpoints and no bindings are loaded: the files carry
the deformed frame whole, scale modifier baked in.  Writes <OUT_DIR>/<view>_<frame>.png (OUT_DIR defaults to
GAUSSIANS_DIR/replay).  The reference looks at a result from elsewhere in its interactive viewer (modules/vis); this is the
counterpart that needs none.

Cameras: those of the dataset's first step, as `render` uses them throughout; the background is white when the config's
video_data.data.white_background (or --white_background) says so.  --sh_degree defaults to the config's gaussian.sh_degree (3
without one) and must match the files' f_rest_* count."""
import argparse
import sys
from pathlib import Path
from typing import Iterable, Iterator, List, Sequence, Tuple

import torch

from . import io as nio
from .config import load_config
from .dataset import CameraDataset
from .evaluate import save_image
from .tune import diff_rasterization


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--source", "-s", type=str, required=True, help="Folder of NNN.ply Gaussian frames.")
    p.add_argument("--config", "-c", type=str, required=True, help="Config whose video_data names the cameras.")
    p.add_argument("--debug_views", "-dv", nargs="+", required=True, help="Views to render.")
    p.add_argument("--out", "-o", type=str, default=None)
    p.add_argument("--sh_degree", type=int, default=None)
    p.add_argument("--white_background", action="store_true")
    p.add_argument("--dataset_path", type=str, default=None, help="Rewrite video dataset path.")
    return p.parse_args(argv)


def sequence_paths(folder) -> List[Path]:
    """the NNN.ply files of a folder in frame order"""
    paths = sorted((p for p in Path(folder).glob("*.ply") if p.stem.isdigit()), key=lambda p: int(p.stem))
    if not paths:
        raise FileNotFoundError(f"no NNN.ply frames in {folder}")
    return paths


@torch.no_grad()
def render_sequence(paths: Iterable, cameras: Sequence, background: torch.Tensor, sh_degree: int) -> Iterator[Tuple[int, List[torch.Tensor]]]:
    """Yields (frame number = the file's stem, [one image per camera]) for every file of `paths`, on the background's device."""
    for path in paths:
        g = nio.load_gaussians_ply(path, sh_degree, device=background.device)
        yield int(Path(path).stem), [diff_rasterization(g.get_xyz, None, g, cam, background) for cam in cameras]


def main(argv=None):
    args = parse_args(argv)
    cfg = load_config(args.config)
    device = torch.device(f"cuda:{cfg.get('gpu', 0)}")
    torch.cuda.set_device(device)
    white = bool(args.white_background or cfg.video_data.data.get("white_background", False))
    background = torch.tensor([1.0, 1.0, 1.0] if white else [0.0, 0.0, 0.0], device=device)
    cfg.video_data.data.used_views = list(args.debug_views)
    if args.dataset_path is not None:
        cfg.video_data.data.path = args.dataset_path
    cfg.video_data.device = str(device)
    dataset = CameraDataset(cfg.video_data)
    missing = [vw for vw in args.debug_views if vw not in dataset.views]
    if missing:
        raise ValueError(f"views {missing} are not in the dataset (it has {dataset.views})")
    views = [vw for vw in dataset.views if vw in args.debug_views]
    cameras = [dataset.getCameras(vw, dataset.steps[0]) for vw in views]
    sh_degree = args.sh_degree
    if sh_degree is None:
        gc = cfg.get("gaussian")
        sh_degree = int(gc.get("sh_degree", 3)) if gc is not None else 3
    out = Path(args.out) if args.out is not None else Path(args.source) / "replay"
    out.mkdir(parents=True, exist_ok=True)
    for frame, images in render_sequence(sequence_paths(args.source), cameras, background, sh_degree):
        for vw, img in zip(views, images):
            save_image(img, out / f"{vw}_{frame:03d}.png")
    return 0


if __name__ == "__main__":
    sys.exit(main())
