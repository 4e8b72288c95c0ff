"""Particle-accuracy evaluation of simulated particle states against the ground truth, reachable as
`python -m neuma_amd.particle_evaluation -p <pred_states_dir> -g <gt_states_dir> [-s start] [-k skip] [-n num] [-d cuda]`.

The reference has no such driver: its metric is modules/tune/metrics.py's `chamfer_distance` (cKDTree nearest neighbours,
chamfer1 + chamfer2), which no reference script calls.  This script applies it to single-frame batches of the particle clouds
that `python -m neuma_amd.render -sp NAME` and `python -m neuma_amd.inference -sp NAME` write (states_<NAME>/<step:03d>.ply).
Frames start + i * skip (i = 0..num, the num + 1 rule and defaults of neuma_amd/evaluation.py) are read from both
directories as <frame:03d>.ply; the ground truth can be another run's states or clouds exported into that layout.
Consecutive frames with the same (N, M) go to the GPU together, at most 64 per nm_chamfer call (`neuma_amd.particle_metrics`).
Per frame: CD = chamfer1 + chamfer2, pred->gt = mean squared distance of each predicted particle to its nearest ground-truth
particle, gt->pred the converse.  They are printed and written to <pred_dir>/../<basename>_chamfer.txt with a final mean."""
import argparse
import os

CHUNK = 64                 # frames per nm_chamfer call


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Calculate particle metrics (Chamfer distance)")
    p.add_argument("--pred_dir", "-p", type=str, help="Path to the directory containing the predicted particle states")
    p.add_argument("--gt_dir", "-g", type=str, help="Path to the directory containing the ground truth particle states")
    p.add_argument("--start", "-s", type=int, default=0, help="Start index")
    p.add_argument("--skip", "-k", type=int, default=1, help="Skip index")
    p.add_argument("--num", "-n", type=int, default=10, help="Number of frames to calculate")
    p.add_argument("--device", "-d", type=str, default="cuda", help="Device to use")
    return p.parse_args(argv)


def frame_indices(start: int, skip: int, num: int):
    """num + 1 frames, as neuma_amd/evaluation.py"""
    return [start + i * skip for i in range(num + 1)]


def frame_paths(pred_dir: str, gt_dir: str, i: int):
    """(pred, gt) paths of frame i; a missing file raises with its path, the prediction checked first."""
    pred_path = os.path.join(pred_dir, f"{i:03d}.ply")
    if not os.path.exists(pred_path):
        raise FileNotFoundError(f"File not exist for {pred_path}")
    gt_path = os.path.join(gt_dir, f"{i:03d}.ply")
    if not os.path.exists(gt_path):
        raise FileNotFoundError(f"File not exist for {gt_path}")
    return pred_path, gt_path


def group_frames(sizes, chunk: int = CHUNK):
    """Runs of consecutive positions with equal (N, M) in `sizes`, each cut to at most `chunk`: a list of position lists."""
    groups = []
    for k, s in enumerate(sizes):
        if groups and sizes[groups[-1][-1]] == s and len(groups[-1]) < chunk:
            groups[-1].append(k)
        else:
            groups.append([k])
    return groups


def metrics_path(pred_dir: str) -> str:
    """<pred_dir>/../<basename>_chamfer.txt (the naming of evaluation.py's metrics file)"""
    return os.path.join(pred_dir, "..", f'{pred_dir.rstrip("/").split("/")[-1]}_chamfer.txt')


def write_metrics(path, frames, cd, c12, c21):
    """One line per frame - frame, CD, pred->gt, gt->pred - then the mean of each column."""
    n = len(frames)
    with open(path, "w") as f:
        f.write("frame CD pred_to_gt gt_to_pred\n")
        for i, a, b, c in zip(frames, cd, c12, c21):
            f.write(f"{i:03d} {a:.8e} {b:.8e} {c:.8e}\n")
        f.write(f"mean {sum(cd) / n:.8e} {sum(c12) / n:.8e} {sum(c21) / n:.8e}\n")


def _score(preds, gts, device):
    """per-frame (chamfer1, chamfer2) lists of a group of clouds of equal sizes: one nm_chamfer call (fp32 coordinates)."""
    import numpy as np
    import torch
    from .particle_metrics import chamfer_distance_kdtree

    p = torch.from_numpy(np.stack(preds).astype(np.float32)).to(device)
    g = torch.from_numpy(np.stack(gts).astype(np.float32)).to(device)
    c1, c2, _, _ = chamfer_distance_kdtree(p, g, give_id=True)
    return c1.double().cpu().tolist(), c2.double().cpu().tolist()


def calculate_particle_metrics(pred_dir, gt_dir, start, skip, num, device="cuda"):
    """Returns (frames, CD, pred->gt, gt->pred) lists and writes the metrics file."""
    import torch
    from .io import load_particles_ply

    device = torch.device(device)
    idx = frame_indices(start, skip, num)
    print(f"current pred_dir: {pred_dir}, skip: {skip}, from {start} to {start + num * skip}")
    paths = [frame_paths(pred_dir, gt_dir, i) for i in idx]
    preds = [load_particles_ply(pp) for pp, _ in paths]
    gts = [load_particles_ply(gp) for _, gp in paths]
    c12, c21 = [0.0] * len(idx), [0.0] * len(idx)
    for grp in group_frames([(len(p), len(g)) for p, g in zip(preds, gts)]):
        a, b = _score([preds[k] for k in grp], [gts[k] for k in grp], device)
        for k, va, vb in zip(grp, a, b):
            c12[k], c21[k] = va, vb
    cd = [a + b for a, b in zip(c12, c21)]
    for i, (pp, gp), p, g, v, a, b in zip(idx, paths, preds, gts, cd, c12, c21):
        print(f"pr: {os.path.basename(pp)} [{len(p)}] | gt: {os.path.basename(gp)} [{len(g)}] | CD: {v:.6e} "
              f"| pred->gt: {a:.6e} | gt->pred: {b:.6e}")
    write_metrics(metrics_path(pred_dir), idx, cd, c12, c21)
    print(f"mean CD: {sum(cd) / len(cd):.6e}")
    return idx, cd, c12, c21


def main(argv=None):
    args = parse_args(argv)
    calculate_particle_metrics(args.pred_dir, args.gt_dir, args.start, args.skip, args.num, args.device)


if __name__ == "__main__":
    main()
