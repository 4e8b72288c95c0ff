"""Particle-accuracy evaluation of simulated particle states against the ground truth, reachable as
`python -m neuma_amd.particle_evaluation -p <pred_states_dir> -g <gt_states_dir> [-s start] [-k skip] [-n num] [-d cuda]
[--emd [--emd_points 4096] [--emd_power 1] [--emd_seed 0]]`.

The reference has no such driver: its metric is modules/tune/metrics.py's `chamfer_distance` (cKDTree nearest neighbours,
chamfer1 + chamfer2), which no reference script calls.  This script applies it to single-frame batches of the particle clouds
that `python -m neuma_amd.render -sp NAME` and `python -m neuma_amd.inference -sp NAME` write (states_<NAME>/<step:03d>.ply).
Frames start + i * skip (i = 0..num, the num + 1 rule and defaults of neuma_amd/evaluation.py) are read from both
directories as <frame:03d>.ply; the ground truth can be another run's states or clouds exported into that layout.
Consecutive frames with the same (N, M) go to the GPU together, at most 64 per nm_chamfer call (`neuma_amd.particle_metrics`).
Per frame: CD = chamfer1 + chamfer2, pred->gt = mean squared distance of each predicted particle to its nearest ground-truth
particle, gt->pred the converse.  They are printed and written to <pred_dir>/../<basename>_chamfer.txt with a final mean.

--emd adds the earth mover's distance, the second column of the state-prediction papers (no reference counterpart): the exact
optimal one-to-one transport cost mean_i |x_i - y_sigma(i)|^power between n = min(N_pred, N_gt, emd_points, 8192) points of each
cloud (`particle_metrics.emd_native`, one nm_emd call per group of frames).  A cloud of more than n points is subsampled with
`particle_metrics.subsample_indices(N, n, emd_seed)`: one index set per distinct cloud size, reused for every frame.  Each frame
line gains ` | EMD: ...`, and <pred_dir>/../<basename>_emd.txt holds frame, EMD, n and the auction's rounds per frame, then the
mean.  The value exceeds the true optimum of the fp32 clouds by at most Cmax * 2^-23 (Cmax = the cost of the joint bounding
box's extent); the largest such bound over the frames is printed.  Without --emd nothing of this runs."""
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
    p.add_argument("--emd", action="store_true", help="Also compute the earth mover's distance (exact assignment)")
    p.add_argument("--emd_points", type=int, default=4096, help="Points per cloud for the EMD (at most 8192)")
    p.add_argument("--emd_power", type=int, default=1, choices=(1, 2), help="EMD cost: distance (1) or squared distance (2)")
    p.add_argument("--emd_seed", type=int, default=0, help="Seed of the EMD subsampling")
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


def emd_path(pred_dir: str) -> str:
    """<pred_dir>/../<basename>_emd.txt"""
    return os.path.join(pred_dir, "..", f'{pred_dir.rstrip("/").split("/")[-1]}_emd.txt')


def write_emd(path, frames, emd, counts, rounds):
    """One line per frame - frame, EMD, points per cloud, auction rounds - then the mean EMD."""
    with open(path, "w") as f:
        f.write("frame EMD n rounds\n")
        for i, v, n, r in zip(frames, emd, counts, rounds):
            f.write(f"{i:03d} {v:.8e} {n} {r}\n")
        f.write(f"mean {sum(emd) / len(frames):.8e}\n")


def emd_points_used(n_pred: int, n_gt: int, emd_points: int) -> int:
    return min(n_pred, n_gt, emd_points, 8192)


def _score_emd(preds, gts, n, power, seed, picks, device):
    """per-frame (emd, rounds, bound) lists of a group of clouds of equal sizes, n points of each: one nm_emd call.  picks caches
    the index set of each distinct cloud size."""
    import numpy as np
    import torch
    from .particle_metrics import emd_native, subsample_indices

    def pick(cloud):
        key = (len(cloud), n)
        if key not in picks:
            picks[key] = subsample_indices(len(cloud), n, seed)
        return np.asarray(cloud, np.float32)[picks[key]]

    p, g = np.stack([pick(c) for c in preds]), np.stack([pick(c) for c in gts])
    ext = (np.maximum(p.max(1), g.max(1)).astype(np.float64) - np.minimum(p.min(1), g.min(1)).astype(np.float64))
    cmax = (ext[:, 0] * ext[:, 0] + ext[:, 1] * ext[:, 1]) + ext[:, 2] * ext[:, 2]
    cmax = np.sqrt(cmax) if power == 1 else cmax
    emd, _, rounds = emd_native(torch.from_numpy(p).to(device), torch.from_numpy(g).to(device), power=power)
    return emd.cpu().tolist(), rounds.cpu().tolist(), (cmax * 2.0 ** -23).tolist()


def _score(preds, gts, device):
    """per-frame (chamfer1, chamfer2) lists of a group of clouds of equal sizes: one nm_chamfer call (fp32 coordinates)."""
    import numpy as np
    import torch
    from .particle_metrics import chamfer_distance_kdtree

    p = torch.from_numpy(np.stack(preds).astype(np.float32)).to(device)
    g = torch.from_numpy(np.stack(gts).astype(np.float32)).to(device)
    c1, c2, _, _ = chamfer_distance_kdtree(p, g, give_id=True)
    return c1.double().cpu().tolist(), c2.double().cpu().tolist()


def calculate_particle_metrics(pred_dir, gt_dir, start, skip, num, device="cuda", emd=False, emd_points=4096, emd_power=1,
                               emd_seed=0):
    """Returns (frames, CD, pred->gt, gt->pred) lists and writes the metrics file; with emd=True the EMD file too, and the
    per-frame EMD list is appended to the result."""
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
    if emd:
        ev, er, eb, en, picks = [0.0] * len(idx), [0] * len(idx), [0.0] * len(idx), [0] * len(idx), {}
        for grp in group_frames([(len(p), len(g)) for p, g in zip(preds, gts)]):
            n = emd_points_used(len(preds[grp[0]]), len(gts[grp[0]]), emd_points)
            va, ra, ba = _score_emd([preds[k] for k in grp], [gts[k] for k in grp], n, emd_power, emd_seed, picks, device)
            for k, v, r, b in zip(grp, va, ra, ba):
                ev[k], er[k], eb[k], en[k] = v, r, b, n
    for k, (i, (pp, gp), p, g, v, a, b) in enumerate(zip(idx, paths, preds, gts, cd, c12, c21)):
        print(f"pr: {os.path.basename(pp)} [{len(p)}] | gt: {os.path.basename(gp)} [{len(g)}] | CD: {v:.6e} "
              f"| pred->gt: {a:.6e} | gt->pred: {b:.6e}" + (f" | EMD: {ev[k]:.6e}" if emd else ""))
    write_metrics(metrics_path(pred_dir), idx, cd, c12, c21)
    print(f"mean CD: {sum(cd) / len(cd):.6e}")
    if emd:
        write_emd(emd_path(pred_dir), idx, ev, en, er)
        print(f"mean EMD: {sum(ev) / len(ev):.6e} (n: {'/'.join(str(v) for v in sorted(set(en)))}, power: {emd_power}, "
              f"seed: {emd_seed}, at most {max(eb):.3e} above the exact optimum: Cmax * 2^-23 of the worst frame)")
        return idx, cd, c12, c21, ev
    return idx, cd, c12, c21


def main(argv=None):
    args = parse_args(argv)
    calculate_particle_metrics(args.pred_dir, args.gt_dir, args.start, args.skip, args.num, args.device, emd=args.emd,
                               emd_points=args.emd_points, emd_power=args.emd_power, emd_seed=args.emd_seed)


if __name__ == "__main__":
    main()
