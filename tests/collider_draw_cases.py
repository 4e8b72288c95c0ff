"""Scenes shared by tests/test_collider_draw_cpu.py and tests/test_gpu_collider_draw.py: cameras (one with an off-centre principal
point), the four collider sets (a tilted plane, a sphere, a rotated box, a set of 8 mixing all three with overlaps), the two
simulation -> render maps and K = 1500 Gaussian centres; plus the fp64 / fp32 evaluations of the definition
(neuma_amd/extras/collider_draw.py) per case, computed once and cached."""
import functools
import math

import numpy as np
import torch

from neuma_amd import synth
from neuma_amd.collider_draw import parse_styles
from neuma_amd.extras import collider_draw as X
from neuma_amd.sim.colliders import parse_colliders

SIZES = ((67, 45), (128, 80))          # (W, H): a tail in both directions and less than one full wave row; several waves per row
MAPS = {"identity": X.IDENTITY, "peraxis": ((2.0, 1.0, 0.5), (0.1, -0.2, 0.3))}
K_GAUSSIANS = 1500

SETS = {
    "plane": [dict(type="plane", point=[0.5, 0.3, 0.5], normal=[0.2, 1.0, 0.1], checker=0.11)],
    "sphere": [dict(type="sphere", center=[0.45, 0.5, 0.55], radius=0.21)],
    "box": [dict(type="box", center=[0.5, 0.45, 0.5], half=[0.2, 0.1, 0.15], euler_xyz_deg=[20, 30, 40])],
    "eight": [dict(type="plane", point=[0.5, 0.22, 0.5], normal=[0.05, 1.0, -0.08]),
              dict(type="sphere", center=[0.3, 0.3, 0.6], radius=0.13),
              dict(type="box", center=[0.62, 0.33, 0.4], half=[0.12, 0.14, 0.1], euler_xyz_deg=[10, 50, -25]),
              dict(type="sphere", center=[0.6, 0.5, 0.45], radius=0.1, color=[0.1, 0.9, 0.4]),
              dict(type="box", center=[0.35, 0.45, 0.3], half=[0.08, 0.2, 0.08], euler_xyz_deg=[0, 0, 33]),
              dict(type="plane", point=[0.9, 0.5, 0.5], normal=[-1.0, 0.3, 0.0], checker=0.07, color=[0.5, 0.6, 0.9]),
              dict(type="sphere", center=[0.97, 0.8, 0.9], radius=0.2),                       # cut by the cube's corner
              dict(type="box", center=[0.5, 0.7, 0.75], half=[0.3, 0.03, 0.12], euler_xyz_deg=[-35, 15, 5])],
}


class Camera(object):
    """Duck-type of the rasterizer's cameras (synth.SynthCamera) with a principal-point offset, in ndc units, in projmatrix."""

    def __init__(self, W, H, eye, target, fov_deg=40.0, principal=(0.0, 0.0), device="cpu"):
        self.image_width, self.image_height = int(W), int(H)
        self.FoVx = math.radians(fov_deg)
        self.FoVy = 2 * math.atan(math.tan(self.FoVx / 2) * H / W)
        eye, target, up = (np.asarray(a, dtype=np.float64) for a in (eye, target, (0.0, -1.0, 0.0)))
        fwd = (target - eye) / np.linalg.norm(target - eye)
        right = np.cross(fwd, up); right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        Rt = np.eye(4); Rt[:3, :3] = np.stack([right, down, fwd], 0); Rt[:3, 3] = -Rt[:3, :3] @ eye
        wv = Rt.T
        znear, zfar = 0.01, 100.0
        P = np.zeros((4, 4))
        P[0, 0], P[1, 1] = 1 / math.tan(self.FoVx / 2), 1 / math.tan(self.FoVy / 2)
        P[0, 2], P[1, 2] = principal
        P[3, 2], P[2, 2], P[2, 3] = 1.0, zfar / (zfar - znear), -(zfar * znear) / (zfar - znear)
        self.world_view_transform = torch.tensor(wv, dtype=torch.float32, device=device)
        self.full_proj_transform = torch.tensor(wv @ P.T, dtype=torch.float32, device=device)
        self.camera_center = torch.tensor(eye, dtype=torch.float32, device=device)
        self.original_image = None

    def to(self, device):
        c = Camera.__new__(Camera)
        c.__dict__.update(self.__dict__)
        for k in ("world_view_transform", "full_proj_transform", "camera_center"):
            setattr(c, k, getattr(self, k).to(device))
        return c


def to_render_point(p, to_render):
    return tuple(a * x + b for a, b, x in zip(to_render[0], to_render[1], p))


def camera(size, map_name, device="cpu"):
    """The case's camera: it looks at the cube's centre from outside the cube; the per-axis case carries the off-centre principal point."""
    W, H = size
    tr = MAPS[map_name]
    eye, target = to_render_point((1.7, 1.25, 2.0), tr), to_render_point((0.5, 0.45, 0.5), tr)
    return Camera(W, H, eye, target, fov_deg=38.0, principal=(0.0, 0.0) if map_name == "identity" else (0.13, -0.09), device=device)


def gaussians(map_name, K=K_GAUSSIANS, seed=3):
    """K centres in render coordinates, spread over a box a little larger than the cube, and opacities (K,1); fp32"""
    g = torch.Generator().manual_seed(seed)
    p_s = -0.1 + 1.2 * torch.rand(K, 3, generator=g, dtype=torch.float64)
    a, b = (torch.tensor(v, dtype=torch.float64) for v in MAPS[map_name])
    return (p_s * a + b).float(), (0.2 + 0.8 * torch.rand(K, 1, generator=g)).float()


CASES = [(s, size, m) for s in SETS for size in SIZES for m in MAPS]


def case_id(case):
    s, (W, H), m = case
    return f"{s}-{W}x{H}-{m}"


@functools.lru_cache(maxsize=None)
def evaluated(case):
    """dict of one case: cam, colliders, styles, to_render, means, opacity; the fp64 definition t, shade, hit, unsure (pixels),
    hidden, hidden_unsure (Gaussians); and err_t (relative) / err_shade (absolute): the distance of the same formulas evaluated in
    torch fp32 from fp64 outside the unsure set - what the kernels' own distance is measured against."""
    name, size, map_name = case
    cam, tr = camera(size, map_name), MAPS[map_name]
    colliders, styles = parse_colliders(SETS[name]), parse_styles(SETS[name])
    means, opacity = gaussians(map_name)
    t, shade, hit, unsure = X.cast(cam, colliders, styles, tr, margins=True)
    t32, shade32, hit32 = X.cast(cam, colliders, styles, tr, dtype=torch.float32)
    hid, hid_unsure = X.hidden(cam.camera_center, colliders, means, tr, margins=True)
    hid32 = X.hidden(cam.camera_center, colliders, means, tr, dtype=torch.float32)
    ok = ~unsure
    return dict(cam=cam, colliders=colliders, styles=styles, to_render=tr, means=means, opacity=opacity, t=t, shade=shade, hit=hit,
                unsure=unsure, hidden=hid, hidden_unsure=hid_unsure, hit32=hit32, hidden32=hid32,
                err_t=t_error(t32, t, hit, ok), err_shade=float((shade32.double() - shade)[:, ok].abs().max()))


def t_error(t_test, t, hit, ok) -> float:
    """max relative error of t over the pixels that hit and are not excluded (0 without any)"""
    m = ok & (hit >= 0)
    if not bool(m.any()):
        return 0.0
    return float(((t_test.double().cpu()[m] - t[m]).abs() / t[m].abs().clamp_min(1e-30)).max())


def bound(err32: float) -> float:
    """the kernels stay within 4 x the fp32 evaluation's distance from fp64, with a floor of 1e-6"""
    return max(4.0 * err32, 1e-6)
