#!/usr/bin/env python3
"""Generate golden vectors for Gaussian registration (experiments/regist.py) and the SSIM loss by EXECUTING THE REFERENCE'S OWN
CODE.

Run in the build container only (needs /root/reference; never runs on the GPU box):
    python tests/golden/gen_regist_golden.py

pytorch3d, e3nn, einops, plyfile and simple_knn are absent.  `tests/golden/pytorch3d_transforms.py` is registered as
`pytorch3d.transforms` (se3_utils.py imports it); e3nn / einops / plyfile / simple_knn get identity stubs (only imported, never
reached).  The reference's modules are then imported unmodified and their code is run:

  modules/d3gs/utils/transform_utils.py  quaternion_multiply, scale_transform, rotate_transform, translate_transform (14-23,
                                         158-220); rotate_transform's `rotmat_to_quat` is bound to a leaf q_R so that R and q_R
                                         get separate gradients (the kernel takes both as independent inputs)
  modules/d3gs/utils/general_utils.py    build_scaling_rotation, strip_symmetric (93-139); their hard-coded device="cuda" /
                                         dtype=torch.float buffers are created on the CPU in the run's precision
  modules/d3gs/utils/loss_utils.py       ssim (26-66), in fp32 (the reference's precision) and fp64
  modules/tune/scheduler/__init__.py     CosineDecayScheduler through LambdaLR, the regist-*.yaml schedule
  experiments/regist.py                  transform_pcd (40-47; the function's source is executed on its own - the module imports
                                         trimesh / torchvision / tqdm)

Inputs are not stored: tests/golden/regist_inputs.py rebuilds them bit for bit (integer hash, IEEE-exact arithmetic) for the
generator and the tests alike.  Outputs (data only), under tests/golden/regist/:
    regist_transform.npz   two cases over the same K = 4096 Gaussians (s < 1 with scaling_modifier 1.0, s > 1 with 1.2): R, q_R,
                           s, t, o; means3D, cov6, the transformed log-scales / rotations of every 16th Gaussian (fp64); the fp64
                           autograd gradients w.r.t. R, q_R, s, t over all K for the seeded upstream dL/dmeans3D, dL/dcov6; the
                           cosine schedule; transform_pcd of regist_inputs.pcd_points()
    ssim.npz               (3,16,16), (3,37,53), (3,135,240): ssim and d ssim / d img1 in fp32 and fp64 (gradient rows:
                           regist_inputs.ssim_rows - all of the small image, three bands of the others)
"""
import ast
import os
import sys
import types
from pathlib import Path

import numpy as np
import torch

REF = Path("/root/reference")
HERE = Path(__file__).resolve().parent
OUT = Path(os.environ.get("NEUMA_GOLDEN_OUT", HERE)) / "regist"   # (tests/test_regist_golden_regen.py regenerates elsewhere)
sys.path.insert(0, str(HERE))

import pytorch3d_transforms as p3d  # noqa: E402
import regist_inputs as ri  # noqa: E402


def install():
    p3d.install(sys.modules)
    oc = types.ModuleType("omegaconf")

    class DictConfig(dict):
        __getattr__ = dict.__getitem__
        __setattr__ = dict.__setitem__

    oc.DictConfig = DictConfig
    oc.OmegaConf = object
    sys.modules["omegaconf"] = oc
    e3nn = types.ModuleType("e3nn")
    e3nn.o3 = types.ModuleType("e3nn.o3")
    sys.modules["e3nn"], sys.modules["e3nn.o3"] = e3nn, e3nn.o3
    if "einops" not in sys.modules:
        try:
            import einops  # noqa: F401
        except ImportError:
            ein = types.ModuleType("einops")
            ein.einsum = torch.einsum
            sys.modules["einops"] = ein
    ply = types.ModuleType("plyfile")
    ply.PlyData = ply.PlyElement = object
    sys.modules["plyfile"] = ply
    sk = types.ModuleType("simple_knn")
    sk._C = types.ModuleType("simple_knn._C")
    sk._C.distCUDA2 = None
    sys.modules["simple_knn"], sys.modules["simple_knn._C"] = sk, sk._C
    sys.path.insert(0, str(REF))
    return DictConfig


DictConfig = install()
import modules.d3gs.utils.transform_utils as tu   # noqa: E402
import modules.d3gs.utils.general_utils as gu     # noqa: E402
import modules.d3gs.utils.loss_utils as lu        # noqa: E402
from modules.tune.scheduler import CosineDecayScheduler  # noqa: E402


def _load_transform_pcd():
    src = (REF / "experiments" / "regist.py").read_text()
    node = next(n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "transform_pcd")
    ns = {"np": np}
    exec(compile(ast.Module(body=[node], type_ignores=[]), str(REF / "experiments" / "regist.py"), "exec"), ns)
    return ns["transform_pcd"]


class _cpu_buffers(object):
    """torch.zeros(..., device="cuda", dtype=torch.float) of general_utils.py -> CPU buffers of the run's dtype."""

    def __init__(self, dtype):
        self.dtype = dtype

    def __enter__(self):
        self.orig = torch.zeros
        orig, dtype = self.orig, self.dtype

        def zeros(*a, device=None, dtype=None, **k):
            return orig(*a, dtype=self.dtype if dtype in (None, torch.float32) else dtype, **k)

        torch.zeros = zeros
        return self

    def __exit__(self, *exc):
        torch.zeros = self.orig


def transform_case(case):
    inp = ri.transform_inputs()
    par = ri.transform_case(case)
    xyz, rot, ls, gm, gc = (inp[k] for k in ("xyz", "rot", "log_scales", "dL_dmeans3D", "dL_dcov6"))
    s, mod = par["s"], par["scaling_modifier"]
    R = p3d.rotation_6d_to_matrix(torch.tensor(par["r6"], dtype=torch.float64)).float().double()
    qR = p3d.matrix_to_quaternion(R).float().double()
    d = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    R_l, q_l = R.clone().requires_grad_(True), qR.clone().requires_grad_(True)
    s_l = torch.tensor([float(s)], dtype=torch.float64, requires_grad=True)
    t_l = d(par["t"]).requires_grad_(True)
    rotations = torch.nn.functional.normalize(d(rot))                                   # GaussianModel.get_rotation
    orig_rq = getattr(tu, "rotmat_to_quat")
    tu.rotmat_to_quat = lambda m: q_l
    try:
        with _cpu_buffers(torch.float64):
            pts, scales = tu.scale_transform(d(xyz), d(ls), s_l)
            origin = torch.mean(d(xyz), dim=0, keepdim=True)
            pts, rots = tu.rotate_transform(pts, rotations, R_l)
            pts = tu.translate_transform(pts, t_l)
            Lm = gu.build_scaling_rotation(float(mod) * torch.exp(scales), rots)
            cov6 = gu.strip_symmetric(Lm @ Lm.transpose(1, 2))
    finally:
        tu.rotmat_to_quat = orig_rq
    loss = (pts * d(gm)).sum() + (cov6 * d(gc)).sum()
    loss.backward()
    rows = slice(0, None, ri.ROW_STRIDE)
    return dict(R=R.numpy(), q_R=qR.numpy(), s=np.array([s], np.float32), t=par["t"], o=origin.numpy(),
                scaling_modifier=np.array([mod], np.float32), means3D=pts.detach().numpy()[rows], cov6=cov6.detach().numpy()[rows],
                out_log_scales=scales.detach().numpy()[rows], out_rot=rots.detach().numpy()[rows], dR=R_l.grad.numpy(),
                dq_R=q_l.grad.numpy(), ds=s_l.grad.numpy(), dt=t_l.grad.numpy())


def schedule():
    """regist-*.yaml: register.scheduler = {max_steps: 20000, learning_rate_alpha: 0.01}; lr_r / lr_t / lr_s groups, lr 0."""
    sch_cfg = DictConfig(max_steps=20000, learning_rate_alpha=0.01)
    ps = [torch.nn.Parameter(torch.zeros(1)) for _ in range(3)]
    opt = torch.optim.RAdam([{"params": [ps[0]], "lr": 1e-4}, {"params": [ps[1]], "lr": 5e-5}, {"params": [ps[2]], "lr": 1e-5}],
                            lr=0.0, eps=1e-15)
    sch = CosineDecayScheduler(sch_cfg).get_scheduler(opt, 0.0)
    at = [0, 1, 2, 10, 500, 5000, 9999, 10000, 15000, 19999, 20000]
    lrs = []
    for step in range(20001):
        if step in at:
            lrs.append([g["lr"] for g in opt.param_groups])
        sch.step()
    return np.array(at, np.int64), np.array(lrs, np.float64)


def main():
    OUT.mkdir(parents=True, exist_ok=True)
    torch.set_num_threads(1)
    out = {}
    for c in (0, 1):
        for k, v in transform_case(c).items():
            out[f"c{c}_{k}"] = v
    out["sched_steps"], out["sched_lr"] = schedule()
    pts = ri.pcd_points()
    out["pcd_out"] = _load_transform_pcd()(pts, out["c1_s"].astype(np.float64), out["c1_o"], out["c1_R"], out["c1_t"].astype(np.float64))
    np.savez_compressed(OUT / "regist_transform.npz", **out)

    sout = {}
    for h, w in ri.SSIM_SIZES:
        tag = f"{h}x{w}"
        a, b = ri.ssim_images(h, w)
        rows = ri.ssim_rows(h)
        for dt, name in ((torch.float32, "32"), (torch.float64, "64")):
            x = torch.tensor(a, dtype=dt, requires_grad=True)
            y = torch.tensor(b, dtype=dt)
            v = lu.ssim(x, y)
            v.backward()
            sout[f"ssim{name}_{tag}"] = np.array(v.item(), dtype=np.float64)
            sout[f"grad{name}_{tag}"] = np.ascontiguousarray(x.grad.numpy()[:, rows])
    np.savez_compressed(OUT / "ssim.npz", **sout)
    print("wrote", OUT / "regist_transform.npz", OUT / "ssim.npz")


if __name__ == "__main__":
    main()
