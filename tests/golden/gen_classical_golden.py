#!/usr/bin/env python3
"""Generate the golden vectors of the classical constitutive laws by IMPORTING the reference's own classes
(modules/nclaw/material/preset.py) under the identity stubs of gen_material_golden.py (`install_stubs`, `TorchSVD`).

Run in the build container only (needs the reference checkout; never runs on the GPU box):
    python tests/golden/gen_classical_golden.py

Outputs (data only: float / integer / boolean arrays, no strings), into NEUMA_GOLDEN_OUT or this directory:
    classical/<law>.npz          F, the constructor scalars, `state.<key>` = the reference module's state_dict, out, grad_out,
                                 grad_F, grad_scalars ({d/d log_E, d/d p2} of the learnable ones), all from the reference class in
                                 fp64; `*_f32` = the SAME class run in fp32 on the same inputs (the yardstick of the tolerances);
                                 branch masks for the two return maps; `F_nan` / `out_nan` for the two laws that are NaN at det F < 0
    classical/rollout_<pair>.npz 12 substeps at G = 32 of oracle.mpm's fp64 substep with a reference elasticity + plasticity
                                 pair: initial state, final x, v, C, F (fp64 and an fp32 run of the same path), the loss weights,
                                 dL/d log_E by autograd (fp64, fp32) and by central differences (steps h and 2h) of this path in fp64

Construction rule of the inputs (so that the tests can compare EVERY stored row): a row is rejected and redrawn when two of its
singular values (signed or by magnitude) are closer than 1e-2, or when a switch variable of its law (sigma - 0.05, delta_gamma,
shifted_trace) is within 1e-3 of zero - such a row may take the other branch in fp32.  The last four rows are reflected
(negative sigma_2) except for the two laws that are NaN there.
"""
import importlib.util
import math
import os
import sys
from pathlib import Path

import numpy as np
import torch

REF = Path("/root/reference")
HERE = Path(__file__).resolve().parent
OUT = Path(os.environ.get("NEUMA_GOLDEN_OUT", HERE))
ROWS, REFLECTED = 68, 4
E0, NU0 = 1e5, 0.3


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


G = _load(HERE / "gen_material_golden.py", "gen_material_golden")


def switch_ok(sig, kind, cfg):
    """rows far enough from every switch of the law (fp64 singular values `sig`, signed)"""
    a = sig.abs()
    ok = torch.ones(sig.shape[0], dtype=torch.bool)
    for i, j in ((0, 1), (0, 2), (1, 2)):
        ok &= ((sig[:, i] - sig[:, j]).abs() >= 1e-2) & ((a[:, i] - a[:, j]).abs() >= 1e-2)
    masks = {}
    if kind in ("von_mises", "drucker_prager"):
        ok &= ((sig - 0.05).abs() >= 1e-3).all(1)
        eps = sig.clamp_min(0.05).log()
        tr = eps.sum(1)
        n = (eps - tr[:, None] / 3).norm(dim=1)
        mu = cfg["E"] / (2 * (1 + cfg["nu"]))
        la = cfg["E"] * cfg["nu"] / ((1 + cfg["nu"]) * (1 - 2 * cfg["nu"]))
        if kind == "von_mises":
            dg = n - cfg["sigma_y"] / (2 * mu)
            ok &= dg.abs() >= 1e-3
            masks["mask_yield"] = dg > 0
        else:
            sp = math.sin(math.radians(cfg["friction_angle"]))
            alpha = math.sqrt(2 / 3) * 2 * sp / (3 - sp)
            sh = tr - 3 * cfg["cohesion"]
            dg = n + (3 * la + 2 * mu) / (2 * mu) * sh * alpha
            ok &= (sh.abs() >= 1e-3) & (dg.abs() >= 1e-3)
            masks["mask_yield"] = sh < 0
            masks["mask_moved"] = dg > 0
    return ok, masks


def draw_F(seed, spread, vol, kind, cfg, reflect):
    """ROWS deformation gradients I + spread N(0,1), times a volumetric factor exp(vol N(0,1)); the last REFLECTED rows with
    their third column negated when `reflect`, every row with det F > 0 otherwise; rows near a switch are redrawn."""
    g = torch.Generator().manual_seed(seed)
    svd = G.TorchSVD()
    plain, mirrored = [], []
    while len(plain) < ROWS - (REFLECTED if reflect else 0) or len(mirrored) < (REFLECTED if reflect else 0):
        F = torch.eye(3, dtype=torch.float64)[None] + spread * torch.randn(64, 3, 3, generator=g, dtype=torch.float64)
        F = F * torch.exp(vol * torch.randn(64, 1, 1, generator=g, dtype=torch.float64))
        F = F[torch.linalg.det(F) > 0]
        Fm = F.clone()
        Fm[:, :, 2] *= -1.0
        for cand, bucket in ((F[: F.shape[0] // 2], plain), (Fm[F.shape[0] // 2:], mirrored)):
            ok, _ = switch_ok(svd(cand)[1], kind, cfg)
            bucket.extend(cand[ok])
    rows = plain[: ROWS - (REFLECTED if reflect else 0)] + (mirrored[:REFLECTED] if reflect else [])
    F = torch.stack(rows)
    _, masks = switch_ok(svd(F)[1], kind, cfg)
    return F, masks


def run(cls, cfg, F, gout, dtype, DictConfig):
    m = cls(DictConfig(cfg)).to(dtype)
    m.svd = G.TorchSVD()
    Fg = F.to(dtype).clone().requires_grad_(True)
    out = m(Fg)
    params = [p for p in (getattr(m, "log_E", None), getattr(m, "sigma_y", None), getattr(m, "friction_angle", None)) if p is not None]
    (out * gout.to(dtype)).sum().backward()
    gs = np.array([float(p.grad) for p in params], dtype=np.float64)
    return m, out.detach().double().numpy(), Fg.grad.double().numpy().copy(), gs


def law_case(material, DictConfig, tag, cls_name, kind, cfg, seed, spread, vol=0.0, reflect=True, nan_rows=False):
    cls = getattr(material, cls_name)
    F, masks = draw_F(seed, spread, vol, kind, cfg, reflect)
    gout = torch.randn(F.shape, generator=torch.Generator().manual_seed(seed + 100), dtype=torch.float64)
    m, out, gF, gs = run(cls, cfg, F, gout, torch.float64, DictConfig)
    _, out32, gF32, gs32 = run(cls, cfg, F, gout, torch.float32, DictConfig)
    rec = {"F": F.numpy(), "grad_out": gout.numpy(), "out": out, "grad_F": gF, "grad_scalars": gs, "out_f32": out32,
           "grad_F_f32": gF32, "grad_scalars_f32": gs32}
    for k, v in cfg.items():
        if k == "mode":
            rec["mode_id"] = np.int32({"ziran": 0, "taichi": 1}[v])
        elif k != "random":
            rec[k] = np.float64(v)
    for k, v in cls(DictConfig(cfg)).state_dict().items():
        rec["state." + k] = v.numpy()
    for k, v in cls(DictConfig(dict(cfg, random=True))).state_dict().items():
        rec["state_random." + k] = v.numpy()
    for k, v in masks.items():
        rec[k] = v.numpy()
        print(f"  {tag}: {k} {int(v.sum())} / {ROWS}")
    if nan_rows:
        Fn = G.make_F(6, seed=seed + 1, spread=spread)[-2:]          # two reflected rows: det F < 0
        with torch.no_grad():
            rec["F_nan"] = Fn.numpy()
            rec["out_nan"] = m(Fn).numpy()
        assert np.isnan(rec["out_nan"]).any(axis=(1, 2)).all()
    assert np.isfinite(out).all() and np.isfinite(gF).all() and np.isfinite(out32).all() and np.isfinite(gF32).all(), tag
    np.savez_compressed(OUT / "classical" / f"{tag}.npz", **rec)


def rollout_case(material, DictConfig, om, tag, e_name, e_cfg, p_name, p_cfg, seed, f_scale=1.0):
    """12 substeps of oracle.mpm.step with the reference pair, in the order of the drivers: stress = e(F); step; F = p(F).
    f_scale < 1 starts the body compressed and the pair has cohesion > 0, so that Drucker-Prager stays on its yielding side: on the expanding side it returns
    exp(cohesion) U Vh, whose three equal singular values make the NEXT substep's SVD adjoint singular (NaN from
    torch.linalg.svd's adjoint, which the generator's path uses)."""
    gen = torch.Generator().manual_seed(seed)
    N, S = 343, 12
    const = om.MPMConstant(num_grids=32, dt=1e-3, bound=1, gravity=(0.0, -9.8, 0.0), eps=6e-7, bc="noslip")
    ax = torch.linspace(0.40, 0.58, 7, dtype=torch.float64)
    x0 = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3) + 0.004 * torch.rand(N, 3, generator=gen, dtype=torch.float64)
    v0 = torch.tensor([0.4, -1.0, 0.2], dtype=torch.float64)[None] + 0.5 * torch.randn(N, 3, generator=gen, dtype=torch.float64)
    C0 = torch.zeros(N, 3, 3, dtype=torch.float64)
    F0 = f_scale * (torch.eye(3, dtype=torch.float64)[None] + 0.03 * torch.randn(N, 3, 3, generator=gen, dtype=torch.float64))
    vol = torch.full((N,), (const.dx / 2) ** 3, dtype=torch.float64)
    rho = torch.full((N,), 1000.0, dtype=torch.float64)
    clip = torch.full((N,), 0.1, dtype=torch.float64)
    en = torch.ones(N, dtype=torch.int32)
    wx = torch.randn(N, 3, generator=gen, dtype=torch.float64)
    wv = 1e-2 * torch.randn(N, 3, generator=gen, dtype=torch.float64)

    def path(dtype, log_E_shift=0.0, grad=False):
        e = getattr(material, e_name)(DictConfig(e_cfg)).to(dtype)
        p = getattr(material, p_name)(DictConfig(p_cfg)).to(dtype)
        e.svd = G.TorchSVD(); p.svd = G.TorchSVD()
        e.log_E.data += log_E_shift
        x, v, C, F = (t.to(dtype) for t in (x0, v0, C0, F0))
        st = [t.to(dtype) for t in (vol, rho, clip)]
        with torch.set_grad_enabled(grad):
            for _ in range(S):
                x, v, C, F = om.step(const, st[0], st[1], st[2], en, x, v, C, F, e(F))
                F = p(F)
            loss = (x * wx.to(dtype)).sum() + (v * wv.to(dtype)).sum()
            if grad:
                loss.backward()
        return x, v, C, F, loss, (e.log_E.grad if grad else None)

    x, v, C, F, loss, g64 = path(torch.float64, grad=True)
    x32, v32, C32, F32, loss32, g32 = path(torch.float32, grad=True)
    h = 1e-4
    fd = (path(torch.float64, +h)[4] - path(torch.float64, -h)[4]) / (2 * h)
    fd2 = (path(torch.float64, +2 * h)[4] - path(torch.float64, -2 * h)[4]) / (4 * h)      # |fd - fd2| / 3 estimates fd's own error
    rec = dict(x0=x0, v0=v0, C0=C0, F0=F0, vol=vol, rho=rho, clip_bound=clip, enabled=en, wx=wx, wv=wv,
               x=x, v=v, C=C, F=F, loss=loss, x_f32=x32, v_f32=v32, C_f32=C32, F_f32=F32, loss_f32=loss32,
               dL_dlogE=g64, dL_dlogE_f32=g32, dL_dlogE_fd=fd, dL_dlogE_fd2=fd2, substeps=np.int32(S), num_grids=np.int32(32), dt=np.float64(1e-3),
               eps=np.float64(6e-7))
    rec = {k: (t.detach().double().numpy() if torch.is_tensor(t) and t.dtype.is_floating_point else (t.numpy() if torch.is_tensor(t) else t))
           for k, t in rec.items()}
    for k, val in list(e_cfg.items()) + [("p_" + k, val) for k, val in p_cfg.items()]:
        if k not in ("random", "p_random"):
            rec["cfg_" + k] = np.float64(val)
    print(f"  rollout {tag}: loss {float(loss.detach()):.6f} dL/dlogE autograd {float(g64):.6e} fd {float(fd):.6e} fd(2h) {float(fd2):.6e} fp32 {float(g32):.6e}")
    # torch.linalg.svd's adjoint (the generator's stand-in for the reference's Warp SVD) is NaN along this path for the
    # Drucker-Prager pair; the central difference of the same fp64 path is the stored gradient then
    rec["has_autograd"] = np.int32(np.isfinite(rec["dL_dlogE"]).all() and np.isfinite(rec["dL_dlogE_f32"]).all())
    if not rec["has_autograd"]:
        del rec["dL_dlogE"], rec["dL_dlogE_f32"]
    assert all(np.isfinite(a).all() for a in rec.values())
    np.savez_compressed(OUT / "classical" / f"rollout_{tag}.npz", **rec)


def main():
    DictConfig = G.install_stubs()
    sys.path.insert(0, str(REF))
    sys.path.insert(0, str(HERE.parent.parent))
    import modules.nclaw.material as material  # noqa: the reference package
    from oracle import mpm as om
    torch.set_num_threads(1)
    (OUT / "classical").mkdir(parents=True, exist_ok=True)
    el = dict(E=E0, nu=NU0, random=False)
    law_case(material, DictConfig, "corotated", "CorotatedElasticity", "elastic", el, 11, 0.08)
    law_case(material, DictConfig, "stvk", "StVKElasticity", "elastic", el, 12, 0.08)
    law_case(material, DictConfig, "volume_ziran", "VolumeElasticity", "elastic", dict(el, mode="ziran"), 13, 0.08)
    law_case(material, DictConfig, "volume_taichi", "VolumeElasticity", "elastic", dict(el, mode="taichi"), 14, 0.08)
    law_case(material, DictConfig, "sigma", "SigmaElasticity", "elastic", el, 15, 0.08, reflect=False, nan_rows=True)
    law_case(material, DictConfig, "identity", "IdentityPlasticity", "elastic", {}, 16, 0.08)
    law_case(material, DictConfig, "sigma_plastic", "SigmaPlasticity", "elastic", {}, 17, 0.08, reflect=False, nan_rows=True)
    # sigma_y / (2 mu) = 0.156: about the median |dev log sigma| at spread 0.08 (5e3 would make 67 of 68 rows yield)
    law_case(material, DictConfig, "von_mises", "VonMisesPlasticity", "von_mises", dict(el, sigma_y=1.2e4), 18, 0.08)
    # a volumetric factor exp(0.06 N(0,1)) puts rows on both sides of tr log sigma = 3 cohesion
    law_case(material, DictConfig, "drucker_prager", "DruckerPragerPlasticity", "drucker_prager",
             dict(el, friction_angle=25.0, cohesion=0.0), 19, 0.08, vol=0.06)
    law_case(material, DictConfig, "drucker_prager_cohesion", "DruckerPragerPlasticity", "drucker_prager",
             dict(el, friction_angle=25.0, cohesion=0.02), 20, 0.08, vol=0.06)
    rollout_case(material, DictConfig, om, "corotated_identity", "CorotatedElasticity", el, "IdentityPlasticity", {}, 31)
    rollout_case(material, DictConfig, om, "sigma_drucker_prager", "SigmaElasticity", el, "DruckerPragerPlasticity",
                 dict(el, friction_angle=25.0, cohesion=0.05), 32, f_scale=0.9)
    print("done")


if __name__ == "__main__":
    main()
