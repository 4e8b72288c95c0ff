"""GPU parity of the classical constitutive laws (material/classical.py on csrc/nm_classical.hip) against the reference's own
classes run in fp64 (tests/golden/classical/*.npz, gen_classical_golden.py).

Bounds.  Every compared array is held to 4 x the error of the reference class's OWN fp32 run against its fp64 run (both stored
in the fixture), with a floor of the relative 1e-6 the neural stress is held to; errors are relative to the fp64 array's largest
magnitude.  The factor 4 covers a different SVD algorithm and summation order at the same precision.  The scalar gradients are
compared as one array {d/d log_E, d/d p2} (d/d log_E of Drucker-Prager is zero analytically: (3 la + 2 mu) / (2 mu) does not
depend on E).  Every stored row is compared: the generator already rejected rows that sit on a switch.
Measured values: profiles/classical_parity_table.md.
"""
import numpy as np
import pytest
import torch

from gpu_util import dev, measured, build_model, build_statics
from test_classical_cpu import CASES, fixture_cfg

pytestmark = pytest.mark.gpu

FLOOR, FACTOR = 1e-6, 4.0


class _Arrays(dict):
    files = property(lambda self: list(self))


def rel(a, ref):
    ref = np.asarray(ref, dtype=np.float64)
    a = a.detach().double().cpu().numpy() if torch.is_tensor(a) else np.asarray(a, dtype=np.float64)
    return float(np.abs(a - ref).max() / max(float(np.abs(ref).max()), 1e-300))


def scalar(a):
    return float(np.asarray(a, dtype=np.float64).reshape(-1)[0])


def bound(d, key):
    return max(FACTOR * rel(d[key + "_f32"], d[key]), FLOOR)


def make(tag, d):
    import neuma_amd.material as m
    return getattr(m, CASES[tag])(fixture_cfg(d)).to(dev())


def run_law(tag, d):
    mod = make(tag, d)
    F = torch.tensor(d["F"], dtype=torch.float32, device=dev(), requires_grad=True)
    out = mod(F)
    (out * torch.tensor(d["grad_out"], dtype=torch.float32, device=dev())).sum().backward()
    params = [p for p in (getattr(mod, n, None) for n in ("log_E", "sigma_y", "friction_angle")) if isinstance(p, torch.nn.Parameter)]
    gs = torch.cat([p.grad for p in params]) if params else torch.zeros(0)
    return out.detach(), F.grad, gs


@pytest.mark.parametrize("tag", sorted(CASES))
def test_forward_and_gradients_against_the_fp64_reference(golden_dir, tag):
    d = np.load(golden_dir / "classical" / f"{tag}.npz", allow_pickle=False)
    out, gF, gs = run_law(tag, d)
    assert out.shape == (68, 3, 3) and bool(torch.isfinite(out).all()) and bool(torch.isfinite(gF).all())
    for name in ("mask_yield", "mask_moved"):
        if name in d.files:
            k = int(d[name].sum())
            print(f"{tag}: {name} {k} / 68")
            assert name == "mask_moved" or 17 <= k <= 51          # each side of the law's switch holds a quarter of the rows
    e_out, e_gF = rel(out, d["out"]), rel(gF, d["grad_F"])
    print(f"CLASSICAL {tag} out {e_out:.3e} bound {bound(d, 'out'):.3e} | grad_F {e_gF:.3e} bound {bound(d, 'grad_F'):.3e}")
    if d["grad_scalars"].size:
        e_gs = rel(gs, d["grad_scalars"])
        print(f"CLASSICAL {tag} grad_scalars {e_gs:.3e} bound {bound(d, 'grad_scalars'):.3e} values {gs.cpu().numpy()} ref {d['grad_scalars']}")
    assert measured(e_out, f"{tag} out (rel)") <= bound(d, "out")
    assert measured(e_gF, f"{tag} grad_F (rel)") <= bound(d, "grad_F")
    if d["grad_scalars"].size:
        assert measured(e_gs, f"{tag} grad_scalars (rel)") <= bound(d, "grad_scalars")


@pytest.mark.parametrize("tag", ["sigma", "sigma_plastic"])
def test_nan_in_the_reference_is_nan_here(golden_dir, tag):
    d = np.load(golden_dir / "classical" / f"{tag}.npz", allow_pickle=False)
    with torch.no_grad():
        out = make(tag, d)(torch.tensor(d["F_nan"], dtype=torch.float32, device=dev())).cpu().numpy()
    assert out.shape == (2, 3, 3) and np.array_equal(np.isnan(out), np.isnan(d["out_nan"]))
    finite = ~np.isnan(d["out_nan"])
    assert np.array_equal(out[finite], d["out_nan"][finite].astype(np.float32))       # (the exact zeros off the diagonal)


@pytest.mark.parametrize("tag", sorted(t for t in CASES if t != "identity"))
def test_two_backward_calls_give_identical_bits(golden_dir, tag):
    d = np.load(golden_dir / "classical" / f"{tag}.npz", allow_pickle=False)
    big = _Arrays({k: (np.tile(d[k], (300, 1, 1)) if k in ("F", "grad_out") else d[k]) for k in d.files})      # 20 400 rows: 80 blocks
    a, b = run_law(tag, big), run_law(tag, big)
    for x, y in zip(a, b):
        assert torch.equal(x.cpu(), y.cpu())


def test_compose_material_mixes_classical_and_neural_sections():
    import neuma_amd.material as m
    from test_classical_cpu import NET
    torch.manual_seed(0)
    el = dict(E=1e5, nu=0.3, random=False)
    mods = [m.CorotatedElasticity(el), m.InvariantFullMetaElasticity(NET), m.StVKElasticity(el), m.SigmaElasticity(el)]
    sections = [40, 30, 0, 25]                                               # an empty section is skipped
    F = (torch.eye(3)[None] + 0.05 * torch.randn(sum(sections), 3, 3)).to(dev())
    comp = m.ComposeMaterial(mods, sections).to(dev())
    with torch.no_grad():
        whole = comp(F)
        parts = [mod(f) for mod, f in zip(comp.materials, torch.split(F, sections)) if f.numel()]
    assert whole.shape == F.shape and torch.equal(whole, torch.cat(parts))
    Fg = F.clone().requires_grad_(True)
    comp(Fg).square().sum().backward()
    assert bool(torch.isfinite(Fg.grad).all()) and mods[0].log_E.grad is not None and mods[2].log_E.grad is None


ROLLOUTS = {"corotated_identity": ("CorotatedElasticity", "IdentityPlasticity"),
            "sigma_drucker_prager": ("SigmaElasticity", "DruckerPragerPlasticity")}


def rollout_setup(d, tag):
    import neuma_amd.material as m
    from oracle import mpm as om
    const = om.MPMConstant(num_grids=int(d["num_grids"]), dt=float(d["dt"]), bound=1, gravity=(0.0, -9.8, 0.0), eps=float(d["eps"]), bc="noslip")
    model = build_model(const, dev())
    st = build_statics(model, torch.tensor(d["vol"]), torch.tensor(d["rho"]), torch.tensor(d["clip_bound"]), torch.tensor(d["enabled"]), dev())
    e_name, p_name = ROLLOUTS[tag]
    e = getattr(m, e_name)(dict(E=float(d["cfg_E"]), nu=float(d["cfg_nu"]), random=False)).to(dev())
    pc = {k[len("cfg_p_"):]: float(d[k]) for k in d.files if k.startswith("cfg_p_")}
    p = getattr(m, p_name)(dict(pc, random=False) if pc else None).to(dev())
    init = [torch.tensor(d[k], dtype=torch.float32, device=dev()) for k in ("x0", "v0", "C0", "F0")]
    return model, st, e, p, init


@pytest.mark.parametrize("tag", sorted(ROLLOUTS))
def test_rollout_through_the_forward_sim(golden_dir, tag):
    from neuma_amd.sim import MPMForwardSim
    d = np.load(golden_dir / "classical" / f"rollout_{tag}.npz", allow_pickle=False)
    model, st, e, p, (x, v, C, F) = rollout_setup(d, tag)
    sim = MPMForwardSim(model)
    with torch.no_grad():
        state = model.state(x.shape[0])
        state.from_torch(x=x, v=v, C=C, F=F, stress=torch.zeros_like(F))
        for _ in range(int(d["substeps"])):
            state.from_torch(stress=e(F))
            x, v, C, F = sim(st, state)
            F = p(F)
            state.from_torch(F=F)
    for k, t in (("x", x), ("v", v), ("C", C), ("F", F)):
        err = rel(t, d[k])
        print(f"CLASSICAL rollout {tag} forward-sim {k} {err:.3e} bound {bound(d, k):.3e}")
        assert measured(err, f"rollout {tag} {k} (rel)") <= bound(d, k)


@pytest.mark.parametrize("tag", sorted(ROLLOUTS))
def test_rollout_through_the_cached_diff_sim_with_a_gradient_to_log_E(golden_dir, tag):
    """dL/d log_E against the central difference of the generator's own fp64 path.  Bound: the central difference's own error
    (|fd(h) - fd(2h)| / 3) plus 4 x the reference's fp32-autograd error where the generator's path has one (floor 1e-6); the
    Drucker-Prager pair has none (torch's SVD adjoint is NaN along it), so it takes the corotated pair's fp32 yardstick."""
    from neuma_amd.sim import MPMCacheDiffSim
    d = np.load(golden_dir / "classical" / f"rollout_{tag}.npz", allow_pickle=False)
    y = np.load(golden_dir / "classical" / "rollout_corotated_identity.npz", allow_pickle=False)
    model, st, e, p, (x, v, C, F) = rollout_setup(d, tag)
    S = int(d["substeps"])
    sim = MPMCacheDiffSim(model, S)
    for s in range(S):
        x, v, C, F = sim(st, s, x, v, C, F, e(F))
        F = p(F)
    for k, t in (("x", x), ("v", v), ("C", C), ("F", F)):
        assert measured(rel(t, d[k]), f"cached rollout {tag} {k} (rel)") <= bound(d, k)
    wx, wv = (torch.tensor(d[k], dtype=torch.float32, device=dev()) for k in ("wx", "wv"))
    ((x * wx).sum() + (v * wv).sum()).backward()
    g, fd = float(e.log_E.grad), scalar(d["dL_dlogE_fd"])
    fd_err = abs(fd - scalar(d["dL_dlogE_fd2"])) / 3 / abs(fd)
    yard = max(FACTOR * abs(scalar(y["dL_dlogE_f32"]) - scalar(y["dL_dlogE"])) / abs(scalar(y["dL_dlogE"])), FLOOR)
    err = abs(g - fd) / abs(fd)
    print(f"CLASSICAL rollout {tag} dL/dlogE {g:.6e} fd {fd:.6e} err {err:.3e} bound {fd_err + yard:.3e} (fd error {fd_err:.3e}, fp32 yardstick {yard:.3e})")
    assert measured(err, f"rollout {tag} dL/dlogE vs central difference (rel)") <= fd_err + yard


def test_inference_entry_point_with_a_classical_object(tmp_path):
    """The tiny demo layout of test_gpu_entrypoints with `name: CorotatedElasticity` / `name: IdentityPlasticity` for one object:
    return code 0 and frames written; the YAML without `name` builds the neural pair from the checkpoint, as before the key."""
    import yaml
    from neuma_amd.config import load_config
    from neuma_amd.inference import load_object, main as inference_main
    import neuma_amd.material as m
    from test_gpu_entrypoints import _write_experiment
    path, _ = _write_experiment(tmp_path, frames=1)
    base = yaml.safe_load(path.read_text())
    raw, assets = tmp_path / "raw", tmp_path / "assets"

    def obj(constitution):
        return dict(sim_data_name="tinyball", pretrained_ckpt=str(raw / "jelly_0300.pt"), gaussian=dict(sh_degree=3),
                    particle_data=dict(shape=dict(asset_root=None, sort=None, ori_bounds=[[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]],
                                                  sim_bounds=[[0.25, 0.3, 0.25], [0.75, 0.8, 0.75]]),
                                       vel=dict(lin_vel=[0.0, -0.5, 0.0], ang_vel=[0.0, 0.0, 0.0]), rho=1000.0, clip_bound=0.1),
                    constitution=dict(constitution, views=["r_0"]))

    def cfg(constitution):
        return dict(gpu=0, seed=42, debug=True, debug_views=["r_0"], resume=False, overwrite=False, denormalize=False, assets_root=str(assets),
                    video_data=dict(base["video_data"], data=dict(base["video_data"]["data"], init_frame=0, used_views=["r_0"])),
                    sim=dict(base["sim"], num_grids=32, eps=6e-7), objects=[obj(constitution)])

    neural = dict(elasticity=base["constitution"]["elasticity"], plasticity=base["constitution"]["plasticity"])
    classical = dict(elasticity=dict(name="CorotatedElasticity", E=1e5, nu=0.3, random=False), plasticity=dict(name="IdentityPlasticity"))
    steps = 6
    for tag, con in (("classical", classical), ("neural", neural)):
        (tmp_path / f"{tag}.yaml").write_text(yaml.safe_dump(cfg(con), sort_keys=False))
        rc = inference_main(["-c", str(tmp_path / f"{tag}.yaml"), "-s", str(steps), "-vn", tag, "-dv", "r_0", "-sp", tag,
                             "--result_root", str(tmp_path / "results")])
        assert not rc
        imgs = sorted(f.name for f in (tmp_path / "results" / "inference" / f"images_{tag}").glob("*.png"))
        assert imgs == [f"r_0_{i:03d}.png" for i in range(steps + 1)]
    o = load_object(load_config(tmp_path / "classical.yaml").objects[0], assets, steps, dev())
    assert type(o.elasticity) is m.CorotatedElasticity and type(o.plasticity) is m.IdentityPlasticity
    o = load_object(load_config(tmp_path / "neural.yaml").objects[0], assets, steps, dev())
    assert type(o.elasticity) is m.InvariantFullMetaElasticity and type(o.plasticity) is m.InvariantFullMetaPlasticity
    ck = torch.load(raw / "jelly_0300.pt")
    assert torch.equal(o.elasticity.layers[0].fc.weight.cpu(), ck["elasticity"]["layers.0.fc.weight"])
    from neuma_amd import io as nio
    xa = nio.load_particles_ply(tmp_path / "results" / "inference_states" / "states_classical" / f"{steps:03d}.ply")
    xb = nio.load_particles_ply(tmp_path / "results" / "inference_states" / "states_neural" / f"{steps:03d}.ply")
    assert np.isfinite(xa).all() and xa.shape == xb.shape and np.abs(xa - xb).max() > 0
