"""CPU: trajectory files, the state-folder reader and the checkpoint format of constitutive pretraining."""
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
NET_CFG = dict(layer_widths=[64, 64], norm=None, nonlinearity="gelu", no_bias=True, normalize_input=True, alpha=1e-3)
META = dict(num_grids=16, dt=1e-3, bound=1, gravity=[0.0, -9.8, 0.0], bc="freeslip", eps=6e-7, substeps=10, rho=1000.0, clip_bound=0.1)


def make(T=3, N=5, v=True, cf=True, mask=True, seed=0):
    from neuma_amd.trajectory import Trajectory
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)      # noqa: E731
    return Trajectory(r(T + 1, N, 3), r(T + 1, N, 3) if v else None, r(T + 1, N, 3, 3) if cf else None, r(T + 1, N, 3, 3) if cf else None,
                      (r(N) < 0.5) if mask else None, META)


class FakeModel(object):
    """what Trajectory.check_against reads of an MPMModel"""

    def __init__(self, **over):
        from types import SimpleNamespace
        m = dict(META, **over)
        self.constant = SimpleNamespace(num_grids=m["num_grids"], dt=m["dt"], bound=m["bound"], gravity=np.array(m["gravity"], np.float32),
                                        eps=m["eps"])
        self.bc = m["bc"]


@pytest.mark.parametrize("v,cf,mask", [(True, True, True), (False, False, False), (True, False, True)])
def test_save_load_round_trip(tmp_path, v, cf, mask):
    from neuma_amd.trajectory import Trajectory
    t = make(v=v, cf=cf, mask=mask)
    t.save(tmp_path / "t.pt")
    raw = torch.load(tmp_path / "t.pt", map_location="cpu")
    assert set(raw) == {"x", "v", "C", "F", "mask", "meta"} and raw["x"].dtype == torch.float32 and not raw["x"].is_cuda
    assert all(not isinstance(val, (torch.Tensor, np.ndarray)) for val in raw["meta"].values())
    u = Trajectory.load(tmp_path / "t.pt")
    assert (u.num_frames, u.num_particles) == (3, 5) and u.meta == t.meta
    for k in ("x", "v", "C", "F"):
        a, b = getattr(t, k), getattr(u, k)
        assert (a is None and b is None) or torch.equal(a, b)
    assert (u.mask is None) if not mask else torch.equal(u.mask != 0, t.mask != 0)


def test_load_refuses_inconsistent_shapes(tmp_path):
    from neuma_amd.trajectory import Trajectory, TrajectoryError
    good = make()
    for key, bad in (("v", torch.zeros(4, 6, 3)), ("C", torch.zeros(3, 5, 3, 3)), ("mask", torch.zeros(4, dtype=torch.uint8)),
                     ("x", torch.zeros(4, 5, 2)), ("F", None)):
        d = dict(x=good.x, v=good.v, C=good.C, F=good.F, mask=good.mask.to(torch.uint8), meta=good.meta)
        d[key] = bad
        torch.save(d, tmp_path / "bad.pt")
        with pytest.raises(TrajectoryError):
            Trajectory.load(tmp_path / "bad.pt")


def test_check_against_names_the_mismatching_key():
    from neuma_amd.trajectory import TrajectoryError
    t = make()
    t.check_against(FakeModel(), substeps=10)
    for key, val in (("num_grids", 32), ("dt", 2e-3), ("bound", 2), ("gravity", [0.0, 0.0, -9.8]), ("bc", "noslip"), ("eps", 1e-5)):
        with pytest.raises(TrajectoryError, match=f"'{key}'"):
            t.check_against(FakeModel(**{key: val}), substeps=10)
    with pytest.raises(TrajectoryError, match="'substeps'"):
        t.check_against(FakeModel(), substeps=20)
    from types import SimpleNamespace
    with pytest.raises(TrajectoryError, match="'rho'"):
        t.check_against(FakeModel(), 10, SimpleNamespace(rho=torch.full((5,), 500.0), clip_bound=torch.full((5,), 0.1)))


def test_teacher_forcing_without_C_and_F_raises():
    from neuma_amd.pretrain import epoch_loss
    from neuma_amd.trajectory import TrajectoryError
    t = make(cf=False)
    assert not t.can_teacher_force
    with pytest.raises(TrajectoryError, match="C, F"):
        t.forcing_state(1)
    with pytest.raises(TrajectoryError):            # the loop refuses before it simulates anything
        epoch_loss(None, t, 3, teacher_steps=1)
    full = make()
    x, v, C, F = full.forcing_state(2)
    assert torch.equal(x, full.x[2]) and x.data_ptr() != full.x[2].data_ptr() and not x.requires_grad


def test_from_state_folder_reads_saved_clouds(tmp_path):
    from neuma_amd import io as nio
    from neuma_amd.trajectory import Trajectory, TrajectoryError
    rng = np.random.default_rng(0)
    clouds = {s: rng.random((7, 3)).astype(np.float32) for s in (3, 4, 5, 10)}
    for s, c in clouds.items():
        nio.save_particles_ply(tmp_path / f"{s:03d}.ply", c)
    nio.save_particles_ply(tmp_path / "kernels.ply", rng.random((2, 3)))          # not a frame: ignored
    t = Trajectory.from_state_folder(tmp_path, meta=dict(substeps=10))
    assert t.v is None and t.C is None and t.F is None and t.num_frames == 3 and t.meta["substeps"] == 10
    for i, s in enumerate(sorted(clouds)):
        assert np.array_equal(t.x[i].numpy(), clouds[s])
    nio.save_particles_ply(tmp_path / "011.ply", rng.random((6, 3)))
    with pytest.raises(TrajectoryError):
        Trajectory.from_state_folder(tmp_path)


def test_neural_checkpoint_has_the_key_set_of_the_shipped_base_models(tmp_path):
    from neuma_amd.material import InvariantFullMetaElasticity, InvariantFullMetaPlasticity
    from neuma_amd.pretrain import checkpoints, load_checkpoint, save_checkpoint
    E, P = InvariantFullMetaElasticity(NET_CFG), InvariantFullMetaPlasticity(NET_CFG)
    save_checkpoint(tmp_path / "0007.pt", E, P, 0.25)
    (tmp_path / "trajectory.pt").write_bytes(b"")
    assert [p.name for p in checkpoints(tmp_path)] == ["0007.pt"]
    ck = torch.load(tmp_path / "0007.pt", map_location="cpu")
    assert set(ck) == {"elasticity", "plasticity", "loss"} and ck["loss"] == 0.25
    names = ("layers.0.fc.weight", "layers.1.fc.weight", "final_layer.fc.weight")
    base = np.load(ROOT / "neuma_amd" / "data" / "base_models.npz")
    materials = sorted({k.split("_")[0] for k in base.files})
    assert materials == ["jelly", "plasticine", "sand"]
    for mat in materials:
        for tag, key in (("e", "elasticity"), ("p", "plasticity")):
            assert list(ck[key]) == list(names)
            for i, nm in enumerate(names):
                assert tuple(ck[key][nm].shape) == base[f"{mat}_{tag}_w{i}"].shape
    E2, P2 = InvariantFullMetaElasticity(NET_CFG), InvariantFullMetaPlasticity(NET_CFG)
    E2.load_state_dict(ck["elasticity"], strict=True)           # the two lines of finetune.setup
    P2.load_state_dict(ck["plasticity"], strict=True)
    assert all(torch.equal(a, b) for a, b in zip(E.state_dict().values(), E2.state_dict().values()))
    load_checkpoint(tmp_path / "0007.pt", E2, P2)


def test_fused_with_a_classical_module_raises():
    from neuma_amd.material import CorotatedElasticity, IdentityPlasticity
    from neuma_amd.pretrain import FrameStepper
    with pytest.raises(ValueError, match="fused"):
        FrameStepper(None, None, CorotatedElasticity(dict(E=1e5, nu=0.3)), IdentityPlasticity(None), 10, 3, fused="true")
