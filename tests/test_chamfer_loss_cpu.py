"""CPU: the Chamfer loss's numpy fp64 statement (extras/chamfer_loss.py) and its torch composition (chamfer_loss_torch) against
torch fp64 autograd of the brute-force composition; point-cloud observations (CloudTrajectory, load_observations); the loss-kind
checks of pretrain; and the host-side argument checks of nm_chamfer_loss on the loaded library."""
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
META = dict(num_grids=16, dt=1e-3, bound=1, gravity=[0.0, -9.8, 0.0], bc="freeslip", eps=6e-7, substeps=10, rho=1000.0, clip_bound=0.1)
SIZES = [(1, 1), (1, 7), (7, 1), (50, 80)]
WEIGHTS = [(1.0, 1.0), (1.0, 0.0), (0.0, 1.0)]


def clouds(n, m, seed=0):
    rng = np.random.default_rng(1000 * n + m + seed)
    return rng, 0.1 + 0.8 * rng.random((n, 3)), 0.1 + 0.8 * rng.random((m, 3))


def mask_of(n, rng, masked):
    if not masked:
        return None
    mask = (rng.random(n) < 0.7).astype(np.uint8)
    mask[n // 2] = 1                      # at least one kept row
    return mask


def autograd_fp64(x, y, mask, wxy, wyx):
    """torch fp64 autograd through gather of the brute-force assignments: (loss, grad)"""
    tx = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    ty = torch.tensor(y, dtype=torch.float64)
    rows = torch.arange(x.shape[0]) if mask is None else torch.nonzero(torch.tensor(mask) != 0).reshape(-1)
    xk = tx[rows]
    d = (xk.detach()[:, None, :] - ty[None, :, :]).pow(2).sum(2)
    a, b = d.argmin(1), d.argmin(0)
    loss = wxy * (xk - ty[a]).pow(2).sum(1).mean() + wyx * (ty - xk[b]).pow(2).sum(1).mean()
    loss.backward()
    return float(loss.detach()), tx.grad.numpy()


def close(got, ref, tol=1e-12):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max()) <= tol * max(float(np.abs(ref).max()), 1e-300)


@pytest.mark.parametrize("wxy,wyx", WEIGHTS)
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n,m", SIZES)
def test_numpy_reference_equals_torch_fp64_autograd(n, m, masked, wxy, wyx):
    from neuma_amd.extras.chamfer_loss import chamfer_loss_reference
    rng, x, y = clouds(n, m)
    mask = mask_of(n, rng, masked)
    loss, grad = autograd_fp64(x, y, mask, wxy, wyx)
    ref = chamfer_loss_reference(x, y, mask, wxy, wyx)
    assert close(ref["loss"], loss) and close(ref["grad"], grad)
    assert close(wxy * ref["term_xy"] + wyx * ref["term_yx"], loss)
    if mask is not None:
        assert not ref["grad"][mask == 0].any() and (ref["idx_xy"][mask == 0] == -1).all() and (mask[ref["idx_yx"]] != 0).all()
    # given indices: the formulas for exactly those assignments
    again = chamfer_loss_reference(x, y, mask, wxy, wyx, idx_xy=ref["idx_xy"], idx_yx=ref["idx_yx"])
    assert again["loss"] == ref["loss"] and np.array_equal(again["grad"], ref["grad"])
    assert (ref["abs_sum"] >= np.abs(ref["grad"]) * (1 - 1e-12)).all()


@pytest.mark.parametrize("wxy,wyx", WEIGHTS)
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n,m", SIZES)
def test_torch_composition_equals_torch_fp64_autograd(n, m, masked, wxy, wyx):
    from neuma_amd.chamfer_loss import chamfer_loss_torch
    from neuma_amd.extras.chamfer_loss import chamfer_loss_reference
    rng, x, y = clouds(n, m)
    mask = mask_of(n, rng, masked)
    loss, grad = autograd_fp64(x, y, mask, wxy, wyx)
    tx = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    got, ixy, iyx = chamfer_loss_torch(tx, torch.tensor(y), None if mask is None else torch.tensor(mask), wxy, wyx, give_id=True)
    got.backward()
    assert close(float(got.detach()), loss) and close(tx.grad.numpy(), grad)
    ref = chamfer_loss_reference(x, y, mask, wxy, wyx)
    assert np.array_equal(ixy.numpy(), ref["idx_xy"]) and np.array_equal(iyx.numpy(), ref["idx_yx"])


def test_ties_take_the_lowest_index_and_an_empty_mask_gives_zero():
    from neuma_amd.chamfer_loss import chamfer_loss_torch
    from neuma_amd.extras.chamfer_loss import chamfer_loss_reference
    x = np.array([[0.5, 0.5, 0.5], [0.5, 0.5, 0.5], [0.25, 0.5, 0.5]])          # rows 0 and 1 coincide
    y = np.array([[0.5, 0.5, 0.75], [0.5, 0.5, 0.25], [0.5, 0.5, 0.5]])          # y0, y1 equally far from x0
    ref = chamfer_loss_reference(x, y)
    assert list(ref["idx_yx"]) == [0, 0, 0] and list(ref["idx_xy"]) == [2, 2, 2]
    _, ixy, iyx = chamfer_loss_torch(torch.tensor(x), torch.tensor(y), give_id=True)
    assert list(iyx) == [0, 0, 0] and list(ixy) == [2, 2, 2]
    none = np.zeros(3, np.uint8)
    ref = chamfer_loss_reference(x, y, none)
    assert ref["loss"] == 0.0 and not ref["grad"].any() and (ref["idx_xy"] == -1).all() and (ref["idx_yx"] == -1).all()
    tx = torch.tensor(x, requires_grad=True)
    loss = chamfer_loss_torch(tx, torch.tensor(y), torch.tensor(none))
    loss.backward()
    assert float(loss) == 0.0 and not bool(tx.grad.any())


def test_cpu_tensor_is_rejected_by_the_native_operator():
    from neuma_amd import NeumaHipError
    from neuma_amd.chamfer_loss import chamfer_loss, chamfer_loss_raw
    with pytest.raises(NeumaHipError):
        chamfer_loss(torch.zeros(4, 3), torch.zeros(5, 3))
    with pytest.raises(NeumaHipError):
        chamfer_loss_raw(torch.zeros(4, 3), torch.zeros(5, 3))


# ---------------------------------------------------------------- observations

def make_clouds(sizes=(4, 9, 6), n=5, full=True, mask=True, seed=0):
    from neuma_amd.trajectory import CloudTrajectory
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)      # noqa: E731
    return CloudTrajectory(r(n, 3), [r(m, 3) for m in sizes], r(n, 3) if full else None, r(n, 3, 3) if full else None,
                           r(n, 3, 3) if full else None, (r(n) < 0.5) if mask else None, META)


def test_cloud_trajectory_offers_what_the_epoch_loop_touches():
    from neuma_amd.trajectory import TrajectoryError
    t = make_clouds()
    assert (t.num_frames, t.num_particles) == (3, 5) and t.v is None and not t.can_teacher_force
    assert t.x[0] is t.x0 and [t.x[f].shape[0] for f in (1, 2, 3)] == [4, 9, 6] and len(t.x) == 4
    with pytest.raises(IndexError):
        t.x[4]
    x, v, C, F = t.frame(0)
    assert x is t.x0 and v is t.v0 and C is t.C0 and F is t.F0
    assert make_clouds(full=False).frame(0)[1:] == (None, None, None)
    with pytest.raises(TrajectoryError, match="teacher"):
        t.forcing_state(0)
    u = t.to("cpu")
    assert torch.equal(u.x[2], t.x[2]) and u.meta == t.meta


def test_cloud_trajectory_validation_errors():
    from neuma_amd.trajectory import CloudTrajectory, TrajectoryError
    x0, c = torch.zeros(5, 3), [torch.zeros(4, 3)]
    for args, kw in (((torch.zeros(5, 2), c), {}), ((torch.zeros(0, 3), c), {}), ((x0, []), {}), ((x0, torch.zeros(2, 4, 3)), {}),
                     ((x0, [torch.zeros(0, 3)]), {}), ((x0, [torch.zeros(4, 2)]), {}), ((x0, [np.zeros((4, 3))]), {}),
                     ((x0, c), dict(v0=torch.zeros(4, 3))), ((x0, c), dict(C0=torch.zeros(5, 3))), ((x0, c), dict(F0=torch.zeros(5, 9))),
                     ((x0, c), dict(mask=torch.zeros(6)))):
        with pytest.raises(TrajectoryError):
            CloudTrajectory(*args, **kw)


def test_check_against_names_the_mismatching_key():
    from test_pretrain_cpu import FakeModel
    from neuma_amd.trajectory import TrajectoryError
    t = make_clouds()
    t.check_against(FakeModel(), substeps=10)
    with pytest.raises(TrajectoryError, match="'num_grids'"):
        t.check_against(FakeModel(num_grids=32), substeps=10)
    with pytest.raises(TrajectoryError, match="'substeps'"):
        t.check_against(FakeModel(), substeps=20)


@pytest.mark.parametrize("full,mask", [(True, True), (False, False)])
def test_ragged_save_load_round_trip_and_dispatch(tmp_path, full, mask):
    from test_pretrain_cpu import make
    from neuma_amd.trajectory import CloudTrajectory, Trajectory, TrajectoryError, load_observations
    t = make_clouds(full=full, mask=mask)
    t.save(tmp_path / "obs.pt")
    raw = torch.load(tmp_path / "obs.pt", map_location="cpu")
    assert set(raw) == {"x0", "clouds", "v0", "C0", "F0", "mask", "meta"} and [c.shape[0] for c in raw["clouds"]] == [4, 9, 6]
    u = CloudTrajectory.load(tmp_path / "obs.pt")
    assert u.num_frames == 3 and u.meta == t.meta and all(torch.equal(a, b) for a, b in zip(u.clouds, t.clouds))
    for k in ("x0", "v0", "C0", "F0"):
        a, b = getattr(t, k), getattr(u, k)
        assert (a is None and b is None) or torch.equal(a, b)
    assert (u.mask is None) if not mask else torch.equal(u.mask != 0, t.mask != 0)
    with pytest.raises(TrajectoryError, match="not a trajectory file"):          # Trajectory.load's own message
        Trajectory.load(tmp_path / "obs.pt")
    make().save(tmp_path / "traj.pt")
    with pytest.raises(TrajectoryError):
        CloudTrajectory.load(tmp_path / "traj.pt")
    assert isinstance(load_observations(tmp_path / "obs.pt"), CloudTrajectory)
    assert type(load_observations(tmp_path / "traj.pt")) is Trajectory


def test_from_state_folder_takes_clouds_of_differing_sizes(tmp_path):
    from neuma_amd import io as nio
    from neuma_amd.trajectory import CloudTrajectory, Trajectory, TrajectoryError, load_observations
    rng = np.random.default_rng(0)
    obs = {f: rng.random((m, 3)).astype(np.float32) for f, m in ((0, 3), (1, 7), (2, 4), (3, 9))}
    for f, c in obs.items():
        nio.save_particles_ply(tmp_path / f"{f:03d}.ply", c)
    nio.save_particles_ply(tmp_path / "kernels.ply", rng.random((2, 3)))          # not a frame: ignored
    x0 = torch.rand(5, 3)
    t = CloudTrajectory.from_state_folder(tmp_path, x0, meta=dict(substeps=10))
    assert t.num_frames == 3 and t.num_particles == 5 and t.x[0] is x0 and t.meta["substeps"] == 10
    for f in (1, 2, 3):
        assert np.array_equal(t.x[f].numpy(), obs[f])                              # (the frame-0 file is not used)
    with pytest.raises(TrajectoryError, match="3 particles|7 particles"):          # the ordered reader still refuses them
        Trajectory.from_state_folder(tmp_path)
    assert isinstance(load_observations(tmp_path, x0=x0), CloudTrajectory)
    (tmp_path / "002.ply").unlink()
    with pytest.raises(TrajectoryError, match="frame 2"):
        CloudTrajectory.from_state_folder(tmp_path, x0)
    only0 = tmp_path / "only0"
    only0.mkdir()
    nio.save_particles_ply(only0 / "000.ply", obs[0])
    with pytest.raises(TrajectoryError):
        CloudTrajectory.from_state_folder(only0, x0)


# ---------------------------------------------------------------- pretrain: what does not go together raises before device work

def test_loss_kind_and_observation_kind_mismatches_raise_before_any_device_work(tmp_path):
    from test_pretrain_cpu import make
    from neuma_amd import io as nio
    from neuma_amd.pretrain import PRETRAIN_CFG, check_loss_kind, epoch_loss, pretrain, pretrain_constitutive
    from neuma_amd.trajectory import TrajectoryError
    assert PRETRAIN_CFG["weight_xy"] == 1.0 and PRETRAIN_CFG["weight_yx"] == 1.0 and PRETRAIN_CFG["loss"] == "l2"
    obs, traj = make_clouds(), make()
    assert check_loss_kind(obs, dict(PRETRAIN_CFG, loss="chamfer")) and check_loss_kind(traj, dict(PRETRAIN_CFG, loss="chamfer"))
    assert not check_loss_kind(traj, dict(PRETRAIN_CFG, loss="l1"))
    # model = None: anything that reached the simulator would fail with another exception
    for kind in ("l1", "l2"):
        with pytest.raises(TrajectoryError, match="'loss'"):
            pretrain_constitutive(None, None, obs, None, None, dict(loss=kind))
    with pytest.raises(TrajectoryError, match="'teacher_steps'"):
        pretrain_constitutive(None, None, obs, None, None, dict(loss="chamfer", teacher_steps=1))
    with pytest.raises(ValueError, match="'loss'"):
        pretrain_constitutive(None, None, traj, None, None, dict(loss="huber"))
    with pytest.raises(TrajectoryError):
        epoch_loss(None, obs, 3, teacher_steps=1)
    # the entry point's body: a file and a folder, refused before the device is touched (gpu 99 does not exist anywhere)
    obs.save(tmp_path / "obs.pt")
    folder = tmp_path / "scan"
    folder.mkdir()
    for f, m in ((1, 6), (2, 4)):
        nio.save_particles_ply(folder / f"{f:03d}.ply", np.random.default_rng(f).random((m, 3)))
    for source in (tmp_path / "obs.pt", folder):
        cfg = SimpleNamespace(get=dict(pretrain=dict(loss="l2", substeps=5), gpu=99).get)
        with pytest.raises(TrajectoryError, match="'loss'"):
            pretrain(cfg, trajectory=str(source))
        cfg = SimpleNamespace(get=dict(pretrain=dict(loss="chamfer", substeps=5, teacher_steps=2), gpu=99).get)
        with pytest.raises(TrajectoryError, match="'teacher_steps'"):
            pretrain(cfg, trajectory=str(source))


def test_chamfer_adaptor_has_the_loss_fn_signature_and_ignores_velocities():
    from neuma_amd.chamfer_loss import chamfer_loss_torch
    from neuma_amd.pretrain import chamfer_frame_loss
    x, y, v = torch.rand(6, 3, dtype=torch.float64), torch.rand(9, 3, dtype=torch.float64), torch.rand(6, 3)
    mask = torch.tensor([1, 1, 0, 1, 0, 1], dtype=torch.uint8)
    fn = chamfer_frame_loss(0.25, 2.0, loss=chamfer_loss_torch)
    got = fn(x, v, y, None, mask, kind="chamfer", weight_x=7.0, weight_v=9.0)
    assert float(got) == float(chamfer_loss_torch(x, y, mask, 0.25, 2.0))


# ---------------------------------------------------------------- ABI

def test_entry_point_is_declared_exported_and_checks_its_arguments_on_the_host():
    from neuma_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "neuma_hip.h").read_text(), flags=re.S)
    lib = _lib.lib()
    for name in ("nm_chamfer_loss_workspace", "nm_chamfer_loss"):
        m = re.search(r"\b" + name + r"\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
        assert m, f"{name} is not declared in neuma_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert len(_lib.SIGNATURES[name][1]) == len(m.group(1).split(","))
    assert "nm_chamfer_loss.hip" in (ROOT / "neuma_amd" / "csrc" / "Makefile").read_text()
    assert lib.nm_chamfer_loss_workspace(0, 5) == 0 and lib.nm_chamfer_loss_workspace(5, 0) == 0
    assert lib.nm_chamfer_loss_workspace(-1, 5) == 0 and lib.nm_chamfer_loss_workspace(100, 50) > 0
    p = 4096        # (never dereferenced: every case below is refused on the host)
    for args, word in (((0, 4, p, p, None, 1.0, 1.0, p, None, None, None, None, p, 1 << 30, None), b"empty point cloud"),
                       ((4, 0, p, p, None, 1.0, 1.0, p, None, None, None, None, p, 1 << 30, None), b"empty point cloud"),
                       ((4, 4, None, p, None, 1.0, 1.0, p, None, None, None, None, p, 1 << 30, None), b"null pointer"),
                       ((4, 4, p, None, None, 1.0, 1.0, p, None, None, None, None, p, 1 << 30, None), b"null pointer"),
                       ((4, 4, p, p, None, 1.0, 1.0, None, None, None, None, None, p, 1 << 30, None), b"null pointer"),
                       ((4, 4, p, p, None, 1.0, 1.0, p, None, None, None, None, None, 1 << 30, None), b"null pointer"),
                       ((4, 4, p, p, None, 1.0, 1.0, p, None, None, None, None, p, lib.nm_chamfer_loss_workspace(4, 4) - 1, None),
                        b"workspace too small")):
        assert lib.nm_chamfer_loss(*args) == -1
        assert word in lib.nm_last_error()
