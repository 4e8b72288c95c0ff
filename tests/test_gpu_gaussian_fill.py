"""neuma_amd.gaussian_fill (csrc/nm_fill.hip) against extras/gaussian_fill.py, the numpy fp64 statement of the same algorithm:
the density field to a bound taken from the extras path's own fp32 evaluation, the integer stage (classification, emission)
bit for bit on the GPU's own field, the whole fill bit for bit on a scene with no cell near the threshold, the shapes where
the kernels could go wrong, run-to-run reproducibility, and prepare_simulation_data(fill=...) end to end."""
import os
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from gaussian_fill_scenes import SHELL, cov6_from, random_cloud, shell_scene
from gpu_util import dev, parity

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GPU_OVER_FP32 = 8.0      # the GPU may be this many times as far from fp64 as numpy's own fp32 evaluation: another summation
#                          order (fma contraction) and the hardware exp


def _cpu():
    from neuma_amd.extras import gaussian_fill
    return gaussian_fill


def _gpu():
    from neuma_amd import gaussian_fill
    return gaussian_fill


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


class Scene:
    """One input, its lattice, the extras fields (fp64 and fp32) and the GPU field, each computed once."""

    def __init__(self, mu, cv, op, resolution, cutoff=9.0):
        cpu, gpu = _cpu(), _gpu()
        self.mu, self.cv, self.op, self.cutoff = mu, cv, op, cutoff
        self.origin, self.h, self.dims = cpu.fill_lattice(mu, cv, resolution, cutoff)
        self.f64, self.skipped = cpu.density_field(mu, cv, op, self.origin, self.h, self.dims, cutoff)
        self.f32, _ = cpu.density_field(mu, cv, op, self.origin, self.h, self.dims, cutoff, dtype=np.float32)
        self.gpu_field, self.gpu_skipped = gpu.density_field(_up(mu), _up(cv), _up(op), self.origin, self.h, self.dims, cutoff)
        torch.cuda.synchronize()


def check_field(sc: Scene, tau: float):
    """Test 1: relative error over the cells with d64 > 0.05 tau against 8 x the extras path's own fp32 error there; cells with
    d64 = 0 are exactly 0."""
    g = sc.gpu_field.cpu().numpy()
    assert g.dtype == np.float32 and g.shape == sc.f64.shape and sc.gpu_skipped == sc.skipped
    m = sc.f64 > 0.05 * tau
    assert m.any()
    noise = float((np.abs(sc.f32[m].astype(np.float64) - sc.f64[m]) / sc.f64[m]).max())
    err = float((np.abs(g[m].astype(np.float64) - sc.f64[m]) / sc.f64[m]).max())
    print(f"field: gpu vs fp64 {err:.3e}, numpy fp32 vs fp64 {noise:.3e}, cells {int(m.sum())}")
    assert noise > 0
    parity(os.environ.get("PYTEST_CURRENT_TEST", "?").split(" (")[0], "field rel_max over d64 > 0.05 tau", err, GPU_OVER_FP32 * noise,
           noise=noise)
    stray = int(((sc.f64 == 0) & (g != 0)).sum())       # could only be a term within rounding of the cutoff radius
    assert stray == 0


def check_integer_stage(sc: Scene, tau: float, per_cell=1, include_shell=True):
    """Test 2: the GPU's classify + emit on its own field equals the extras functions on that same field, no tolerance."""
    cpu, gpu = _cpu(), _gpu()
    kc = cpu.classify_cells(sc.gpu_field.cpu().numpy(), sc.dims, tau)
    want_p, want_k = cpu.emit_points(kc, sc.origin, sc.h, sc.dims, per_cell, include_shell)
    p, k, cnt = gpu.classify_emit(sc.gpu_field, sc.origin, sc.h, sc.dims, tau, per_cell, include_shell)
    assert p.dtype == torch.float32 and k.dtype == torch.uint8 and tuple(p.shape) == (len(want_p), 3)
    assert cnt["n_shell"] == int((kc == 1).sum()) and cnt["n_enclosed"] == int((kc == 2).sum())
    assert np.array_equal(k.cpu().numpy(), want_k)
    assert np.array_equal(p.cpu().numpy().view(np.uint32), want_p.view(np.uint32))
    return len(want_p)


@pytest.fixture(scope="module")
def shell():
    return Scene(*shell_scene(), SHELL["resolution"], SHELL["cutoff"])


def test_shell_field_parity(shell):
    assert tuple(shell.dims)[0] == 32 and (shell.f64 > 0).sum() > 5000
    check_field(shell, SHELL["density_thres"])


def test_shell_integer_stage_is_exact(shell):
    tau = SHELL["density_thres"]
    assert check_integer_stage(shell, tau) > 3000
    check_integer_stage(shell, tau, per_cell=2)
    check_integer_stage(shell, tau, per_cell=3, include_shell=False)
    check_integer_stage(shell, 0.05)                    # another threshold: fatter shell, other cavity
    # any field: noise, with plateaus of equal values and NaN / inf cells
    rng = np.random.default_rng(3)
    f = rng.random(shell.f64.shape).astype(np.float32)
    f[rng.integers(0, f.size, 50)] = np.nan
    f[rng.integers(0, f.size, 50)] = np.inf
    f[rng.integers(0, f.size, 500)] = 0.7
    noise = Scene.__new__(Scene)
    noise.origin, noise.h, noise.dims, noise.gpu_field = shell.origin, shell.h, shell.dims, _up(f)
    assert check_integer_stage(noise, 0.7) > 1000


def test_shell_end_to_end_is_exact(shell):
    cpu, gpu = _cpu(), _gpu()
    tau = SHELL["density_thres"]
    assert not (np.abs(shell.f64 - tau) <= 1e-4 * tau).any()           # a condition on the input, from the fp64 reference alone
    for n in (1, 2):
        want_p, want_k, want_i = cpu.fill_from_gaussians(shell.mu, shell.cv, shell.op, per_cell=n, **SHELL)
        p, k, info = gpu.fill_from_gaussians(shell.mu, shell.cv, shell.op, per_cell=n, device=dev(), **SHELL)
        assert want_i["n_enclosed"] > 0 and len(want_p) > 3000 * n ** 3
        assert np.array_equal(p.view(np.uint32), want_p.view(np.uint32)) and np.array_equal(k, want_k)
        assert info["dims"] == want_i["dims"] and info["h"] == want_i["h"] and np.array_equal(info["origin"], want_i["origin"])
        assert all(info[key] == want_i[key] for key in ("n_shell", "n_enclosed", "n_skipped"))
    # tensors on the device are taken as they are
    p2, _, _ = gpu.fill_from_gaussians(_up(shell.mu), _up(shell.cv), _up(shell.op), device=dev(), **SHELL)
    assert np.array_equal(p2, cpu.fill_from_gaussians(shell.mu, shell.cv, shell.op, **SHELL)[0])


def _batch_size():
    src = (ROOT / "neuma_amd" / "csrc" / "nm_fill.hip").read_text()
    return int(re.search(r"^#define\s+NM_FILL_BATCH\s+(\d+)", src, flags=re.M).group(1))


def _list_lengths(sc: Scene):
    """Gaussians per 4^3 block, from the extras path's own block boxes."""
    cpu = _cpu()
    b0, b1 = cpu.gaussian_blocks(sc.mu, sc.cv, sc.origin, sc.h, sc.dims, sc.cutoff)
    nb = [(int(d) + cpu.BLOCK - 1) // cpu.BLOCK for d in sc.dims]
    n = np.zeros(nb, np.int64)
    for lo, hi in zip(b0, b1):
        n[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] += 1
    return n


def _single():
    return np.array([[0.3, -0.1, 0.2]], np.float32), cov6_from([[0.9, 0.1, -0.3, 0.2]], [[0.3, 0.15, 0.08]]), np.array([0.9], np.float32), 16


def _partial_blocks():
    return random_cloud(11, 150, (0.5, 0.45, 0.4), 0.03, 0.1) + (37,)


def _planar():
    mu, cv, op = random_cloud(12, 200, (1.0, 1.0, 0.0), 0.02, 0.03)
    return mu, cv, op, 40


def _one_everywhere():
    mu, cv, op = random_cloud(13, 200, (0.5, 0.5, 0.5), 0.03, 0.08)
    mu = np.concatenate([np.zeros((1, 3), np.float32), mu])
    cv = np.concatenate([np.array([[0.09, 0, 0, 0.09, 0, 0.09]], np.float32), cv])      # sigma 0.3: its box is the lattice
    return mu, cv, np.concatenate([np.array([0.6], np.float32), op]), 24


def _crowded():
    mu, cv, op = random_cloud(14, 700, (0.5, 0.5, 0.5), 0.03, 0.08)
    mu[:] = (mu * 0.02).astype(np.float32)       # every centre within +-0.01 of the origin: less than one cell
    return mu, cv, op * np.float32(0.01), 20


@pytest.mark.parametrize("make", [_single, _partial_blocks, _planar, _one_everywhere, _crowded], ids=lambda f: f.__name__.strip("_"))
def test_shapes_where_the_kernels_can_go_wrong(make):
    mu, cv, op, res = make()
    sc = Scene(mu, cv, op, res)
    lengths = _list_lengths(sc)
    if make is _partial_blocks:
        assert int(sc.dims[0]) == 37 and sum(int(d) % 4 != 0 for d in sc.dims) >= 2      # partial blocks at the high faces
    if make is _planar:
        assert int(sc.dims[2]) <= 4 and lengths.shape[2] == 1 and lengths.shape[0] > 4
    if make is _one_everywhere:
        assert lengths.min() >= 1 and lengths.size > 100
        b0, b1 = _cpu().gaussian_blocks(mu, cv, sc.origin, sc.h, sc.dims)
        assert (b0[0] == 0).all() and (b1[0] == np.array(lengths.shape) - 1).all()
    if make is _crowded:
        assert sc.h > 0.02 and lengths.max() >= 700 > 2 * _batch_size()   # a block list that takes many LDS batches
    tau = 0.3 * float(sc.f64.max())
    check_field(sc, tau)
    assert check_integer_stage(sc, tau, per_cell=2) > 0
    # a threshold above the field's maximum: nothing to emit is an empty result, not an error
    p, k, cnt = _gpu().classify_emit(sc.gpu_field, sc.origin, sc.h, sc.dims, 2.0 * float(sc.f64.max()) + 1.0)
    assert tuple(p.shape) == (0, 3) and tuple(k.shape) == (0,) and cnt == dict(n_kept=0, n_shell=0, n_enclosed=0)


def test_threshold_above_the_maximum_gives_an_empty_fill(shell):
    p, k, info = _gpu().fill_from_gaussians(shell.mu, shell.cv, shell.op, resolution=32, density_thres=1e3, device=dev())
    assert p.shape == (0, 3) and p.dtype == np.float32 and k.shape == (0,) and info["n_shell"] == 0 and info["n_enclosed"] == 0


def test_degenerate_gaussians_are_skipped_on_the_gpu_too(shell):
    flat = np.array([[0.01, 0, 0, 0.01, 0, 0.0], [0.01, 0.02, 0, 0.01, 0, 0.01]], np.float32)
    mu = np.concatenate([shell.mu, np.zeros((2, 3), np.float32)])
    cv = np.concatenate([shell.cv, flat])
    op = np.concatenate([shell.op, np.ones(2, np.float32)])
    f, skipped = _gpu().density_field(_up(mu), _up(cv), _up(op), shell.origin, shell.h, shell.dims, SHELL["cutoff"])
    assert skipped == 2 and torch.equal(f, shell.gpu_field)


def test_density_is_bitwise_reproducible(shell):
    again, _ = _gpu().density_field(_up(shell.mu), _up(shell.cv), _up(shell.op), shell.origin, shell.h, shell.dims, SHELL["cutoff"])
    assert torch.equal(again, shell.gpu_field)
    # ... whatever order the Gaussians come in, the lists are summed in ascending index: a permuted input is another sum
    # order, so only closeness is asked of it
    perm = np.random.default_rng(0).permutation(len(shell.mu))
    other, _ = _gpu().density_field(_up(shell.mu[perm]), _up(shell.cv[perm]), _up(shell.op[perm]), shell.origin, shell.h, shell.dims,
                                    SHELL["cutoff"])
    assert torch.allclose(other, shell.gpu_field, rtol=1e-5, atol=1e-6)


def test_bad_arguments_fail_before_any_device_work(shell):
    gpu = _gpu()
    with pytest.raises(ValueError):
        gpu.density_field(torch.from_numpy(shell.mu), _up(shell.cv), _up(shell.op), shell.origin, shell.h, shell.dims)
    with pytest.raises(ValueError):
        gpu.classify_emit(shell.gpu_field[:-1], shell.origin, shell.h, shell.dims)
    with pytest.raises(ValueError, match="K = 0"):
        gpu.fill_from_gaussians(shell.mu[:0], shell.cv[:0], shell.op[:0], device=dev())
    from neuma_amd import _lib
    lib = _lib.lib()
    assert lib.nm_fill_density_workspace(0, 10, 10) == 0 and lib.nm_fill_density_workspace(10, 1 << 31, 10) == 0
    import ctypes as C
    assert lib.nm_fill_classify_workspace((C.c_int32 * 3)(1024, 1024, 1024)) == 0


def _write_shell_kernels(path):
    from neuma_amd import io as nio
    from neuma_amd.render.gaussian_model import GaussianModel
    mu, _, op, quat, scales = shell_scene(return_raw=True)
    K = len(mu)
    t = lambda a: torch.tensor(np.asarray(a, np.float32))
    gm = GaussianModel(0)
    gm.set_params(t(mu), torch.zeros(K, 1, 3), torch.zeros(K, 0, 3), t(np.log(scales)), t(quat), t(np.log(op / (1 - op)))[:, None])
    nio.save_gaussians_ply(gm, path)
    return K


def test_prepare_simulation_data_fills_on_the_gpu(tmp_path, capsys):
    from neuma_amd import io as nio
    from neuma_amd.binding import build_bindings
    from neuma_amd.config import Cfg
    from neuma_amd.finetune import _prepare
    from neuma_amd.prepare import prepare_simulation_data
    K = _write_shell_kernels(tmp_path / "point_cloud.ply")
    fill = dict(resolution=32, density_thres=0.5)
    out = tmp_path / "assets"
    prepare_simulation_data(out, tmp_path / "point_cloud.ply", sh_degree=0, device=dev(), fill=fill)
    assert all((out / n).is_file() for n in ("kernels.ply", "particles.ply", "bindings.pt"))
    g = nio.load_gaussians_ply(out / "kernels.ply", 0, device=dev())
    assert g.get_xyz.shape[0] == K
    pts, _, _ = _gpu().fill_from_gaussians(g.get_xyz, g.get_covariance(), g.get_opacity.squeeze(-1), device=dev(), **fill)
    counts, _, _ = build_bindings(g.get_xyz, g.get_covariance(), _up(pts), 0.95, 10)
    lonely = int((counts == 0).sum())
    particles = nio.load_particles_ply(out / "particles.ply")
    assert len(pts) > 3000 and len(particles) == len(pts) + lonely
    assert np.array_equal(particles[:len(pts)].astype(np.float32), pts)
    _, n_particles = nio.load_bindings(out / "bindings.pt")
    assert n_particles.shape[0] == K and int(n_particles.min()) >= 1
    capsys.readouterr()
    stamp = (out / "particles.ply").stat().st_mtime_ns
    prepare_simulation_data(out, tmp_path / "point_cloud.ply", sh_degree=0, device=dev(), fill=fill)
    assert "already prepared" in capsys.readouterr().out and (out / "particles.ply").stat().st_mtime_ns == stamp
    # finetune's helper with a config that names nothing but particle_data.fill
    cfg = Cfg(sim_data_name="shell", particle_data=dict(fill=fill),
              gaussian=dict(kernels_path=str(tmp_path / "point_cloud.ply"), sh_degree=0, opacity_thres=0.02, confidence=0.95,
                            max_particles=10))
    _prepare(cfg, tmp_path / "ft", dev())
    assert (tmp_path / "ft" / "particles.ply").read_bytes() == (out / "particles.ply").read_bytes()
    from neuma_amd.inference import _prepare as prepare_object
    prepare_object(cfg, tmp_path / "inf", dev())
    assert (tmp_path / "inf" / "particles.ply").read_bytes() == (out / "particles.ply").read_bytes()
