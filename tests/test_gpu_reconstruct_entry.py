"""GPU: `python -m neuma_amd.reconstruct` in a fresh child process on a dataset folder in the reference's synthetic layout (the
writers of tests/test_gpu_entrypoints.py): it writes a kernels.ply that io.py reads back with the configured sh_degree and that
prepare.prepare_simulation_data accepts."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from test_gpu_entrypoints import _write_experiment

pytestmark = pytest.mark.gpu


def test_reconstruct_entry_point_writes_kernels_that_prepare_accepts(tmp_path):
    from neuma_amd import io as nio
    from neuma_amd.config import load_config
    from neuma_amd.prepare import prepare_simulation_data
    path, scene = _write_experiment(tmp_path)
    cfg = load_config(path)
    out = tmp_path / "fit" / "kernels.ply"
    out.parent.mkdir()
    root = Path(__file__).resolve().parent.parent
    env = dict(os.environ, PYTHONPATH=str(root))
    p = subprocess.run([sys.executable, "-m", "neuma_amd.reconstruct", "-c", str(path), "-o", str(out), "--iterations", "60",
                        "--init_random", "1500", "--init_box", "0", "0", "0", "1", "1", "1", "--seed", "1"],
                       cwd=str(root), env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "views of step 0" in p.stdout and "wrote 1500 Gaussians" in p.stdout       # no densification before iteration 500
    sh_degree = int(cfg.gaussian.sh_degree)
    g = nio.load_gaussians_ply(out, sh_degree)
    n_rest = (sh_degree + 1) ** 2 - 1
    assert g.get_xyz.shape == (1500, 3) and g.get_features.shape == (1500, n_rest + 1, 3)
    for t in (g.get_xyz, g.get_features, g.get_scaling, g.get_rotation, g.get_opacity):
        assert bool(torch.isfinite(t).all())
    # 60 iterations moved the start: the opacities left inverse_sigmoid(0.1) and the means left the drawn points' bits
    assert float((g.get_opacity - 0.1).abs().max()) > 1e-3
    assert float(g.get_xyz.min()) > -0.5 and float(g.get_xyz.max()) < 1.5
    assets = tmp_path / "assets_from_fit"
    prepare_simulation_data(assets, out, particles_path=Path(cfg.particle_data.particles_path), sh_degree=sh_degree,
                            opacity_thres=float(cfg.gaussian.opacity_thres), particles_downsample_factor=1,
                            confidence=float(cfg.gaussian.confidence), max_particles=int(cfg.gaussian.max_particles), device="cuda")
    kept = nio.load_gaussians_ply(assets / "kernels.ply", sh_degree).get_xyz.shape[0]
    assert 0 < kept <= 1500 and (assets / "particles.ply").is_file() and (assets / "bindings.pt").is_file()
    B, n_p = nio.load_bindings(assets / "bindings.pt")
    assert B.K == kept and np.isfinite(n_p.cpu().numpy()).all()
