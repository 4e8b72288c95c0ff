"""Build-container-only: tests/golden/chamfer/*.npz ARE what the reference's own modules/tune/metrics.py produces
(gen_chamfer_golden.py loads it by path and runs it).  The generator is re-run into a temporary directory and every array must
equal the committed one exactly.  Skipped where the reference is not readable (the GPU box)."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

REF = Path("/root/reference")
GOLD = Path(__file__).resolve().parent / "golden"


# (os.path.exists, not Path.exists: where the reference's parent directory is not readable the check must skip, not raise)
@pytest.mark.skipif(not os.path.exists(REF / "modules" / "tune" / "metrics.py"),
                    reason="needs the reference project's checkout, which the repository does not hold")
def test_chamfer_generator_reproduces_the_committed_fixtures(tmp_path):
    env = dict(os.environ, NEUMA_GOLDEN_OUT=str(tmp_path), OMP_NUM_THREADS="1", MKL_NUM_THREADS="1")
    p = subprocess.run([sys.executable, str(GOLD / "gen_chamfer_golden.py")], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    made = sorted(f.name for f in (tmp_path / "chamfer").glob("*.npz"))
    committed = sorted(f.name for f in (GOLD / "chamfer").glob("*.npz"))
    assert made == committed == ["clusters.npz", "duplicates.npz", "lattice.npz", "naive.npz", "outside.npz", "uniform.npz"]
    for name in committed:
        a, b = np.load(GOLD / "chamfer" / name, allow_pickle=False), np.load(tmp_path / "chamfer" / name, allow_pickle=False)
        assert sorted(a.files) == sorted(b.files), name
        for k in a.files:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (name, k)
            assert np.array_equal(a[k], b[k]), (name, k)
