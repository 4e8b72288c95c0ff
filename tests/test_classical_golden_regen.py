"""Build-container-only: tests/golden/classical/*.npz ARE what the reference's own modules/nclaw/material/preset.py classes
produce (gen_classical_golden.py imports and runs them).  The generator is re-run into a temporary directory and every array
must equal the committed one exactly.  Skipped where the reference is not readable (the GPU box)."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

REF = Path("/root/reference")
GOLD = Path(__file__).resolve().parent / "golden"


@pytest.mark.skipif(not os.path.exists(REF / "modules" / "nclaw" / "material" / "preset.py"),
                    reason="needs the reference project's checkout, which the repository does not hold")
def test_classical_generator_reproduces_the_committed_fixtures(tmp_path):
    env = dict(os.environ, NEUMA_GOLDEN_OUT=str(tmp_path), OMP_NUM_THREADS="1", MKL_NUM_THREADS="1")
    p = subprocess.run([sys.executable, str(GOLD / "gen_classical_golden.py")], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    made = sorted(f.name for f in (tmp_path / "classical").glob("*.npz"))
    committed = sorted(f.name for f in (GOLD / "classical").glob("*.npz"))
    assert made == committed and len(committed) == 12
    for name in committed:
        a, b = np.load(GOLD / "classical" / name, allow_pickle=False), np.load(tmp_path / "classical" / name, allow_pickle=False)
        assert sorted(a.files) == sorted(b.files), name
        for k in a.files:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (name, k)
            assert a[k].dtype.kind in "fib", (name, k)                  # data only: no strings, no object arrays
            assert np.array_equal(a[k], b[k], equal_nan=True), (name, k)
