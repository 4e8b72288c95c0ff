"""CPU: the HOST half of nm_svd3 / nm_svd3_adj (both are __host__ __device__) on the families of svd_cases.py, against the
fp64 yardstick.  tests/svd_host/svd_host_main.hip is built into tmp_path and run as a program; it makes no HIP call.

What this does NOT cover: the device path.  On the host NM_RCP / NM_RSQ / NM_SQRT are IEEE division and sqrtf; on the
device they are the v_rcp_f32 / v_rsq_f32 / v_sqrt_f32 approximations.  The device is held to the same bounds by
tests/test_gpu_svd_edges.py.  This test holds the host-callable half, lets nm_svd3 be developed without a GPU, and its
program is the target for a host sanitizer build.

Bound for each metric: max(4 x the error of oracle.material.svd3 run in fp32 on that family, 2e-6), relative to sigma_max."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import svd_cases as sc
from oracle import material as om

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "svd_host" / "svd_host_main.hip"
FLOOR = 2e-6


def _hipcc():
    return shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else None)


@pytest.fixture(scope="module")
def host_svd(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    d = tmp_path_factory.mktemp("svd_host")
    exe = d / "svd_host_main"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", str(SRC), "-o", str(exe)], check=True)

    def run(F, grads=None):
        n = F.shape[0]
        fin, fout = d / "F.bin", d / "out.bin"
        with open(fin, "wb") as fh:
            fh.write(np.int32(n).tobytes())
            fh.write(F.numpy().astype(np.float32).tobytes())
        cmd = [str(exe), str(fin), str(fout)]
        if grads is not None:
            with open(d / "G.bin", "wb") as fh:
                for t in grads:
                    fh.write(t.numpy().astype(np.float32).tobytes())
            cmd.append(str(d / "G.bin"))
        subprocess.run(cmd, check=True, timeout=60)
        raw = np.fromfile(fout, dtype=np.float32)
        assert raw.size == n * (21 + (9 if grads is not None else 0))
        U = torch.from_numpy(raw[:9 * n].reshape(n, 3, 3).copy())
        s = torch.from_numpy(raw[9 * n:12 * n].reshape(n, 3).copy())
        V = torch.from_numpy(raw[12 * n:21 * n].reshape(n, 3, 3).copy())
        gF = torch.from_numpy(raw[21 * n:].reshape(n, 3, 3).copy()) if grads is not None else None
        return U, s, V.transpose(1, 2).contiguous(), gF

    return run


@pytest.fixture(scope="module")
def fams():
    return sc.families(0)


def test_families_are_what_the_gpu_tests_assume(fams):
    """Checked from the fp64 yardstick alone: the row filters of tests/test_gpu_svd_edges.py keep enough of each family."""
    assert list(fams)[0] == "baseline" and all(F.dtype == torch.float32 and 0 < F.shape[0] <= sc.MAX_ROWS for F in fams.values())
    again = sc.families(0)
    assert all(torch.equal(fams[k], again[k]) for k in fams)
    for name in sc.NET_FAMILIES:
        kept = float(sc.polar_defined(sc.yardstick(fams[name])).double().mean())
        assert kept >= sc.POLAR_KEEP_FLOOR[name], (name, kept)
    for name in ("baseline", "cond1e3"):
        assert float(sc.gap_separated(sc.yardstick(fams[name])).double().mean()) >= 0.5, name
    for name in sc.FULL_RANK:
        y = sc.yardstick(fams[name])
        assert bool((y["s"][:, 2].abs() > 1e-7 * y["s"][:, 0]).all()), name


@pytest.mark.parametrize("name", list(sc.families(0)))
def test_host_svd_family_within_reference_noise(host_svd, fams, name):
    F = fams[name]
    yard = sc.yardstick(F)
    U, s, Vh, _ = host_svd(F)
    assert torch.isfinite(U).all() and torch.isfinite(s).all() and torch.isfinite(Vh).all()
    m = sc.metrics(F, U, s, Vh, yard)
    got, ref = sc.worst(m), sc.worst(sc.noise(F, yard))
    print(name, {k: f"{got[k]:.2e} (noise {ref[k]:.2e})" for k in sc.METRIC_KEYS})
    bad = {k: (got[k], max(4 * ref[k], FLOOR)) for k in sc.METRIC_KEYS if not got[k] <= max(4 * ref[k], FLOOR)}
    assert not bad, f"{name}: metric (measured, bound) {bad}"
    if name in sc.FULL_RANK:
        assert bool(m["sign_ok"].all()), f"{name}: sign(sigma_2) != sign(det F) on {int((~m['sign_ok']).sum())} rows"
    if name == "zero":
        assert bool((s == 0).all())


def test_host_svd_is_scale_equivariant_bit_for_bit(host_svd, fams):
    F = fams["baseline"]
    U0, s0, Vh0, _ = host_svd(F)
    for k in (-100, -20, -3, 5, 20, 60):
        U, s, Vh, _ = host_svd(F * 2.0 ** k)
        assert torch.equal(U, U0) and torch.equal(Vh, Vh0) and torch.equal(s, s0 * 2.0 ** k), k


@pytest.mark.parametrize("name", ["baseline", "cond1e3", "tie01", "tie12", "tie1m2", "tie012", "near_tie", "rank2", "rotations",
                                  "zero", "rank1"])
def test_host_svd_adjoint_matches_clamped_adjoint(host_svd, fams, name):
    """nm_svd3_adj on the program's own factors (so the arbitrary basis at ties is shared) against
    oracle.material.svd3_adjoint in fp64; bound max(4 x that function's own fp32 error on those factors, 1e-6) of max|ref|."""
    F = fams[name]
    n = F.shape[0]
    g = torch.Generator().manual_seed(5)
    grads = [torch.randn(n, 3, 3, generator=g), torch.randn(n, 3, generator=g), torch.randn(n, 3, 3, generator=g)]
    U, s, Vh, gF = host_svd(F, grads)
    assert torch.isfinite(gF).all()
    ref = om.svd3_adjoint(U.double(), s.double(), Vh.double(), *[t.double() for t in grads])
    r32 = om.svd3_adjoint(U, s, Vh, *grads)
    scale = float(ref.abs().max())
    noise = float((r32.double() - ref).abs().max()) / scale
    err = float((gF.double() - ref).abs().max()) / scale
    print(name, f"adjoint err {err:.2e} noise {noise:.2e}")
    assert err <= max(4 * noise, 1e-6), (name, err, noise)
