"""CPU: the export of deformed Gaussians as 3DGS parameters - the numpy fp64 path (neuma_amd/extras/gaussian_export.py) against the
definition Sigma' = F L L^T F^T, the file save_frame writes, and the HOST half of the kernel body (nm_gaussian_deform_one is
__host__ __device__): tests/export_host/export_host_main.hip is built into tmp_path and run as a program; it makes no HIP call and
is the target for a host sanitizer build.

What this does NOT cover: the device path (v_rcp / v_rsq / v_sqrt inside nm_svd3, the device's expf / logf), which
tests/test_gpu_gaussian_export.py holds to the same bound.

Bound of the host program per family (gaussian_export_cases.py): the largest over kept rows of
max|activate(outputs) - Sigma'_64| / max|Sigma'_64| is at most max(4 x yardstick, 2e-6), the yardstick being the same computation by
code older than the kernel (F @ L in torch fp32, oracle.material.svd3 in fp32, log, exp, square, U diag U^T).  The families `zero`
and `scaled_out` are dropped from that comparison (their Sigma' leaves [1e-30, 1e30] by definition, see gaussian_export_cases.py);
their rows still have to come out finite, with unit quaternions and r >= 0."""
import math
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import gaussian_export_cases as gc
from neuma_amd.extras import gaussian_export as ge
from oracle import material as om

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "export_host" / "export_host_main.hip"


@pytest.fixture(scope="module")
def cases():
    return gc.inputs(0)


def test_row_filter_keeps_nine_tenths_of_every_compared_family(cases):
    """From the fp64 definition alone, before anything is compared."""
    assert set(gc.DROPPED) <= set(cases)
    for name, (F, ls, rot) in cases.items():
        share = float(gc.kept(gc.sigma64(F, ls, rot)).mean())
        if name in gc.DROPPED:
            assert share < gc.KEEP_SHARE, (name, share)          # (a family that survives must not stay dropped)
        else:
            assert share >= gc.KEEP_SHARE, (name, share)
    ls = torch.cat([c[1] for c in cases.values()])
    assert float(ls.min()) >= math.log(1e-3) - 1e-6 and float(ls.max()) <= math.log(1e-1) + 1e-6
    n = torch.cat([c[2] for c in cases.values()]).double().norm(dim=1)
    assert float(n.min()) >= 0.5 - 1e-6 and float(n.max()) <= 2.0 + 1e-6


def _check_quats(q, tol):
    q = np.asarray(q, dtype=np.float64)
    assert np.isfinite(q).all()
    assert np.abs(np.linalg.norm(q, axis=1) - 1.0).max() <= tol
    assert (q[:, 0] >= 0).all()


# random F; reflections; rank 2, rank 1 and zero F (finite outputs, the covariance still agrees absolutely)
@pytest.mark.parametrize("name", ["baseline", "cond1e3", "perm_refl", "tie1m2", "rotations", "rank2", "rank1", "zero", "zero_column",
                                  "single_entry"])
def test_fp64_path_reproduces_the_definition(cases, name):
    F, ls, rot = cases[name]
    if name in ("perm_refl", "tie1m2", "cond1e3"):
        assert int((torch.linalg.det(F.double()) < 0).sum()) >= 10                  # these carry the reflections
    for mod in (1.0, 0.5):
        S = gc.sigma64(F, ls, rot, mod)
        lo, q = ge.gaussian_deform(ls.double().numpy(), rot.double().numpy(), F.double().numpy(), mod)
        assert lo.dtype == np.float64 and np.isfinite(lo).all()
        _check_quats(q, 1e-14)
        err = np.abs(gc.activated64(lo, q) - S).max(axis=(1, 2))
        bound = 1e-12 * np.abs(S).max(axis=(1, 2))
        worst = float((err / np.maximum(bound, 1e-300)).max())
        print(name, mod, f"worst err / bound = {worst:.3e}")
        assert (err <= bound).all(), (name, mod, worst)


def test_fp64_path_identity_returns_the_rest_covariance(cases):
    _, ls, rot = cases["baseline"]
    lsn, rn = ls.double().numpy(), rot.double().numpy()
    rest = ge.covariance(lsn, rn)
    eye = np.broadcast_to(np.eye(3), (ls.shape[0], 3, 3))
    a = ge.gaussian_deform(lsn, rn, None)
    b = ge.gaussian_deform(lsn, rn, eye)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    S = gc.activated64(*a)
    assert (np.abs(S - rest).max(axis=(1, 2)) <= 1e-12 * np.abs(rest).max(axis=(1, 2))).all()
    assert np.abs(np.sort(a[0], axis=1) - np.sort(lsn, axis=1)).max() <= 1e-9          # the scales are the rest scales, in some order
    with pytest.raises(ValueError):
        ge.gaussian_deform(lsn, rn, np.full((ls.shape[0], 3, 3), np.nan))


def test_rot_to_quat_takes_every_branch_and_inverts_build_rotation():
    g = torch.Generator().manual_seed(3)
    q = torch.randn(4000, 4, generator=g, dtype=torch.float64).numpy()
    q[:8] = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [0, 1, 1, 0], [0, 0, 1, 1], [0, 1, 0, 1], [1e-9, 1, 0, 0]])
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    R = ge.build_rotation(q)
    t = R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]
    branch = np.argmax(np.stack([t, R[:, 0, 0], R[:, 1, 1], R[:, 2, 2]], -1), axis=1)
    assert set(branch.tolist()) == {0, 1, 2, 3}
    back = ge.rot_to_quat(R)
    _check_quats(back, 1e-14)
    assert np.abs(ge.build_rotation(back) - R).max() <= 1e-14


# ---------------------------------------------------------------------------------------------------------------- the file

def _model(K=60, deg=1, seed=2):
    from neuma_amd.render.gaussian_model import GaussianModel
    g = torch.Generator().manual_seed(seed)
    n = (deg + 1) ** 2
    m = GaussianModel(deg)
    return m.set_params(torch.randn(K, 3, generator=g), torch.randn(K, 1, 3, generator=g), torch.randn(K, n - 1, 3, generator=g),
                        math.log(1e-2) + torch.randn(K, 3, generator=g), torch.randn(K, 4, generator=g), torch.randn(K, 1, generator=g))


def _header(path):
    raw = Path(path).read_bytes()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    return raw[:end]


def test_saved_frame_is_a_kernels_ply(tmp_path):
    from neuma_amd import io as nio
    from neuma_amd.export import deformed_gaussians, save_frame
    from neuma_amd import NeumaHipError
    m = _model()
    K = m.get_xyz.shape[0]
    g = torch.Generator().manual_seed(7)
    means = torch.randn(K, 3, generator=g)
    F = torch.eye(3)[None] + 0.3 * torch.randn(K, 3, 3, generator=g)
    F[1] = 0.0                                                                    # a crushed Gaussian is a legitimate frame
    shs = torch.randn(K, 4, 3, generator=g)
    nio.save_gaussians_ply(m, tmp_path / "kernels.ply")
    save_frame(tmp_path / "001.ply", m, means, F, scaling_modifier=0.7)
    save_frame(tmp_path / "002.ply", m, means, F.reshape(K, 9), shs, 0.7)
    assert _header(tmp_path / "001.ply") == _header(tmp_path / "kernels.ply") == _header(tmp_path / "002.ply")
    ref, a, b = (nio.read_ply_vertices(tmp_path / f) for f in ("kernels.ply", "001.ply", "002.ply"))
    assert list(a) == list(ref) == list(b) == nio.gaussian_attribute_names(3, 9)
    same = lambda u, v, k: np.array_equal(np.asarray(u[k]).view(np.uint32), np.asarray(v[k]).view(np.uint32))
    for k in ["opacity"] + [f"f_dc_{i}" for i in range(3)]:
        assert same(a, ref, k) and same(b, ref, k), k
    for i in range(9):
        assert same(a, ref, f"f_rest_{i}"), i
    want = shs[:, 1:].transpose(1, 2).flatten(start_dim=1).numpy()                # channel-major, as save_gaussians_ply stores them
    assert np.array_equal(np.stack([b[f"f_rest_{i}"] for i in range(9)], 1), want)
    assert np.array_equal(np.stack([a[k] for k in "xyz"], 1), means.numpy())
    for f in ("001.ply", "002.ply"):
        back = nio.load_gaussians_ply(tmp_path / f, 1)
        assert torch.isfinite(back._scaling).all() and torch.isfinite(back._rotation).all()
        _check_quats(back._rotation.numpy(), 1e-6)
        S = gc.sigma64(F, m._scaling, m._rotation, 0.7)
        got = gc.activated64(back._scaling.numpy(), back._rotation.numpy())
        keep = np.ones(K, dtype=bool); keep[1] = False
        assert gc.family_error(got, S, keep) <= 1e-5                              # fp32 log-scales of a frame computed in fp64
        assert np.abs(got[1]).max() == 0.0
    # the native path does not take CPU tensors
    with pytest.raises((NeumaHipError, ValueError)):
        deformed_gaussians(m, means, F)


# ---------------------------------------------------------------------------------------------------------------- host half

def _hipcc():
    return shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else None)


@pytest.fixture(scope="module")
def host_deform(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    d = tmp_path_factory.mktemp("export_host")
    exe = d / "export_host_main"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", str(SRC), "-o", str(exe)], check=True)

    def run(ls, rot, F=None, mod=1.0):
        n = ls.shape[0]
        fin, fout = d / "in.bin", d / "out.bin"
        with open(fin, "wb") as fh:
            fh.write(np.array([n, 0 if F is None else 1], dtype=np.int32).tobytes() + np.float32(mod).tobytes())
            for t in (ls, rot) + (() if F is None else (F,)):
                fh.write(t.numpy().astype(np.float32).tobytes())
        subprocess.run([str(exe), str(fin), str(fout)], check=True, timeout=60)
        raw = np.fromfile(fout, dtype=np.float32)
        assert raw.size == 7 * n
        return raw[:3 * n].reshape(n, 3).copy(), raw[3 * n:].reshape(n, 4).copy()

    return run


@pytest.mark.parametrize("name", list(gc.inputs(0)))
def test_host_body_family_within_existing_code_noise(host_deform, cases, name):
    F, ls, rot = cases[name]
    lo, q = host_deform(ls, rot, F)
    assert np.isfinite(lo).all()
    _check_quats(q, 1e-6)
    if name in gc.DROPPED:
        return
    S = gc.sigma64(F, ls, rot)
    keep = gc.kept(S)
    err = gc.family_error(gc.activated64(lo, q), S, keep)
    yard = gc.family_error(gc.yardstick_cov(F, ls, rot, om.svd3).double().numpy(), S, keep)
    print(name, f"err {err:.3e} yardstick {yard:.3e} kept {int(keep.sum())}/{keep.size}")
    assert err <= max(gc.MARGIN * yard, gc.FLOOR), (name, err, yard)


def test_host_body_identity_and_modifier(host_deform, cases):
    _, ls, rot = cases["baseline"]
    n = ls.shape[0]
    a = host_deform(ls, rot, None)
    b = host_deform(ls, rot, torch.eye(3).expand(n, 3, 3).contiguous())
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    F = cases["cond1e3"][0]
    S = gc.sigma64(F, ls, rot, 0.5)
    keep = gc.kept(S)
    half = host_deform(ls, rot, F, 0.5)
    yard = gc.family_error(gc.yardstick_cov(F, ls, rot, om.svd3, 0.5).double().numpy(), S, keep)
    assert gc.family_error(gc.activated64(*half), S, keep) <= max(gc.MARGIN * yard, gc.FLOOR)
