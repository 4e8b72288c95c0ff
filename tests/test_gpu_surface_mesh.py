"""GPU: nm_surface_count / nm_surface_emit (csrc/nm_surface.hip) against the numpy fp64 statement neuma_amd/extras/surface_mesh.py
on the lattices of tests/surface_mesh_cases.py, and the layers above them: surface_from_gaussians, `render --save_mesh`, and a
mesh going back into mesh_sdf.

Bounds (eps32 = 2^-23, numpy's finfo(float32).eps):
  connectivity  masks, counts, offsets, triangles: integers, equal to the yardstick's.
  positions     per component <= 64 eps32 (h + max|p|).  t = (iso - f_a) / (f_b - f_a) in fp32: every case field lies in [0, 1]
                and iso = 1/2, so each of the two differences is either exact (operands within a factor two of each other:
                Sterbenz) or carries an absolute error <= eps32 / 2 next to |f_b - f_a| >= 2^-4 (the random case by rejection;
                the others because an inexact difference means one end below iso / 2 = 1/4 and the other at or above iso): at
                most 16 eps32 on t for numerator and denominator together, one more rounding for the division, times the
                edge's extent per component, h; plus the rounding of the fp64 coordinate to fp32, eps32 / 2 max|p|.
  attributes    the same bound with the attribute's range in place of h + max|p| (attributes in [0, 1]: range 1).
  normals       angle <= 32 eps32 (|g_a| + |g_b|) / |g| + 8 eps32, from the yardstick's own end gradients g_a, g_b and their
                interpolant g: a central difference of values in [0, 1] is one rounding (eps32 / 2 each), t carries <= 16 eps32,
                the interpolation three more roundings - together <= 18 eps32 (|g_a| + |g_b|) on g, a rotation of at most
                |dg| / |g| (doubled for margin against the second-order term); the normalisation (scaling, three squares, a
                square root, a division) adds a few eps32.  Where the bound exceeds 1 rad (|g| cancels) nothing is claimed."""
import numpy as np
import pytest
import torch

import surface_mesh_cases as sc
from gpu_util import dev, parity
from neuma_amd import surface_mesh
from neuma_amd.extras import surface_mesh as sm

pytestmark = pytest.mark.gpu

CASES = sc.all_cases()
EPS = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def yard():
    """name -> the yardstick's crossings and mesh (with three attributes), computed once"""
    out = {}
    for name, c in CASES.items():
        a = sc.attrs_for(c)
        out[name] = dict(x=sm.edge_crossings(c["field"], c["origin"], c["h"], c["dims"], c["iso"]), attrs=a,
                         mesh=sm.extract(c["field"], c["origin"], c["h"], c["dims"], c["iso"], a))
    return out


@pytest.fixture(scope="module")
def native(yard):
    out = {}
    for name, c in CASES.items():
        f = torch.from_numpy(c["field"]).to(dev())
        a = torch.from_numpy(yard[name]["attrs"]).to(dev())
        out[name] = surface_mesh.extract(f, c["origin"], c["h"], c["dims"], c["iso"], a, return_count=True)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_connectivity_equals_the_yardstick(yard, native, name):
    x = yard[name]["x"]
    v, n, a, tri, cnt = native[name]
    assert (cnt["V"], cnt["T"]) == (x["V"], x["T"]) and tuple(v.shape) == (x["V"], 3) and tuple(tri.shape) == (x["T"], 3)
    assert tri.dtype == torch.int32 and v.dtype == torch.float32
    assert np.array_equal(cnt["mask"].cpu().numpy(), x["mask"])
    assert np.array_equal(cnt["tri_count"].cpu().numpy(), x["tri_count"])
    assert np.array_equal(cnt["vert_offset"].cpu().numpy().astype(np.int64), x["vert_offset"])
    assert np.array_equal(cnt["tri_offset"].cpu().numpy().astype(np.int64), x["tri_offset"])
    assert np.array_equal(tri.cpu().numpy(), yard[name]["mesh"][3])


@pytest.mark.parametrize("name", sorted(CASES))
def test_positions_attributes_normals(yard, native, name):
    c, x = CASES[name], yard[name]["x"]
    v64, n64, a64, _ = yard[name]["mesh"]
    v, n, a, _, _ = native[name]
    v, n, a = (t.cpu().numpy().astype(np.float64) for t in (v, n, a))
    bound_p = 64 * EPS * (c["h"] + np.abs(v64).max())
    parity("surface_mesh", f"{name}: position (abs, per component)", np.abs(v - v64).max(), bound_p)
    rng = float(yard[name]["attrs"].max() - yard[name]["attrs"].min())
    parity("surface_mesh", f"{name}: attribute (abs)", np.abs(a - a64).max(), 64 * EPS * rng)
    t = x["t"][:, None]
    g = x["grad_a"] + t * (x["grad_b"] - x["grad_a"])
    gl = np.sqrt((g * g).sum(1))
    ends = np.sqrt((x["grad_a"] ** 2).sum(1)) + np.sqrt((x["grad_b"] ** 2).sum(1))
    ln = np.sqrt((n * n).sum(1))
    assert np.all((np.abs(ln - 1.0) < 8 * EPS) | (ln == 0.0))
    assert np.all(ln[ends == 0] == 0.0)                                     # both end gradients zero: (0, 0, 0), as the yardstick
    with np.errstate(divide="ignore", invalid="ignore"):
        bound_a = 32 * EPS * ends / gl + 8 * EPS
    ok = (gl > 0) & (bound_a < 1.0)
    assert ok.sum() >= 0.9 * (gl > 0).sum()
    ang = np.arctan2(np.sqrt((np.cross(n[ok], n64[ok]) ** 2).sum(1)), (n[ok] * n64[ok]).sum(1))
    parity("surface_mesh", f"{name}: normal angle / its bound (max over {int(ok.sum())} vertices)", float((ang / bound_a[ok]).max()), 1.0)


@pytest.mark.parametrize("name", sorted(CASES))
def test_native_mesh_is_closed_and_oriented(native, name):
    """on the device's output directly: a wrong popcount rank or halo index shows here even if the yardstick shared the mistake"""
    v, _, _, tri, _ = native[name]
    topo = sm.mesh_topology(tri.cpu().numpy(), len(v))
    assert topo["in_range"] and topo["all_used"] and topo["closed"] and topo["oriented"], topo


@pytest.mark.parametrize("name,euler", [("sphere_20", 2), ("torus", 0), ("two_spheres", 4), ("one_cell", 2)])
def test_native_topology(native, name, euler):
    v, _, _, tri, _ = native[name]
    assert sm.mesh_topology(tri.cpu().numpy(), len(v))["euler"] == euler
    c = CASES[name]
    vol = sm.mesh_volume(v.cpu().numpy(), tri.cpu().numpy())
    clip = sm.enclosed_volume(c["field"], c["origin"], c["h"], c["dims"], c["iso"])
    area = _area(v.cpu().numpy().astype(np.float64), tri.cpu().numpy())
    delta = 64 * EPS * (c["h"] + float(v.abs().max()))
    parity("surface_mesh", f"{name}: divergence volume of the fp32 mesh vs clipped tetrahedra (abs)", abs(vol - clip), 1.01 * np.sqrt(3) * delta * area)


def _area(v, tri):
    fn = np.cross(v[tri[:, 1]] - v[tri[:, 0]], v[tri[:, 2]] - v[tri[:, 0]])
    return float(0.5 * np.sqrt((fn * fn).sum(1)).sum())


@pytest.mark.parametrize("name", ["random_12", "ties", "flat_5x1x6"])
def test_two_calls_give_identical_bytes(native, yard, name):
    c = CASES[name]
    f = torch.from_numpy(c["field"]).to(dev())
    a = torch.from_numpy(yard[name]["attrs"]).to(dev())
    again = surface_mesh.extract(f, c["origin"], c["h"], c["dims"], c["iso"], a, return_count=True)
    for got, want in zip(again[:4], native[name][:4]):
        assert torch.equal(got.view(torch.uint8) if got.numel() else got, want.view(torch.uint8) if want.numel() else want)
    for k in ("mask", "tri_count", "vert_offset", "tri_offset"):
        assert torch.equal(again[4][k], native[name][4][k])


def test_empty_and_refused_inputs():
    f = torch.full((5 * 4 * 3,), 0.25, device=dev())
    v, n, a, tri = surface_mesh.extract(f, (0, 0, 0), 0.1, (5, 4, 3), 0.5)
    assert tuple(v.shape) == (0, 3) and tuple(n.shape) == (0, 3) and tuple(a.shape) == (0, 0) and tuple(tri.shape) == (0, 3)
    assert v.is_cuda and tri.dtype == torch.int32
    bad = f.clone()
    bad[7] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        surface_mesh.extract(bad, (0, 0, 0), 0.1, (5, 4, 3), 0.5)
    bad[7] = float("inf")
    with pytest.raises(ValueError, match="non-finite"):
        surface_mesh.extract(bad, (0, 0, 0), 0.1, (5, 4, 3), 0.5)
    with pytest.raises(ValueError, match="iso"):
        surface_mesh.extract(f, (0, 0, 0), 0.1, (5, 4, 3), 0.0)
    with pytest.raises(ValueError):
        surface_mesh.extract(f, (0, 0, 0), 0.1, (5, 4, 4), 0.5)
    with pytest.raises(ValueError):
        surface_mesh.extract(f.double(), (0, 0, 0), 0.1, (5, 4, 3), 0.5)


def test_surface_from_gaussians():
    from test_surface_mesh_cpu import _ball_model
    m = _ball_model(K=300, seed=3, sigma=0.06)
    g = m.__class__(0)
    g.set_params(*(t.to(dev()).contiguous() for t in (m._xyz, m._features_dc, m._features_rest, m._scaling, m._rotation, m._opacity)))
    v, n, col, tri, info = surface_mesh.surface_from_gaussians(g, resolution=24)
    assert v.is_cuda and len(v) > 500 and max(info["dims"]) == 24
    topo = sm.mesh_topology(tri.cpu().numpy(), len(v))
    assert topo["closed"] and topo["oriented"] and topo["all_used"] and topo["euler"] == 2
    assert tuple(col.shape) == (len(v), 3) and float(col.min()) >= 0.0 and float(col.max()) <= 1.0 and float(col.std()) > 0.0
    rgb = (0.5 + 0.28209479177387814 * m._features_dc.reshape(-1, 3)).clamp(0, 1)
    assert float(col.min()) >= float(rgb.min()) - 1e-3 and float(col.max()) <= float(rgb.max()) + 1e-3      # a weighted mean of the rgb
    # the yardstick path on the same density: the fp64 mesh's volume, to the position bound summed over the triangles
    field = info["field"].cpu().numpy()
    v64, _, _, t64 = sm.extract(field, info["origin"], info["h"], info["dims"], info["iso"])
    assert np.array_equal(t64, tri.cpu().numpy())
    vol, vol64 = sm.mesh_volume(v.cpu().numpy(), tri.cpu().numpy()), sm.mesh_volume(v64, t64)
    delta = 64 * EPS * (info["h"] + np.abs(v64).max())
    parity("surface_mesh", "surface_from_gaussians: volume vs the yardstick on the same density (abs)", abs(vol - vol64),
           1.01 * np.sqrt(3) * delta * _area(v64, t64))
    assert 0.5 * 4 / 3 * np.pi * 0.4 ** 3 < vol64 < 3.0 * 4 / 3 * np.pi * 0.4 ** 3       # a ball of about the Gaussians' extent
    _, _, none, _, _ = surface_mesh.surface_from_gaussians(g, resolution=12, colors=False)
    assert none is None
    # the CPU model takes the extras path to the same connectivity class: closed, one component
    vc, _, cc, tc, _ = surface_mesh.surface_from_gaussians(m, resolution=12)
    assert not vc.is_cuda and sm.mesh_topology(tc.numpy(), len(vc))["closed"] and float(cc.max()) <= 1.0


def _png(path):
    from PIL import Image
    return np.array(Image.open(path)).astype(np.int32)


def test_render_save_mesh_end_to_end(tmp_path):
    from test_gpu_entrypoints import _write_experiment
    from test_gpu_sh_deform import _write_init
    from neuma_amd import io as nio
    from neuma_amd.evaluate import main as render_main
    path, _ = _write_experiment(tmp_path, frames=1)
    _write_init(tmp_path, path)
    res = tmp_path / "results"
    common = ["-c", str(path), "-es", "2", "-dv", "r_0", "--result_root", str(res)]
    render_main(common + ["-vn", "m", "--save_mesh", "m", "--mesh_resolution", "20"])
    out = res / "tinyball-v1"
    assert sorted(p.name for p in (out / "meshes_m").iterdir()) == ["000.ply", "001.ply", "002.ply"]
    assert not (out / "gaussians_m").exists()                                 # works without --save_gaussians
    for p in sorted((out / "meshes_m").iterdir()):
        v, t = nio.read_ply_mesh(p)
        topo = sm.mesh_topology(t, len(v))
        assert len(t) > 100 and topo["closed"] and topo["oriented"] and sm.mesh_volume(v, t) > 0
        assert "red" in nio.read_ply_vertices(p)
    render_main(common + ["-vn", "plain"])
    assert sorted(p.name for p in out.iterdir() if p.name.endswith("plain")) == ["images_plain"]
    names = sorted(p.name for p in (out / "images_m").glob("*.png"))
    assert names == sorted(p.name for p in (out / "images_plain").glob("*.png")) == [f"r_0_{i:03d}.png" for i in range(3)]
    for nm in names:       # (two runs of one roll-out differ by the order of the scatters' float atomics: one 8-bit level)
        assert np.abs(_png(out / "images_m" / nm) - _png(out / "images_plain" / nm)).max() <= 1
    # with --save_gaussians the mesh comes from the model that was written
    render_main(common + ["-vn", "both", "--save_mesh", "both", "--save_gaussians", "both", "--mesh_resolution", "20", "-es", "1"])
    assert sorted(p.name for p in (out / "meshes_both").iterdir()) == sorted(p.name for p in (out / "gaussians_both").iterdir()) == ["000.ply", "001.ply"]
    v0, t0 = nio.read_ply_mesh(out / "meshes_both" / "000.ply")
    v1, t1 = nio.read_ply_mesh(out / "meshes_m" / "000.ply")
    assert np.array_equal(t0, t1) and np.array_equal(v0, v1)                   # frame 0 does not depend on the roll-out


def test_extracted_mesh_is_a_mesh_collider_source(native, tmp_path):
    from neuma_amd import io as nio, mesh_sdf
    v, n, _, tri, _ = native["sphere_20"]
    nio.save_mesh_ply(tmp_path / "sphere.ply", v.cpu().numpy(), n.cpu().numpy(), None, tri.cpu().numpy())
    vr, tr = nio.read_ply_mesh(tmp_path / "sphere.ply")
    g = mesh_sdf.build_mesh_field(vr, tr, resolution=16, device=dev())
    phi = g.phi.cpu().numpy()
    assert np.isfinite(phi).all()
    _, centre, r = sc.sphere_field(20)
    ic = tuple(int(round((centre[k] - g.origin[k]) / g.spacing)) for k in range(3))
    assert phi[ic] < -0.5 * r and phi[0, 0, 0] > 0 and phi[-1, -1, -1] > 0
