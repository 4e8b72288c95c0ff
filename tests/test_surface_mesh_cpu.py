"""CPU: the numpy fp64 statement of the surface extraction (neuma_amd/extras/surface_mesh.py, the yardstick of csrc/nm_surface.hip)
held to what makes a mesh usable - closed, consistently oriented, of the right topology, enclosing the volume the samples say - on
the smallest lattices at which it can go wrong (tests/surface_mesh_cases.py), and the file layer around it: the PLY writer against
the reader every mesh consumer uses, and the command line on a two-frame folder."""
import numpy as np
import pytest
import torch

import surface_mesh_cases as sc
from neuma_amd.extras import surface_mesh as sm

CASES = sc.all_cases()


@pytest.fixture(scope="module")
def meshes():
    out = {}
    for name, c in CASES.items():
        out[name] = sm.extract(c["field"], c["origin"], c["h"], c["dims"], c["iso"], sc.attrs_for(c))
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_closed_and_oriented(meshes, name):
    v, n, a, tri = meshes[name]
    assert len(v) > 0 and len(tri) > 0 and tri.dtype == np.int32 and v.shape[1] == 3 and n.shape == v.shape and a.shape == (len(v), 3)
    topo = sm.mesh_topology(tri, len(v))
    assert topo["in_range"] and topo["all_used"], topo
    assert topo["closed"], "an undirected edge is not in exactly two triangles"
    assert topo["oriented"], "two triangles traverse a shared edge in the same direction"


def test_one_cell_is_closed_by_the_ring_alone(meshes):
    v, _, _, tri = meshes["one_cell"]
    c = CASES["one_cell"]
    assert len(v) == 14                              # the 14 edges around one sample, all to ring samples
    assert sm.mesh_topology(tri, 14)["euler"] == 2
    centre = c["origin"] + 0.5 * c["h"]
    assert np.abs(v - centre).max() <= c["h"] * (1 - c["iso"] / 0.75) + 1e-12      # t = (iso - 0.75) / (0 - 0.75) along every edge


@pytest.mark.parametrize("name,euler", [("sphere_20", 2), ("torus", 0), ("two_spheres", 4), ("touching", 2)])
def test_topology(meshes, name, euler):
    v, _, _, tri = meshes[name]
    assert sm.mesh_topology(tri, len(v))["euler"] == euler


@pytest.mark.parametrize("name", sorted(CASES))
def test_divergence_volume_equals_the_clipped_tetrahedra(meshes, name):
    """two independent routes to the same number: the triangles (divergence theorem) and the closed-form clip of every
    tetrahedron, which never sees a triangle.  Both are sums of O(ncells) terms of size <= h^3 in fp64."""
    c = CASES[name]
    v, _, _, tri = meshes[name]
    vol, clip = sm.mesh_volume(v, tri), sm.enclosed_volume(c["field"], c["origin"], c["h"], c["dims"], c["iso"])
    box = float(np.prod(np.asarray(c["dims"]) + 2)) * c["h"] ** 3
    assert clip > 0 and abs(vol - clip) <= 1e-12 * box, (vol, clip)


def test_sphere_volume_converges():
    errs = []
    for n in (10, 20, 40):
        c, _, r = sc.sphere_field(n)
        v, _, _, tri = sm.extract(c["field"], c["origin"], c["h"], c["dims"], c["iso"])
        errs.append(abs(sm.mesh_volume(v, tri) - 4.0 / 3.0 * np.pi * r ** 3))
    assert errs[0] > errs[1] > errs[2], errs


def test_normals(meshes):
    for name in CASES:
        n = meshes[name][1]
        ln = np.sqrt((n * n).sum(1))
        assert np.all((np.abs(ln - 1.0) < 1e-12) | (ln == 0.0)), name
    v, n, _, tri = meshes["sphere_20"]
    fn = np.cross(v[tri[:, 1]] - v[tri[:, 0]], v[tri[:, 2]] - v[tri[:, 0]])
    area = np.sqrt((fn * fn).sum(1))
    ok = area > 1e-9 * CASES["sphere_20"]["h"] ** 2
    assert ok.sum() > 0.9 * len(tri)
    for q in range(3):
        assert ((fn[ok] * n[tri[ok, q]]).sum(1) > 0).all()
    # and they point away from the centre
    _, centre, _ = sc.sphere_field(20)
    assert (((v - centre) * n).sum(1) > 0).all()


def test_attributes_interpolate_along_the_edge(meshes):
    c = CASES["random_12"]
    a = sc.attrs_for(c)
    _, _, va, _ = meshes["random_12"]
    assert va.min() >= a.min() and va.max() <= a.max()
    x = sm.edge_crossings(c["field"], c["origin"], c["h"], c["dims"], c["iso"])
    assert x["t"].min() >= 0.0 and x["t"].max() <= 1.0
    lin = np.array([1.0, -2.0, 0.5])                # an attribute linear in the position comes back as that function of the vertex
    d = c["dims"]
    g = np.stack(np.meshgrid(*[c["origin"][k] + (np.arange(-1, d[k] + 1) + 0.5) * c["h"] for k in range(3)], indexing="ij"), -1) @ lin
    inner = g[1:-1, 1:-1, 1:-1].reshape(1, -1)
    v, _, va, _ = sm.extract(c["field"], c["origin"], c["h"], c["dims"], c["iso"], inner)
    real = np.all((x["ea"] >= 1) & (x["eb"] >= 1) & (x["ea"] <= np.array(d)) & (x["eb"] <= np.array(d)), 1)      # no ring end
    assert real.sum() > 100 and np.abs(va[real, 0] - v[real] @ lin).max() < 1e-12


def test_ties_keep_zero_area_triangles(meshes):
    v, _, _, tri = meshes["ties"]
    fn = np.cross(v[tri[:, 1]] - v[tri[:, 0]], v[tri[:, 2]] - v[tri[:, 0]])
    assert (np.sqrt((fn * fn).sum(1)) == 0).sum() > 0          # kept: dropping them would open the surface (test_closed_and_oriented)


def test_empty_and_refused_inputs():
    f = np.full(5 * 4 * 3, 0.25, dtype=np.float32)
    v, n, a, tri = sm.extract(f, (0, 0, 0), 0.1, (5, 4, 3), 0.5)
    assert v.shape == (0, 3) and n.shape == (0, 3) and a.shape == (0, 0) and tri.shape == (0, 3) and tri.dtype == np.int32
    assert sm.enclosed_volume(f, (0, 0, 0), 0.1, (5, 4, 3), 0.5) == 0.0 and sm.mesh_volume(v, tri) == 0.0
    bad = f.copy()
    bad[7] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        sm.extract(bad, (0, 0, 0), 0.1, (5, 4, 3), 0.5)
    for iso in (0.0, -1.0, np.inf):
        with pytest.raises(ValueError, match="iso"):
            sm.extract(f, (0, 0, 0), 0.1, (5, 4, 3), iso)
    with pytest.raises(ValueError):
        sm.extract(f, (0, 0, 0), 0.1, (5, 4, 4), 0.5)
    with pytest.raises(ValueError, match="2\\^27"):
        sm.extract(f, (0, 0, 0), 0.1, (1 << 14, 1 << 14, 1), 0.5)
    with pytest.raises(ValueError, match="attrs"):
        sm.extract(f, (0, 0, 0), 0.1, (5, 4, 3), 0.5, np.zeros((5, 60)))


def test_entry_points_validate_on_the_host():
    """null pointers, dims, iso, h, counts: refused before any launch, so this runs without a device (the pointers are never read)"""
    import ctypes as C
    from neuma_amd import _lib
    lib = _lib.lib()
    d, o, P = (C.c_int32 * 3)(4, 5, 6), (C.c_double * 3)(0, 0, 0), 4096
    assert lib.nm_surface_workspace(d) > 0
    assert lib.nm_surface_workspace((C.c_int32 * 3)(0, 5, 6)) == 0 and lib.nm_surface_workspace((C.c_int32 * 3)(1 << 14, 1 << 14, 1)) == 0
    count = lambda field, iso, ws: lib.nm_surface_count(d, field, iso, P, P, P, P, P, P, ws, None)
    assert count(None, 0.5, 1 << 20) == -1 and b"null" in lib.nm_last_error()
    for iso in (0.0, -1.0, float("nan"), float("inf")):
        assert count(P, iso, 1 << 20) == -1 and b"iso" in lib.nm_last_error()
    assert count(P, 0.5, 0) != 0 and b"workspace too small" in lib.nm_last_error()
    assert lib.nm_surface_count((C.c_int32 * 3)(4, 0, 6), P, 0.5, P, P, P, P, P, P, 1 << 20, None) == -1 and b"dims" in lib.nm_last_error()
    emit = lambda h, iso, A, attrs, V, T, tris: lib.nm_surface_emit(d, o, h, P, iso, A, attrs, P, P, P, P, V, T, P, P, None, tris, None)
    assert emit(0.0, 0.5, 0, None, 1, 1, P) == -1 and b"cell edge" in lib.nm_last_error()
    assert emit(0.1, 0.0, 0, None, 1, 1, P) == -1 and b"iso" in lib.nm_last_error()
    assert emit(0.1, 0.5, 5, None, 1, 1, P) == -1 and b"n_attrs" in lib.nm_last_error()
    assert emit(0.1, 0.5, 1, None, 1, 1, P) == -1 and b"null attributes" in lib.nm_last_error()
    assert emit(0.1, 0.5, 0, None, 1, 1, None) == -1 and b"null output" in lib.nm_last_error()
    assert emit(0.1, 0.5, 0, None, 1 << 31, 1, P) == -1 and b"int32" in lib.nm_last_error()
    assert emit(0.1, 0.5, 0, None, 0, 0, None) == 0                        # an empty surface: nothing to do, no launch
    bad_o = (C.c_double * 3)(0, float("inf"), 0)
    assert lib.nm_surface_emit(d, bad_o, 0.1, P, 0.5, 0, None, P, P, P, P, 1, 1, P, P, None, P, None) == -1 and b"origin" in lib.nm_last_error()


def test_cpu_tensors_take_the_extras_path(meshes):
    from neuma_amd import surface_mesh
    c = CASES["odd_9x8x7"]
    v, n, a, tri = surface_mesh.extract(torch.from_numpy(c["field"]), c["origin"], c["h"], c["dims"], c["iso"])
    assert v.dtype == torch.float32 and tri.dtype == torch.int32 and a.shape == (len(v), 0)
    assert np.array_equal(tri.numpy(), meshes["odd_9x8x7"][3]) and np.allclose(v.numpy(), meshes["odd_9x8x7"][0], atol=1e-6)


@pytest.mark.parametrize("colors", [True, False])
def test_ply_round_trip(tmp_path, meshes, colors):
    from neuma_amd import io as nio
    v, n, a, tri = meshes["torus"]
    path = tmp_path / "sub" / "torus.ply"
    nio.save_mesh_ply(path, v, n, a if colors else None, tri)
    v2, t2 = nio.read_ply_mesh(path)
    assert np.array_equal(v2, v.astype(np.float32).astype(np.float64)) and np.array_equal(t2, tri)
    props = nio.read_ply_vertices(path)
    assert list(props) == ["x", "y", "z", "nx", "ny", "nz"] + (["red", "green", "blue"] if colors else [])
    assert np.array_equal(props["nx"], n[:, 0].astype(np.float32))
    if colors:
        assert props["red"].dtype == np.uint8 and np.abs(props["red"] / 255.0 - a[:, 0]).max() <= 0.5 / 255 + 1e-9
    head = path.read_bytes().split(b"end_header\n")[0].decode()
    assert "format binary_little_endian 1.0" in head and "property list uchar int vertex_indices" in head
    with pytest.raises(ValueError, match="index"):
        nio.save_mesh_ply(tmp_path / "bad.ply", v[:10], n[:10], None, tri)


def _ball_model(K=120, seed=0, radius=0.4, sigma=0.12):
    from neuma_amd.render.gaussian_model import GaussianModel
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(K, 3, generator=g)
    p = p / p.norm(dim=1, keepdim=True) * radius * torch.rand(K, 1, generator=g) ** (1.0 / 3.0) + torch.tensor([0.5, 0.4, 0.6])
    m = GaussianModel(0)
    rot = torch.zeros(K, 4)
    rot[:, 0] = 1
    m.set_params(p.contiguous(), torch.rand(K, 1, 3, generator=g) * 2 - 1, torch.zeros(K, 0, 3), torch.full((K, 3), float(np.log(sigma))), rot,
                 torch.full((K, 1), 2.0))
    return m


def test_command_line_on_a_two_frame_folder(tmp_path, capsys):
    from neuma_amd import io as nio
    from neuma_amd.surface_mesh import main
    src = tmp_path / "gaussians_run"
    src.mkdir()
    m = _ball_model()
    nio.save_gaussians_ply(m, src / "000.ply")
    m._xyz = m._xyz + torch.tensor([0.0, -0.1, 0.0])
    nio.save_gaussians_ply(m, src / "001.ply")
    (src / "notes.ply").write_bytes(b"")             # not a frame: ignored
    out = tmp_path / "meshes"
    assert main(["-s", str(src), "-o", str(out), "--resolution", "14", "--sh_degree", "0", "--device", "cpu"]) == 0
    lines = [l for l in capsys.readouterr().out.splitlines() if "V =" in l]
    assert len(lines) == 2 and lines[0].startswith("000.ply") and "volume" in lines[0]
    assert sorted(p.name for p in out.iterdir()) == ["000.ply", "001.ply"]
    ys = []
    for name in ("000.ply", "001.ply"):
        v, t = nio.read_ply_mesh(out / name)
        topo = sm.mesh_topology(t, len(v))
        assert len(t) > 100 and topo["closed"] and topo["oriented"] and sm.mesh_volume(v, t) > 0
        c = nio.read_ply_vertices(out / name)
        assert "red" in c and c["red"].dtype == np.uint8
        ys.append(v[:, 1].mean())
    assert abs(ys[0] - ys[1] - 0.1) < 0.02           # the second frame's body sits 0.1 lower
    # one file, OBJ, no colours
    assert main(["-k", str(src / "000.ply"), "-o", str(tmp_path / "one.obj"), "--resolution", "10", "--sh_degree", "0", "--device", "cpu",
                 "--format", "obj", "--no_colors"]) == 0
    from neuma_amd.extras.mesh_sampling import read_obj_mesh
    v, t = read_obj_mesh(tmp_path / "one.obj")
    assert sm.mesh_topology(t, len(v))["closed"]
