"""Mesh / field colliders without a GPU: the fp64 definition (extras/colliders.py apply_field_collider) on fields whose answer is
known, the `type: mesh` parser with its messages, the ctypes layout of nm_field_collider against the header as a compiler sees
it, the host-only setter, and the refusals that need no device."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import mesh_sdf_cases as cases
from neuma_amd.extras import colliders as xc
from neuma_amd.sim import colliders as sc
from neuma_amd.sim.colliders import FieldCollider, MeshCollider, Plane, parse_colliders

ROOT = Path(__file__).resolve().parent.parent
G = 16
VC = (0.0531, 0.0217, -0.0293)


def _u(seed=0):
    return torch.randn(G ** 3, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


def _linear_field(n, pt, origin, h, dims, **kw):
    idx = np.stack(np.meshgrid(*[np.arange(d) for d in dims], indexing="ij"), -1)
    phi = ((np.asarray(origin) + idx * h) - np.asarray(pt)) @ np.asarray(n)
    return FieldCollider(phi=phi, origin=tuple(origin), spacing=h, dims=dims, **kw)


def _on_lattice(c, p):
    q = (p - torch.tensor(c.origin, dtype=p.dtype)) / c.spacing
    return ((q >= 0) & (q <= torch.tensor(c.dims) - 1)).all(-1)


@pytest.mark.parametrize("surface", ["sticky", "slip", "friction"])
def test_a_linear_field_is_the_plane_node_for_node(surface):
    n, pt = (0.6, 0.8, 0.0), (0.5, 0.4, 0.5)
    kw = dict(surface=surface, friction=0.4 if surface == "friction" else 0.0, velocity=VC)
    fc = _linear_field(n, pt, (0.1, 0.05, 0.2), 0.11, (9, 10, 7), **kw)
    pl = Plane(point=pt, normal=n, **kw)
    p, u = xc.node_positions(G), _u()
    lat = _on_lattice(fc, p)
    assert 100 < int(lat.sum()) < G ** 3
    inside, phi, nrm = xc.field_phi_normal(fc, p)
    want = (p - torch.tensor(pt, dtype=torch.float64)) @ torch.tensor(n, dtype=torch.float64)
    assert float((phi[lat] - want[lat]).abs().max()) <= 1e-15           # a trilinear interpolant reproduces a linear phi
    assert float((nrm[lat] - torch.tensor(n, dtype=torch.float64)).abs().max()) <= 1e-13
    assert torch.equal(inside, lat & (want < 0)) and int(inside.sum()) > 50 and not bool((want[lat].abs() < 1e-9).any())
    a, b = xc.apply_field_collider(fc, p, u), xc.apply_collider(pl, p, u)
    assert float((a - b)[lat].abs().max()) <= 4e-15
    assert torch.equal(a[~lat], u[~lat])                                   # off the lattice: outside, whatever the plane says
    assert torch.equal(xc.apply_colliders([fc], u, G), a)                 # apply_colliders takes field colliders in its list


def test_cell_choice_boundaries_and_nan():
    """nodes exactly on the last lattice plane use the last cell (t = 1); one ulp beyond is outside; NaN is outside"""
    fc = _linear_field((0.0, 1.0, 0.0), (0.0, 10.0, 0.0), (0.25, 0.25, 0.25), 0.125, (5, 4, 3), surface="sticky", velocity=VC)
    hi = [0.25 + 0.125 * (d - 1) for d in fc.dims]
    p = torch.tensor([[0.25, 0.25, 0.25], hi, [hi[0], 0.3, 0.3], [np.nextafter(hi[0], 2.0), 0.3, 0.3], [np.nextafter(0.25, 0.0), 0.3, 0.3],
                      [float("nan"), 0.3, 0.3], [0.3, 0.3, float("inf")]], dtype=torch.float64)
    inside, phi, _ = xc.field_phi_normal(fc, p)
    assert inside.tolist() == [True, True, True, False, False, False, False]
    assert float((phi[:3] - (p[:3, 1] - 10.0)).abs().max()) <= 1e-14
    u = torch.ones(7, 3, dtype=torch.float64)
    out = xc.apply_field_collider(fc, p, u)
    assert torch.equal(out[3:], u[3:]) and torch.allclose(out[:3], torch.tensor(VC, dtype=torch.float64).expand(3, 3))


def test_zero_gradient_takes_plus_x():
    fc = FieldCollider(phi=np.full((3, 3, 3), -0.5), origin=(0.0, 0.0, 0.0), spacing=0.5, dims=(3, 3, 3), surface="slip")
    p = torch.tensor([[0.3, 0.6, 0.2]], dtype=torch.float64)
    inside, _, n = xc.field_phi_normal(fc, p)
    assert bool(inside[0]) and n[0].tolist() == [1.0, 0.0, 0.0]
    out = xc.apply_field_collider(fc, p, torch.tensor([[-2.0, 3.0, 4.0]], dtype=torch.float64))
    assert out[0].tolist() == [0.0, 3.0, 4.0]


def test_mesh_field_of_a_box_pushes_out_along_the_nearest_face():
    """deep inside one face of a big axis-aligned box the field is linear: the normal is that face's"""
    v = np.array([(x, y, z) for x in (0.2, 0.8) for y in (0.1, 0.5) for z in (0.2, 0.8)], dtype=np.float64)
    t = cases._outward(v, np.array([(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6),
                                    (0, 6, 4), (1, 5, 7), (1, 7, 3)]))
    fc = MeshCollider(verts=v, tris=t, resolution=24, surface="slip").build("cpu")
    assert isinstance(fc, FieldCollider) and fc.source.path is None and fc.phi.shape == fc.dims
    p = torch.tensor([[0.5, 0.47, 0.5], [0.5, 0.13, 0.5], [0.23, 0.3, 0.5]], dtype=torch.float64)
    inside, phi, n = xc.field_phi_normal(fc, p)
    assert inside.all() and torch.allclose(phi, torch.tensor([-0.03, -0.03, -0.03], dtype=torch.float64), atol=1e-6)
    assert torch.allclose(n, torch.tensor([[0, 1, 0], [0, -1, 0], [-1, 0, 0]], dtype=torch.float64), atol=1e-5)


def test_autograd_of_the_definition_is_the_transposed_jacobian():
    v, t = cases.MESHES["torus"]()
    fc = MeshCollider(verts=v, tris=t, resolution=20, surface="friction", friction=0.4, velocity=VC).build("cpu")
    p = xc.node_positions(G)
    inside, _, _ = xc.field_phi_normal(fc, p)
    idx = torch.nonzero(inside)[:6, 0]
    assert len(idx) == 6
    u = _u(4)[idx].clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda w: xc.apply_field_collider(fc, p[idx], w), (u,), eps=1e-7, atol=1e-6)


def test_parser_accepts_a_mesh_entry_and_maps_it(tmp_path):
    v, t = cases.MESHES["box"]()
    path = tmp_path / "prop.obj"
    cases.write_obj(path, v, t)
    node = dict(type="mesh", path=str(path), scale=0.5, euler_xyz_deg=[0, 0, 90], translate=[0.5, 0.2, 0.5], resolution=16,
                surface="friction", friction=0.4, velocity=[0, 0.1, 0])
    cs = parse_colliders([dict(type="sphere", center=[0.5, 0.5, 0.5], radius=0.1), node])
    assert isinstance(cs[1], MeshCollider) and cs[1].path == str(path) and len(cs[1].tris) == 12
    assert (cs[1].surface, cs[1].friction, cs[1].velocity, cs[1].resolution, cs[1].margin_cells) == ("friction", 0.4, (0.0, 0.1, 0.0), 16, 2)
    v9 = np.array([[float(f"{x:.9g}") for x in row] for row in v])
    want = 0.5 * np.stack([-v9[:, 1], v9[:, 0], v9[:, 2]], -1) + np.array([0.5, 0.2, 0.5])       # Rz(90): (x, y) -> (-y, x)
    assert np.abs(cs[1].verts - want).max() <= 1e-15
    analytic, fields = sc.split(cs)
    assert len(analytic) == 1 and fields == [cs[1]] and sc.pack(analytic) is not None
    # arrays in place of a path; objects pass through
    m = parse_colliders([dict(type="mesh", verts=v, tris=t)])[0]
    assert m.path is None and np.array_equal(m.verts, v) and parse_colliders([m]) == [m]
    text = sc.describe_fields([cs[1].build("cpu")], draw_wanted=True)
    assert "mesh colliders: 1 (mesh colliders are not drawn in renders)" in text
    assert f"[0] mesh path={path} triangles=12 lattice=" in text and "surface=friction mu=0.4" in text
    assert "not drawn" not in sc.describe_fields([cs[1]])


def test_parser_rejects_with_messages(tmp_path):
    v, t = cases.MESHES["box"]()
    ok = dict(type="mesh", verts=v, tris=t)
    sph = dict(type="sphere", center=[0.5, 0.5, 0.5], radius=0.1)
    with pytest.raises(ValueError, match=r"collider 0: a mesh collider in front of an analytic one"):
        parse_colliders([ok, sph])
    with pytest.raises(ValueError, match=r"collider 1: a mesh collider in front"):
        parse_colliders([sph, ok, sph, ok])
    with pytest.raises(ValueError, match=r"5 mesh colliders, at most 4"):
        parse_colliders([ok] * 5)
    assert len(parse_colliders([sph] * 8 + [ok] * 4)) == 12
    with pytest.raises(ValueError, match=r"colliders: n = 9 outside 0\.\.8"):
        parse_colliders([sph] * 9 + [ok])
    with pytest.raises(ValueError, match=r"collider 1: mesh is not closed: 3 edges"):
        parse_colliders([sph, dict(ok, tris=t[:-1])])
    with pytest.raises(ValueError, match=r"collider 0: mesh is inverted"):
        parse_colliders([dict(ok, tris=t[:, ::-1])])
    with pytest.raises(ValueError, match=r"collider 0: path: give either"):
        parse_colliders([dict(type="mesh")])
    with pytest.raises(ValueError, match=r"collider 0: path: give either"):
        parse_colliders([dict(ok, path="x.obj")])
    with pytest.raises(ValueError, match=r"collider 0: path: an \.obj or \.ply"):
        parse_colliders([dict(type="mesh", path=str(tmp_path / "x.stl"))])
    with pytest.raises(ValueError, match=r"collider 0: scale: must be positive"):
        parse_colliders([dict(ok, scale=-1.0)])
    with pytest.raises(ValueError, match=r"collider 0: surface: unknown surface"):
        parse_colliders([dict(ok, surface="bouncy")])
    with pytest.raises(ValueError, match=r"collider 0: friction: must not be negative"):
        parse_colliders([dict(ok, surface="friction", friction=-0.1)])
    with pytest.raises(ValueError, match=r"collider 0: translate: three finite numbers"):
        parse_colliders([dict(ok, translate=[0, float("nan"), 0])])
    with pytest.raises(ValueError, match=r"collider 0: resolution: must be >= 1"):
        parse_colliders([dict(ok, resolution=0)])
    with pytest.raises(ValueError, match=r"collider 0: shape: unknown shape 'cone'"):
        parse_colliders([dict(type="cone")])
    for bad in (dict(spacing=0.0), dict(dims=(1, 3, 3)), dict(origin=(0.0, float("inf"), 0.0)), dict(phi=np.zeros((2, 2, 2)))):
        kw = dict(phi=np.zeros((3, 3, 3)), origin=(0.0, 0.0, 0.0), spacing=0.1, dims=(3, 3, 3))
        kw.update(bad)
        with pytest.raises(ValueError, match=next(iter(bad))):
            FieldCollider(**kw)


def test_ctypes_layout_matches_the_header_as_a_compiler_lays_it_out(tmp_path):
    from neuma_amd import _lib
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang") if shutil.which(c)), None)
    assert cc is not None, "no C compiler to lay out nm_field_collider with"
    fields = [f[0] for f in _lib.nm_field_collider._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "neuma_hip.h"\nint main(void) {\n'
                   '  printf("%zu %d %d", sizeof(nm_field_collider), NM_MAX_FIELD_COLLIDERS, NM_MAX_COLLIDERS);\n'
                   + "".join(f'  printf(" %zu", offsetof(nm_field_collider, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == C.sizeof(_lib.nm_field_collider) == 56
    assert (out[1], out[2]) == (sc.MAX_FIELD_COLLIDERS, sc.MAX_COLLIDERS) == (4, 8)
    assert out[3:] == [getattr(_lib.nm_field_collider, f).offset for f in fields]
    assert C.sizeof(_lib.nm_collider) == 100          # the analytic struct keeps its pinned 25-field layout


def test_setter_is_host_only_and_refuses_a_null_handle():
    from neuma_amd import _lib
    lib = _lib.lib()
    one = (_lib.nm_field_collider * 1)()
    assert lib.nm_mpm_set_field_colliders(None, 1, one) == -1 and b"field colliders: null handle" in lib.nm_last_error()
    with pytest.raises(ValueError, match=r"n = 5 outside 0\.\.4"):
        sc.pack_fields([None] * 5)
    assert sc.pack_fields([]) is None


def test_builder_shard_and_training_refusals_without_a_device():
    from neuma_amd import NeumaHipError
    from neuma_amd.sim import MPMModelBuilder
    v, t = cases.MESHES["box"]()
    base = dict(gravity=[0, -9.8, 0], bc="noslip", num_grids=16, dt=1e-3, bound=1, eps=6e-7)
    b = MPMModelBuilder().parse_cfg(dict(base, colliders=[dict(type="plane", point=[0.5, 0.1, 0.5], normal=[0, 1, 0]),
                                                          dict(type="mesh", verts=v, tris=t, resolution=8, velocity=[0, 0.5, 0])]))
    assert [type(c).__name__ for c in b.colliders] == ["Plane", "MeshCollider"]
    m = b.finalize("cpu")                      # (no handle yet: the field is built on the CPU path, nothing is uploaded)
    assert len(m.colliders) == 1 and isinstance(m.colliders[0], Plane)
    assert len(m.field_colliders) == 1 and isinstance(m.field_colliders[0], FieldCollider) and m.field_colliders[0].source is b.colliders[1]
    o0 = m.field_colliders[0].origin
    for _ in range(3):
        m.step_colliders()
    o3 = m.field_colliders[0].origin
    assert (o3[0], o3[2]) == (o0[0], o0[2]) and abs(o3[1] - (o0[1] + 3 * 1e-3 * 0.5)) < 1e-15
    assert m.colliders[0].point == (0.5, 0.1, 0.5)
    with pytest.raises(NeumaHipError, match="colliders: per-operator path only"):
        m.shard(None)
    m.set_colliders(m.colliders)               # analytic only again
    assert m.field_colliders == []
    with pytest.raises(NotImplementedError, match=r"sim\.colliders"):
        sc.refuse_in_training({"sim": {"colliders": [dict(type="mesh", verts=v, tris=t)]}}, "python -m neuma_amd.finetune")


@pytest.mark.parametrize("mesh,kind", [("torus", "dyadic"), ("torus", "odd"), ("box", "dyadic"), ("box", "odd")])
def test_gpu_cases_are_clean_in_the_fp64_reference(mesh, kind):
    """The condition tests/test_gpu_field_colliders.py relies on, asserted without a GPU: in the fp64 reference of every one of its
    cases no node with mass has |phi| < 1e-5, a lattice fraction within 1e-5 of a cell face (odd lattice) or sits at a jump of
    the response's Jacobian - nothing needs to be excluded (the cap would be 1 % of the nodes with mass)."""
    import field_collider_cases as fcc
    _, origin, h, dims = fcc.field(mesh, kind)
    if kind == "dyadic":
        assert all((o * 64).is_integer() for o in origin) and h == 1.0 / 32
    for N, Gc in fcc.SIZES:
        for bc in ("noslip", "freeslip"):
            _, _, _, (_, gm, gv) = fcc.mpm_grid(N, Gc, bc)
            for surface in ("sticky", "slip", "friction"):
                fcc.assert_clean([fcc.collider(mesh, kind, surface)], gv, gm, Gc, kind)
