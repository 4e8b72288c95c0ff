"""Colliders without a GPU: properties of the fp64 definition (neuma_amd/extras/colliders.py), its gradient, the config
parser (neuma_amd/sim/colliders.py) and the host-only ABI call."""
import ctypes as C
import math

import pytest
import torch

from neuma_amd.extras import colliders as xc
from neuma_amd.sim.colliders import Box, Plane, Sphere, euler_xyz_deg_to_rot, pack, parse_colliders, refuse_in_training

G = 8
N_HAT = (0.6, 0.8, 0.0)


def _u(seed=0, n=G ** 3):
    return torch.randn(n, 3, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _inside(c):
    return xc.sdf_normal(c, xc.node_positions(G))[0] < 0


def _plane(**kw):
    return Plane(point=(0.5, 0.43, 0.5), normal=N_HAT, **kw)


def test_nodes_outside_every_collider_are_unchanged():
    cs = [_plane(surface="friction", friction=0.3, velocity=(0.1, 0.0, 0.0)), Sphere(center=(0.7, 0.8, 0.6), radius=0.2, surface="sticky")]
    u = _u()
    out = xc.apply_colliders(cs, u, G)
    outside = ~(_inside(cs[0]) | _inside(cs[1]))
    assert int(outside.sum()) > 0 and int((~outside).sum()) > 0
    assert torch.equal(out[outside], u[outside])
    assert not torch.equal(out[~outside], u[~outside])
    assert torch.equal(xc.apply_colliders([], u, G), u)
    assert xc.apply_colliders(cs, u.view(G, G, G, 3), G).shape == (G, G, G, 3)


def test_sticky_gives_the_collider_velocity():
    vc = (0.3, -0.2, 0.1)
    for c in (_plane(surface="sticky", velocity=vc), Sphere(center=(0.5, 0.5, 0.5), radius=0.3, surface="sticky", velocity=vc),
              Box(center=(0.5, 0.5, 0.5), half=(0.3, 0.2, 0.25), rot=euler_xyz_deg_to_rot((10, 20, 30)), surface="sticky", velocity=vc)):
        out = xc.apply_colliders([c], _u(), G)
        ins = _inside(c)
        assert int(ins.sum()) > 0
        assert torch.equal(out[ins], torch.tensor(vc, dtype=torch.float64).expand(int(ins.sum()), 3))


def test_slip_removes_the_approaching_normal_part_only():
    vc = torch.tensor((0.0, 0.1, 0.0), dtype=torch.float64)
    c = _plane(surface="slip", velocity=tuple(vc.tolist()))
    n = torch.tensor(c.normal, dtype=torch.float64)
    u = _u(1)
    out = xc.apply_colliders([c], u, G)
    ins = _inside(c)
    vn = (u - vc) @ n
    app, sep = ins & (vn < 0), ins & (vn >= 0)
    assert int(app.sum()) > 0 and int(sep.sum()) > 0
    assert torch.equal(out[sep], u[sep])                                             # any velocity with vn >= 0 is kept
    tang = lambda t: (t - vc) - ((t - vc) @ n)[:, None] * n
    assert float((tang(out[app]) - tang(u[app])).abs().max()) < 1e-15                # the tangential part is kept
    assert float(((out[app] - vc) @ n).abs().max()) < 1e-15                          # no relative normal velocity left


def test_friction_limits():
    u = _u(2)
    vc = (0.05, 0.0, -0.1)
    slip = xc.apply_colliders([_plane(surface="slip", velocity=vc)], u, G)
    f0 = xc.apply_colliders([_plane(surface="friction", friction=0.0, velocity=vc)], u, G)
    assert float((f0 - slip).abs().max()) < 1e-15                                    # mu = 0 is slip
    big = xc.apply_colliders([_plane(surface="friction", friction=1e9, velocity=vc)], u, G)
    c = _plane(surface="sticky", velocity=vc)
    n, vct = torch.tensor(c.normal, dtype=torch.float64), torch.tensor(vc, dtype=torch.float64)
    app = _inside(c) & (((u - vct) @ n) < 0)
    assert torch.equal(big[app], vct.expand(int(app.sum()), 3))                      # a large mu is sticky for approaching nodes
    assert torch.equal(big[~app], u[~app])
    # Coulomb: the tangential speed drops by mu |vn|, the direction stays
    mu = 0.4
    fr = xc.apply_colliders([_plane(surface="friction", friction=mu, velocity=vc)], u, G)
    w = u[app] - vct
    vn = w @ n
    vt = w - vn[:, None] * n
    s = vt.norm(dim=-1)
    expect = vct + torch.clamp(s + mu * vn, min=0.0)[:, None] * vt / s[:, None]
    assert float((fr[app] - expect).abs().max()) < 1e-14


def test_box_normal_is_the_face_of_smallest_penetration_ties_to_the_lowest_axis():
    box = Box(center=(0.5, 0.5, 0.5), half=(0.25, 0.25, 0.25), surface="slip")
    # (0.375, 0.375, 0.5): penetration 0.125 along x and y, 0.25 along z -> tie x/y -> x; its normal is -x
    p = torch.tensor([[0.375, 0.375, 0.5], [0.5, 0.625, 0.375], [0.5, 0.5, 0.625], [0.5, 0.5, 0.5], [0.3, 0.5, 0.9]],
                     dtype=torch.float64)
    sdf, n = xc.sdf_normal(box, p)
    assert (sdf[:4] < 0).all() and sdf[4] > 0
    assert n[:4].tolist() == [[-1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 0, 0]]         # y/z tie -> y; unique z; full tie -> +x
    rot = euler_xyz_deg_to_rot((0, 0, 90))                                           # box x axis = world y
    rb = Box(center=(0.5, 0.5, 0.5), half=(0.4, 0.1, 0.3), rot=rot, surface="slip")
    sdf, n = xc.sdf_normal(rb, torch.tensor([[0.5, 0.85, 0.5], [0.45, 0.5, 0.5], [0.65, 0.5, 0.5]], dtype=torch.float64))
    assert sdf[0] < 0 and sdf[1] < 0 and sdf[2] > 0                                  # long along world y, thin along world x
    assert float((n[0] - torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64)).abs().max()) < 1e-15
    assert float((n[1] - torch.tensor([-1.0, 0.0, 0.0], dtype=torch.float64)).abs().max()) < 1e-15


def test_two_colliders_compose_in_list_order():
    a = _plane(surface="sticky", velocity=(0.2, 0.0, 0.0))
    b = Sphere(center=(0.5, 0.4, 0.5), radius=0.3, surface="slip")
    u = _u(3)
    p = xc.node_positions(G)
    ab = xc.apply_colliders([a, b], u, G)
    assert torch.equal(ab, xc.apply_collider(b, p, xc.apply_collider(a, p, u)))
    ba = xc.apply_colliders([b, a], u, G)
    both = _inside(a) & _inside(b)
    assert int(both.sum()) > 0
    assert torch.equal(ba[both], torch.tensor(a.velocity, dtype=torch.float64).expand(int(both.sum()), 3))
    assert not torch.equal(ab[both], ba[both])


def test_gradcheck_on_a_patch_away_from_every_branch_threshold():
    """4^3 nodes, all inside a friction plane, a slip sphere and (some) a sticky box; the velocities are drawn and then checked to
    sit away from vn = 0, |vt| = 0 and the edge of the Coulomb cone at every collider of the chain."""
    g = 4
    cs = [Plane(point=(0.5, 2.0, 0.5), normal=N_HAT, surface="friction", friction=0.3, velocity=(0.1, 0.0, 0.0)),
          Sphere(center=(0.4, 0.4, 0.4), radius=2.0, surface="slip", velocity=(0.0, 0.2, 0.0)),
          Box(center=(0.1, 0.1, 0.1), half=(0.3, 0.3, 0.3), rot=euler_xyz_deg_to_rot((0, 0, 20)), surface="sticky")]
    p = xc.node_positions(g)
    u = torch.randn(g ** 3, 3, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    cur, approaching = u, 0
    for c in cs[:2]:
        sdf, n = xc.sdf_normal(c, p)
        assert (sdf < 0).all()
        w = cur - torch.tensor(c.velocity, dtype=torch.float64)
        vn = (w * n).sum(-1)
        vt = w - vn[:, None] * n
        s = vt.norm(dim=-1)
        assert float(vn.abs().min()) > 1e-3 and float(s.min()) > 1e-3
        if c.surface == "friction":
            assert float((1.0 + c.friction * vn / s)[vn < 0].abs().min()) > 1e-3
        approaching += int((vn < 0).sum())
        cur = xc.apply_collider(c, p, cur)
    assert approaching > 20
    assert 0 < int((xc.sdf_normal(cs[2], p)[0] < 0).sum()) < g ** 3
    u.requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t: xc.apply_colliders(cs, t, g), (u,), eps=1e-6, atol=1e-7, rtol=1e-6)


def test_parse_colliders_validates_and_normalises():
    cs = parse_colliders([
        {"type": "plane", "point": [0.5, 0.3, 0.5], "normal": [0.2, 1, 0], "surface": "friction", "friction": 0.4},
        {"type": "sphere", "center": [0.5, 0.4, 0.5], "radius": 0.08, "surface": "slip", "velocity": [0, 0.1, 0]},
        {"type": "box", "center": [0.5, 0.2, 0.5], "half": [0.2, 0.05, 0.2], "euler_xyz_deg": [0, 0, 20], "surface": "sticky"},
        {"type": "box", "center": [0.5, 0.2, 0.5], "half": [0.2, 0.05, 0.2], "rot": [[0, -1, 0], [1, 0, 0], [0, 0, 1]]}])
    assert isinstance(cs[0], Plane) and isinstance(cs[1], Sphere) and isinstance(cs[2], Box)
    assert abs(math.sqrt(sum(a * a for a in cs[0].normal)) - 1.0) < 1e-15            # a non-unit normal is normalised
    assert abs(cs[0].normal[0] / cs[0].normal[1] - 0.2) < 1e-15
    c20, s20 = math.cos(math.radians(20)), math.sin(math.radians(20))
    assert max(abs(a - b) for a, b in zip(cs[2].rot, (c20, -s20, 0, s20, c20, 0, 0, 0, 1))) < 1e-15
    assert cs[3].rot == (0, -1, 0, 1, 0, 0, 0, 0, 1) and cs[3].surface == "sticky"
    assert cs[1].moving and not cs[0].moving
    assert cs[1].advanced(0.5).center == (0.5, 0.45, 0.5)
    assert parse_colliders(None) == [] and parse_colliders(cs) == cs
    ok = {"type": "sphere", "center": [0.5, 0.5, 0.5], "radius": 0.1}
    bad = [({"type": "torus"}, "shape"), (dict(ok, surface="bouncy"), "surface"), (dict(ok, friction=-0.1), "friction"),
           (dict(ok, radius=0.0), "radius"), (dict(ok, radius=-1.0), "radius"),
           ({"type": "plane", "normal": [0, 0, 0]}, "normal"),
           ({"type": "box", "half": [0.1, 0.0, 0.1]}, "half"),
           ({"type": "box", "half": [0.1, 0.1, 0.1], "rot": [1, 0, 0, 0, 1, 0, 0, 0, 1.1]}, "rot"),
           ({"type": "box", "half": [0.1, 0.1, 0.1], "rot": [1, 0, 0, 0, 1, 0, 0, 0.2, 1]}, "rot"),
           ({"type": "box", "half": [0.1, 0.1, 0.1], "rot": [1, 0, 0], "euler_xyz_deg": [0, 0, 1]}, "rot"),
           ({"type": "box", "half": [0.1, 0.1, 0.1], "rot": [1, 0, 0, 0, 1, 0, 0, 0, -1]}, "rot"),      # a reflection
           (dict(ok, center=[0.5, float("nan"), 0.5]), "center"), (dict(ok, velocity=[0, float("inf"), 0]), "velocity")]
    for i, (node, field) in enumerate(bad):
        with pytest.raises(ValueError, match=rf"collider 1: {field}:"):
            parse_colliders([ok, node])
    with pytest.raises(ValueError, match="colliders: n = 9 outside 0..8"):
        parse_colliders([ok] * 9)
    assert len(parse_colliders([ok] * 8)) == 8


def test_training_configs_with_colliders_are_refused_by_name():
    refuse_in_training({"sim": {"num_grids": 32}}, "x")
    refuse_in_training({"sim": {"colliders": []}}, "x")
    with pytest.raises(NotImplementedError, match=r"sim\.colliders"):
        refuse_in_training({"sim": {"colliders": [{"type": "plane"}]}}, "python -m neuma_amd.finetune")
    from neuma_amd.config import Cfg
    from neuma_amd import finetune, pretrain
    cfg = Cfg(sim=dict(colliders=[{"type": "plane"}]), gaussian=dict(rotate_sh=False))
    with pytest.raises(NotImplementedError, match=r"sim\.colliders"):
        finetune.finetune(cfg)
    with pytest.raises(NotImplementedError, match=r"sim\.colliders"):
        pretrain.pretrain(cfg)


def test_builder_reads_the_optional_colliders_key():
    from neuma_amd.sim import MPMModelBuilder
    base = dict(gravity=[0, -9.8, 0], bc="noslip", num_grids=16, dt=1e-3, bound=1, eps=6e-7)
    m = MPMModelBuilder().parse_cfg(base).finalize("cpu")
    assert m.colliders == []
    m = MPMModelBuilder().parse_cfg(dict(base, colliders=[{"type": "sphere", "center": [0.5, 0.5, 0.5], "radius": 0.1,
                                                           "velocity": [0, 1, 0]}])).finalize("cpu")
    assert len(m.colliders) == 1 and isinstance(m.colliders[0], Sphere)
    with pytest.raises(ValueError, match="collider 0: radius:"):
        MPMModelBuilder().parse_cfg(dict(base, colliders=[{"type": "sphere", "radius": 0}]))


def test_packed_struct_matches_the_abi_and_null_handle_is_refused():
    """The ctypes struct is 25 four-byte fields like the header's; a packed array goes through nm_mpm_set_colliders' validation
    (host only: a null handle is refused before the array is looked at, so the call needs no GPU)."""
    import re
    from pathlib import Path
    from neuma_amd import _lib
    text = (Path(__file__).resolve().parent.parent / "include" / "neuma_hip.h").read_text()
    body = re.search(r"typedef struct nm_collider \{(.*?)\} nm_collider;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    words = sum(int(m.group(1) or 1) for m in re.finditer(r"\b(?:int32_t|float)\s+\w+(?:\[(\d+)\])?;", body))
    assert C.sizeof(_lib.nm_collider) == 4 * words == 100
    names = re.findall(r"\b(?:int32_t|float)\s+(\w+)", body)
    assert names == [f[0] for f in _lib.nm_collider._fields_]
    arr = pack(parse_colliders([{"type": "plane", "point": [0.5, 0.25, 0.5], "normal": [0, 2, 0], "surface": "friction", "friction": 0.5},
                                {"type": "box", "center": [0.1, 0.2, 0.3], "half": [0.1, 0.2, 0.3], "euler_xyz_deg": [0, 0, 90],
                                 "velocity": [1, 2, 3]}]))
    assert C.sizeof(arr) == 2 * C.sizeof(_lib.nm_collider)
    assert (arr[0].shape, arr[0].surface, arr[0].friction, list(arr[0].center), list(arr[0].normal)) == (0, 2, 0.5, [0.5, 0.25, 0.5], [0, 1, 0])
    assert (arr[1].shape, arr[1].surface, list(arr[1].velocity)) == (2, 0, [1, 2, 3])
    assert max(abs(a - b) for a, b in zip(arr[1].rot, (0, -1, 0, 1, 0, 0, 0, 0, 1))) < 1e-7
    assert pack([]) is None
    lib = _lib.lib()
    assert lib.nm_mpm_set_colliders(None, 2, arr) == -1
    assert b"colliders: null handle" in lib.nm_last_error()
    assert lib.nm_mpm_set_colliders(None, 0, None) == -1


def test_sharding_and_colliders_exclude_each_other():
    from neuma_amd import NeumaHipError
    from neuma_amd.sim import MPMModelBuilder
    base = dict(gravity=[0, -9.8, 0], bc="noslip", num_grids=16, dt=1e-3, bound=1, eps=6e-7)
    sphere = {"type": "sphere", "center": [0.5, 0.5, 0.5], "radius": 0.1}
    m = MPMModelBuilder().parse_cfg(dict(base, colliders=[sphere])).finalize("cpu")
    with pytest.raises(NeumaHipError, match="colliders: per-operator path only"):
        m.shard(None)
    m = MPMModelBuilder().parse_cfg(base).finalize("cpu")
    m.exchange = object()                    # what shard() leaves behind: this model steps one rank's share
    with pytest.raises(NeumaHipError, match="colliders: per-operator path only"):
        m.set_colliders([sphere])
    assert m.colliders == []
