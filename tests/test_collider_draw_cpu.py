"""Drawing colliders, without a GPU: the fp64 definition (neuma_amd/extras/collider_draw.py) against closed forms, the style parser,
the start-up line, and the cap on the share of pixels / Gaussians the GPU parity tests may exclude, on their own scenes."""
import math
import re
from pathlib import Path

import pytest
import torch

import collider_draw_cases as cc
from neuma_amd import collider_draw as CD
from neuma_amd.extras import collider_draw as X
from neuma_amd.sim.colliders import Box, Plane, Sphere, describe, parse_colliders

ROOT = Path(__file__).resolve().parent.parent
GREY = [CD.Style((0.5, 0.6, 0.7), 0.0)]


def _dirs(cam):
    H, W = cam.image_height, cam.image_width
    return X.pixel_dirs(cam).reshape(H, W, 3)


def test_sphere_on_the_optical_axis():
    """Centre pixel: t = |c - o| - r, lit head-on; the disc's width on the centre row is that of the tangent cone."""
    W = H = 65
    r, dist = 0.2, 2.5
    cam = cc.Camera(W, H, (0.5, 0.5, 0.5 + dist), (0.5, 0.5, 0.5), fov_deg=30.0)
    t, shade, hit = X.cast(cam, [Sphere(center=(0.5, 0.5, 0.5), radius=r)], GREY)
    assert int(hit[32, 32]) == 0 and abs(float(t[32, 32]) - (dist - r)) < 1e-6          # (the camera matrices are fp32)
    assert torch.allclose(shade[:, 32, 32], torch.tensor(GREY[0].color, dtype=torch.float64), atol=1e-6)
    half_px = W / 2 * (r / math.sqrt(dist * dist - r * r)) / math.tan(math.radians(15.0))
    assert abs(int((hit[32] >= 0).sum()) - 2 * half_px) <= 1.0 and abs(int((hit[:, 32] >= 0).sum()) - 2 * half_px) <= 1.0
    assert bool(torch.isinf(t[hit < 0]).all()) and bool((shade[:, hit < 0] == 0).all())
    # the shade falls off towards the rim: n.l = cos of the angle between the normal and the ray
    assert float(shade[0, 32, 32]) > float(shade[0, 32, 32 + int(half_px) - 1]) > 0.35 * 0.5 - 1e-9


def test_half_space_clipped_by_the_cube():
    """A half-space z < 0.6 seen from the side: the plane's own face inside the cube's silhouette, the cube's face x = 1 at the rim."""
    eye = (2.0, 0.5, 3.0)
    cam = cc.Camera(96, 64, eye, (0.5, 0.5, 0.5), fov_deg=40.0)
    t, shade, hit = X.cast(cam, [Plane(point=(0.5, 0.5, 0.6), normal=(0, 0, 1))], GREY)
    d = _dirs(cam)
    o = torch.tensor(eye, dtype=torch.float64)
    tp = (0.6 - o[2]) / d[..., 2]
    pp = o + tp[..., None] * d
    on_plane = (pp[..., 0] > 0) & (pp[..., 0] < 1) & (pp[..., 1] > 0) & (pp[..., 1] < 1)
    tx = (1.0 - o[0]) / d[..., 0]
    px = o + tx[..., None] * d
    on_side = ~on_plane & (d[..., 0] < 0) & (px[..., 1] > 0) & (px[..., 1] < 1) & (px[..., 2] > 0) & (px[..., 2] < 0.6)
    assert int(on_plane.sum()) > 300 and int(on_side.sum()) > 100
    edge = ((pp[..., :2] - pp[..., :2].round()).abs().min(-1).values < 1e-6) | ((px[..., 2] - 0.6).abs() < 1e-6)      # nothing sits on one
    assert not bool(edge.any())
    assert torch.equal(hit >= 0, on_plane | on_side)
    assert float((t[on_plane] - tp[on_plane]).abs().max()) < 1e-12 and float((t[on_side] - tx[on_side]).abs().max()) < 1e-12
    col = torch.tensor(GREY[0].color, dtype=torch.float64)[:, None]
    for mask, n in ((on_plane, (0.0, 0.0, 1.0)), (on_side, (1.0, 0.0, 0.0))):
        ndl = -(d[mask] * torch.tensor(n, dtype=torch.float64)).sum(-1)
        assert float((shade[:, mask] - col * (0.35 + 0.65 * ndl.clamp_min(0))[None]).abs().max()) < 1e-12


def test_checkerboard_on_a_plane():
    """k = 0.8 on the odd cells, in the documented frame: for the normal +y the frame is u = -z, v = -x (e = x, u = n x e, v = n x u)."""
    assert X.plane_frame((0.0, 1.0, 0.0)) == ((0.0, 0.0, -1.0), (-1.0, 0.0, 0.0))
    u, v = X.plane_frame((0.6, 0.0, 0.8))
    assert abs(sum(a * b for a, b in zip(u, v))) < 1e-15 and abs(sum(a * a for a in u) - 1) < 1e-15 and u == (-0.8, 0.0, 0.6)
    eye = (0.5, 3.0, 0.5001)
    cam = cc.Camera(64, 64, eye, (0.5, 0.0, 0.5), fov_deg=20.0)
    plane = Plane(point=(0.5, 0.5, 0.5), normal=(0, 1, 0))
    t, plain, hit = X.cast(cam, [plane], GREY)
    _, check, _ = X.cast(cam, [plane], [CD.Style(GREY[0].color, 0.25)])
    p = torch.tensor(eye, dtype=torch.float64) + t[..., None] * _dirs(cam)
    odd = ((torch.floor(-(p[..., 2] - 0.5) / 0.25) + torch.floor(-(p[..., 0] - 0.5) / 0.25)) % 2 == 1) & (hit >= 0)
    assert int(odd.sum()) > 500 and int(((hit >= 0) & ~odd).sum()) > 500
    assert torch.allclose(check[:, odd], 0.8 * plain[:, odd], rtol=0, atol=1e-15) and torch.equal(check[:, ~odd], plain[:, ~odd])


def test_box_given_through_a_rotation_agrees_with_the_axis_aligned_one():
    cam = cc.camera((67, 45), "identity")
    a = Box(center=(0.5, 0.4, 0.55), half=(0.2, 0.1, 0.15))
    b = Box(center=(0.5, 0.4, 0.55), half=(0.1, 0.2, 0.15), rot=(0, -1, 0, 1, 0, 0, 0, 0, 1))      # its axes: +y, -x, +z
    ta, sa, ha = X.cast(cam, [a], GREY)
    tb, sb, hb = X.cast(cam, [b], GREY)
    assert int((ha >= 0).sum()) > 100 and torch.equal(ha, hb)
    assert torch.equal(torch.isinf(ta), torch.isinf(tb)) and float((ta - tb)[ha >= 0].abs().max()) < 1e-14
    assert float((sa - sb).abs().max()) < 1e-14


def test_camera_inside_a_solid():
    cam = cc.Camera(40, 30, (0.5, 0.5, 0.6), (0.5, 0.5, 0.0), fov_deg=60.0)
    for c in (Sphere(center=(0.5, 0.5, 0.5), radius=0.3), Plane(point=(0.5, 0.9, 0.5), normal=(0, 1, 0)),
              Box(center=(0.5, 0.5, 0.5), half=(0.3, 0.3, 0.3))):
        t, shade, hit = X.cast(cam, [c], [CD.Style((0.2, 0.4, 0.6), 0.125)])
        assert bool((t == 0).all()) and bool((hit == 0).all())
        assert torch.allclose(shade, torch.tensor([0.2, 0.4, 0.6], dtype=torch.float64)[:, None, None].expand_as(shade), rtol=0, atol=1e-15)
    # and a Gaussian anywhere is hidden from a camera inside a solid it would have to look through
    assert bool(X.hidden(cam.camera_center, [Sphere(center=(0.5, 0.5, 0.5), radius=0.3)], torch.tensor([[0.5, 0.5, 0.1], [0.5, 0.5, 0.55]])).all())


def test_per_axis_map_equals_the_identity_map_with_the_camera_moved():
    """p_r = a p_s + b with a = (2, 1, 0.5): casting with the map from a render-space camera gives the hit image of the identity map
    with the camera pulled back into simulation space (projmatrix_s = M projmatrix_r, campos_s = (campos_r - b) / a), from where
    the render-space scene is the ellipsoidal image of this one; t differs (it is a render-space distance)."""
    tr = cc.MAPS["peraxis"]
    cam_r = cc.camera((67, 45), "peraxis")
    M = torch.diag(torch.tensor(list(tr[0]) + [1.0], dtype=torch.float64))
    M[3, :3] = torch.tensor(tr[1], dtype=torch.float64)
    cam_s = cam_r.to("cpu")
    cam_s.full_proj_transform = M @ cam_r.full_proj_transform.double()
    cam_s.camera_center = ((cam_r.camera_center.double() - M[3, :3]) / torch.tensor(tr[0], dtype=torch.float64))
    colliders, styles = parse_colliders(cc.SETS["eight"]), CD.parse_styles(cc.SETS["eight"])
    t_r, _, hit_r, unsure_r = X.cast(cam_r, colliders, styles, tr, margins=True)
    t_s, _, hit_s, unsure_s = X.cast(cam_s, colliders, styles, X.IDENTITY, margins=True)
    ok = ~(unsure_r | unsure_s)
    assert float(ok.double().mean()) > 0.9 and len(set(hit_r.reshape(-1).tolist())) >= 6
    assert torch.equal(hit_r[ok], hit_s[ok])
    assert float((t_r - t_s)[ok & (hit_r >= 0)].abs().max()) > 0.1


def test_hidden_flags_on_known_sides_of_a_plane():
    plane = [Plane(point=(0.5, 0.5, 0.5), normal=(0, 1, 0))]          # solid: y < 0.5 inside the cube
    campos = torch.tensor([0.5, 2.0, 2.0])
    g = torch.Generator().manual_seed(0)
    xz = 0.05 + 0.9 * torch.rand(200, 2, generator=g, dtype=torch.float64)
    below = torch.stack([xz[:, 0], 0.02 + 0.45 * torch.rand(200, generator=g, dtype=torch.float64), xz[:, 1]], -1)
    above = torch.stack([xz[:, 0], 0.52 + 0.45 * torch.rand(200, generator=g, dtype=torch.float64), xz[:, 1]], -1)
    assert bool(X.hidden(campos, plane, below).all()) and not bool(X.hidden(campos, plane, above).any())
    special = torch.tensor([[0.5, -0.5, 0.5],       # under the cube: the segment runs through the solid
                            [3.0, 0.2, 0.5]],       # beside the cube, below the plane's level: the segment leaves the cube above it
                           dtype=torch.float64)
    assert X.hidden(campos, plane, special).tolist() == [True, False]
    op = torch.full((400, 1), 0.7)
    front = CD.front_opacity(cc.Camera(8, 8, campos.tolist(), (0.5, 0.5, 0.5)), plane, torch.cat([below, above]).float(), op)
    assert bool((front[:200] == 0).all()) and torch.equal(front[200:], op[200:])
    # with a map the same Gaussians, moved with it, get the same flags
    tr = cc.MAPS["peraxis"]
    a, b = (torch.tensor(v, dtype=torch.float64) for v in tr)
    pts = torch.cat([below, above, special])
    assert torch.equal(X.hidden(campos.double() * a + b, plane, pts * a + b, tr), X.hidden(campos, plane, pts))


def test_style_parsing_and_the_start_up_line():
    nodes = [dict(type="plane", point=[0.5, 0.3, 0.5], normal=[0, 1, 0]), dict(type="sphere", center=[0.5, 0.5, 0.5], radius=0.1),
             dict(type="box", center=[0.5, 0.5, 0.5], half=[0.1, 0.1, 0.1], color=[1, 0.5, 0], checker=0.3),
             dict(type="plane", normal=[1, 0, 0], checker=0)]
    styles = CD.parse_styles(nodes)
    assert [s.color for s in styles] == [CD.PALETTE[0], CD.PALETTE[1], (1.0, 0.5, 0.0), CD.PALETTE[3]]
    assert [s.checker for s in styles] == [0.125, 0.0, 0.0, 0.0]            # planes default to 0.125; the key means nothing elsewhere
    colliders = parse_colliders(nodes)                                       # the collider parser ignores the drawing keys
    assert CD.parse_styles(colliders) == [CD.Style(CD.PALETTE[i], 0.125 if i in (0, 3) else 0.0) for i in range(4)]
    assert CD.parse_styles(None) == []
    for bad, field in ((dict(type="sphere", color=[1, 2]), "color"), (dict(type="sphere", color=[0.1, 0.2, 1.5]), "color"),
                       (dict(type="sphere", color="red"), "color"), (dict(type="plane", checker=-1), "checker"),
                       (dict(type="plane", checker=float("nan")), "checker"), (dict(type="plane", checker="wide"), "checker")):
        with pytest.raises(ValueError, match=rf"collider 1: {field}"):
            CD.parse_styles([nodes[0], bad])
    with pytest.raises(ValueError, match="outside 0..8"):
        CD.parse_styles([nodes[1]] * 9)
    assert describe(colliders).splitlines()[0] == "colliders: 4 (not drawn in renders)"
    assert describe(colliders, drawn=True).splitlines()[0] == "colliders: 4 (drawn in renders)"
    assert describe(colliders, drawn=True).splitlines()[1:] == describe(colliders).splitlines()[1:]
    assert CD.map_from_alignment([0.5, 0.5, 0.5], [0.25, 0.1, 0.25]) == ((2.0, 2.0, 2.0), (-0.5, -0.2, -0.5))
    with pytest.raises(ValueError, match="a <= 0"):
        X.cast(cc.camera((67, 45), "identity"), [], [], ((1.0, 0.0, 1.0), (0.0, 0.0, 0.0)))


def test_compose_on_the_cpu_and_without_colliders():
    g = torch.Generator().manual_seed(1)
    cam = cc.camera((67, 45), "identity")
    img, rgb, shade = (torch.rand(3, 45, 67, generator=g) for _ in range(3))
    alpha = torch.rand(3, 45, 67, generator=g)
    hit = (torch.rand(45, 67, generator=g) < 0.4).to(torch.int32) - 1
    out = CD.compose(cam, img, rgb, alpha, shade, hit)
    m = hit >= 0
    assert torch.equal(out[:, ~m], img[:, ~m]) and torch.equal(out[:, m], (rgb + (1 - alpha[0]) * shade)[:, m])
    stripe = CD.compose(cam, img, rgb, alpha, shade, hit, tile_rows=(1, 2), out=torch.full_like(img, 7.0))
    assert torch.equal(stripe[:, 16:32], out[:, 16:32]) and bool((stripe[:, :16] == 7).all()) and bool((stripe[:, 32:] == 7).all())
    t, sh, h = CD.cast(cam, [], [])
    assert bool(torch.isinf(t).all()) and bool((h == -1).all()) and bool((sh == 0).all())
    assert CD.draw(img, cam, [], [], X.IDENTITY, None, None, None) is img


@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_parity_scenes_stay_inside_the_exclusion_cap(case):
    """The scenes of the GPU parity tests: at most 2 % of the pixels and 1 % of the Gaussians sit within the decision margins, each
    case shows something, and outside the margins the fp32 evaluation of the definition takes the branches fp64 takes."""
    e = cc.evaluated(case)
    assert float(e["unsure"].double().mean()) <= 0.02 and float(e["hidden_unsure"].double().mean()) <= 0.01
    assert 0.03 < float((e["hit"] >= 0).double().mean()) < 0.9 and 0.05 < float(e["hidden"].double().mean()) < 0.7
    assert torch.equal(e["hit32"][~e["unsure"]], e["hit"][~e["unsure"]])
    assert torch.equal(e["hidden32"][~e["hidden_unsure"]], e["hidden"][~e["hidden_unsure"]])
    assert 0 < e["err_t"] < 1e-4 and 0 < e["err_shade"] < 1e-4
    if case[0] == "eight":
        assert len(set(e["hit"].reshape(-1).tolist())) >= 7


def test_abi_and_build_list_carry_the_drawing_calls():
    from neuma_amd import _lib
    text = (ROOT / "include" / "neuma_hip.h").read_text()
    for name in ("nm_collider_cast", "nm_collider_hide", "nm_collider_compose"):
        m = re.search(rf"\bint {name}\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert m and name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(m.group(1).split(","))
    body = re.search(r"typedef struct nm_collider_style \{(.*?)\} nm_collider_style;", text, flags=re.S).group(1)
    assert [n for n in re.findall(r"float (\w+)", body)] == [f[0] for f in _lib.nm_collider_style._fields_]
    import ctypes
    assert ctypes.sizeof(_lib.nm_collider_style) == 16
    mk = (ROOT / "neuma_amd" / "csrc" / "Makefile").read_text()
    assert "nm_draw.hip" in mk and "nm_collide_ray.h" in mk
