"""Scenes shared by tests/test_mesh_draw_cpu.py and tests/test_gpu_mesh_draw.py: signed distance fields built on the CPU
(extras.mesh_sdf.build_mesh_field, margin_cells = 2) from the torus, the rotated box and the icosahedron of tests/mesh_sdf_cases.py
at resolutions 24 and 48; the cameras, maps, image sizes and the 1500 Gaussians of tests/collider_draw_cases.py; one combined set
(the analytic set `eight` plus two fields that overlap it) and one field pushed half-way out of the unit cube, so that a cube-face
hit occurs.  Plus the fp64 / fp32 evaluations of the definition (neuma_amd/extras/collider_draw.py, then
neuma_amd/extras/mesh_draw.py on its buffers) per case, computed once and cached."""
import functools
from dataclasses import replace

import torch

import collider_draw_cases as cc
import mesh_sdf_cases as cases
from neuma_amd.collider_draw import parse_mesh_styles, parse_styles
from neuma_amd.extras import collider_draw as X
from neuma_amd.extras import mesh_draw as XM
from neuma_amd.extras import mesh_sdf
from neuma_amd.sim.colliders import FieldCollider, parse_colliders

MESHES = ("torus", "box", "icosahedron")
RESOLUTIONS = (24, 48)
MARGIN_CELLS = 2
PUSH = (0.5, 0.0, 0.0)          # the icosahedron (centre x = 0.5, radius 0.3) moved to centre x = 1: the cube's face x = 1 cuts it

# (fields, analytic set or None, size, map)
SINGLE = [((m, r), None, size, mp) for m in MESHES for r in RESOLUTIONS for size in cc.SIZES for mp in cc.MAPS]
COMBINED = [(("torus", 24, "box", 24), "eight", (128, 80), mp) for mp in cc.MAPS]
PUSHED = [(("icosahedron", 24, "pushed"), None, size, "identity") for size in cc.SIZES]
CASES = SINGLE + COMBINED + PUSHED


def case_id(case):
    f, s, (W, H), m = case
    return "-".join(str(x) for x in f) + (f"+{s}" if s else "") + f"-{W}x{H}-{m}"


@functools.lru_cache(maxsize=None)
def field(mesh: str, resolution: int) -> FieldCollider:
    """The mesh's field as the simulator would hold it, on the CPU: phi in fp32 (what the kernels read)"""
    v, t = cases.MESHES[mesh]()
    f = mesh_sdf.build_mesh_field(v, t, None, resolution, MARGIN_CELLS)
    return FieldCollider(phi=torch.from_numpy(f.phi).float().contiguous(), origin=f.origin, spacing=f.spacing, dims=f.dims)


def fields_of(spec):
    """('torus', 24) / ('torus', 24, 'box', 24) / ('icosahedron', 24, 'pushed') -> the FieldColliders"""
    if spec[-1] == "pushed":
        c = field(spec[0], spec[1])
        return [replace(c, origin=tuple(o + p for o, p in zip(c.origin, PUSH)))]
    return [field(spec[i], spec[i + 1]) for i in range(0, len(spec), 2)]


def on_device(fields, device):
    return [replace(c, phi=c.phi.to(device).contiguous()) for c in fields]


def cast_both(cam, colliders, styles, fields, field_styles, tr, dtype=torch.float64, margins=False, **kw):
    """the analytic cast, then the field pass on its buffers: (t, shade, hit[, unsure, steps])"""
    res = X.cast(cam, colliders, styles, tr, dtype=dtype, margins=margins)
    out = XM.cast_field(cam, fields, field_styles, tr, res[0], res[1], res[2], len(colliders), dtype=dtype, margins=margins, **kw)
    if margins:
        return out[:3] + (out[3] | res[3], out[4])
    return out


@functools.lru_cache(maxsize=None)
def evaluated(case):
    """dict of one case: cam, colliders, styles, fields, field_styles, to_render, means, opacity; the fp64 definition t, shade, hit,
    unsure, steps (pixels), hidden, hidden_unsure (Gaussians); the fp32 evaluation's hit32 / hidden32 and err_t (relative) /
    err_shade (absolute): its distance from fp64 outside the unsure set - what the kernels' own distance is measured against."""
    spec, analytic, size, map_name = case
    cam, tr = cc.camera(size, map_name), cc.MAPS[map_name]
    nodes = cc.SETS[analytic] if analytic else []
    colliders, styles = parse_colliders(nodes), parse_styles(nodes)
    fields = fields_of(spec)
    field_styles = parse_mesh_styles([{} for _ in fields], len(colliders))
    means, opacity = cc.gaussians(map_name)
    t, shade, hit, unsure, steps = cast_both(cam, colliders, styles, fields, field_styles, tr, margins=True)
    t32, shade32, hit32 = cast_both(cam, colliders, styles, fields, field_styles, tr, dtype=torch.float32)
    hid_a, unsure_a = X.hidden(cam.camera_center, colliders, means, tr, margins=True)
    hid, unsure_f = XM.hidden_field(cam.camera_center, fields, means, tr, hid_a, margins=True)
    hid32 = XM.hidden_field(cam.camera_center, fields, means, tr, X.hidden(cam.camera_center, colliders, means, tr, dtype=torch.float32),
                            dtype=torch.float32)
    ok = ~unsure
    return dict(cam=cam, colliders=colliders, styles=styles, fields=fields, field_styles=field_styles, to_render=tr, means=means,
                opacity=opacity, t=t, shade=shade, hit=hit, unsure=unsure, steps=steps, hidden=hid, hidden_unsure=unsure_a | unsure_f,
                hit32=hit32, hidden32=hid32, err_t=cc.t_error(t32, t, hit, ok), err_shade=float((shade32.double() - shade)[:, ok].abs().max()))
