"""Drawing colliders in renders (no reference counterpart): a ray cast of the collider set per pixel, occlusion per Gaussian and the
composition with the rasterizer's images, on the native kernels of csrc/nm_draw.hip.  Definition: include/neuma_hip.h ("Drawing
colliders") and DESIGN.md section 7; the same in torch fp64: neuma_amd/extras/collider_draw.py, which is also what runs for
tensors on the CPU.  The rasterizer itself is untouched: a drawn frame is the usual image plus two more renders with the hidden
Gaussians' opacities zeroed (`render_front`) and three small launches.

    sim:
      draw_colliders: true            # or --draw_colliders on python -m neuma_amd.inference / neuma_amd.render
      colliders:
        - {type: plane, point: [0.5, 0.3, 0.5], normal: [0, 1, 0], color: [0.8, 0.8, 0.75], checker: 0.125}
        - {type: sphere, center: [0.5, 0.4, 0.5], radius: 0.08, color: [0.9, 0.3, 0.2]}

`color` (rgb in 0..1) defaults to a fixed palette by index, `checker` (cell size in simulation units, planes only; 0 = plain) to
0.125.  Occlusion is per Gaussian: one whose centre is behind or inside a drawn solid is dropped as a whole.  Not differentiated.

Mesh colliders (`type: mesh`) are drawn with `draw_mesh_colliders: true` / --draw_mesh_colliders, which implies draw_colliders: a
sphere trace of each collider's signed distance field (k_field_cast / k_field_hide, csrc/nm_field_ray.h; definition:
include/neuma_hip.h "Drawing mesh colliders", fp64: neuma_amd/extras/mesh_draw.py) merged into the analytic cast's buffers - what
is drawn is the solid the simulator collides with, at the lattice's resolution.  Mesh entries take `color`; `checker` is ignored.
"""
import ctypes as C
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import _lib as L
from .extras import collider_draw as X
from .extras import mesh_draw as XM
from .sim.colliders import MAX_COLLIDERS, MAX_FIELD_COLLIDERS, Plane, pack, pack_fields

IDENTITY = X.IDENTITY
PALETTE = ((0.78, 0.78, 0.74), (0.85, 0.33, 0.25), (0.25, 0.52, 0.85), (0.35, 0.72, 0.40),
           (0.90, 0.72, 0.25), (0.62, 0.42, 0.80), (0.30, 0.75, 0.75), (0.85, 0.50, 0.65))
DEFAULT_CHECKER = 0.125


@dataclass(frozen=True)
class Style:
    color: Tuple[float, float, float]
    checker: float = 0.0


def parse_style(node, index: int = 0) -> Style:
    """The drawing keys of one `sim.colliders` entry (a dict, or a collider object: defaults).  Errors name the entry and the field."""
    get = node.get if hasattr(node, "get") else (lambda k, d=None: d)
    is_plane = isinstance(node, Plane) or get("type") == "plane"
    color, checker = get("color", PALETTE[index % len(PALETTE)]), get("checker", DEFAULT_CHECKER if is_plane else 0.0)
    try:
        col = tuple(float(a) for a in color)
    except (TypeError, ValueError):
        col = ()
    if len(col) != 3 or not all(0.0 <= a <= 1.0 for a in col):
        raise ValueError(f"collider {index}: color: three numbers in 0..1 expected, got {color!r}")
    try:
        chk = float(checker)
    except (TypeError, ValueError):
        chk = float("nan")
    if not (0.0 <= chk < float("inf")):
        raise ValueError(f"collider {index}: checker: a finite cell size >= 0 expected, got {checker!r}")
    return Style(col, chk if is_plane else 0.0)


def parse_styles(nodes) -> List[Style]:
    """A `sim.colliders` list -> one Style per entry, in order (parse_collider ignores the keys read here)."""
    nodes = [] if nodes is None else list(nodes)
    if len(nodes) > MAX_COLLIDERS:
        raise ValueError(f"colliders: n = {len(nodes)} outside 0..{MAX_COLLIDERS}")
    return [parse_style(n, i) for i, n in enumerate(nodes)]


def parse_mesh_styles(nodes, first_index: int = 0) -> List[Style]:
    """The mesh entries of a `sim.colliders` list (those behind its `first_index` analytic entries) -> one Style per entry.  Only
    `color` is read - the palette default goes by the index in the whole list - and `checker` is ignored."""
    nodes = [] if nodes is None else list(nodes)
    if len(nodes) > MAX_FIELD_COLLIDERS:
        raise ValueError(f"colliders: {len(nodes)} mesh colliders, at most {MAX_FIELD_COLLIDERS}")
    out = []
    for i, n in enumerate(nodes):
        get = n.get if hasattr(n, "get") else (lambda k, d=None: d)
        out.append(Style(parse_style({"color": get("color", PALETTE[(first_index + i) % len(PALETTE)])}, first_index + i).color, 0.0))
    return out


def mesh_wanted(cfg, sim_cfg) -> bool:
    """--draw_mesh_colliders on the command line or `sim.draw_mesh_colliders: true` in the config (it implies draw_colliders)"""
    return bool(cfg.get("draw_mesh_colliders", False) or (sim_cfg is not None and sim_cfg.get("draw_mesh_colliders", False)))


def wanted(cfg, sim_cfg) -> bool:
    """--draw_colliders on the command line or `sim.draw_colliders: true` in the config"""
    return bool(cfg.get("draw_colliders", False) or (sim_cfg is not None and sim_cfg.get("draw_colliders", False)))


def map_from_alignment(size, center) -> Tuple[Tuple[float, ...], Tuple[float, ...]]:
    """to_render of de-normalised renders: the inverse of the ori_bounds -> sim_bounds alignment p_s = size * p_r + center
    (denormalize_points_helper_func), per axis."""
    import numpy as np
    s = np.broadcast_to(np.asarray(size, dtype=np.float64).reshape(-1), (3,))
    c = np.broadcast_to(np.asarray(center, dtype=np.float64).reshape(-1), (3,))
    return tuple(float(1.0 / a) for a in s), tuple(float(-b / a) for a, b in zip(s, c))


def _vec(values, ctype=C.c_float):
    v = [float(a) for a in values]
    return (ctype * len(v))(*v)


def _cfg(cam, tile_rows: Optional[Tuple[int, int]] = None) -> L.nm_raster_cfg:
    """The fields of nm_raster_cfg the drawing calls read: image size, campos and the stripe."""
    cfg = L.nm_raster_cfg()
    cfg.image_height, cfg.image_width = int(cam.image_height), int(cam.image_width)
    cfg.campos = _vec(cam.camera_center.detach().float().cpu().reshape(3))
    pm = cam.full_proj_transform.detach().float().cpu().reshape(16)
    cfg.projmatrix = _vec(pm)
    cfg.tile_y0, cfg.tile_y1 = tile_rows if tile_rows is not None else (0, 0)
    return cfg


def _styles(styles: Sequence[Style]):
    if not styles:
        return None
    arr = (L.nm_collider_style * len(styles))()
    for out, s in zip(arr, styles):
        out.color = _vec(s.color)
        out.checker = float(s.checker)
    return arr


def cast(cam, colliders: Sequence, styles: Sequence[Style], to_render=IDENTITY, device=None):
    """t (H,W; +inf where nothing is hit), shade (3,H,W), hit (H,W int32: collider index or -1) of the camera's pixel rays.
    device: a GPU -> k_collider_cast; None / cpu -> the fp64 definition (returned as fp32)."""
    if len(colliders) != len(styles):
        raise ValueError(f"styles: {len(styles)} for {len(colliders)} colliders")
    dev = torch.device(device) if device is not None else cam.full_proj_transform.device
    if dev.type != "cuda":
        t, shade, hit = X.cast(cam, colliders, styles, to_render)
        return t.float(), shade.float(), hit
    H, W = int(cam.image_height), int(cam.image_width)
    t = torch.empty(H, W, dtype=torch.float32, device=dev)
    shade = torch.empty(3, H, W, dtype=torch.float32, device=dev)
    hit = torch.empty(H, W, dtype=torch.int32, device=dev)
    inv = _vec(X.inverse_projection(cam).reshape(16), C.c_double)
    L.check(L.lib().nm_collider_cast(C.byref(_cfg(cam)), inv, _vec(to_render[0]), _vec(to_render[1]), len(colliders), pack(colliders),
                                     _styles(styles), L.ptr(t), L.ptr(shade), L.ptr(hit), L.stream_ptr(dev)), "nm_collider_cast")
    return t, shade, hit


def front_opacity(cam, colliders: Sequence, means3D: Tensor, opacity: Tensor, to_render=IDENTITY, want_hidden: bool = False):
    """opacity (K,1) with the entries of the Gaussians hidden from the camera zeroed [, the hidden flags (K,) uint8]."""
    if not means3D.is_cuda:
        hid = X.hidden(cam.camera_center, colliders, means3D, to_render)
        out = torch.where(hid[:, None], torch.zeros_like(opacity), opacity)
        return (out, hid.to(torch.uint8)) if want_hidden else out
    m = means3D.detach().float().contiguous()
    op = opacity.detach().float().contiguous()
    K = m.shape[0]
    if op.numel() != K:
        raise ValueError(f"opacity: {op.numel()} values for {K} Gaussians")
    out = torch.empty_like(op)
    hid = torch.empty(K, dtype=torch.uint8, device=m.device) if want_hidden else None
    campos = _vec(cam.camera_center.detach().float().cpu().reshape(3))
    L.check(L.lib().nm_collider_hide(campos, _vec(to_render[0]), _vec(to_render[1]), len(colliders), pack(colliders), K, L.ptr(m),
                                     L.ptr(op), L.ptr(out), L.ptr(hid), L.stream_ptr(m.device)), "nm_collider_hide")
    return (out, hid) if want_hidden else out


def cast_field(cam, fields: Sequence, styles: Sequence[Style], t: Tensor, shade: Tensor, hit: Tensor, hit_base: int,
               to_render=IDENTITY):
    """The field pass behind `cast`: the pixel rays' nearest hits of the field colliders' drawn solids merged into t, shade, hit
    (what `cast` returned; a field hit replaces a pixel only where its t is strictly smaller; hit becomes hit_base + index).
    GPU tensors are updated in place by k_field_cast and returned; CPU tensors go through the fp64 definition (new fp32 tensors)."""
    if len(fields) != len(styles):
        raise ValueError(f"styles: {len(styles)} for {len(fields)} field colliders")
    if not t.is_cuda:
        t2, shade2, hit2 = XM.cast_field(cam, fields, styles, to_render, t, shade, hit, hit_base)
        return t2.float(), shade2.float(), hit2
    H, W = int(cam.image_height), int(cam.image_width)
    for x, shape, dt in ((t, (H, W), torch.float32), (shade, (3, H, W), torch.float32), (hit, (H, W), torch.int32)):
        if tuple(x.shape) != shape or x.dtype != dt or not x.is_contiguous():
            raise ValueError(f"cast_field: a contiguous {dt} tensor of shape {shape} expected, got {x.dtype} {tuple(x.shape)}")
    inv = _vec(X.inverse_projection(cam).reshape(16), C.c_double)
    L.check(L.lib().nm_collider_cast_field(C.byref(_cfg(cam)), inv, _vec(to_render[0]), _vec(to_render[1]), len(fields), pack_fields(fields),
                                           _styles(styles), int(hit_base), L.ptr(t), L.ptr(shade), L.ptr(hit), L.stream_ptr(t.device)),
            "nm_collider_cast_field")
    return t, shade, hit


def front_opacity_field(cam, fields: Sequence, means3D: Tensor, opacity_front: Tensor, to_render=IDENTITY, hidden: Optional[Tensor] = None):
    """The field pass behind `front_opacity`: opacity_front (K,1) with the entries of the Gaussians the field colliders hide zeroed
    too [and `hidden` (K,) uint8 with their flags set].  GPU tensors (contiguous fp32 / uint8) are updated in place by k_field_hide."""
    if not means3D.is_cuda:
        more = XM.hidden_field(cam.camera_center, fields, means3D, to_render)
        out = torch.where(more[:, None], torch.zeros_like(opacity_front), opacity_front)
        return out if hidden is None else (out, (more | hidden.bool()).to(torch.uint8))
    m = means3D.detach().float().contiguous()
    K = m.shape[0]
    if opacity_front.numel() != K or opacity_front.dtype != torch.float32 or not opacity_front.is_contiguous():
        raise ValueError(f"opacity_front: {K} contiguous fp32 values expected")
    if hidden is not None and (hidden.numel() != K or hidden.dtype != torch.uint8 or not hidden.is_contiguous()):
        raise ValueError(f"hidden: {K} contiguous uint8 values expected")
    campos = _vec(cam.camera_center.detach().float().cpu().reshape(3))
    L.check(L.lib().nm_collider_hide_field(campos, _vec(to_render[0]), _vec(to_render[1]), len(fields), pack_fields(fields), K, L.ptr(m),
                                           L.ptr(opacity_front), L.ptr(hidden), L.stream_ptr(m.device)), "nm_collider_hide_field")
    return opacity_front if hidden is None else (opacity_front, hidden)


def compose(cam, img_all: Tensor, rgb_front: Tensor, a_front: Tensor, shade: Tensor, hit: Tensor,
            tile_rows: Optional[Tuple[int, int]] = None, out: Optional[Tensor] = None) -> Tensor:
    """rgb_front + (1 - a_front) shade where hit >= 0, img_all elsewhere.  a_front: (3,H,W) (channel 0 is used) or (H,W).
    tile_rows = (tile_y0, tile_y1): only the pixel rows of that stripe of 16-row tiles are written (into `out`, or into zeros)."""
    H, W = int(cam.image_height), int(cam.image_width)
    alpha = a_front[0] if a_front.dim() == 3 else a_front
    if not img_all.is_cuda:
        rows = None if tile_rows is None or tile_rows[1] <= tile_rows[0] else (min(16 * tile_rows[0], H), min(16 * tile_rows[1], H))
        return X.compose(img_all, rgb_front, alpha, shade, hit, rows, out)
    full = tile_rows is None or tile_rows[1] <= tile_rows[0]
    if out is None:
        out = (torch.empty if full else torch.zeros)(3, H, W, dtype=torch.float32, device=img_all.device)
    ins = [t.detach().float().contiguous() for t in (img_all, rgb_front, alpha, shade)]
    for t, shape in zip(ins + [out], ((3, H, W), (3, H, W), (H, W), (3, H, W), (3, H, W))):
        if tuple(t.shape) != shape:
            raise ValueError(f"compose: an image of shape {tuple(t.shape)} where {shape} is expected")
    if tuple(hit.shape) != (H, W) or hit.dtype != torch.int32:
        raise ValueError("compose: hit must be (H,W) int32")
    L.check(L.lib().nm_collider_compose(C.byref(_cfg(cam, tile_rows)), L.ptr(ins[0]), L.ptr(ins[1]), L.ptr(ins[2]), L.ptr(ins[3]),
                                        L.ptr(hit.contiguous()), L.ptr(out), L.stream_ptr(out.device)), "nm_collider_compose")
    return out


_BG0 = {}      # device -> the black background of the front passes (one tensor: the rasterizer caches cameras by it)


def draw(img_all: Tensor, cam, colliders: Sequence, styles: Sequence[Style], to_render,
         render_front: Callable[[Tensor, Tensor], Tuple[Tensor, Tensor]], means3D: Tensor, opacity: Tensor,
         fields: Sequence = (), field_styles: Sequence[Style] = ()) -> Tensor:
    """One drawn view.  img_all: the view as rendered today; means3D (K,3), opacity (K,1): what it was rendered from.
    render_front(opacity_front, bg0) -> (rgb_front, a_front): the frame's colours and a colors_precomp = 1 pass, both with the
    given opacities over the black background bg0 (front_renderer builds it from diff_rasterization).  fields, field_styles:
    the model's field (mesh) colliders and parse_mesh_styles of their entries; their two passes run behind the analytic ones.
    Without colliders the image is returned as it is."""
    if not colliders and not fields:
        return img_all
    t, shade, hit = cast(cam, colliders, styles, to_render, device=img_all.device)
    op_front = front_opacity(cam, colliders, means3D, opacity, to_render)
    if fields:
        _, shade, hit = cast_field(cam, fields, field_styles, t, shade, hit, len(colliders), to_render)
        op_front = front_opacity_field(cam, fields, means3D, op_front, to_render)
    bg0 = _BG0.get(img_all.device)
    if bg0 is None:
        bg0 = _BG0[img_all.device] = torch.zeros(3, dtype=torch.float32, device=img_all.device)
    rgb_front, a_front = render_front(op_front, bg0)
    return compose(cam, img_all, rgb_front, a_front, shade, hit)


def front_renderer(means3D: Tensor, deform_grad: Optional[Tensor], cam, sh_degree: int, cov3D: Tensor, shs: Tensor):
    """render_front for `draw` through tune.diff_rasterization: the same Gaussians as img_all, other opacities and background."""
    from .tune import diff_rasterization

    def render_front(opacity_front: Tensor, bg0: Tensor):
        rgb = diff_rasterization(means3D, deform_grad, None, cam, bg0, sh_degree, cov3D, opacity_front, shs)
        alpha = diff_rasterization(means3D, deform_grad, None, cam, bg0, sh_degree, cov3D, opacity_front, shs, force_mask_data=True)
        return rgb, alpha
    return render_front
