"""Forward-only multi-object driver: counterpart of /root/reference/experiments/inference.py:225-362 (and of the
single-object render.py:eval 260-332).

Order of one step, as the reference runs it (inference.py:309-314):
    stress = elasticity(F); state.from_torch(stress=stress)
    x, v, C, F = sim(statics, state)            # MPMForwardSim: in place on `state`
    F = plasticity(F); state.from_torch(F=F)
    statics_initializer.update(statics, step)   # span-based enabling takes effect AFTER the step
then, per object: particle positions (optionally de-normalised per object, nclaw/utils.py:121-135) and F are split by
`sections`, bound to the object's Gaussians with positions of the PREVIOUS rendered frame (tune/utils.py:475-523) and the
concatenated set is rasterised once per view with the camera of the first step.  The first frame is rendered from the
un-deformed Gaussians (deform_grad=None, inference.py:285-298).

Everything numeric runs in the HIP kernels; ComposeMaterial (material/preset.py) dispatches each section to its own net.
"""
from dataclasses import dataclass
from typing import Callable, Dict, Iterator, List, Optional, Sequence

import torch
import torch.nn as nn

from . import collider_draw
from .export import concat_gaussians, deformed_gaussians
from .field_paint import painted_gaussians
from .material import ComposeMaterial
from .render.transform_utils import scale_gaussians, translate_gaussians
from .sim import MPMForwardSim, MPMStateInitializer, MPMStaticsInitializer
from .sim.mpm import MPMInitData, MPMModel
from .tune import denormalize_points_helper_func, diff_rasterization, preprocess_for_rasterization


@dataclass
class SceneObject:
    """One simulated body: particles + statics (MPMInitData), its constitutive pair, its Gaussians and bindings."""
    init_data: MPMInitData
    elasticity: nn.Module
    plasticity: nn.Module
    gaussians: object            # GaussianModel
    bindings: object             # tune.Bindings or a torch sparse COO tensor (K x N_obj)
    scaling: float = 1.0         # scaling_modifier of the covariances (inference.py obj_scalings)
    rotate_sh: bool = False      # `gaussian.rotate_sh`: its SH colours turn with its Gaussians' deformation (no reference counterpart)
    name: str = ""               # the object's asset folder (`sim_data_name`)
    drive_mesh: Optional[str] = None   # `drive_mesh`: a triangle mesh in the asset frame that follows the object (inference.py)


def denormalize_points(points: torch.Tensor, sections: Sequence[int], state_init) -> torch.Tensor:
    """nclaw/utils.py:121-135"""
    out = []
    for gd, gx in zip(state_init.groups, torch.split(points, list(sections), dim=0)):
        out.append(denormalize_points_helper_func(gx, gd.size, gd.center))
    return torch.cat(out, dim=0)


@torch.no_grad()
def simulate_objects(model: MPMModel, objects: List[SceneObject], eval_steps: int, cameras: Sequence, background: torch.Tensor,
                     denormalize: bool = False, on_frame: Optional[Callable[[int, Dict], None]] = None,
                     render: bool = True, export: bool = False, draw_styles=None, draw_mesh_styles=None, painter=None, meter=None,
                     init_state=None, rigid_log=None) -> Iterator[Dict]:
    """Generator over frames 0..eval_steps.  Yields {'step', 'x', 'F', 'means3D', 'images': [per camera]}, from frame 1
    'deform_grad', the bound deformation gradients (K,3,3), and with `render` 'shs', the coefficients the frame was rendered with:
    those of an object with `rotate_sh` are rotated once per frame, before the views, by the polar rotations of its bound
    deformation gradients; frame 0 (un-deformed) carries them as loaded.  `init_state` = (x, v, C, F) replaces the particle state
    the objects' init_data give (the render driver's fitted initial positions and velocities).
    With `export` every frame also carries 'gaussians': one GaussianModel of all objects in object order, the frame as a standard
    3DGS parameter set (export.deformed_gaussians per object: its own `scaling` baked in, its own `rotate_sh` honoured).
    With `draw_styles` (collider_draw.parse_styles of the model's colliders) every image has the colliders drawn in, at the centres
    the model holds for that frame; `denormalize` then needs one alignment for all objects (ValueError otherwise).  With
    `draw_mesh_styles` too (collider_draw.parse_mesh_styles of the mesh entries) the model's field colliders are drawn as well.
    With `painter` (field_paint.FieldPainter) every frame also carries 'values' (N,), the painter's quantity per particle (frame 0:
    F = I, the initial velocities, the stress of I), 'paint_shs' (K,1,3), each object's Gaussians painted through its own bindings
    over one shared range, with `render` 'paint_images', the views once more at sh_degree 0 with those coefficients (colliders
    drawn in alike), and with `export` 'paint_gaussians', the frame's Gaussians with the painted DC colour and no rest coefficients.
    With `meter` (contact.ContactMeter of the model) every step's contact rows are recorded before the colliders move, one frame per
    step; nothing is read back here.  With `rigid_log` (rigid.RigidLog of a model with rigid bodies) every step's body states are
    kept on the device after the bodies moved, with the contact mass each was moved by."""
    device = model.device
    state_initializer = MPMStateInitializer(model)
    statics_initializer = MPMStaticsInitializer(model)
    for o in objects:
        state_initializer.add_group(o.init_data)
        statics_initializer.add_group(o.init_data)
    state, sections = state_initializer.finalize()
    statics = statics_initializer.finalize()
    if init_state is not None:
        state.from_torch(*init_state)
    x, v, C, F, stress = state.to_torch()
    elasticity = ComposeMaterial([o.elasticity for o in objects], sections).to(device).eval()
    plasticity = ComposeMaterial([o.plasticity for o in objects], sections).to(device).eval()
    sim = MPMForwardSim(model)
    gs = [o.gaussians for o in objects]
    scal = [o.scaling for o in objects]
    sec_gaussians = [int(g.get_xyz.shape[0]) for g in gs]
    if not denormalize:                                                # inference.py:275-281
        for g, gd in zip(gs, state_initializer.groups):
            scale_gaussians(g, float(gd.size[0]), torch.zeros(3, device=device))
            translate_gaussians(g, torch.as_tensor(gd.center, dtype=torch.float32, device=device))
    sh_deg = gs[0].active_sh_degree
    to_render = collider_draw.IDENTITY
    if draw_styles is not None and denormalize:
        maps = [collider_draw.map_from_alignment(gd.size, gd.center) for gd in state_initializer.groups]
        if any(m != maps[0] for m in maps[1:]):
            raise ValueError("draw_colliders with denormalize: the objects' ori_bounds -> sim_bounds alignments differ, so there is no "
                             "single render space to draw the colliders in (render without denormalize, or align the objects alike)")
        to_render = maps[0]

    def drawn(img, cam, means3D, deform_grad, cov, opa, shs, degree=None):
        if draw_styles is None:
            return img
        front = collider_draw.front_renderer(means3D, deform_grad, cam, sh_deg if degree is None else degree, cov, shs)
        fields = model.field_colliders if draw_mesh_styles is not None else ()
        return collider_draw.draw(img, cam, model.colliders, draw_styles, to_render, front, means3D, opa, fields, draw_mesh_styles or ())

    def painted(frame, v, F_now, means3D, deform_grad, cov, opa):
        """the painter's part of a frame (see the docstring)"""
        shs = painter.frame(frame["x"], v, F_now, elasticity, bindings, sections=sections)
        frame["values"], frame["paint_shs"] = painter.last_q, shs
        if render:
            frame["paint_images"] = [drawn(diff_rasterization(means3D, deform_grad, None, cam, background, 0, cov, opa, shs), cam, means3D,
                                           deform_grad, cov, opa, shs, 0) for cam in cameras]
        if export:
            frame["paint_gaussians"] = painted_gaussians(frame["gaussians"], shs)

    bindings = [o.bindings for o in objects]
    first = dict(step=0, x=x.clone(), F=F.clone(), means3D=torch.cat([g.get_xyz for g in gs], 0), images=[])
    if render:
        cov = torch.cat([g.get_covariance(s) for g, s in zip(gs, scal)], 0)
        opa = torch.cat([g.get_opacity for g in gs], 0)
        shs = torch.cat([g.get_features for g in gs], 0)
        for cam in cameras:
            img = diff_rasterization(first["means3D"], None, None, cam, background, sh_deg, cov, opa, shs)
            first["images"].append(drawn(img, cam, first["means3D"], None, cov, opa, shs))
        first["shs"] = shs
    if export:
        first["gaussians"] = concat_gaussians([deformed_gaussians(g, g.get_xyz, scaling_modifier=s) for g, s in zip(gs, scal)])
    if painter is not None:
        painted(first, v, torch.eye(3, dtype=F.dtype, device=device).expand_as(F).contiguous(), first["means3D"], None,
                cov if render else None, opa if render else None)
    if on_frame:
        on_frame(0, first)
    yield first
    de_x = denormalize_points(x, sections, state_initializer) if denormalize else x
    p_prev = [t.clone().detach() for t in torch.split(de_x, sections, dim=0)]
    k_prev = [g.get_xyz.clone().detach() for g in gs]
    rotate_sh = [bool(o.rotate_sh) for o in objects] if (render or export) and any(o.rotate_sh for o in objects) else None
    for step in range(1, eval_steps + 1):
        stress = elasticity(F)
        state.from_torch(stress=stress)
        x, v, C, F = sim(statics, state)
        if meter is not None:
            meter.record()
            meter.frame()
        model.step_colliders()                                         # moving colliders and rigid bodies: one substep further
        if rigid_log is not None:
            rigid_log.after_step()
        F = plasticity(F)
        state.from_torch(F=F)
        statics_initializer.update(statics, step)
        de_x = denormalize_points(x, sections, state_initializer) if denormalize else x
        p_curr = list(torch.split(de_x, sections, dim=0))
        dgs = list(torch.split(F, sections, dim=0))
        pack = preprocess_for_rasterization(obj_gaussians=gs, obj_deform_grad=dgs, obj_kernels_prev=k_prev, obj_particles_curr=p_curr,
                                            obj_particles_prev=p_prev, obj_bindings=bindings, obj_scalings=scal,
                                            obj_rotate_sh=rotate_sh)
        frame = dict(step=step, x=x.clone(), F=F.clone(), means3D=pack["means3D"], deform_grad=pack["deform_grad"], images=[])
        if render:
            for cam in cameras:
                img = diff_rasterization(pack["means3D"], pack["deform_grad"], None, cam, background,
                                         pack["active_sh_degree"], pack["cov3D"], pack["opacity"], pack["shs"])
                frame["images"].append(drawn(img, cam, pack["means3D"], pack["deform_grad"], pack["cov3D"], pack["opacity"], pack["shs"]))
            frame["shs"] = pack["shs"]
        if export:
            parts = [torch.split(pack[k], sec_gaussians, dim=0) for k in ("means3D", "deform_grad", "shs")]
            frame["gaussians"] = concat_gaussians([
                deformed_gaussians(g, m, dg, sh if (rotate_sh is not None and rotate_sh[i]) else None, s)
                for i, (g, m, dg, sh, s) in enumerate(zip(gs, *parts, scal))])
        if painter is not None:
            painted(frame, v, F, pack["means3D"], pack["deform_grad"], pack["cov3D"], pack["opacity"])
        if on_frame:
            on_frame(step, frame)
        yield frame
        p_prev = [t.clone().detach() for t in torch.split(de_x, sections, dim=0)]
        k_prev = [t.clone().detach() for t in torch.split(pack["means3D"], sec_gaussians, dim=0)]
