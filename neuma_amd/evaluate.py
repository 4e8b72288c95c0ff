"""Forward-only roll-out + rendering of a fine-tuned experiment: counterpart of /root/reference/experiments/render.py:109-347
(`eval`), reachable as `python -m neuma_amd.render -c <config.yaml> -vn <name> [-es N] [-l 0100_lora.pt] [-dv view ...]`.

Per step (render.py:304-332): stress = E(F) -> state.from_torch(stress) -> in-place MPMForwardSim -> F = P(F) ->
state.from_torch(F) -> statics_initializer.update(statics, step) -> de-normalise, bind with the PREVIOUS frame's positions,
render the debug views with the camera of the FIRST step -> <result>/<name>/images_<video_name>/<view>_<frame:03d>.png.
The YAML's own sim.eps is used here (the reference only overrides it in finetune.py).  Packing the frames into an mp4
(mediapy) is left to external tools.

`gaussian.rotate_sh: true` (or --rotate_sh; no reference counterpart): from sh_degree 1 the SH colours turn with each
Gaussian's deformation - rotate_shs_by_deformation once per frame, before the views; the first frame is untouched.

`--save_gaussians NAME` (no reference counterpart): every frame, the first one included, also goes to
<result>/<name>/gaussians_NAME/<frame:03d>.ply as a standard 3DGS parameter set (export.save_frame: scaling_modifier baked in, the
rotated coefficients when rotate_sh is on), also with an empty -dv list; `python -m neuma_amd.replay` renders such a folder from
any camera.

`--draw_colliders` (or `sim.draw_colliders: true`; no reference counterpart): the colliders of `sim.colliders` are drawn into every
frame, under the inverse of the ori_bounds -> sim_bounds alignment (neuma_amd/collider_draw.py).  `--draw_mesh_colliders` (or
`sim.draw_mesh_colliders: true`) implies it and draws the mesh colliders too.

`--report_contacts` (or `sim.report_contacts: true`; no reference counterpart): the force and the torque on the box walls and on each
collider per frame -> <result>/<name>/contacts_<video_name>.csv, and a summary at the end (neuma_amd/contact.py; simulation units).
Images and particle files are what they are without it.

`--color_by QUANTITY [--color_range LO HI] [--colormap NAME]` (or `gaussian.color_by` / `color_range` / `colormap`; no reference
counterpart): every frame, the first included, is rendered a second time per view with each Gaussian coloured by the mean of
speed, displacement, volume, strain, pressure or von_mises over its bound particles (neuma_amd/field_paint.py) ->
images_<video_name>_<quantity>/; colliders are drawn in as in the ordinary frames.  Without --color_range every frame is scaled by
its own range and the sequence's overall range is printed at the end.  With --save_gaussians NAME the painted frames also go to
gaussians_NAME_<quantity>/ (degree-0 files: `python -m neuma_amd.replay ... --sh_degree 0`), and with --save_particles the particle
files gain a fourth float property named after the quantity.

`--save_mesh NAME [--mesh_resolution R] [--mesh_density_thres T]` (or `save_mesh` / `mesh_resolution` / `mesh_density_thres`; no
reference counterpart): every frame, the first included, also goes to <result>/<name>/meshes_NAME/<frame:03d>.ply as a closed
triangle mesh with vertex colours (neuma_amd/surface_mesh.py), built from the deformed model save_frame builds - with or without
--save_gaussians, also with an empty -dv list.  `mesh_density_thres` = 0.5 is a default nobody has tuned on a real capture yet.

`--drive_mesh PATH [--drive_mesh_name NAME] [--drive_mesh_k K] [--drive_mesh_format ply|obj]` (or config keys of the same names, top
level or under `gaussian`; no reference counterpart): the user's own mesh PATH (.obj / .ply, in the frame of kernels.ply and the
original particles - the de-normalised frame rendered here) follows the roll-out with its vertices, faces, UVs and materials as
they are (neuma_amd/mesh_drive.py); bound to frame 0's particles, every frame, the first included, goes to
<result>/<name>/driven_NAME/<frame:03d>.{ply,obj} (NAME: the file stem), also with an empty -dv list; with --color_by the vertices
carry the frame's colours."""
import argparse
import random
from pathlib import Path

import numpy as np
import torch

from . import collider_draw, contact, field_paint, io as nio
from .config import Cfg, load_config
from .export import deformed_gaussians, save_frame
from .finetune import particle_init_data, setup
from .sim import MPMForwardSim, MPMModelBuilder, MPMStateInitializer, MPMStaticsInitializer
from .sim.colliders import describe as describe_colliders, describe_fields as describe_field_colliders
from .render.transform_utils import rotate_shs_by_deformation
from .tune import compute_bindings_F, compute_bindings_xyz, denormalize_points_helper_func, diff_rasterization

RESULT = "experiments/results"


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--config", "-c", type=str, required=True)
    p.add_argument("--eval_steps", "-es", type=int, default=400)
    p.add_argument("--init_frame", "-if", type=int, default=None)
    p.add_argument("--skip_frames", "-sf", type=int, default=1)
    p.add_argument("--load_lora", "-l", type=str, default=None)
    p.add_argument("--video_name", "-vn", type=str, required=True)
    p.add_argument("--sim_dt", "-dt", type=float, default=None)
    p.add_argument("--debug_views", "-dv", nargs="+", default=[])
    p.add_argument("--save_particles", "-sp", type=str, default=None)
    p.add_argument("--save_gaussians", type=str, default=None,
                   help="Write every frame as a 3DGS .ply into gaussians_<name>/ (replay them with python -m neuma_amd.replay).")
    p.add_argument("--save_mesh", type=str, default=None,
                   help="Write every frame as a closed triangle mesh into meshes_<name>/ (neuma_amd/surface_mesh.py).")
    p.add_argument("--mesh_resolution", type=int, default=128, help="Lattice cells along the longest side of a frame's mesh.")
    p.add_argument("--mesh_density_thres", type=float, default=0.5,
                   help="Density level of the mesh surface (default not tuned on a real capture).")
    p.add_argument("--drive_mesh", type=str, default=None,
                   help="Drive this triangle mesh (.obj / .ply, in the frame of kernels.ply) with the roll-out into driven_<name>/ (neuma_amd/mesh_drive.py).")
    p.add_argument("--drive_mesh_name", type=str, default=None, help="Folder suffix of the driven frames (default: the file stem).")
    p.add_argument("--drive_mesh_k", type=int, default=None, help="Rest particles a vertex follows, 1..16 (default 16).")
    p.add_argument("--drive_mesh_format", type=str, default=None, choices=("ply", "obj"), help="Default ply.")
    p.add_argument("--change_base_model", "-cbm", type=str, default=None)
    p.add_argument("--dataset_path", type=str, default=None)
    p.add_argument("--transform_file", type=str, default=None)
    p.add_argument("--alpha", type=float, default=None)
    p.add_argument("--result_root", type=str, default=RESULT)
    p.add_argument("--rotate_sh", action="store_true", help="Rotate the SH colours with the deformation (gaussian.rotate_sh).")
    p.add_argument("--draw_colliders", action="store_true", help="Draw the colliders of sim.colliders into every frame (sim.draw_colliders).")
    p.add_argument("--draw_mesh_colliders", action="store_true",
                   help="Draw the mesh colliders too (sim.draw_mesh_colliders); implies --draw_colliders.")
    p.add_argument("--report_contacts", action="store_true",
                   help="Write the force and torque on the walls and on each collider per frame to contacts_<video_name>.csv (sim.report_contacts).")
    p.add_argument("--color_by", type=str, default=None, choices=field_paint.QUANTITIES,
                   help="Render every frame a second time, coloured by this particle quantity (gaussian.color_by).")
    p.add_argument("--color_range", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                   help="The value range of the colour map (gaussian.color_range); default: every frame's own range.")
    p.add_argument("--colormap", type=str, default=None, choices=sorted(field_paint.COLORMAPS), help="gaussian.colormap")
    return p.parse_args(argv)


def save_image(img: torch.Tensor, path) -> None:
    """torchvision.utils.save_image for one (3,H,W) image in [0,1].  No image leaves the GPU unchecked: a render whose bin lists
    overflowed (incomplete image) raises here (render.flush_pending)."""
    from .render import flush_pending
    flush_pending()
    from PIL import Image
    a = (img.detach().clamp(0, 1) * 255 + 0.5).to(torch.uint8).permute(1, 2, 0).cpu().numpy()
    Image.fromarray(a, "RGB").save(path)


@torch.no_grad()
def evaluate(cfg: Cfg, on_frame=None):
    seed = cfg.seed
    random.seed(seed); np.random.seed(seed); torch.manual_seed(seed)
    device = torch.device(f"cuda:{cfg.gpu}")
    torch.cuda.set_device(device)
    background = torch.tensor([1.0, 1.0, 1.0] if cfg.video_data.data.get("white_background", False) else [0.0, 0.0, 0.0], device=device)
    if cfg.get("alpha") is not None:
        cfg.constitution.lora.alpha = cfg.alpha
    exp_root = Path(cfg.root) / cfg.name
    assert exp_root.exists(), f"Experiment {exp_root} does not exist."
    tune_root = exp_root / "finetune"
    image_root = Path(cfg.get("result_root", RESULT)) / cfg.name / f"images_{cfg.video_name}"
    image_root.mkdir(exist_ok=True, parents=True)
    state_root = None
    if cfg.get("save_particles") is not None:
        state_root = Path(cfg.get("result_root", RESULT)) / cfg.name / f"states_{cfg.save_particles}"
        state_root.mkdir(parents=True, exist_ok=True)
    gauss_root = None
    if cfg.get("save_gaussians") is not None:
        gauss_root = Path(cfg.get("result_root", RESULT)) / cfg.name / f"gaussians_{cfg.save_gaussians}"
        gauss_root.mkdir(parents=True, exist_ok=True)
    mesh_root = None
    if cfg.get("save_mesh") is not None:
        mesh_root = Path(cfg.get("result_root", RESULT)) / cfg.name / f"meshes_{cfg.save_mesh}"
        mesh_root.mkdir(parents=True, exist_ok=True)
    painter = field_paint.painter_from_cfg(cfg, cfg.get("gaussian"))
    paint_root, paint_gauss_root = None, None
    if painter is not None:
        paint_root = Path(cfg.get("result_root", RESULT)) / cfg.name / f"images_{cfg.video_name}_{painter.quantity}"
        paint_root.mkdir(exist_ok=True, parents=True)
        if gauss_root is not None:
            paint_gauss_root = gauss_root.with_name(f"{gauss_root.name}_{painter.quantity}")
            paint_gauss_root.mkdir(parents=True, exist_ok=True)
        print(painter.describe())
    cfg.video_data.data.init_frame = cfg.get("init_frame")               # NOTE: manually setting (render.py:186-188)
    if cfg.get("debug_views"):
        cfg.video_data.data.used_views = list(cfg.debug_views)
    if cfg.get("dataset_path") is not None:
        cfg.video_data.data.path = cfg.dataset_path
    if cfg.get("transform_file") is not None:
        cfg.video_data.data.transformsfile = cfg.transform_file
    env = setup(cfg, device, for_eval=True)
    dataset, gaussians, bindings = env["dataset"], env["gaussians"], env["bindings"]
    E, P = env["elasticity"].eval().requires_grad_(False), env["plasticity"].eval().requires_grad_(False)
    first_step = dataset.steps[0]
    ix, iv = nio.load_init_state(tune_root / "init.pt")
    dataset.set_init_x_and_v(init_x=ix, init_v=iv)
    lora_name = cfg.get("load_lora") or cfg.constitution.get("load_lora")
    if lora_name is not None:
        E.init_lora_layers(r=cfg.constitution.lora.r, lora_alpha=cfg.constitution.lora.alpha)
        P.init_lora_layers(r=cfg.constitution.lora.r, lora_alpha=cfg.constitution.lora.alpha)
        lora = torch.load(tune_root / lora_name, map_location=device)
        E.load_state_dict(lora["elasticity"], strict=False)
        P.load_state_dict(lora["plasticity"], strict=False)
        E.to(device); P.to(device)
        print(f"Loaded lora weights from {tune_root / lora_name}")
    eval_steps = int(cfg.eval_steps)
    if cfg.get("sim_dt") is not None:
        cfg.sim.dt = cfg.sim_dt
    model = MPMModelBuilder().parse_cfg(cfg.sim).finalize(device, False)
    draw_styles, mesh_styles = None, None
    draw_mesh = collider_draw.mesh_wanted(cfg, cfg.sim)                      # implies draw_colliders
    if collider_draw.wanted(cfg, cfg.sim) or draw_mesh:
        nodes = list(cfg.sim.get("colliders") or [])
        if draw_mesh and model.field_colliders:
            mesh_styles = collider_draw.parse_mesh_styles(nodes[len(model.colliders):], len(model.colliders))
        if model.colliders or mesh_styles:
            draw_styles = collider_draw.parse_styles(nodes[:len(model.colliders)])      # (mesh entries follow them)
        else:
            print("draw_colliders: sim.colliders is empty, nothing to draw")
    if model.colliders:
        print(describe_colliders(model.colliders, drawn=draw_styles is not None))
    if model.field_colliders:
        print(describe_field_colliders(model.field_colliders, draw_wanted=collider_draw.wanted(cfg, cfg.sim), drawn=mesh_styles is not None))
    meter = None
    if contact.wanted(cfg, cfg.sim):
        meter = contact.ContactMeter(model)
        if not (model.colliders or model.field_colliders):
            print("report_contacts: sim.colliders is empty, reporting the box walls alone")
    sim = MPMForwardSim(model)
    state_initializer, statics_initializer = MPMStateInitializer(model), MPMStaticsInitializer(model)
    init_data = particle_init_data(cfg, eval_steps)
    state_initializer.add_group(init_data); statics_initializer.add_group(init_data)
    state, _ = state_initializer.finalize()
    statics = statics_initializer.finalize()
    assert init_data.pos.shape[0] == dataset.get_init_x.shape[0], \
        f"Shape mismatch: init_data {init_data.pos.shape[0]} dataset {dataset.get_init_x.shape[0]}"
    x, v, C, F, _ = dataset.get_init_material_data()
    state.from_torch(x=x, v=v, C=C, F=F)
    views = [vw for vw in dataset.views if vw in cfg.get("debug_views", [])]
    scal = cfg.gaussian.get("scaling_modifier", 1.0)
    rotate_sh = bool(cfg.get("rotate_sh", False) or cfg.gaussian.get("rotate_sh", False)) and gaussians.active_sh_degree > 0
    to_render = collider_draw.map_from_alignment(init_data.size, init_data.center)      # renders are de-normalised (below)

    def drawn(img, cam, means3D, deform_grad, shs, sh_degree=None):
        """the view with the colliders drawn in, at the centres the model holds now (collider_draw.draw)"""
        if draw_styles is None:
            return img
        cov, opa = gaussians.get_covariance(scaling_modifier=scal), gaussians.get_opacity
        front = collider_draw.front_renderer(means3D, deform_grad, cam, gaussians.active_sh_degree if sh_degree is None else sh_degree, cov,
                                             gaussians.get_features if shs is None else shs)
        fields = model.field_colliders if mesh_styles is not None else ()
        return collider_draw.draw(img, cam, model.colliders, draw_styles, to_render, front, means3D, opa, fields, mesh_styles or ())

    def meshed(step, exported, means3D, deform_grad=None, shs=None):
        """the frame's surface mesh, from the model save_frame wrote or its like"""
        from .surface_mesh import save_surface
        model_ = exported if exported is not None else deformed_gaussians(gaussians, means3D, deform_grad, shs, scal)
        save_surface(mesh_root / f"{step:03d}.ply", model_, int(cfg.get("mesh_resolution") or 128), float(cfg.get("mesh_density_thres") or 0.5))

    def painted(step, shs, means3D, deform_grad, exported):
        """the frame once more with the painted coefficients `shs` (painter.frame): the images and the painted Gaussian file"""
        cov, opa = gaussians.get_covariance(scaling_modifier=scal), gaussians.get_opacity
        for vw in views:
            cam = dataset.getCameras(vw, first_step)
            img = diff_rasterization(means3D, deform_grad, None, cam, background, 0, cov, opa, shs)
            save_image(drawn(img, cam, means3D, deform_grad, shs, 0), paint_root / f"{vw}_{step:03d}.png")
        if paint_gauss_root is not None:
            nio.save_gaussians_ply(field_paint.painted_gaussians(exported, shs), paint_gauss_root / f"{step:03d}.ply")

    gsec = cfg.get("gaussian")
    drive_key = lambda key: cfg.get(key) if cfg.get(key) is not None or gsec is None else gsec.get(key)
    driver, driven = None, None
    if drive_key("drive_mesh") is not None:
        from . import mesh_drive
        d_verts, d_tris, d_text = mesh_drive.read_mesh(drive_key("drive_mesh"))
        d_fmt = drive_key("drive_mesh_format") or "ply"
        drive_root = Path(cfg.get("result_root", RESULT)) / cfg.name / f"driven_{drive_key('drive_mesh_name') or Path(drive_key('drive_mesh')).stem}"
        drive_root.mkdir(parents=True, exist_ok=True)

        def driven(step, de_x_now):
            """the user's mesh at this frame; with a painter its vertices carry the frame's colours (range and map of the Gaussians')"""
            if painter is None:
                pos, nrm = driver.frame(de_x_now)
                rgb = None
            else:
                pos, nrm, rgb = driver.frame(de_x_now, painter.last_q, painter.frame_range, painter.colormap)
            mesh_drive.save_frame(drive_root / f"{step:03d}.{d_fmt}", pos, nrm, rgb, driver.triangles_np, d_fmt, d_text)

    for vw in views:                                                       # first frame: un-deformed kernels (render.py:292-297)
        cam = dataset.getCameras(vw, first_step)
        render = diff_rasterization(gaussians.get_xyz, None, gaussians, cam, background, scaling_modifier=scal)
        save_image(drawn(render, cam, gaussians.get_xyz, None, None), image_root / f"{vw}_{first_step:03d}.png")
    exported = None
    if gauss_root is not None:
        exported = save_frame(gauss_root / f"{first_step:03d}.ply", gaussians, gaussians.get_xyz, scaling_modifier=scal)
    if mesh_root is not None:
        meshed(first_step, exported, gaussians.get_xyz)
    if painter is not None:                                                # frame 0: F = I, v = v0, the stress of I
        eye = torch.eye(3, dtype=torch.float32, device=device).expand(x.shape[0], 3, 3).contiguous()
        painted(first_step, painter.frame(x.to(device), v.to(device), eye, E, bindings), gaussians.get_xyz, None, exported)
    de_x = denormalize_points_helper_func(x, init_data.size, init_data.center)
    if driven is not None:                                                 # bound to frame 0's particles, in the frame rendered here
        driver = mesh_drive.MeshDriver(d_verts, d_tris, de_x, int(drive_key("drive_mesh_k") or 16), device=device)
        print(driver.describe())
        driven(first_step, de_x)
    de_x_prev, g_prev = de_x.clone().detach(), gaussians.get_xyz.clone().detach()
    for step in range(1, eval_steps + 1):
        stress = E(F)
        state.from_torch(stress=stress)
        x, v, C, F = sim(statics, state)
        if meter is not None:
            meter.record()
            meter.frame()
        model.step_colliders()                                               # moving colliders: one substep further (sim/colliders.py)
        F = P(F)
        state.from_torch(F=F)
        statics_initializer.update(statics, step)
        de_x = denormalize_points_helper_func(x, init_data.size, init_data.center)
        means3D = compute_bindings_xyz(de_x, de_x_prev, g_prev, bindings)
        deform_grad = compute_bindings_F(F, bindings)
        images = {}
        shs = None
        if rotate_sh and (views or gauss_root is not None or mesh_root is not None):                                                        # once per frame
            shs = rotate_shs_by_deformation(gaussians.get_features, deform_grad)
        for vw in views:
            cam = dataset.getCameras(vw, first_step)
            if shs is None:
                images[vw] = diff_rasterization(means3D, deform_grad, gaussians, cam, background, scaling_modifier=scal)
            else:
                images[vw] = diff_rasterization(means3D, deform_grad, None, cam, background, gaussians.active_sh_degree,
                                                gaussians.get_covariance(scaling_modifier=scal), gaussians.get_opacity, shs)
            images[vw] = drawn(images[vw], cam, means3D, deform_grad, shs)
            save_image(images[vw], image_root / f"{vw}_{first_step + step:03d}.png")
        paint_shs = painter.frame(x, v, F, E, bindings) if painter is not None else None
        if state_root is not None and painter is None:
            nio.save_particles_ply(state_root / f"{first_step + step:03d}.ply", x.detach().cpu().numpy())
        elif state_root is not None:
            field_paint.save_particles_ply(state_root / f"{first_step + step:03d}.ply", x, painter.last_q, painter.quantity)
        exported = None
        if gauss_root is not None:
            exported = save_frame(gauss_root / f"{first_step + step:03d}.ply", gaussians, means3D, deform_grad, shs, scal)
        if mesh_root is not None:
            meshed(first_step + step, exported, means3D, deform_grad, shs)
        if painter is not None:
            painted(first_step + step, paint_shs, means3D, deform_grad, exported)
        if driven is not None:
            driven(first_step + step, de_x)
        if on_frame is not None:
            on_frame(step, dict(x=x, F=F, means3D=means3D, deform_grad=deform_grad, images=images))
        de_x_prev, g_prev = de_x.clone().detach(), means3D.clone().detach()
    said = painter.summary() if painter is not None else None
    if said is not None:
        print(said)
    if meter is not None:
        print(f"contacts: {meter.write_csv(image_root.parent / f'contacts_{cfg.video_name}.csv')}")
        print(meter.summary())
    return image_root


def main(argv=None):
    args = parse_args(argv)
    cfg = load_config(args.config)
    for k, val in vars(args).items():
        if k != "config":
            cfg[k] = val
    evaluate(cfg)
