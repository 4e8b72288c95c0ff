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
carry the frame's colours.

The frames come from infer.simulate_objects, the one frame loop, run on a single object; the flags shared with
`python -m neuma_amd.inference`, the output paths and the writers of every product are neuma_amd/frame_outputs.py."""
import argparse
import random
from pathlib import Path

import numpy as np
import torch

from . import io as nio
from .config import Cfg, load_config
from .finetune import particle_init_data, setup
from .frame_outputs import DrivenMesh, FrameWriter, add_flags, save_image  # noqa: F401  (evaluate.save_image is public: regist, replay)
from .infer import SceneObject, simulate_objects
from .sim import MPMModelBuilder
from .tune import diff_rasterization  # noqa: F401  (evaluate.diff_rasterization: the operator a frame can be re-rendered with by hand)

RESULT = "experiments/results"


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--config", "-c", type=str, required=True)
    p.add_argument("--eval_steps", "-es", type=int, default=400)
    p.add_argument("--init_frame", "-if", type=int, default=None)
    p.add_argument("--skip_frames", "-sf", type=int, default=1)
    p.add_argument("--load_lora", "-l", type=str, default=None)
    p.add_argument("--sim_dt", "-dt", type=float, default=None)
    p.add_argument("--drive_mesh", type=str, default=None,
                   help="Drive this triangle mesh (.obj / .ply, in the frame of kernels.ply) with the roll-out into driven_<name>/ (neuma_amd/mesh_drive.py).")
    p.add_argument("--drive_mesh_name", type=str, default=None, help="Folder suffix of the driven frames (default: the file stem).")
    p.add_argument("--drive_mesh_k", type=int, default=None, help="Rest particles a vertex follows, 1..16 (default 16).")
    p.add_argument("--drive_mesh_format", type=str, default=None, choices=("ply", "obj"), help="Default ply.")
    p.add_argument("--change_base_model", "-cbm", type=str, default=None)
    p.add_argument("--dataset_path", type=str, default=None)
    p.add_argument("--transform_file", type=str, default=None)
    p.add_argument("--alpha", type=float, default=None)
    add_flags(p, RESULT)
    return p.parse_args(argv)


@torch.no_grad()
def evaluate(cfg: Cfg, on_frame=None):
    """render.py:109-347 (`eval`): one SceneObject through infer.simulate_objects, de-normalised, from the fitted initial state;
    the products are frame_outputs.FrameWriter's.  `on_frame(step, dict(x, F, means3D, deform_grad, images: {view: image}))` is
    called for the steps from 1 on.  Returns the image folder."""
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
    writer = FrameWriter("render", cfg, cfg.get("result_root", RESULT), cfg.name)
    cfg.video_data.data.init_frame = cfg.get("init_frame")               # NOTE: manually setting (render.py:186-188)
    if cfg.get("debug_views"):
        cfg.video_data.data.used_views = list(cfg.debug_views)
    if cfg.get("dataset_path") is not None:
        cfg.video_data.data.path = cfg.dataset_path
    if cfg.get("transform_file") is not None:
        cfg.video_data.data.transformsfile = cfg.transform_file
    env = setup(cfg, device, for_eval=True)
    dataset, gaussians = env["dataset"], env["gaussians"]
    E, P = env["elasticity"].eval().requires_grad_(False), env["plasticity"].eval().requires_grad_(False)
    first_step = writer.image_offset = writer.state_offset = dataset.steps[0]
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
    options = writer.loop_options(model)
    init_data = particle_init_data(cfg, eval_steps)
    assert init_data.pos.shape[0] == dataset.get_init_x.shape[0], \
        f"Shape mismatch: init_data {init_data.pos.shape[0]} dataset {dataset.get_init_x.shape[0]}"
    body = SceneObject(init_data=init_data, elasticity=E, plasticity=P, gaussians=gaussians, bindings=env["bindings"],
                       scaling=cfg.gaussian.get("scaling_modifier", 1.0),
                       rotate_sh=bool(cfg.get("rotate_sh", False) or cfg.gaussian.get("rotate_sh", False)) and gaussians.active_sh_degree > 0)
    gsec = cfg.get("gaussian")
    drive_key = lambda key: cfg.get(key) if cfg.get(key) is not None or gsec is None else gsec.get(key)
    if drive_key("drive_mesh") is not None:          # in the frame of kernels.ply: the de-normalised frame rendered here
        root = writer.paths["images"].parent / f"driven_{drive_key('drive_mesh_name') or Path(drive_key('drive_mesh')).stem}"
        writer.driven.append(DrivenMesh(drive_key("drive_mesh"), root, 0, init_data.pos.shape[0], device, (init_data.size, init_data.center),
                                        k=drive_key("drive_mesh_k"), fmt=drive_key("drive_mesh_format") or "ply", painter=writer.painter))
    views = [vw for vw in dataset.views if vw in cfg.get("debug_views", [])]
    cameras = [dataset.getCameras(vw, first_step) for vw in views]           # the camera of the FIRST step throughout
    for frame in simulate_objects(model, [body], eval_steps, cameras, background, denormalize=True, render=bool(views),
                                  init_state=dataset.get_init_material_data()[:4], **options):
        writer.write(frame, views)
        if on_frame is not None and frame["step"] > 0:
            on_frame(frame["step"], dict(x=frame["x"], F=frame["F"], means3D=frame["means3D"], deform_grad=frame["deform_grad"],
                                         images=dict(zip(views, frame["images"]))))
    writer.finish()
    return writer.paths["images"]


def main(argv=None):
    args = parse_args(argv)
    cfg = load_config(args.config)
    for k, val in vars(args).items():
        if k != "config":
            cfg[k] = val
    evaluate(cfg)
