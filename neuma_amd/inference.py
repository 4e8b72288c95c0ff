"""`python -m neuma_amd.inference -c <config.yaml> -vn <name> [-s N] [-dv view ...] [-sp folder]` - the config-driven multi-object
forward roll-out + renderer, counterpart of /root/reference/experiments/inference.py (args 48-84, `eval` 87-377, main 380-386)
for the `experiments/configs/demo/*.yaml` schema (multiobj-bb-cc.yaml, generalize-*.yaml):

    seeds, device, background (white only if video_data.data.white_background)                              :91-113
    <result_root>/inference/images_<video_name>/, <result_root>/inference_states/states_<save_particles>/  :117-125
    one MPMModel for the scene (cfg.sim), CameraDataset (cameras only; --dataset_path / --debug_views)      :129-143
    per entry of cfg.objects                                                                                :159-254
        assets in <assets_root>/<sim_data_name>/ (prepare_simulation_data when particles_path / mesh_path is given)
        bindings.pt, kernels.ply, scaling_modifier; the constitutive pair from `pretrained_ckpt` (+ `constitution.load_lora`
        with lora.{r, alpha}); MPMInitData with span [0, eval_steps] and `particle_data.vel.{lin_vel, ang_vel}`
    ComposeMaterial over the sections, Gaussians mapped into the simulation box unless `denormalize`        :256-281
    frame 0 from the un-deformed kernels, then per step the loop of infer.simulate_objects                  :283-362
    -> <view>_<step:03d>.png per debug view, <first_step + step:03d>.ply per step when --save_particles
    -> <result_root>/inference/gaussians_<name>/<step:03d>.ply per frame when --save_gaussians <name> (no reference counterpart): all
       objects in one standard 3DGS file, each with its own scaling_modifier baked in (infer.simulate_objects(export=True));
       `python -m neuma_amd.replay` renders the folder from any camera
    -> <result_root>/inference/meshes_<name>/<step:03d>.ply per frame when --save_mesh <name> [--mesh_resolution R]
       [--mesh_density_thres T] (no reference counterpart): all objects as one closed triangle mesh with vertex colours
       (neuma_amd/surface_mesh.py), from the same exported model, with or without --save_gaussians
    -> <result_root>/inference/driven_<object folder>/<step:03d>.ply per frame for every object with a `drive_mesh: PATH` key (no
       reference counterpart): the user's own mesh (.obj / .ply, in that object's asset frame) with its vertices and faces as they
       are, carried by the object's particles (neuma_amd/mesh_drive.py).  The mesh goes through the mapping the object's Gaussian
       centres go through (scaled and translated into the simulation box unless `denormalize`); an object that joins late writes
       its rest mesh until it is enabled

    -> with --draw_colliders (or `sim.draw_colliders: true`; no reference counterpart) the colliders of `sim.colliders` are drawn into
       every frame (neuma_amd/collider_draw.py), and with --draw_mesh_colliders (`sim.draw_mesh_colliders: true`; it implies the
       former) its mesh colliders too, by a sphere trace of their distance fields; with `denormalize` the objects must then share one ori_bounds -> sim_bounds alignment
    -> with --color_by QUANTITY [--color_range LO HI] [--colormap NAME] (or the top-level keys `color_by`, `color_range`, `colormap`; no
       reference counterpart) every frame is rendered a second time per view, each Gaussian coloured by the mean of speed, displacement,
       volume, strain, pressure or von_mises over its bound particles (neuma_amd/field_paint.py; every object through its own bindings,
       one range for the scene) -> images_<video_name>_<quantity>/; with --save_gaussians NAME also gaussians_NAME_<quantity>/ (degree-0
       files for `python -m neuma_amd.replay ... --sh_degree 0`), and with --save_particles the particle files gain a fourth float
       property named after the quantity.  Without --color_range every frame is scaled by its own range and the overall range is
       printed at the end
    -> with --report_contacts (or `sim.report_contacts: true`; no reference counterpart) the force and the torque on the box walls and
       on each collider per frame -> <result_root>/inference/contacts_<video_name>.csv, and a summary at the end (neuma_amd/contact.py;
       simulation units); images and particle files are what they are without it

The numeric work is infer.simulate_objects (the operators of SURVEY 8 f3) on the HIP kernels; the flags shared with
`python -m neuma_amd.render`, the output paths and the writers of every product are neuma_amd/frame_outputs.py.  Not reproduced: packing the
frames into an mp4 (mediapy; --skip_frames / --remove_images are accepted, the latter removes the frames) and the random
initial velocity of an object without `particle_data.vel` - the reference's own fallback `sample_vel(seed=42)` raises (it
needs a cfg with lin_vel_bound / ang_vel_bound, nclaw/utils.py:15-30): here such an object samples when its `particle_data`
carries those bounds and raises otherwise."""
import argparse
import random
import shutil
import sys
from pathlib import Path

import numpy as np
import torch

from . import io as nio
from .config import Cfg, load_config
from .dataset import CameraDataset
from .frame_outputs import DrivenMesh, FrameWriter, add_flags
from .infer import SceneObject, simulate_objects
from .material import InvariantFullMetaElasticity, InvariantFullMetaPlasticity, build as build_material
from .prepare import prepare_simulation_data
from .sim import MPMInitData, MPMModelBuilder

RESULT = "results"


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--config", "-c", type=str, required=True, help="Path to the config file.")
    p.add_argument("--eval_steps", "-s", type=int, default=600, help="Number of simulation steps.")
    p.add_argument("--skip_frames", "-f", type=int, default=1, help="Number of skip frames when packing the video.")
    p.add_argument("--remove_images", "-ri", action="store_true", help="Whether to remove images after packing video.")
    p.add_argument("--dataset_path", type=str, default=None, help="Rewrite video dataset path.")
    add_flags(p, RESULT)
    return p.parse_args(argv)


def sample_vel(cfg, seed=None):
    """nclaw/utils.py:15-30: a random downward linear velocity of magnitude in cfg.lin_vel_bound and an angular velocity with
    components in cfg.ang_vel_bound, from numpy's PCG64 stream of `seed`."""
    if seed is None:
        seed = cfg.seed
    rng = np.random.Generator(np.random.PCG64(seed))
    lin_dir = rng.uniform(-1, 1, size=3)
    if lin_dir[1] > 0:
        lin_dir[1] = -lin_dir[1]
    lin_dir /= np.linalg.norm(lin_dir)
    lin_vel = lin_dir * rng.uniform(*cfg.lin_vel_bound)
    ang_vel = rng.uniform(*cfg.ang_vel_bound, size=3)
    return lin_vel, ang_vel


def _prepare(obj_cfg: Cfg, data_root: Path, device) -> None:
    """The object's assets from what its particle_data names (particles_path, then mesh_path, then fill: the keywords of
    gaussian_fill.fill_from_gaussians); with none of them the assets already in data_root are used."""
    pd, gc = obj_cfg.particle_data, obj_cfg.gaussian
    if pd.get("particles_path") is None and pd.get("mesh_path") is None and pd.get("fill") is None:
        return
    data_root.mkdir(parents=True, exist_ok=True)
    common = dict(save_dir=data_root, kernels_path=Path(gc.kernels_path), sh_degree=gc.sh_degree, opacity_thres=gc.opacity_thres,
                  confidence=gc.confidence, max_particles=gc.max_particles, device=device)
    if pd.get("particles_path") is not None:
        prepare_simulation_data(particles_path=Path(pd.particles_path), particles_downsample_factor=pd.downsample_factor, **common)
    elif pd.get("mesh_path") is not None:
        prepare_simulation_data(mesh_path=Path(pd.mesh_path), mesh_sample_mode=pd.mesh_sample_mode,
                                mesh_sample_resolution=pd.mesh_sample_resolution, particles_downsample_factor=1, **common)
    else:
        prepare_simulation_data(fill=dict(pd.fill), particles_downsample_factor=1, **common)


def load_object(obj_cfg: Cfg, assets: Path, eval_steps: int, device, rotate_sh: bool = False) -> SceneObject:
    """One entry of cfg.objects -> SceneObject (inference.py:159-254).  `gaussian.rotate_sh: true` in the entry (or `rotate_sh`,
    the command line's --rotate_sh, for every entry) turns the object's SH colours with its deformation; the reference has no
    such key."""
    data_root = assets / obj_cfg.sim_data_name
    print(f"\nLoad data for {obj_cfg.sim_data_name} ...")
    pd, gc = obj_cfg.particle_data, obj_cfg.gaussian
    _prepare(obj_cfg, data_root, device)
    bindings, n_particles = nio.load_bindings(data_root / "bindings.pt", device=device)
    print(f"#Gaussians with particle bindings: {int((n_particles > 0).sum())}")
    print(f"#Avg particles: {float(n_particles.mean())}")
    print(f"#Max particles: {float(n_particles.max())}, index: {int(torch.argmax(n_particles))}")
    gaussians = nio.load_gaussians_ply(data_root / "kernels.ply", gc.sh_degree, device=device)
    cc = obj_cfg.constitution
    # an optional `name` in a constitution block picks a classical law (material/classical.py), which takes its constants from
    # the block itself; without it the block is the neural net of the checkpoint, as in the reference
    elasticity = build_material(cc.elasticity, InvariantFullMetaElasticity).to(device)
    plasticity = build_material(cc.plasticity, InvariantFullMetaPlasticity).to(device)
    nets = [(k, m) for k, m in (("elasticity", elasticity), ("plasticity", plasticity))
            if isinstance(m, (InvariantFullMetaElasticity, InvariantFullMetaPlasticity))]
    if nets:
        pretrained = torch.load(obj_cfg.pretrained_ckpt, map_location=device)
        for k, m in nets:
            m.load_state_dict(pretrained[k])
        print(f"Loaded pretrained weights from {obj_cfg.pretrained_ckpt}")
    if nets and cc.get("load_lora") is not None:
        for k, m in nets:
            m.init_lora_layers(r=cc.lora.r, lora_alpha=cc.lora.alpha)
        lora = torch.load(cc.load_lora, map_location=device)
        for k, m in nets:
            m.load_state_dict(lora[k], strict=False)
            m.to(device)
        print(f"Loaded lora weights from {cc.load_lora}")
    pd.span = [0, eval_steps]                                   # NOTE: manually setting (inference.py:234)
    pd.shape.name = obj_cfg.sim_data_name + "/particles"        # NOTE: manually setting (inference.py:235)
    if pd.shape.get("asset_root") is None:
        pd.shape.asset_root = str(assets)
    init_data = MPMInitData.get(pd)
    if pd.get("vel") is not None:
        print(f"Use initial velocity: {dict(pd.vel)} ...")
        lin_vel, ang_vel = np.array(pd.vel.lin_vel, dtype=np.float64), np.array(pd.vel.ang_vel, dtype=np.float64)
    elif pd.get("lin_vel_bound") is not None and pd.get("ang_vel_bound") is not None:
        print("Randomly sample initial velocity ...")
        lin_vel, ang_vel = sample_vel(pd, seed=42)
    else:
        raise ValueError(f"object {obj_cfg.sim_data_name!r}: particle_data.vel (lin_vel, ang_vel) is required - the reference's fallback "
                         "sample_vel(seed=42) needs lin_vel_bound / ang_vel_bound (nclaw/utils.py:15-30), which this entry does not carry")
    init_data.set_lin_vel(lin_vel)
    init_data.set_ang_vel(ang_vel)
    return SceneObject(init_data=init_data, elasticity=elasticity, plasticity=plasticity, gaussians=gaussians, bindings=bindings,
                       scaling=float(gc.get("scaling_modifier", 1.0)), rotate_sh=bool(rotate_sh or gc.get("rotate_sh", False)),
                       name=str(obj_cfg.sim_data_name), drive_mesh=obj_cfg.get("drive_mesh"))


@torch.no_grad()
def inference(cfg: Cfg, on_frame=None):
    """inference.py:87-377 (`eval`).  Returns the image folder."""
    seed = cfg.seed
    random.seed(seed); np.random.seed(seed); torch.manual_seed(seed)
    device = torch.device(f"cuda:{cfg.gpu}")
    torch.cuda.set_device(device)
    background = torch.tensor([1.0, 1.0, 1.0] if cfg.video_data.data.get("white_background", False) else [0.0, 0.0, 0.0], device=device)
    writer = FrameWriter("inference", cfg, cfg.get("result_root", RESULT))
    eval_steps = int(cfg.eval_steps)
    model = MPMModelBuilder().parse_cfg(cfg.sim).finalize(device, False)          # the YAML's own sim.eps (no override here)
    options = writer.loop_options(model)
    if cfg.get("dataset_path") is not None:
        cfg.video_data.data.path = cfg.dataset_path
        print(f"Rewrite video dataset path to\n\t{cfg.dataset_path}")
    debug_views = list(cfg.get("debug_views") or [])
    if len(debug_views) > 0:
        cfg.video_data.data.used_views = debug_views
    cfg.video_data.device = str(device)
    dataset = CameraDataset(cfg.video_data)
    first_step = writer.state_offset = dataset.steps[0]
    assets = Path(cfg.get("assets_root", "experiments/assets"))
    objects = [load_object(o, assets, eval_steps, device, rotate_sh=bool(cfg.get("rotate_sh", False))) for o in cfg.objects]
    denormalize, offset = bool(cfg.get("denormalize", False)), 0
    for o in objects:              # a drive_mesh goes through the mapping the object's Gaussian centres go through
        n, align = int(o.init_data.num_particles), (o.init_data.size, o.init_data.center)
        if o.drive_mesh is not None:
            writer.driven.append(DrivenMesh(o.drive_mesh, writer.paths["images"].parent / f"driven_{o.name}", offset, offset + n, device,
                                            align if denormalize else None, None if denormalize else align,
                                            first_live=int(o.init_data.span[0]), label=f"{o.name}: "))
        offset += n
    views = [vw for vw in dataset.views if vw in debug_views]
    cameras = [dataset.getCameras(vw, first_step) for vw in views]               # the camera of the FIRST step throughout
    for frame in simulate_objects(model, objects, eval_steps, cameras, background, denormalize=denormalize, **options):
        writer.write(frame, views)
        if on_frame is not None:
            on_frame(frame["step"], frame)
    writer.finish()
    if cfg.get("remove_images"):
        shutil.rmtree(writer.paths["images"], ignore_errors=True)
    return writer.paths["images"]


def main(argv=None):
    args = parse_args(argv)
    cfg = load_config(args.config)
    for k, val in vars(args).items():               # cfg.update(vars(args)), inference.py:383: the command line wins, also an empty -dv
        if k != "config":
            cfg[k] = val
    inference(cfg)


if __name__ == "__main__":
    sys.exit(main())
