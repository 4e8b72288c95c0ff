"""What `python -m neuma_amd.render` (evaluate.py) and `python -m neuma_amd.inference` (inference.py) make of the frames of
infer.simulate_objects, written once for both: the shared flags, the output paths, the collider-style and contact-meter set-up,
and the writers.  The products (only the images and the particle files have a reference counterpart):

    images             <view>_<n:03d>.png per debug view, every frame
    states             --save_particles NAME: the particle positions as <n:03d>.ply from step 1 on; with a painter a fourth float
                       property named after the quantity
    gaussians          --save_gaussians NAME: every frame as a standard 3DGS parameter set, all objects in one file, each object's
                       scaling_modifier baked in and its rotated coefficients when rotate_sh is on (export.py; also with an empty
                       -dv list); `python -m neuma_amd.replay` renders the folder from any camera
    meshes             --save_mesh NAME [--mesh_resolution R] [--mesh_density_thres T]: every frame as one closed triangle mesh with
                       vertex colours (surface_mesh.py), from the same exported model, with or without --save_gaussians
    painted images     --color_by QUANTITY [--color_range LO HI] [--colormap NAME]: every frame once more per view, each Gaussian
                       coloured by the mean of the quantity over its bound particles (field_paint.py), colliders drawn in alike;
                       with --save_gaussians also painted gaussians (degree-0 files).  Without --color_range every frame is scaled
                       by its own range and the overall range is printed at the end
    drawn colliders    --draw_colliders (`sim.draw_colliders`), --draw_mesh_colliders (`sim.draw_mesh_colliders`, implies the
                       former): the colliders of `sim.colliders` in every image (collider_draw.py)
    contacts           --report_contacts (`sim.report_contacts`): force and torque on the box walls and on each collider per frame
                       -> contacts_<video_name>.csv and a summary at the end (contact.py; simulation units)
    rigid bodies       a `sim.colliders` entry with `dynamic: true` / `kinematic: true`: pose and velocities of every body per frame
                       -> rigid_<video_name>.csv, always, and a note per body whose contact mass exceeded its own (rigid.py)
    driven meshes      `drive_mesh`: a user's triangle mesh carried by an object's particles -> driven_<name>/ (mesh_drive.py)

`output_paths` says where each goes.  Render numbers images and products first_step + step, inference numbers them step; the
particle files are numbered first_step + step by both."""
from pathlib import Path
from typing import Dict, Optional, Sequence

import torch

from . import collider_draw, contact, field_paint, io as nio, rigid
from .sim.colliders import describe as describe_colliders, describe_fields as describe_field_colliders
from .tune import denormalize_points_helper_func


def add_flags(p, result_root: str) -> None:
    """The flags both drivers take, on the driver's parser; `result_root` is the driver's own default."""
    p.add_argument("--video_name", "-vn", type=str, required=True, help="Save video name.")
    p.add_argument("--debug_views", "-dv", nargs="+", default=[], help="Views for rendering.")
    p.add_argument("--save_particles", "-sp", type=str, default=None, help="Specify the folder name for saving simulated particles.")
    p.add_argument("--save_gaussians", type=str, default=None,
                   help="Write every frame as one 3DGS .ply into gaussians_<name>/ (replay them with python -m neuma_amd.replay).")
    p.add_argument("--save_mesh", type=str, default=None,
                   help="Write every frame as one closed triangle mesh into meshes_<name>/ (neuma_amd/surface_mesh.py).")
    p.add_argument("--mesh_resolution", type=int, default=128, help="Lattice cells along the longest side of a frame's mesh.")
    p.add_argument("--mesh_density_thres", type=float, default=0.5,
                   help="Density level of the mesh surface (default not tuned on a real capture).")
    p.add_argument("--result_root", type=str, default=result_root)
    p.add_argument("--rotate_sh", action="store_true", help="Rotate the SH colours with the deformation (gaussian.rotate_sh).")
    p.add_argument("--draw_colliders", action="store_true", help="Draw the colliders of sim.colliders into every frame (sim.draw_colliders).")
    p.add_argument("--draw_mesh_colliders", action="store_true",
                   help="Draw the mesh colliders too (sim.draw_mesh_colliders); implies --draw_colliders.")
    p.add_argument("--report_contacts", action="store_true",
                   help="Write the force and torque on the walls and on each collider per frame to contacts_<video_name>.csv (sim.report_contacts).")
    p.add_argument("--color_by", type=str, default=None, choices=field_paint.QUANTITIES,
                   help="Render every frame a second time, coloured by this particle quantity (color_by).")
    p.add_argument("--color_range", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                   help="The value range of the colour map (color_range); default: every frame's own range.")
    p.add_argument("--colormap", type=str, default=None, choices=sorted(field_paint.COLORMAPS), help="colormap")


def output_paths(driver: str, result_root, name: str, video_name: str, save_particles: Optional[str] = None,
                 save_gaussians: Optional[str] = None, save_mesh: Optional[str] = None, quantity: Optional[str] = None) -> Dict:
    """Where `driver` ("render" or "inference") writes each product; None for one that is not asked for.  Render keeps everything
    under <result_root>/<name>/; inference ignores `name` and uses <result_root>/inference/, with the particle files beside it."""
    root = Path(result_root)
    base = root / name if driver == "render" else root / "inference"
    tagged = lambda folder, stem, tag: None if tag is None else folder / f"{stem}_{tag}"
    gauss = tagged(base, "gaussians", save_gaussians)
    return dict(images=base / f"images_{video_name}",
                states=tagged(base if driver == "render" else root / "inference_states", "states", save_particles),
                gaussians=gauss, meshes=tagged(base, "meshes", save_mesh), paint_images=tagged(base, f"images_{video_name}", quantity),
                paint_gaussians=None if gauss is None else tagged(base, gauss.name, quantity),
                contacts=base / f"contacts_{video_name}.csv", videos=None if driver == "render" else root / "inference_videos")


def save_image(img: torch.Tensor, path) -> None:
    """torchvision.utils.save_image for one (3,H,W) image in [0,1].  No image leaves the GPU unchecked: a render whose bin lists
    overflowed (incomplete image) raises here (render.flush_pending)."""
    from .render import flush_pending
    flush_pending()
    from PIL import Image
    a = (img.detach().clamp(0, 1) * 255 + 0.5).to(torch.uint8).permute(1, 2, 0).cpu().numpy()
    Image.fromarray(a, "RGB").save(path)


class DrivenMesh(object):
    """One `drive_mesh` file: bound at its first frame to the particles [lo, hi) of the roll-out, in the frame the Gaussians are
    rendered in - the particles de-normalised by `denormalize` = (size, center) if given, the vertices scaled and translated by
    `into_box` = (size, center) if given, which is what scale_gaussians / translate_gaussians do to the centres (infer.py).  Before
    step `first_live` (an object that joins late) the rest mesh is written; with `painter` the vertices carry the frame's colours
    (range and map of the Gaussians')."""

    def __init__(self, path, root: Path, lo: int, hi: int, device, denormalize=None, into_box=None, k: Optional[int] = None,
                 fmt: str = "ply", painter=None, first_live: int = 0, label: str = ""):
        from . import mesh_drive
        self.md, self.lo, self.hi, self.denormalize, self.k, self.fmt = mesh_drive, lo, hi, denormalize, int(k or 16), fmt
        self.painter, self.first_live, self.label, self.root, self.driver = painter, first_live, label, root, None
        verts, self.tris, self.text = mesh_drive.read_mesh(path)
        self.verts = torch.as_tensor(verts, dtype=torch.float32, device=device)
        if into_box is not None:
            self.verts = self.verts * float(into_box[0][0])
            self.verts = self.verts + torch.as_tensor(into_box[1], dtype=torch.float32, device=device)
        root.mkdir(parents=True, exist_ok=True)

    def write(self, step: int, number: int, x: torch.Tensor) -> None:
        part = x[self.lo:self.hi]
        if self.denormalize is not None:
            part = denormalize_points_helper_func(part, *self.denormalize)
        if self.driver is None:
            self.driver = self.md.MeshDriver(self.verts, self.tris, part, self.k, device=x.device)
            print(f"{self.label}{self.driver.describe()}")
        rgb = None
        if step < self.first_live:
            pos, nrm = self.driver.rest_frame()
        elif self.painter is None:
            pos, nrm = self.driver.frame(part)
        else:
            pos, nrm, rgb = self.driver.frame(part, self.painter.last_q[self.lo:self.hi], self.painter.frame_range, self.painter.colormap)
        self.md.save_frame(self.root / f"{number:03d}.{self.fmt}", pos, nrm, rgb, self.driver.triangles_np, self.fmt, self.text)


class FrameWriter(object):
    """A driver's outputs: makes the folders and the painter the config asks for (and says which), then writes every frame
    dictionary of infer.simulate_objects, and at the end prints the painter's summary and writes the contacts.  A frame's images and
    products are numbered step + image_offset, its particle file step + state_offset: the driver sets the two once it knows its
    dataset's first step, and puts the run's DrivenMesh objects into `driven`."""

    def __init__(self, driver: str, cfg, result_root, name: Optional[str] = None):
        self.cfg, self.image_offset, self.state_offset, self.driven, self.meter, self.rigid_log = cfg, 0, 0, [], None, None
        self.painter = field_paint.painter_from_cfg(cfg, cfg.get("gaussian"))
        self.paths = output_paths(driver, result_root, name, cfg.video_name, cfg.get("save_particles"), cfg.get("save_gaussians"),
                                  cfg.get("save_mesh"), None if self.painter is None else self.painter.quantity)
        for key, path in self.paths.items():
            if path is not None and key != "contacts":
                path.mkdir(parents=True, exist_ok=True)
        if self.painter is not None:
            print(self.painter.describe())

    def loop_options(self, model) -> Dict:
        """The keywords of infer.simulate_objects the config asks for on `model`: export, the styles of the colliders to draw, the
        painter, the contact meter (kept for `finish`) - and the lines the drivers print about them."""
        cfg = self.cfg
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
        if contact.wanted(cfg, cfg.sim):
            self.meter = contact.ContactMeter(model)
            if not (model.colliders or model.field_colliders):
                print("report_contacts: sim.colliders is empty, reporting the box walls alone")
        options = dict(export=self.paths["gaussians"] is not None or self.paths["meshes"] is not None, draw_styles=draw_styles,
                       draw_mesh_styles=mesh_styles, painter=self.painter, meter=self.meter)
        if model.rigid_bodies:
            self.rigid_log = rigid.RigidLog(model)
            options["rigid_log"] = self.rigid_log
        return options

    def targets(self, step: int, views: Sequence[str]) -> Dict:
        """The files of frame `step`, by the keys of output_paths: a list per view for the images, one path or None otherwise."""
        n, p = step + self.image_offset, self.paths
        per_view = lambda root: [] if root is None else [root / f"{vw}_{n:03d}.png" for vw in views]
        one = lambda root, no=n: None if root is None else root / f"{no:03d}.ply"
        return dict(images=per_view(p["images"]), states=one(p["states"], step + self.state_offset) if step > 0 else None,
                    gaussians=one(p["gaussians"]), meshes=one(p["meshes"]), paint_images=per_view(p["paint_images"]),
                    paint_gaussians=one(p["paint_gaussians"]))

    def write(self, frame: Dict, views: Sequence[str]) -> None:
        t, painter = self.targets(frame["step"], views), self.painter
        for path, img in zip(t["images"], frame["images"]):
            save_image(img, path)
        if t["states"] is not None and painter is None:
            nio.save_particles_ply(t["states"], frame["x"].detach().cpu().numpy())
        elif t["states"] is not None:
            field_paint.save_particles_ply(t["states"], frame["x"], frame["values"], painter.quantity)
        if t["gaussians"] is not None:
            nio.save_gaussians_ply(frame["gaussians"], t["gaussians"])
        if t["meshes"] is not None:
            from .surface_mesh import save_surface
            save_surface(t["meshes"], frame["gaussians"], int(self.cfg.get("mesh_resolution") or 128),
                         float(self.cfg.get("mesh_density_thres") or 0.5))
        for path, img in zip(t["paint_images"], frame.get("paint_images", ())):
            save_image(img, path)
        if t["paint_gaussians"] is not None:
            nio.save_gaussians_ply(frame["paint_gaussians"], t["paint_gaussians"])
        for d in self.driven:
            d.write(frame["step"], frame["step"] + self.image_offset, frame["x"])

    def finish(self) -> None:
        said = self.painter.summary() if self.painter is not None else None
        if said is not None:
            print(said)
        if self.meter is not None:
            print(f"contacts: {self.meter.write_csv(self.paths['contacts'])}")
            print(self.meter.summary())
        if self.rigid_log is not None:
            path = self.paths["contacts"].with_name(f"rigid_{self.cfg.video_name}.csv")      # beside the contacts file
            print(f"rigid bodies: {self.rigid_log.write_csv(path)}")
            for line in self.rigid_log.mass_ratio_notes():
                print(line)
