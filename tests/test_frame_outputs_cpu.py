"""CPU: what `python -m neuma_amd.render` and `python -m neuma_amd.inference` share through neuma_amd/frame_outputs.py - the
parsed command lines (held to the dictionaries the two drivers gave when each carried its own copy of the flags), the output
paths and the numbering of the files."""
import pytest

from neuma_amd import evaluate, inference
from neuma_amd.config import Cfg
from neuma_amd.frame_outputs import FrameWriter, output_paths

MIN = ["-c", "x", "-vn", "y"]
SHARED = ["--debug_views", "r_0", "r_1", "--save_particles", "sp", "--save_gaussians", "sg", "--save_mesh", "sm", "--mesh_resolution", "24",
          "--mesh_density_thres", "0.25", "--result_root", "out", "--rotate_sh", "--draw_colliders", "--draw_mesh_colliders",
          "--report_contacts", "--color_by", "von_mises", "--color_range", "0", "2.5", "--colormap", "heat"]
SHARED_OFF = dict(config="x", video_name="y", debug_views=[], save_particles=None, save_gaussians=None, save_mesh=None, mesh_resolution=128,
                  mesh_density_thres=0.5, rotate_sh=False, draw_colliders=False, draw_mesh_colliders=False, report_contacts=False,
                  color_by=None, color_range=None, colormap=None)
SHARED_ON = dict(config="x", video_name="y", debug_views=["r_0", "r_1"], save_particles="sp", save_gaussians="sg", save_mesh="sm",
                 mesh_resolution=24, mesh_density_thres=0.25, result_root="out", rotate_sh=True, draw_colliders=True, draw_mesh_colliders=True,
                 report_contacts=True, color_by="von_mises", color_range=[0.0, 2.5], colormap="heat")
RENDER_OFF = dict(eval_steps=400, init_frame=None, skip_frames=1, load_lora=None, sim_dt=None, drive_mesh=None, drive_mesh_name=None,
                  drive_mesh_k=None, drive_mesh_format=None, change_base_model=None, dataset_path=None, transform_file=None, alpha=None,
                  result_root="experiments/results")
RENDER_OWN = ["-es", "7", "-if", "2", "-sf", "3", "-l", "0100_lora.pt", "-dt", "0.004", "-cbm", "base.pt", "--drive_mesh", "m.obj",
              "--drive_mesh_name", "dm", "--drive_mesh_k", "4", "--drive_mesh_format", "obj", "--dataset_path", "d", "--transform_file",
              "t.json", "--alpha", "0.5"]
RENDER_ON = dict(eval_steps=7, init_frame=2, skip_frames=3, load_lora="0100_lora.pt", sim_dt=0.004, drive_mesh="m.obj", drive_mesh_name="dm",
                 drive_mesh_k=4, drive_mesh_format="obj", change_base_model="base.pt", dataset_path="d", transform_file="t.json", alpha=0.5,
                 result_root="experiments/results")
INFER_OFF = dict(eval_steps=600, skip_frames=1, remove_images=False, dataset_path=None, result_root="results")
INFER_OWN = ["-s", "7", "-f", "3", "-ri", "--dataset_path", "d"]
INFER_ON = dict(eval_steps=7, skip_frames=3, remove_images=True, dataset_path="d", result_root="results")


@pytest.mark.parametrize("mod,argv,want", [
    (evaluate, MIN, {**SHARED_OFF, **RENDER_OFF}), (evaluate, MIN + SHARED, {**RENDER_OFF, **SHARED_ON}),
    (evaluate, MIN + RENDER_OWN, {**SHARED_OFF, **RENDER_ON}),
    (inference, MIN, {**SHARED_OFF, **INFER_OFF}), (inference, MIN + SHARED, {**INFER_OFF, **SHARED_ON}),
    (inference, MIN + INFER_OWN, {**SHARED_OFF, **INFER_ON})],
    ids=["render-min", "render-shared", "render-own", "inference-min", "inference-shared", "inference-own"])
def test_command_lines_parse_to_what_they_did(mod, argv, want):
    assert vars(mod.parse_args(argv)) == want


def test_output_paths_are_the_two_drivers_layouts():
    as_str = lambda d: {k: None if v is None else str(v) for k, v in d.items()}
    assert as_str(output_paths("render", "root", "exp", "vn", "sp", "n", "m", "speed")) == dict(
        images="root/exp/images_vn", states="root/exp/states_sp", gaussians="root/exp/gaussians_n", meshes="root/exp/meshes_m",
        paint_images="root/exp/images_vn_speed", paint_gaussians="root/exp/gaussians_n_speed", contacts="root/exp/contacts_vn.csv", videos=None)
    assert as_str(output_paths("inference", "root", "exp", "vn", "sp", "n", "m", "speed")) == dict(
        images="root/inference/images_vn", states="root/inference_states/states_sp", gaussians="root/inference/gaussians_n",
        meshes="root/inference/meshes_m", paint_images="root/inference/images_vn_speed", paint_gaussians="root/inference/gaussians_n_speed",
        contacts="root/inference/contacts_vn.csv", videos="root/inference_videos")
    # only what is asked for; painted Gaussians need both --save_gaussians and --color_by
    assert as_str(output_paths("render", "root", "exp", "vn")) == dict(
        images="root/exp/images_vn", states=None, gaussians=None, meshes=None, paint_images=None, paint_gaussians=None,
        contacts="root/exp/contacts_vn.csv", videos=None)
    assert output_paths("inference", "root", None, "vn", quantity="speed")["paint_gaussians"] is None
    assert output_paths("inference", "root", None, "vn", save_gaussians="n")["paint_gaussians"] is None


@pytest.mark.parametrize("driver,offsets,numbers", [("render", (3, 3), [3, 4, 5]), ("inference", (0, 3), [0, 1, 2])])
def test_file_numbering(tmp_path, capsys, driver, offsets, numbers):
    """first_step = 3, steps 0..2: render numbers everything first_step + step, inference numbers images and products step and the
    particle files first_step + step; both write particle files from step 1 only"""
    cfg = Cfg(video_name="vn", save_particles="sp", save_gaussians="n", save_mesh="m", color_by="speed", gaussian={})
    w = FrameWriter(driver, cfg, tmp_path, "exp")
    assert capsys.readouterr().out.startswith("color_by speed")
    base = tmp_path / ("exp" if driver == "render" else "inference")
    assert all(p.is_dir() for k, p in w.paths.items() if p is not None and k != "contacts") and not w.paths["contacts"].exists()
    assert (tmp_path / "inference_videos").is_dir() == (driver == "inference")
    w.image_offset, w.state_offset = offsets
    got = [w.targets(step, ["r_0", "r_1"]) for step in range(3)]
    rel = lambda p, root=base: str(p.relative_to(root))
    for key, folder in (("images", "images_vn"), ("paint_images", "images_vn_speed")):
        assert [[rel(p) for p in t[key]] for t in got] == [[f"{folder}/r_0_{n:03d}.png", f"{folder}/r_1_{n:03d}.png"] for n in numbers]
    for key, folder in (("gaussians", "gaussians_n"), ("meshes", "meshes_m"), ("paint_gaussians", "gaussians_n_speed")):
        assert [rel(t[key]) for t in got] == [f"{folder}/{n:03d}.ply" for n in numbers]
    states = tmp_path / ("exp" if driver == "render" else "inference_states")
    assert got[0]["states"] is None and [rel(t["states"], states) for t in got[1:]] == ["states_sp/004.ply", "states_sp/005.ply"]
    # nothing asked for: the images alone
    plain = FrameWriter(driver, Cfg(video_name="vn"), tmp_path / "plain", "exp")
    assert plain.painter is None and capsys.readouterr().out == ""
    t = plain.targets(1, ["r_0"])
    assert [p.name for p in t.pop("images")] == ["r_0_001.png"] and t == dict(states=None, gaussians=None, meshes=None, paint_images=[],
                                                                                 paint_gaussians=None)
