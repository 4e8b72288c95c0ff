"""GPU: `python -m neuma_amd.render` (evaluate.evaluate) is a caller of the one frame loop, infer.simulate_objects: its frames
are those of the loop called by hand on one SceneObject made from the same setup() and the same fitted initial state."""
import numpy as np
import pytest
import torch

from gpu_util import dev, measured

pytestmark = pytest.mark.gpu


def _levels(img):
    return (img.clamp(0, 1) * 255 + 0.5).to(torch.uint8).permute(1, 2, 0).cpu().numpy().astype(np.int32)


def test_render_frames_are_those_of_the_frame_loop_by_hand(tmp_path):
    from PIL import Image
    from test_gpu_entrypoints import _write_experiment
    from test_gpu_sh_deform import _eval_cfg, _write_init
    from neuma_amd import io as nio
    from neuma_amd.evaluate import evaluate
    from neuma_amd.finetune import particle_init_data, setup
    from neuma_amd.infer import SceneObject, simulate_objects
    from neuma_amd.sim import MPMModelBuilder
    path, _ = _write_experiment(tmp_path, frames=1)
    _write_init(tmp_path, path)
    steps = 3
    seen = {}
    image_root = evaluate(_eval_cfg(path, tmp_path, "loop"), on_frame=lambda step, f: seen.__setitem__(
        step, dict(keys=sorted(f), views=sorted(f["images"]), x=f["x"].clone(), image=f["images"]["r_0"].clone())))
    # the payload of on_frame: the steps from 1 on, five keys, the images by view name
    assert sorted(seen) == [1, 2, 3]
    assert all(s["keys"] == ["F", "deform_grad", "images", "means3D", "x"] and s["views"] == ["r_0"] for s in seen.values())
    # ---- the loop by hand
    c = _eval_cfg(path, tmp_path, "hand")
    c.video_data.data.init_frame = c.get("init_frame")
    c.video_data.data.used_views = ["r_0"]
    env = setup(c, dev(), for_eval=True)
    ds = env["dataset"]
    ds.set_init_x_and_v(*nio.load_init_state(tmp_path / "logs" / c.name / "finetune" / "init.pt"))
    model = MPMModelBuilder().parse_cfg(c.sim).finalize(dev(), False)
    body = SceneObject(init_data=particle_init_data(c, steps), elasticity=env["elasticity"].eval(), plasticity=env["plasticity"].eval(),
                       gaussians=env["gaussians"], bindings=env["bindings"])
    cam = ds.getCameras("r_0", ds.steps[0])
    frames = list(simulate_objects(model, [body], steps, [cam], torch.ones(3, device=dev()), denormalize=True,
                                   init_state=ds.get_init_material_data()[:4]))
    assert [f["step"] for f in frames] == [0, 1, 2, 3] and "deform_grad" not in frames[0] and all("deform_grad" in f for f in frames[1:])
    # frame 0 has no simulation behind it: bit for bit
    first = np.array(Image.open(image_root / f"r_0_{ds.steps[0]:03d}.png")).astype(np.int32)
    assert first.shape == _levels(frames[0]["images"][0]).shape and (first == _levels(frames[0]["images"][0])).all()
    assert (first < 250).any(axis=2).sum() > 50, "empty render"
    # two runs of one scene differ by the order of the scatters' float atomics (tests/test_gpu_entrypoints.py): positions to 2e-6,
    # 8-bit frames to one level
    for f in frames[1:]:
        s = seen[f["step"]]
        assert measured(float((s["x"] - f["x"]).abs().max()), f"x after step {f['step']}: evaluate vs the loop by hand (abs)") < 2e-6
        assert measured(np.abs(_levels(s["image"]) - _levels(f["images"][0])).max(), f"frame {f['step']}: 8-bit levels, evaluate vs the loop by hand") <= 1
    assert np.abs(_levels(frames[-1]["images"][0]) - first).max() > 0, "the body must move, or the comparison says nothing"
