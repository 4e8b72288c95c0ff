"""GPU: the contact report of the per-operator MPM path (csrc/nm_contact.h, k_contact_rows / k_contact_sum, MPMModel.contact())
against the fp64 definition neuma_amd/extras/contact.py FED THE GPU'S OWN grid_export() {mv, m} - which isolates the new reduction
from the scatter in front of it -, the momentum identity that ties the rows to the particle states, read-only / bitwise
repeatability, the refusals and both entry points with --report_contacts.  Cases and their fp64 geometry margins:
tests/contact_cases.py.

Bound of every row: 7e-7, the project's bound for the mass-weighted node velocities of these very cases (tests/test_gpu_colliders.py,
field_collider_cases.BOUNDS): the same fp32 arithmetic per node, summed in fp64, over the scale S_r = sum_inside m (|u^(r)| + |u^(r+1)|)."""
import csv
import math
import shutil

import pytest
import torch
import yaml

import contact_cases as cc
from contact_cases import BCS, BOUND, SHAPES, SIZES, SURFACES
from gpu_util import dev, build_model, build_statics, parity
from neuma_amd.extras import contact as xk
from test_gpu_colliders import _case

pytestmark = pytest.mark.gpu


def _model(const, colliders):
    model = build_model(const, dev())
    model.set_colliders(colliders)
    return model


def _gpu_step(model, st, ins):
    from neuma_amd.sim import MPMDiffSim
    return MPMDiffSim(model, reorder=False)(st, *[t.float().to(dev()).requires_grad_(True) for t in ins])


def _row_parity(case, model, const, cs):
    """model.contact() after a substep against the twin on the GPU's own grid; returns (rows, twin rows, scale) on the CPU"""
    rep = model.contact()
    mv, m, _ = model.grid_export()
    ref, scale = cc.twin(const, mv, m, cs)
    rows = rep.rows.cpu()
    assert rows.shape == ref.shape == (1 + len(cs), 9) and rows.dtype == torch.float64 and len(rep.names) == 1 + len(cs)
    assert bool(torch.isfinite(rows).all())
    for r, name in enumerate(rep.names):
        S = float(scale[r])
        assert S > 0, f"row {name} holds no node with mass"
        parity(case, f"{name} J / S", float((rows[r, xk.J] - ref[r, xk.J]).abs().max()) / S, BOUND)
        parity(case, f"{name} N / S", abs(float(rows[r, xk.N] - ref[r, xk.N])) / S, BOUND)
        parity(case, f"{name} L / (sqrt3 S)", float((rows[r, xk.L] - ref[r, xk.L]).abs().max()) / (math.sqrt(3.0) * S), BOUND)
        parity(case, f"{name} mass (rel)", abs(float(rows[r, xk.MASS] - ref[r, xk.MASS])) / float(ref[r, xk.MASS]), 1e-12)
        assert float(rows[r, xk.NODES]) == float(ref[r, xk.NODES]) > 0, name
    assert float(rows[0, xk.J].abs().max()) > 0 and float(rows[0, xk.N]) == 0.0      # near_wall: the walls row is not empty
    return rows, ref, scale


def _one_step(N, G, bc, cs):
    const, (vol, rho, clip, en), ins, _ = _case(N, G, bc)
    model = _model(const, cs)
    st = build_statics(model, vol, rho, clip, en, dev())
    outs = _gpu_step(model, st, ins)
    return const, model, (vol, rho, en), outs


@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("N,G", SIZES)
@pytest.mark.parametrize("surface", SURFACES)
@pytest.mark.parametrize("shape", SHAPES)
def test_rows_of_one_collider(shape, surface, N, G, bc):
    cs = cc.single(shape, surface, G)
    const, model, _, _ = _one_step(N, G, bc, cs)
    rows, _, _ = _row_parity(f"contact {shape}/{surface} N={N} G={G} {bc} vs fp64 definition on the exported grid", model, const, cs)
    assert model.contact().names == ["walls", f"0:{shape}"]
    if surface != "sticky":
        assert float(rows[1, xk.N]) > 0


@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("N,G", SIZES)
def test_rows_of_two_overlapping_colliders(N, G, bc):
    cs = cc.pair(G)
    assert cc.nodes_in_both(cs, _case(N, G, bc)[3][1], G) >= 8
    const, model, _, _ = _one_step(N, G, bc, cs)
    _row_parity(f"contact plane/friction + sphere/slip N={N} G={G} {bc} vs fp64 definition on the exported grid", model, const, cs)


@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("N,G", SIZES)
def test_rows_of_an_analytic_and_a_field_collider(N, G, bc):
    cs = cc.analytic_and_field(N, G, bc)
    const, model, _, _ = _one_step(N, G, bc, cs)
    assert len(model.colliders) == 1 and len(model.field_colliders) == 1
    _row_parity(f"contact sphere/slip + torus field/friction N={N} G={G} {bc} vs fp64 definition on the exported grid", model, const, cs)
    assert model.contact().names == ["walls", "0:sphere", "1:mesh"]


@pytest.mark.parametrize("surface", ["sticky", "friction"])
def test_padding_nodes_are_skipped(surface):
    """G = 10: 3 blocks of 4 nodes per axis, padding lanes in every edge block"""
    const, (vol, rho, clip, en), ins = cc.padding_case()
    cs = cc.padding_sphere(surface)
    model = _model(const, cs)
    st = build_statics(model, vol, rho, clip, en, dev())
    _gpu_step(model, st, ins)
    rows, _, _ = _row_parity(f"contact sphere/{surface} N=1000 G=10 (padding lanes) vs fp64 definition on the exported grid", model, const, cs)
    assert float(rows[1, xk.NODES]) == 19.0


@pytest.mark.parametrize("tape", [False, True])
@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("N,G", SIZES)
def test_momentum_identity_on_the_device(N, G, bc, tape):
    """sum_enabled m_p v_p' = sum_i m_i u_free,i - sum_r J_r with the GPU's v', the GPU's rows and u_free of the exported grid in
    fp64.  Bound: 7e-7 max|v'| sum m_p (the v parity bound of these cases as a momentum) + 7e-7 sum_r S_r (the rows' own bound)."""
    from neuma_amd.sim.mpm import GridTape
    const, (vol, rho, clip, en), ins, _ = _case(N, G, bc)
    cs = cc.pair(G)
    model = _model(const, cs)
    st = build_statics(model, vol, rho, clip, en, dev())
    cur, nxt = model.state(N), model.state(N)
    cur.from_torch(**{k: t.float().to(dev()) for k, t in zip(("x", "v", "C", "F", "stress"), ins)})
    nb = (G + 2 + 3) // 4
    model.forward(st, cur, nxt, GridTape(nb ** 3, dev()) if tape else None)      # tape: nm_mpm_forward_ex
    v_next = nxt.to_torch()[1]
    rows = model.contact().rows.cpu()
    mv, m, _ = model.grid_export()
    _, scale = cc.twin(const, mv, m, cs)
    m64 = m.cpu().double().reshape(-1)
    free = (m64[:, None] * xk.free_velocity(mv.cpu().double().reshape(-1, 3), m64, const.dt, const.gravity, const.eps)).sum(0)
    mp = (vol.float() * rho.float()).double()             # the particle masses as the scatter forms them
    got = (mp[:, None] * v_next.cpu().double())[en != 0].sum(0)
    residual = float((got - (free - rows[:, xk.J].sum(0))).abs().max())
    bound = BOUND * float(v_next.abs().max()) * float(mp[en != 0].sum()) + BOUND * float(scale.sum())
    parity(f"contact momentum identity N={N} G={G} {bc}{' (GridTape)' if tape else ''}", "momentum residual (abs)", residual, bound)


def test_contact_is_read_only_and_repeatable():
    N, G, bc = 4096, 32, "noslip"
    cs = cc.pair(G)
    const, model, _, _ = _one_step(N, G, bc, cs)
    before = model.grid_export()
    a = model.contact().rows.clone()
    b = model.contact().rows.clone()
    after = model.grid_export()
    assert torch.equal(a, b)
    assert all(torch.equal(x, y) for x, y in zip(before, after))
    blocks = model.grid_stats()
    model.contact()
    assert model.grid_stats() == blocks


def test_steps_are_bitwise_the_same_with_contact_calls_in_between():
    """3 in-place substeps against a moving sphere, with and without contact() / a ContactMeter between them.  100 particles: one
    scatter workgroup, whose fp64 LDS sums are exact in any order, so that two runs of one model agree bitwise at all (with several
    workgroups the order of their float atomics is free: tests/test_gpu_colliders.py, the empty-list test)."""
    from gpu_util import mpm_case
    from neuma_amd.contact import ContactMeter
    from neuma_amd.sim import MPMForwardSim
    const, vol, rho, clip, en, x, v, C_, F, S = mpm_case(N=100, G=16, near_wall=False)
    sphere = dict(type="sphere", center=[0.5, 0.42, 0.5], radius=0.1, surface="friction", friction=0.4, velocity=[0.0, 2.0, 0.5])
    res, per_step, meter = [], [], None
    for with_contact in (False, True):
        model = _model(const, [sphere])
        st = build_statics(model, vol, rho, clip, en, dev())
        state = model.state(100)
        state.from_torch(**{k: t.float().to(dev()) for k, t in zip(("x", "v", "C", "F", "stress"), (x, v, C_, F, S))})
        sim = MPMForwardSim(model)
        if with_contact:
            meter = ContactMeter(model)
        for _ in range(3):
            outs = sim(st, state)
            if with_contact:
                meter.record()
                per_step.append(model.contact().rows.clone())
            model.step_colliders()
        res.append([t.clone() for t in outs] + list(model.grid_export()))
    assert all(torch.equal(p, q) for p, q in zip(*res))
    assert float(torch.stack(per_step)[:, 1, xk.NODES].min()) > 0 and float(torch.stack(per_step)[:, 1, xk.J].abs().max()) > 0
    assert not torch.equal(per_step[0], per_step[2])                       # the sphere moved, the body too
    frame = meter.frame()
    assert torch.equal(frame.rows, torch.stack(per_step).sum(0))
    assert meter.frames[0][2] == 3 and meter.frames[0][1] == 3 * const.dt


def test_refusals_and_the_model_without_colliders():
    from neuma_amd import NeumaHipError
    const, model, _, _ = _one_step(3001, 16, "freeslip", [])
    rep = model.contact()
    assert rep.rows.shape == (1, 9) and rep.names == ["walls"] and rep.rows.is_cuda
    mv, m, _ = model.grid_export()
    ref, scale = cc.twin(const, mv, m, [])
    parity("contact without colliders N=3001 G=16 freeslip: walls row vs fp64 definition", "walls J / S",
           float((rep.rows.cpu()[0, xk.J] - ref[0, xk.J]).abs().max()) / float(scale[0]), BOUND)
    assert float(rep.rows[0, xk.NODES]) == float(ref[0, xk.NODES]) > 0
    assert torch.equal(rep.force(const.dt), rep.impulse / const.dt) and rep.torque(const.dt, (0.1, 0.2, 0.3)).shape == (1, 3)
    model.exchange = object()                    # what shard() leaves behind: this model steps one rank's share
    with pytest.raises(NeumaHipError, match="colliders: per-operator path only"):
        model.contact()
    model.exchange = None


def _read_csv(path):
    lines = list(csv.reader(open(path)))
    from neuma_amd.contact import CSV_COLUMNS
    assert tuple(lines[0]) == CSV_COLUMNS
    return lines[1:]


def _files(root):
    return {str(p.relative_to(root)): p.read_bytes() for p in sorted(root.rglob("*")) if p.is_file()}


def _byte_for_byte(plain, flag, extra, rerun_plain, rerun_flag, steps):
    """The flag run wrote the plain run's files, byte for byte, and `extra` besides.  Two runs of one command WITHOUT the flag do
    not always agree: with several scatter workgroups the order of their float atomics is free (measured on the render scene below,
    2018 particles, five runs: one of three runs without the flag had one particle's x one ulp, 6e-8, off the other two from step 1
    on, while both runs with the flag matched those two byte for byte; tests/test_gpu_field_paint.py and
    tests/test_gpu_collider_draw.py meet the same noise).  No tolerance is given for it: where the first pair differs, up to three
    more pairs of runs are made, and a run with the flag must equal a run without it in every byte of every file.  A flag that moved
    a byte would fail every pair; the bitwise test above (one workgroup: no noise) holds the substeps themselves."""
    plains, flags = [plain], [flag]
    for _ in range(3):
        if any([k for k in a if b.get(k) != a[k]] == [] for a in plains for b in flags):
            break
        plains.append(rerun_plain(len(plains)))
        flags.append(rerun_flag(len(flags)))
    assert all(sorted(b) == sorted(list(a) + [extra]) for a in plains for b in flags) and len(plain) >= 2 * steps + 1
    differing = [[k for k in a if b[k] != a[k]] for a in plains for b in flags]
    assert [] in differing, differing


def _only_contact_lines_are_new(plain_out, flag_out, tmp_path):
    """five new lines - the file, the summary's head and its three rows - and every other line is one the plain run printed too
    (the plain run, first, may print more: it fills the scene's caches)"""
    plain = plain_out.splitlines()
    new = [l for l in flag_out.splitlines() if l.startswith("contacts") or l.startswith(("  walls: ", "  0:", "  1:"))]
    rest = [l for l in flag_out.splitlines() if l not in new]
    assert len(new) == 5 and all(l.replace(str(tmp_path / "flag"), str(tmp_path / "plain")) in plain for l in rest)


def test_inference_entry_point_reports_contacts(tmp_path, capsys):
    """The two-object collider scene of tests/test_gpu_colliders.py::test_inference_entry_point_with_a_plane_collider (one body
    wholly inside a sticky half-space, the other falling above it, a moving sphere away from both): with --report_contacts the run
    writes contacts_<video_name>.csv and prints the summary; images and particle files are those of the run without the flag, byte
    for byte (_byte_for_byte)."""
    from test_gpu_entrypoints import _write_experiment
    from neuma_amd import synth
    from neuma_amd.inference import main as inference_main
    path, _ = _write_experiment(tmp_path, frames=1)
    base = yaml.safe_load(path.read_text())
    raw, assets = tmp_path / "raw", tmp_path / "assets"
    w = synth.load_base_weights("plasticine")
    keys = ("layers.0.fc.weight", "layers.1.fc.weight", "final_layer.fc.weight")
    torch.save({t: {k: torch.tensor(a) for k, a in zip(keys, w[s])} for t, s in (("elasticity", "e"), ("plasticity", "p"))},
               raw / "plasticine_0300.pt")
    shutil.copytree(assets / "tinyball", assets / "tinycat")
    for f in (assets / "tinycat").glob("particles.npz"):
        f.unlink()

    def obj(name, ckpt, lo):
        return dict(sim_data_name=name, pretrained_ckpt=str(raw / ckpt), gaussian=dict(sh_degree=3),
                    particle_data=dict(shape=dict(asset_root=None, sort=None, ori_bounds=[[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]],
                                                  sim_bounds=[[0.25, lo, 0.25], [0.75, lo + 0.5, 0.75]]),
                                       vel=dict(lin_vel=[0.0, -0.5, 0.0], ang_vel=[0.0, 0.0, 0.0]), rho=1000.0, clip_bound=0.1),
                    constitution=dict(elasticity=base["constitution"]["elasticity"], plasticity=base["constitution"]["plasticity"],
                                      views=["r_0"]))

    G, steps = 32, 2
    colliders = [dict(type="plane", point=[0.5, 14.6 / G, 0.5], normal=[0, 2, 0], surface="sticky"),
                 dict(type="sphere", center=[0.1, 0.9, 0.1], radius=0.04, surface="slip", velocity=[0.5, 0, 0])]
    cfg = dict(gpu=0, seed=42, debug=True, debug_views=["r_0"], resume=False, overwrite=False, denormalize=False, assets_root=str(assets),
               video_data=dict(base["video_data"], data=dict(base["video_data"]["data"], init_frame=0, used_views=["r_0"])),
               sim=dict(base["sim"], num_grids=G, eps=6e-7, colliders=colliders),
               objects=[obj("tinyball", "jelly_0300.pt", 0.45), obj("tinycat", "plasticine_0300.pt", 0.02)])
    demo = tmp_path / "scene-tiny.yaml"
    demo.write_text(yaml.safe_dump(cfg, sort_keys=False))
    common = ["-c", str(demo), "-s", str(steps), "-vn", "col", "-dv", "r_0", "-sp", "col"]
    capsys.readouterr()
    inference_main(common + ["--result_root", str(tmp_path / "plain")])
    plain_out = capsys.readouterr().out
    inference_main(common + ["--result_root", str(tmp_path / "flag"), "--report_contacts"])
    flag_out = capsys.readouterr().out
    assert not any(l.startswith(("contacts", "report_contacts")) for l in plain_out.splitlines())
    _only_contact_lines_are_new(plain_out, flag_out, tmp_path)

    def again(name, extra):
        inference_main(common + ["--result_root", str(tmp_path / name)] + extra)
        capsys.readouterr()
        return _files(tmp_path / name)

    _byte_for_byte(_files(tmp_path / "plain"), _files(tmp_path / "flag"), "inference/contacts_col.csv", lambda i: again(f"plain{i}", []),
                   lambda i: again(f"flag{i}", ["--report_contacts"]), steps)
    body = _read_csv(tmp_path / "flag" / "inference" / "contacts_col.csv")
    assert len(body) == steps * 3 and [l[3] for l in body[:3]] == ["walls", "0:plane", "1:sphere"]
    assert all(math.isfinite(float(a)) for l in body for a in l[4:])
    plane = [l for l in body if l[3] == "0:plane"]
    assert float(plane[0][10]) > 0 and float(plane[0][5]) < 0 and float(plane[0][12]) > 0       # the lower body is stopped: pushed down on the plane
    assert all(float(l[12]) == 0 and float(l[10]) == 0 for l in body if l[3] == "1:sphere")     # nothing near the sphere
    assert "contacts: 2 frames" in flag_out and "0:plane: peak |F| = " in flag_out and "at frame 1" in flag_out
    # the key in the config does what the flag does; without colliders: one note and the walls row alone
    cfg["sim"]["report_contacts"] = True
    del cfg["sim"]["colliders"]
    none = tmp_path / "none-tiny.yaml"
    none.write_text(yaml.safe_dump(cfg, sort_keys=False))
    inference_main(["-c", str(none), "-s", "1", "-vn", "none", "-dv", "r_0", "--result_root", str(tmp_path / "none")])
    text = capsys.readouterr().out
    assert text.count("report_contacts: sim.colliders is empty, reporting the box walls alone") == 1
    body = _read_csv(tmp_path / "none" / "inference" / "contacts_none.csv")
    assert len(body) == 1 and body[0][3] == "walls"


def test_render_entry_point_reports_contacts(tmp_path, capsys):
    """`python -m neuma_amd.render --report_contacts` on the single-object experiment writer (the scene of
    tests/test_gpu_collider_draw.py's render test with the half-space raised to the middle of the body - the body spans the middle
    quarter of its sim_bounds, y = 0.53 .. 0.67 -, so that its lower half lands on it from the first step; the box stays beside it)."""
    from test_gpu_entrypoints import _write_experiment
    from neuma_amd.config import load_config
    from neuma_amd.evaluate import main as render_main
    from neuma_amd.finetune import particle_init_data
    path, _ = _write_experiment(tmp_path, frames=1)
    cfg = yaml.safe_load(path.read_text())
    cfg["particle_data"]["shape"]["sim_bounds"] = [[0.2, 0.3, 0.25], [0.8, 0.9, 0.75]]
    nodes = [dict(type="plane", point=[0.5, 0.6, 0.5], normal=[0.1, 1, 0], surface="friction", friction=0.3),
             dict(type="box", center=[0.68, 0.62, 0.36], half=[0.04, 0.08, 0.05], euler_xyz_deg=[0, 30, 10], surface="slip")]
    cfg["sim"] = dict(cfg["sim"], eps=6e-7, colliders=nodes)
    path.write_text(yaml.safe_dump(cfg, sort_keys=False))
    init = particle_init_data(load_config(path), 2)
    tune = tmp_path / "logs" / cfg["name"] / "finetune"
    tune.mkdir(parents=True)
    torch.save({"init_x": torch.tensor(init.pos).float(), "init_v": torch.tensor([[0.0, -0.5, 0.0]]).repeat(init.pos.shape[0], 1)}, tune / "init.pt")
    steps = 2
    common = ["-c", str(path), "-es", str(steps), "-dv", "r_0", "-vn", "v", "-sp", "v"]
    capsys.readouterr()
    render_main(common + ["--result_root", str(tmp_path / "plain")])
    plain_out = capsys.readouterr().out
    render_main(common + ["--result_root", str(tmp_path / "flag"), "--report_contacts"])
    flag_out = capsys.readouterr().out
    assert not any(l.startswith(("contacts", "report_contacts")) for l in plain_out.splitlines())
    _only_contact_lines_are_new(plain_out, flag_out, tmp_path)

    def again(name, extra):
        render_main(common + ["--result_root", str(tmp_path / name)] + extra)
        capsys.readouterr()
        return _files(tmp_path / name)

    _byte_for_byte(_files(tmp_path / "plain"), _files(tmp_path / "flag"), f"{cfg['name']}/contacts_v.csv", lambda i: again(f"plain{i}", []),
                   lambda i: again(f"flag{i}", ["--report_contacts"]), steps)
    body = _read_csv(tmp_path / "flag" / cfg["name"] / "contacts_v.csv")
    assert len(body) == steps * 3 and [l[3] for l in body[:3]] == ["walls", "0:plane", "1:box"]
    assert all(math.isfinite(float(a)) for l in body for a in l[4:])
    plane = [l for l in body if l[3] == "0:plane"]
    assert float(plane[0][12]) > 0 and float(plane[0][10]) > 0               # a normal force on the half-space the body lands on
    assert "contacts: 2 frames" in flag_out and "total impulse" in flag_out
