"""GPU parity: SVD operator and the fused constitutive nets against the oracle and the reference-generated
golden vectors.  Tolerances: SURVEY.md §8d (stress rtol 1e-4 of max|stress|, F_p atol 1e-6, grads 2e-3)."""
import numpy as np
import pytest
import torch

from oracle import material as om
from gpu_util import dev, rel_max, abs_max, parity, material_nets as _nets

pytestmark = pytest.mark.gpu
NAMES = ["jelly", "plasticine", "sand"]


def test_svd_forward_convention():
    from neuma_amd.svd import SVD
    torch.manual_seed(0)
    F = torch.eye(3) + 0.3 * torch.randn(5000, 3, 3)
    F[-64:, :, 1] *= -1          # reflections -> negative sigma_2
    F[0] = torch.eye(3)          # degenerate sigma
    F[1] = torch.diag(torch.tensor([2.0, 2.0, 0.5]))
    F[2] = 0.0; F[2, 0, 0] = 1.0  # rank 1
    U, s, Vh = SVD()(F.to(dev()))
    U, s, Vh = U.cpu().double(), s.cpu().double(), Vh.cpu().double()
    Fd = F.double()
    assert (U @ torch.diag_embed(s) @ Vh - Fd).abs().max() < 2e-6
    I = torch.eye(3, dtype=torch.float64)
    assert (U.transpose(1, 2) @ U - I).abs().max() < 2e-6 and (Vh @ Vh.transpose(1, 2) - I).abs().max() < 2e-6
    assert (torch.linalg.det(U) - 1).abs().max() < 1e-5 and (torch.linalg.det(Vh) - 1).abs().max() < 1e-5
    assert (s[:, 0] >= s[:, 1] - 1e-6).all() and (s[:, 1] >= s[:, 2].abs() - 1e-6).all()
    nz = torch.linalg.det(Fd).abs() > 1e-3
    assert (torch.sign(s[nz, 2]) == torch.sign(torch.linalg.det(Fd[nz]))).all()
    _, so, _ = om.svd3(Fd)
    assert (s - so).abs().max() < 2e-6


def test_svd_backward_matches_clamped_adjoint():
    from neuma_amd.svd import SVD
    torch.manual_seed(1)
    F = (torch.eye(3) + 0.3 * torch.randn(2048, 3, 3))
    Fg = F.to(dev()).requires_grad_(True)
    U, s, Vh = SVD()(Fg)
    gU, gs, gVh = torch.randn_like(U), torch.randn_like(s), torch.randn_like(Vh)
    (gF,) = torch.autograd.grad((U * gU).sum() + (s * gs).sum() + (Vh * gVh).sum(), Fg)
    ref = om.svd3_adjoint(U.detach().cpu().double(), s.detach().cpu().double(), Vh.detach().cpu().double(),
                          gU.cpu().double(), gs.cpu().double(), gVh.cpu().double())
    assert rel_max(gF, ref) < 5e-6      # measured 1.4e-06
    # and against fp64 autograd through torch.linalg.svd on well separated spectra
    Fd = F.double().requires_grad_(True)
    Uo, so, Vho = om.svd3(Fd)
    gap = torch.minimum((so[:, 0] - so[:, 1]).abs(), (so[:, 1] - so[:, 2].abs()).abs()) > 0.05
    (gFo,) = torch.autograd.grad((so * gs.cpu().double()).sum(), Fd)
    Fg2 = F.to(dev()).requires_grad_(True)
    _, s2, _ = SVD()(Fg2)
    (gF2,) = torch.autograd.grad((s2 * gs).sum(), Fg2)
    assert abs_max(gF2[gap.to(dev())], gFo[gap]) < 7e-6      # measured 1.8e-06


@pytest.mark.parametrize("name", NAMES)
def test_material_forward_matches_reference_golden(golden_dir, name):
    g, E, P = _nets(name, golden_dir, lora=False)
    F = torch.tensor(g["F"]).float().to(dev())
    with torch.no_grad():
        s, fp = E(F), P(F)
    parity(f"constitutive nets, {name} checkpoint, vs golden made by the reference classes", "stress (rel)", rel_max(s, torch.tensor(g["stress_plain"])), 3e-6)      # measured 1.0e-6
    parity(f"constitutive nets, {name} checkpoint, vs golden made by the reference classes", "F_p (abs)", abs_max(fp, torch.tensor(g["Fp_plain"])), 3.5e-7)      # 1.1e-7


@pytest.mark.parametrize("name", NAMES)
def test_material_lora_forward_backward_matches_reference_golden(golden_dir, name):
    g, E, P = _nets(name, golden_dir, lora=True)
    for net, t, key in ((E, "e", "stress_lora"), (P, "p", "Fp_lora")):
        net.train()
        F = torch.tensor(g["F"]).float().to(dev()).requires_grad_(True)
        out = net(F)
        case = f"constitutive nets + LoRA, {name} checkpoint, {'elasticity' if t == 'e' else 'plasticity'}, vs reference golden"
        if t == "e":
            parity(case, "stress (rel)", rel_max(out, torch.tensor(g[key])), 3e-6)
        else:
            parity(case, "F_p (abs)", abs_max(out, torch.tensor(g[key])), 3.5e-7)
        (out * torch.tensor(g[f"gout_{t}"]).float().to(dev())).sum().backward()
        parity(case, "dL/dF (rel)", rel_max(F.grad, torch.tensor(g[f"gF_{t}"])), 1e-5)      # measured <= 2.8e-6
        ga = max(rel_max(lin.lora_A.grad, torch.tensor(g[f"{t}_gA{i}"])) for i, lin in enumerate((net.layers[0].fc, net.layers[1].fc, net.final_layer.fc)))
        gb = max(rel_max(lin.lora_B.grad, torch.tensor(g[f"{t}_gB{i}"])) for i, lin in enumerate((net.layers[0].fc, net.layers[1].fc, net.final_layer.fc)))
        parity(case, "dL/dA (rel, worst layer)", ga, 1e-5)      # <= 2.5e-6
        parity(case, "dL/dB (rel, worst layer)", gb, 1e-5)      # <= 2.6e-6
        # eval() merges (loralib.py:199-214) and must give the same function
        net.eval()
        with torch.no_grad():
            merged = net(torch.tensor(g["F"]).float().to(dev()))
        mk = "stress_lora_merged" if t == "e" else "Fp_lora_merged"
        assert (rel_max(merged, torch.tensor(g[mk])) < 5e-6) if t == "e" else (abs_max(merged, torch.tensor(g[mk])) < 5e-7)
        net.train()


def test_material_large_batch_and_ragged_tail_vs_oracle(golden_dir):
    """N not a multiple of 64/256, > one workgroup sweep; F = I rows (every roll-out starts there)."""
    g, E, P = _nets("jelly", golden_dir, lora=True)
    b = np.load(golden_dir / "base_models.npz")
    torch.manual_seed(3)
    N = 70_001
    F = torch.eye(3) + 0.05 * torch.randn(N, 3, 3)
    F[:1000] = torch.eye(3)
    Fd = F.double()
    for net, t in ((E, "e"), (P, "p")):
        W = [om.lora_effective_weight(torch.tensor(b[f"jelly_{t}_w{i}"]).double(), torch.tensor(g[f"{t}_A{i}"]),
                                      torch.tensor(g[f"{t}_B{i}"]), float(g[f"{t}_scaling"])) for i in range(3)]
        Fg = F.to(dev()).requires_grad_(True)
        out = net(Fg)
        Fo = Fd.clone().requires_grad_(True)
        Wo = [w.clone().requires_grad_(True) for w in W]
        ref = om.elasticity(Fo, Wo) if t == "e" else om.plasticity(Fo, Wo, 1e-3)
        if t == "e":
            assert rel_max(out, ref) < 3e-6      # measured 8.1e-07
        else:
            assert abs_max(out, ref) < 2e-7      # measured 6.0e-08
        go = torch.randn(N, 3, 3)
        (out * go.to(dev())).sum().backward()
        grads = torch.autograd.grad((ref * go.double()).sum(), [Fo] + Wo)
        nd = slice(1000, None)     # at F = I the reference's own SVD adjoint is clamped noise; compare away from it
        assert rel_max(Fg.grad[nd], grads[0][nd]) < 7e-5      # measured 1.7e-05
        assert torch.isfinite(Fg.grad).all()
        # weight gradients through the LoRA factors: dA = s B^T dW, dB = s dW A^T
        sc = float(g[f"{t}_scaling"])
        for i, lin in enumerate((net.layers[0].fc, net.layers[1].fc, net.final_layer.fc)):
            dW = grads[1 + i]
            A, B = torch.tensor(g[f"{t}_A{i}"]), torch.tensor(g[f"{t}_B{i}"])
            # exclude the F = I rows' (clamped) contribution by construction: they enter dW only through z,
            # which is smooth, so the full sum is comparable
            assert rel_max(lin.lora_A.grad, sc * B.T @ dW) < 2e-5, (t, i)      # measured 5.6e-06
            assert rel_max(lin.lora_B.grad, sc * dW @ A.T) < 2e-5, (t, i)      # measured 6.4e-06
        net.zero_grad()


def test_material_empty_and_compose(golden_dir):
    from neuma_amd.material import ComposeMaterial
    g, E, P = _nets("jelly", golden_dir, lora=False)
    _, E2, _ = _nets("sand", golden_dir, lora=False)
    F = torch.tensor(g["F"]).float().to(dev())
    with torch.no_grad():
        assert E(F[:0]).shape == (0, 3, 3)
        comp = ComposeMaterial([E, E2, E], [20, 0, 48])(F)       # empty section skipped (preset.py:23-25)
        assert torch.equal(comp[:20], E(F[:20])) and torch.equal(comp[20:], E(F[20:]))


def test_lora_merge_kernel_matches_loralib_expression():
    """nm_lora_merge / nm_lora_merge_bwd == W + (B @ A) * scaling and its autograd (loralib.py:209-224), all three layer
    shapes of the constitutive nets."""
    from neuma_amd.material.loralib import LinearLoRA
    torch.manual_seed(0)
    for out_f, in_f in ((64, 13), (64, 64), (9, 64)):
        lin = LinearLoRA(in_f, out_f, r=16, lora_alpha=16, bias=False).to(dev())
        lin.lora_B.data.normal_(0, 0.1)
        w = lin.effective_weight()
        ref_B = lin.lora_B.detach().double().cpu().requires_grad_(True)
        ref_A = lin.lora_A.detach().double().cpu().requires_grad_(True)
        ref = lin.weight.detach().double().cpu() + (ref_B @ ref_A) * lin.scaling
        assert abs_max(w, ref) < 2e-7      # measured 2.3e-08
        g = torch.randn(out_f, in_f, device=dev())
        gB, gA = torch.autograd.grad((w * g).sum(), [lin.lora_B, lin.lora_A])
        rB, rA = torch.autograd.grad((ref * g.double().cpu()).sum(), [ref_B, ref_A])
        assert rel_max(gB, rB) < 7e-7 and rel_max(gA, rA) < 7e-7      # measured <= 1.9e-7
        lin.eval()       # merged path: plain weight, loralib.py:199-214
        assert abs_max(lin.effective_weight(), ref) < 2e-7      # measured 2.3e-08


def test_lora_merge_of_a_whole_net_in_one_launch():
    """nm_lora_merge_layers / nm_lora_merge_layers_bwd (the three layers of a constitutive net per launch) against the
    per-layer expression W + (B @ A) * scaling and its autograd; the merged tuple is reused until a parameter changes."""
    from neuma_amd.material import InvariantFullMetaElasticity
    cfg = dict(layer_widths=[64, 64], norm=None, nonlinearity="gelu", no_bias=True, normalize_input=True, alpha=1e-3)
    torch.manual_seed(1)
    net = InvariantFullMetaElasticity(cfg).to(dev())
    net.init_lora_layers(16, 16)
    net.freeze_all_except_lora()
    fcs = (net.layers[0].fc, net.layers[1].fc, net.final_layer.fc)
    for fc in fcs:
        fc.lora_B.data.normal_(0, 0.1)
    ws = net.effective_weights()
    assert net.effective_weights() is ws                        # cached
    gs = [torch.randn_like(w) for w in ws]
    params = [p for fc in fcs for p in (fc.lora_B, fc.lora_A)]
    grads = torch.autograd.grad(sum((w * g).sum() for w, g in zip(ws, gs)), params)
    k = 0
    for fc, w, g in zip(fcs, ws, gs):
        rB = fc.lora_B.detach().double().cpu().requires_grad_(True)
        rA = fc.lora_A.detach().double().cpu().requires_grad_(True)
        ref = fc.weight.detach().double().cpu() + (rB @ rA) * fc.scaling
        assert abs_max(w, ref) < 2e-7      # measured 4.1e-08
        eB, eA = torch.autograd.grad((ref * g.double().cpu()).sum(), [rB, rA])
        assert rel_max(grads[k], eB) < 1e-6 and rel_max(grads[k + 1], eA) < 1e-6      # measured <= 2.8e-7
        k += 2
    with torch.no_grad():
        fcs[1].lora_A.mul_(2.0)
    ws2 = net.effective_weights()
    assert ws2 is not ws and abs_max(ws2[0], ws[0]) == 0.0 and abs_max(ws2[1], ws[1]) > 0.0


def _operator_chain_grad(F, W, gout, kind, alpha=1e-3):
    """dL/dF of L = <net(F), gout> composed the way the reference composes it (meta.py:196-221 / 468-489): the stand-alone
    `SVD` operator - whose adjoint is the clamped one of warp's adj_svd3, pinned against oracle.material.svd3_adjoint in
    test_svd_* above - followed by plain torch ops (fp64).  At coinciding singular values the factors U, V are only defined
    up to a rotation of the degenerate plane and the gradient depends on that choice (the sigma - 1 features are fed to
    different weights), so the comparison must use the SAME factors: the fused kernel and the operator share nm_svd3."""
    from neuma_amd.svd import SVD
    F = F.float().to(dev()).requires_grad_(True)
    U, s, Vh = SVD()(F)
    Fd, U, s, Vh = F.double(), U.double(), s.double(), Vh.double()
    R = U @ Vh
    I = torch.eye(3, dtype=torch.float64, device=dev())
    z = torch.cat([s - 1.0, (Fd.transpose(1, 2) @ Fd - I).reshape(-1, 9), torch.linalg.det(Fd).unsqueeze(1) - 1.0], 1)
    h = z
    for i, w in enumerate(W):
        h = h @ w.to(dev()).T
        if i < 2:
            h = torch.nn.functional.gelu(h)
    X = h.reshape(-1, 3, 3)
    X = 0.5 * (X + X.transpose(1, 2))
    out = R @ X @ Fd.transpose(1, 2) if kind == "e" else Fd + alpha * (R @ X)
    (out * gout.to(dev())).sum().backward()
    return F.grad.double().cpu()


def test_svd_adjoint_modes_reference_is_the_clamped_adjoint_polar_is_opt_in(golden_dir):
    """The constitutive backward's default is the reference's gradient INCLUDING its behaviour where singular values
    coincide - per operator and inside the fused roll-out; "polar" is the opt-in exact derivative.  The clamp
    (|s_j^2 - s_i^2| < 1e-6) only bites at (fp32-)exact coincidences.  Rows: exactly I; diag(a, a, b) and diag(a, b, b) -
    two equal singular values with a non-zero network output, where the reference's rotation path drops that pair and
    the polar derivative does not; generic."""
    g, E, P = _nets("jelly", golden_dir, lora=False)
    b = np.load(golden_dir / "base_models.npz")
    gen = torch.Generator().manual_seed(11)
    N = 600
    F = torch.eye(3, dtype=torch.float64).repeat(N, 1, 1)
    ab = 0.8 + 0.5 * torch.rand(200, 2, generator=gen, dtype=torch.float64)
    F[200:300] = torch.diag_embed(torch.stack([ab[:100, 0], ab[:100, 0], ab[:100, 1]], 1))
    F[300:400] = torch.diag_embed(torch.stack([ab[100:, 0], ab[100:, 1], ab[100:, 1]], 1))
    F[400:] += 0.08 * torch.randn(200, 3, 3, generator=gen, dtype=torch.float64)
    F = F.float().double()                                     # the values the GPU sees
    gout = torch.randn(N, 3, 3, generator=gen, dtype=torch.float64)
    for net, t in ((E, "e"), (P, "p")):
        W = [torch.tensor(b[f"jelly_{t}_w{i}"]).double() for i in range(3)]
        ref = _operator_chain_grad(F, W, gout, t)
        res = {}
        for mode in ("reference", "polar"):
            net.svd_adjoint = mode
            Fg = F.float().to(dev()).requires_grad_(True)
            (net(Fg) * gout.float().to(dev())).sum().backward()
            res[mode] = Fg.grad.double().cpu()
            assert torch.isfinite(res[mode]).all()
        net.svd_adjoint = "reference"
        scale = float(ref.abs().max())
        # default mode == the reference's operator chain: F = I and generic rows to fp32 accuracy ...
        keep = torch.ones(N, dtype=torch.bool); keep[200:400] = False
        assert float((res["reference"][keep] - ref[keep]).abs().max()) <= 2e-3 * scale
        # ... and on rows with two coinciding singular values up to what the clamp itself amplifies: the operator evaluates
        # E (U^T Ubar - ...) s_j + s_i E (V^T Vbar - ...) with E = -1e6 there, i.e. 1e6 x the fp32 rounding difference of two
        # quantities that are equal in exact arithmetic (the fused kernel factors (s_j - s_i) out and gets an exact zero)
        tied_err = float((res["reference"][200:400] - ref[200:400]).abs().max())
        assert tied_err <= 5e-2 * scale
        print(f"[{t}] tied rows: |fused reference - operator chain| max {tied_err:.3g}, |polar - reference| max "
              f"{float((res['polar'][200:400] - res['reference'][200:400]).abs().max()):.3g}, scale {scale:.3g}")
        # generic rows: the clamp is inactive, the exact polar derivative is the same thing
        assert float((res["polar"][400:] - ref[400:]).abs().max()) <= 2e-3 * scale
        # two coinciding singular values: the reference drops that pair's rotation term, the polar derivative does not
        assert float((res["polar"][200:400] - res["reference"][200:400]).abs().max()) > max(3.0 * tied_err, (1e-2 if t == "e" else 1e-5) * scale)


def test_fused_rollout_svd_adjoint_default_matches_per_operator_reference_mode():
    """The fused roll-out and the per-operator path take the same adjoint mode.  Away from coinciding singular values both
    modes are the same function, so all four results agree; starting at F = I (free fall keeps every F within ~1e-6 of I:
    inside the clamp, where the reference's gradient is 1e6 x rounding noise and differs between any two evaluation
    orders) only the noise-free "polar" mode can be compared between the two paths - "reference" must merely stay finite."""
    from neuma_amd import synth
    from neuma_amd.harness import SceneRuntime
    rt = SceneRuntime(synth.make_scene("tiny", override=dict(S=3)), dev(), fused=True)
    assert rt.sim_fused.svd_adjoint == "reference"
    params = rt.parameters()
    gws = [torch.randn(rt.N, 3, generator=torch.Generator().manual_seed(i)).to(dev()) for i in range(2)]
    gen = torch.Generator().manual_seed(4)
    F_generic = (torch.eye(3) + 0.05 * torch.randn(rt.N, 3, 3, generator=gen)).to(dev())
    for F0, label in ((F_generic, "generic"), (rt.F0, "identity")):
        res = {}
        for mode in ("reference", "polar"):
            rt.sim_fused.svd_adjoint = mode
            rt.elasticity.svd_adjoint = rt.plasticity.svd_adjoint = mode
            for fused in (True, False):
                rt.fused = fused
                for p in params:
                    p.grad = None
                ins = [t.clone().requires_grad_(True) for t in (rt.x0, rt.v0)]
                out = rt.rollout(ins[0], ins[1], rt.C0, F0)
                ((out[0] * gws[0]).sum() + (out[1] * gws[1]).sum()).backward()
                res[(mode, fused)] = [t.grad.clone() for t in ins + params]
                assert all(torch.isfinite(t).all() for t in res[(mode, fused)])
        # From F = I the singular values of the first substeps coincide to rounding, the singular BASIS is then decided by
        # the last bit of F, and the nets are not symmetric in (s0, s1, s2): the sigma channels' gradient is mapped back
        # through that arbitrary basis, so two correct evaluation orders differ at the 1e-2 level there (a 1-ulp change of
        # the GELU moved this figure from 4e-3 to 6e-3).  Away from the degeneracy the two paths agree to 5e-3.
        for a, b_ in zip(res[("polar", True)], res[("polar", False)]):
            assert rel_max(a, b_) < (7e-6 if label == "generic" else 3e-2), label      # measured 4.3e-7 .. 2.3e-6 | 9.6e-3 over four runs
        if label == "generic":
            for a, b_ in zip(res[("reference", True)], res[("reference", False)]):
                assert rel_max(a, b_) < 7e-6      # measured <= 2.3e-06 over four runs
            for a, b_ in zip(res[("reference", True)], res[("polar", True)]):
                assert rel_max(a, b_) < 7e-6      # measured 6.2e-07 .. 2.4e-06 over four runs
    rt.sim_fused.svd_adjoint = "reference"


def test_kernel_timing_hooks_count_and_sample_launches():
    """nm_prof_enable(1, name): HIP events around every launch of that kernel; nm_prof_enable(n, name): around every n-th one
    (what bench.py uses inside its timed region for a kernel launched many times per frame); nm_prof_enable(0): none."""
    import ctypes as C
    from neuma_amd import _lib as L
    lib = L.lib()
    n = 4096
    F = (torch.eye(3, device=dev()).repeat(n, 1, 1) + 0.05 * torch.randn(n, 3, 3, device=dev())).contiguous()
    U, s, Vh = torch.empty_like(F), torch.empty(n, 3, device=dev()), torch.empty_like(F)

    def run(times):
        for _ in range(times):
            L.check(lib.nm_svd3_fwd(n, L.ptr(F), L.ptr(U), L.ptr(s), L.ptr(Vh), L.stream_ptr(dev())), "nm_svd3_fwd")

    def report():
        buf = C.create_string_buffer(1 << 14)
        lib.nm_prof_report(buf, len(buf))
        out = {}
        for line in buf.value.decode().splitlines():
            name, calls, ms = line.rsplit(" ", 2)
            out[name.strip("()")] = (int(calls), float(ms))
        return out

    try:
        for stride, launches, expect in ((1, 6, 6), (3, 7, 3), (8, 8, 1)):
            lib.nm_prof_reset()
            lib.nm_prof_enable(stride, b"k_svd_fwd")
            run(launches)
            lib.nm_prof_enable(0, None)
            run(2)                                  # not timed
            torch.cuda.synchronize()
            rep = report()
            assert list(rep) == ["k_svd_fwd"] and rep["k_svd_fwd"][0] == expect and rep["k_svd_fwd"][1] > 0.0, (stride, rep)
    finally:
        lib.nm_prof_enable(0, None)
        lib.nm_prof_reset()
