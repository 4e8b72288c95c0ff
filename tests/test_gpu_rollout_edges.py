"""GPU parity: the fused roll-out (pair kernels, SVD cache, activation cache, grid prologue) at particle counts where the
constitutive kernels' work split has an edge - a partial tile, an empty wave, a second round, the look-ahead across a round
boundary, the unsplit prologue - against the per-operator path and the fp64 oracle chain, as
test_gpu_rollout.py::test_fused_rollout_equals_per_operator_path_and_oracle does at 2000 particles (125 full tiles, one per
wave, prologue on workgroups of its own).  Same bounds as there, widened for a gradient only where the oracle's own fp32
run says so (`_bounds`); the per-operator path is held to the oracle as well.

The per-operator result and the oracle's are computed once per case and shared by the case's launch / cache modes."""
import pytest
import torch

import material_edge_cases as mc
from gpu_util import dev, rel_max, abs_max
from test_gpu_rollout import _oracle_rollout, _lora_factor_grads

pytestmark = pytest.mark.gpu

# case: (n, substeps, grid cells per axis, geometry) - material_edge_cases.ROLLOUT_EDGES; the geometry is asserted on the CPU.
# Case e (65 553: rounds of 4 + 1 tiles, look-ahead across the round boundary) has the per-operator path as its yardstick, whose
# kernels test_gpu_material_edges.py holds to fp64 at that count; the oracle runs there too (1.9 s, fp64 and fp32 together),
# because among 65 553 rows of I + 0.05 randn some have nearly tied singular values and how far two fp32 paths may be apart
# can only be read off the oracle's own fp32 run (`_bounds`)
EDGE = mc.ROLLOUT_EDGES
CACHES = {"recompute": (False, "0"), "cached": (True, "1")}
MODES = [(c, k, 1) for c in EDGE for k in CACHES] + [(c, k, 0) for c in "bc" for k in CACHES]
_shared = {}


def _oracle(rt, S, ins, gws, dtype):
    """test_gpu_rollout._oracle_rollout and its gradients, run in `dtype`: (states, the sixteen gradients in the order of
    `ins + rt.parameters()`), as fp64"""
    oins = [t.detach().cpu().to(dtype).requires_grad_(True) for t in ins]
    oouts, We, Wp = _oracle_rollout(rt, S, *oins, dtype=dtype)
    og = torch.autograd.grad(sum((o * w.to(dtype)).sum() for o, w in zip(oouts, gws)), oins + We + Wp)
    return [o.detach().double() for o in oouts], [g.double() for g in og[:4]] + _lora_factor_grads(rt, og[4:7], og[7:10])


ISSUE_VS_ORACLE = [7e-5] * 4 + [1.5e-5, 1e-5] * 6          # input gradients, LoRA A / B: test_gpu_rollout.py


def _bounds(oracle64, oracle32):
    """Per gradient tensor: (bound between the fused and the per-operator path, bound of either against the fp64 oracle), both
    from the oracle alone: nu = the distance of the oracle's own fp32 run from its fp64 run on this very roll-out.

    Against the oracle: the suite's bound (7e-5 inputs, 1.5e-5 / 1e-5 LoRA A / B), or 2 nu where that is larger
    (material_edge_cases.bound, capped there): at 33 particles a LoRA gradient is a sum of few terms and the oracle's fp32 run
    itself comes within a factor of two of 1e-5.  BOTH paths are held to it, the per-operator path too.

    Between the paths: the suite's 1e-5, or 2 nu where that is larger.  The two paths are two fp32 evaluations - the pair
    launch takes the trial F from registers, the per-operator path rebuilds it from memory: other roundings from the first
    substep on - of a gradient that an fp32 evaluation gets right to nu; if each were a mere nu from the truth they would be
    up to 2 nu apart.  For dL/dF0 nu is 1e-5 .. 5e-5 (I + 0.05 randn: some of n rows have nearly tied singular values, more
    of them the larger n), so 1e-5 would ask each path to be closer to the other than fp32 is to the truth."""
    out = []
    for o64, o32, issue in zip(oracle64, oracle32, ISSUE_VS_ORACLE):
        nu = mc.rel(o32, o64)
        out.append((mc.bound(1e-5, nu), mc.bound(issue, nu)))
    return out


def _case(case, fresh=False):
    """runtime, start state, cotangents, the per-operator path's result, the oracle's and the gradient bounds: once per case"""
    if case in _shared and not fresh:
        return _shared[case]
    from neuma_amd import synth
    from neuma_amd.harness import SceneRuntime
    n, S, G, _ = EDGE[case]
    rt = SceneRuntime(synth.make_scene("tiny", override=dict(N=n, S=S, K=500, G=G)), dev(), fused=True)
    assert rt.N == n
    g = torch.Generator().manual_seed(40 + n)
    F0 = (torch.eye(3) + 0.05 * torch.randn(n, 3, 3, generator=g)).to(dev())       # away from F = I (clamped adjoint)
    gws = [torch.randn(n, 3, generator=g), torch.randn(n, 3, generator=g), torch.randn(n, 3, 3, generator=g),
           torch.randn(n, 3, 3, generator=g)]
    if fresh:
        return rt, F0, gws
    ref = _run(rt, F0, gws, fused=False)
    oracle = _oracle(rt, S, (rt.x0, rt.v0, rt.C0, F0), gws, torch.float64)
    o32 = _oracle(rt, S, (rt.x0, rt.v0, rt.C0, F0), gws, torch.float32)
    bounds = _bounds(oracle[1], o32[1])
    _shared[case] = (rt, F0, gws, ref, oracle, bounds)
    return _shared[case]


def _run(rt, F0, gws, fused):
    rt.fused = fused
    params = rt.parameters()
    try:
        ins = [t.clone().requires_grad_(True) for t in (rt.x0, rt.v0, rt.C0, F0)]
        outs = rt.rollout(*ins)
        loss = sum((o * w.to(dev())).sum() for o, w in zip(outs, gws))
        grads = torch.autograd.grad(loss, ins + params)
    finally:
        rt.fused = True
    return [o.detach().clone() for o in outs], [g.detach().clone() for g in grads]


def _fused_in_mode(rt, F0, gws, caches, pair):
    import neuma_amd.rollout as R
    from neuma_amd import _lib
    saved = (R._SVD_CACHE, R._ACT_CACHE)
    try:
        R._SVD_CACHE, R._ACT_CACHE = CACHES[caches]
        assert _lib.lib().nm_rollout_set_forward_pair(pair) == 0
        return _run(rt, F0, gws, fused=True)
    finally:
        R._SVD_CACHE, R._ACT_CACHE = saved
        _lib.lib().nm_rollout_set_forward_pair(1)


@pytest.mark.parametrize("case", list(EDGE))
def test_per_operator_path_at_a_work_split_edge(case):
    """the yardstick of the tests below is itself held to the fp64 oracle, under the same oracle-derived bounds as the fused
    path: it cannot drift from the truth unnoticed"""
    rt, F0, gws, ref, oracle, bounds = _case(case)
    for nme, a, b, tol in zip("xvCF", ref[0], oracle[0], [3e-7, 3e-6, 1.5e-5, 1.5e-6]):      # measured <= 3.9e-06 (a .. d), 7.3e-06 (e): the largest of the four
        assert abs_max(a, b) / max(1.0, float(b.abs().max())) < tol, nme
    for k, (a, b, (_, vs_oracle)) in enumerate(zip(ref[1], oracle[1], bounds)):
        assert rel_max(a, b) < vs_oracle, k      # measured <= 1.5e-05 (a .. d), 6.3e-05 (e, dL/dF0; the oracle's fp32 run: 4.9e-05)


@pytest.mark.parametrize("case,caches,pair", MODES, ids=[f"{c}-{k}-pair{p}" for c, k, p in MODES])
def test_fused_rollout_at_a_work_split_edge(case, caches, pair):
    rt, F0, gws, ref, oracle, bounds = _case(case)
    states, grads = _fused_in_mode(rt, F0, gws, caches, pair)
    assert all(torch.isfinite(t).all() for t in states + grads)
    for a, b in zip(states, ref[0]):
        assert abs_max(a, b) / max(1.0, float(b.abs().max())) < 5e-6      # measured <= 2.4e-06
    for a, b, (vs_ref, _) in zip(grads, ref[1], bounds):
        assert rel_max(a, b) < vs_ref      # measured <= 1.5e-05 (a .. d), 4.4e-05 (e), both dL/dF0
    for nme, a, b, tol in zip("xvCF", states, oracle[0], [3e-7, 3e-6, 1.5e-5, 1.5e-6]):      # measured <= 7.6e-06: the largest of the four
        assert abs_max(a, b) / max(1.0, float(b.abs().max())) < tol, nme
    for k, (a, b, (_, vs_oracle)) in enumerate(zip(grads, oracle[1], bounds)):
        assert rel_max(a, b) < vs_oracle, k      # measured <= 1.5e-05 (a .. d), 5.1e-05 (e, dL/dF0)


@pytest.mark.parametrize("caches", list(CACHES))
def test_disabled_particles_in_the_last_wave(caches):
    """case b with particle n - 1 and the first particle of the last wave disabled: their rows are the fresh state's (zeros,
    F = plasticity(I)), nothing flows back into them, and every row and gradient equals the per-operator path's (within the
    bounds that the oracle's two runs of case b give: the same scene with those two of 1991 particles enabled).  A runtime of its own: the per-operator path reuses its state buffers, and a disabled
    particle's rows are whatever the buffer held - zeros in a fresh one."""
    bounds = _case("b")[5]
    rt, F0, gws = _case("b", fresh=True)
    n = rt.N
    off = [(n - 1) // 16 * 16, n - 1]
    assert off == [1984, 1990]
    rt.statics.enabled[off] = 0
    ref = _run(rt, F0, gws, fused=False)
    states, grads = _fused_in_mode(rt, F0, gws, caches, 1)
    with torch.no_grad():
        FI = rt.plasticity(torch.eye(3, device=dev()).repeat(len(off), 1, 1))
    for x, v, C, F in (states, ref[0]):
        assert float(x[off].abs().max()) == 0 and float(v[off].abs().max()) == 0 and float(C[off].abs().max()) == 0
        assert abs_max(F[off], FI) < 2e-7      # measured 0.0e+00
    for gi in grads[:4] + ref[1][:4]:
        assert float(gi[off].abs().max()) == 0
    for a, b in zip(states, ref[0]):
        assert abs_max(a, b) / max(1.0, float(b.abs().max())) < 5e-6      # measured <= 1.0e-06
    for a, b, (vs_ref, _) in zip(grads, ref[1], bounds):
        assert torch.isfinite(a).all() and rel_max(a, b) < vs_ref      # measured <= 1.5e-05 (dL/dF0)
