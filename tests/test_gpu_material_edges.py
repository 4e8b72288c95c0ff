"""GPU parity: the constitutive kernels (k_material_fwd / k_material_bwd / k_wgrad_reduce through nm_material_fwd and
nm_material_bwd_ex) against fp64 at every edge of their work split - partial tiles, empty waves, second rounds, each change
of the per-wave quota, 1 to 256 workgroups and every exit of the reduce kernel's loops (tests/material_edge_cases.py).

Bounds are the ones the golden and ragged-tail tests of test_gpu_svd_material.py hold the same quantities to: stress 3e-6
(rel), F_p 3.5e-7 (abs), dL/dF 1e-5 (rel), weight gradients 2e-5 (rel) - except where the reference's own fp32 run is further
than half of that from its fp64 run on these (50 % strain) inputs: material_edge_cases.bound has the derivation, every
comparison logs that run's distance next to its own.  Two cotangents per case: a dense one, and one that is
non-zero only on the particles next to a boundary of the work split, so that the fp64 weight gradient is a sum of a dozen
terms and a lost, doubled or misplaced particle or partial is an error of order 1/12.  A particle is one lane and one MFMA
column: results of the first n rows do not depend on how many rows follow, bit for bit."""
import ctypes as C

import pytest
import torch

import material_edge_cases as mc
from gpu_util import dev, rel_max, abs_max, parity

pytestmark = pytest.mark.gpu

B_STRESS, B_FP, B_GF, B_GW = 3e-6, 3.5e-7, 1e-5, 2e-5
KIND_ID = {"e": 0, "p": 1}
KIND_NAME = {"e": "elasticity", "p": "plasticity"}
NM_BWD_ACCUMULATE, NM_BWD_POLAR_ADJOINT = 1, 2
NM_ERR_INVALID, NM_ERR_WORKSPACE = -1, -3
SENTINEL = 0x7FA5C3E1       # a NaN's bit pattern: compared as integers
PAD = 8                     # sentinel rows behind the n rows a call may write
_gpu = {}


def _L():
    from neuma_amd import _lib as L
    return L


def _once(key, make):
    if key not in _gpu:
        _gpu[key] = make()
    return _gpu[key]


def _F_all():
    return _once("F", lambda: mc.separated_F().float().to(dev()))


def _go_all():
    return _once("go", lambda: mc.dense_gout().float().to(dev()))


def _W(name, kind, lora):
    return _once(("W", name, kind, lora), lambda: [w.float().to(dev()).contiguous() for w in mc.weights(name, kind, lora)])


def _sentinel_rows(rows, offset_floats=0):
    """(buffer, view of `rows` x 3 x 3 floats starting `offset_floats` into it), every word the sentinel"""
    buf = torch.full((offset_floats + rows * 9 + 4,), SENTINEL, dtype=torch.int32, device=dev()).view(torch.float32)
    return buf, buf[offset_floats:offset_floats + rows * 9].view(rows, 3, 3)


def _untouched(t):
    return bool((t.contiguous().view(torch.int32) == SENTINEL).all())


def _shifted(t):
    """a copy of t that starts one float behind a 16-byte boundary"""
    buf = torch.empty(t.numel() + 8, dtype=torch.float32, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _fwd(n, kind, F, W, out=None):
    """nm_material_fwd on F[:n]; returns the whole n + PAD rows of a sentinel-filled buffer (or the caller's `out`)"""
    L = _L()
    if out is None:
        _, out = _sentinel_rows(n + PAD)
    mlp = L.nm_mlp(L.ptr(W[0]), L.ptr(W[1]), L.ptr(W[2]))
    L.check(L.lib().nm_material_fwd(n, KIND_ID[kind], mc.ALPHA, L.ptr(F), C.byref(mlp), L.ptr(out), L.stream_ptr(dev())), "nm_material_fwd")
    return out


def _workspace(n):
    nbytes = int(_L().lib().nm_material_bwd_workspace(n))
    return torch.empty(nbytes, dtype=torch.uint8, device=dev()), nbytes


def _bwd(n, kind, F, W, gout, flags=0, gF=None, gw=None, ws=None, want_w=True):
    """nm_material_bwd_ex; returns (gF with PAD sentinel rows, [gw0, gw1, gw2])"""
    L = _L()
    if gF is None:
        _, gF = _sentinel_rows(n + PAD)
    if gw is None and want_w:
        gw = [torch.full_like(w, float("nan")) for w in W]
    wsbuf, nbytes = ws if ws is not None else (_workspace(n) if want_w else (None, 0))
    mlp = L.nm_mlp(L.ptr(W[0]), L.ptr(W[1]), L.ptr(W[2]))
    g = gw if want_w else [None, None, None]
    L.check(L.lib().nm_material_bwd_ex(n, KIND_ID[kind], mc.ALPHA, L.ptr(F), C.byref(mlp), L.ptr(gout), L.ptr(gF), L.ptr(g[0]),
                                       L.ptr(g[1]), L.ptr(g[2]), flags, L.ptr(wsbuf), nbytes, L.stream_ptr(dev())), "nm_material_bwd_ex")
    return gF, gw


def _whole(kind, what):
    """forward values / dense dL/dF of all N_MAX rows in one call (jelly + LoRA): what every case's rows must equal bit for bit"""
    W = _W("jelly", kind, True)
    if what == "fwd":
        return _once(("whole", kind, what), lambda: _fwd(mc.N_MAX, kind, _F_all(), W)[:mc.N_MAX].clone())
    return _once(("whole", kind, what), lambda: _bwd(mc.N_MAX, kind, _F_all(), W, _go_all(), want_w=False)[0][:mc.N_MAX].clone())


def test_case_list_matches_the_librarys_grid():
    """NM_BWD_GRID = 256 workgroups of NM_WACC = 6144 floats: a change of either moves every edge of the case list"""
    lib = _L().lib()
    for n in (1, 2000, mc.N_MAX):
        assert int(lib.nm_material_bwd_workspace(n)) // (mc.NM_WACC * 4) == mc.NM_BWD_GRID == 256
        assert int(lib.nm_material_bwd_workspace(n)) % (mc.NM_WACC * 4) == 0
    assert mc.coverage_gaps() == []


@pytest.mark.parametrize("n", mc.CASES)
def test_forward_matches_fp64_at_every_edge(n):
    F = _F_all()[:n].contiguous()
    Fd = mc.degenerate_F(n).float().to(dev())
    for name in mc.NAMES:
        for kind in mc.KINDS:
            W = _W(name, kind, False)
            case = f"work-split edges, forward, {name} checkpoint, {KIND_NAME[kind]}, vs fp64 oracle"
            for tag, x, ref in (("", F, mc.forward_ref(name, kind, n)), (", F = I and tied rows", Fd, mc.degenerate_forward_ref(name, kind, n))):
                out = _fwd(n, kind, x, W)
                assert _untouched(out[n:]), (name, kind, tag)
                assert torch.isfinite(out[:n]).all()
                if kind == "e":
                    parity(case, "stress (rel)" + tag, rel_max(out[:n], ref), B_STRESS)      # measured <= 6.0e-07
                else:
                    parity(case, "F_p (abs)" + tag, abs_max(out[:n], ref), B_FP)      # measured <= 7.9e-08


@pytest.mark.parametrize("n", mc.CASES)
def test_backward_matches_fp64_at_every_edge(n):
    F = _F_all()[:n].contiguous()
    for kind in mc.KINDS:
        W = _W("jelly", kind, True)
        case = f"work-split edges, backward, jelly + LoRA, {KIND_NAME[kind]}, vs fp64 autograd"
        _, gF_ref, dW_ref, noise = mc.dense_ref(kind, n)
        gFb_ref, dWb_ref, noise_b = mc.boundary_ref(kind, n)
        gob = mc.boundary_gout(n).float().to(dev())
        for tag, go, gF_r, dW_r, nz in ((" dense", _go_all()[:n].contiguous(), gF_ref, dW_ref, noise),
                                        (" boundary", gob, gFb_ref, dWb_ref, noise_b)):
            gF, gw = _bwd(n, kind, F, W, go)
            assert _untouched(gF[n:]), (kind, tag)
            assert torch.isfinite(gF[:n]).all() and all(torch.isfinite(g).all() for g in gw)
            parity(case, "dL/dF (rel)," + tag, rel_max(gF[:n], gF_r), mc.bound(B_GF, nz["gF"]), nz["gF"])      # measured <= 1.3e-05 where the fp32 run is 1.2e-05 off (e), 4.9e-08 (p)
            for i in range(3):
                parity(case, f"dL/dW{i} (rel)," + tag, rel_max(gw[i], dW_r[i]), mc.bound(B_GW, nz["dW"][i]), nz["dW"][i])      # measured <= 3.3e-05 where the fp32 run is 2.9e-05 off (e, dL/dW1, boundary), 1.5e-06 (p)
        # the further block: F = I and tied singular values, where the reference's own adjoint is clamped noise - finite only
        gF, gw = _bwd(n, kind, mc.degenerate_F(n).float().to(dev()), W, _go_all()[:n].contiguous())
        assert _untouched(gF[n:]) and torch.isfinite(gF[:n]).all() and all(torch.isfinite(g).all() for g in gw)


@pytest.mark.parametrize("n", mc.CASES)
def test_rows_do_not_depend_on_the_rows_behind_them(n):
    """fwd(F[:n]) == fwd(F[:n_max])[:n] and likewise dL/dF, bit for bit: another n is another quota, another lane and another
    wave for the same particle, and nothing else"""
    F, go = _F_all()[:n].contiguous(), _go_all()[:n].contiguous()
    for kind in mc.KINDS:
        W = _W("jelly", kind, True)
        assert torch.equal(_fwd(n, kind, F, W)[:n], _whole(kind, "fwd")[:n]), kind
        assert torch.equal(_bwd(n, kind, F, W, go, want_w=False)[0][:n], _whole(kind, "bwd")[:n]), kind
        gF, _ = _bwd(n, kind, F, W, go)                       # with and without weight gradients: the same dL/dF
        assert torch.equal(gF[:n], _whole(kind, "bwd")[:n]), kind


@pytest.mark.parametrize("n", (17, 16_385, 65_537))
def test_autograd_wrappers_at_the_edges(n, golden_dir):
    """the nets' forward() / backward() (LoRA merge kernels + MaterialFunction) on the same rows: values, dL/dF and the LoRA
    factors' gradients against the fp64 chain rule through W + s B A"""
    import numpy as np
    from gpu_util import material_nets
    g, E, P = material_nets("jelly", golden_dir, lora=True)
    for net, kind in ((E, "e"), (P, "p")):
        case = f"work-split edges, autograd wrappers, jelly + LoRA, {KIND_NAME[kind]}, vs fp64 autograd"
        out_ref, gF_ref, dW_ref, noise = mc.dense_ref(kind, n)
        Fg = _F_all()[:n].clone().requires_grad_(True)
        out = net(Fg)
        if kind == "e":
            parity(case, "stress (rel)", rel_max(out, out_ref), B_STRESS)      # measured <= 5.8e-07
        else:
            parity(case, "F_p (abs)", abs_max(out, out_ref), B_FP)      # measured <= 6.0e-08
        (out * _go_all()[:n]).sum().backward()
        parity(case, "dL/dF (rel)", rel_max(Fg.grad, gF_ref), mc.bound(B_GF, noise["gF"]), noise["gF"])      # measured <= 9.7e-06
        sc = float(g[f"{kind}_scaling"])
        for i, lin in enumerate((net.layers[0].fc, net.layers[1].fc, net.final_layer.fc)):
            A, B = torch.tensor(g[f"{kind}_A{i}"]).double(), torch.tensor(g[f"{kind}_B{i}"]).double()
            gA, gB, dW32 = sc * B.T @ dW_ref[i], sc * dW_ref[i] @ A.T, noise["dW32"][i]
            nA, nB = mc.rel(sc * B.T @ dW32, gA), mc.rel(sc * dW32 @ A.T, gB)          # the fp32 run's dL/dW through the same chain rule
            parity(case, "dL/dA (rel, worst layer)", rel_max(lin.lora_A.grad, gA), mc.bound(B_GW, nA), nA)      # measured <= 2.5e-06
            parity(case, "dL/dB (rel, worst layer)", rel_max(lin.lora_B.grad, gB), mc.bound(B_GW, nB), nB)      # measured <= 3.2e-06
        net.zero_grad()


@pytest.mark.parametrize("n", mc.CASES)
def test_accumulate_adds_once_and_the_order_is_fixed(n):
    """NM_BWD_ACCUMULATE: gw = preset + g with exactly one fp32 addition per element (k_wgrad_reduce's `*dst + acc`); two
    identical calls: identical weight gradients (the partials and their sum have a fixed order)"""
    F, go = _F_all()[:n].contiguous(), mc.boundary_gout(n).float().to(dev())
    gen = torch.Generator().manual_seed(n)
    for kind in mc.KINDS:
        W = _W("jelly", kind, True)
        for cot in (go, _go_all()[:n].contiguous()):
            _, g1 = _bwd(n, kind, F, W, cot)
            _, g2 = _bwd(n, kind, F, W, cot)
            assert all(torch.equal(a, b) for a, b in zip(g1, g2)), kind
            # dyadic presets of every magnitude around the gradients': preset + g rounds once, in the kernel as in torch
            preset = [(torch.ldexp(torch.ones(w.shape), torch.randint(-6, 14, w.shape, generator=gen))
                       * (1 - 2 * torch.randint(0, 2, w.shape, generator=gen))).to(dev()) for w in W]
            _, g3 = _bwd(n, kind, F, W, cot, flags=NM_BWD_ACCUMULATE, gw=[p.clone() for p in preset])
            assert all(torch.equal(a, p + b) for a, p, b in zip(g3, preset, g1)), kind


@pytest.mark.parametrize("n", mc.POLAR_CASES)
def test_polar_adjoint_is_the_same_function_away_from_ties(n):
    F, go = _F_all()[:n].contiguous(), _go_all()[:n].contiguous()
    for kind in mc.KINDS:
        W = _W("jelly", kind, True)
        case = f"work-split edges, backward, jelly + LoRA, {KIND_NAME[kind]}, vs fp64 autograd"
        _, gF_ref, _, noise = mc.dense_ref(kind, n)
        gF, gw = _bwd(n, kind, F, W, go, flags=NM_BWD_POLAR_ADJOINT)
        assert _untouched(gF[n:])
        parity(case, "dL/dF (rel), polar adjoint", rel_max(gF[:n], gF_ref), mc.bound(B_GF, noise["gF"]), noise["gF"])      # measured <= 9.7e-06
        gF0, gw0 = _bwd(n, kind, F, W, go)
        # ... and equals the default mode: the same function of these rows, the suite's dL/dF bound between the two
        parity(f"work-split edges, backward, jelly + LoRA, {KIND_NAME[kind]}, polar vs default adjoint", "dL/dF (rel)",
               rel_max(gF[:n], gF0[:n].double().cpu()), B_GF)      # measured <= 9.5e-08
        assert all(torch.equal(a, b) for a, b in zip(gw, gw0))          # the weight gradients do not pass through the SVD adjoint


@pytest.mark.parametrize("n", mc.MISALIGNED_CASES)
def test_pointers_one_float_past_a_16_byte_boundary(n):
    F, go = _F_all()[:n].contiguous(), _go_all()[:n].contiguous()
    for kind in mc.KINDS:
        W = _W("jelly", kind, True)
        out = _fwd(n, kind, F, W)
        buf, out_s = _sentinel_rows(n + PAD, offset_floats=1)
        assert out_s.data_ptr() % 16 == 4
        _fwd(n, kind, _shifted(F), W, out=out_s)
        assert torch.equal(out_s[:n], out[:n]) and _untouched(out_s[n:]) and _untouched(buf[:1]), kind
        gF, gw = _bwd(n, kind, F, W, go)
        buf, gF_s = _sentinel_rows(n + PAD, offset_floats=1)
        _, gw_s = _bwd(n, kind, _shifted(F), W, _shifted(go), gF=gF_s)
        assert torch.equal(gF_s[:n], gF[:n]) and _untouched(gF_s[n:]) and _untouched(buf[:1]), kind
        assert all(torch.equal(a, b) for a, b in zip(gw_s, gw)), kind


def test_backward_protocol_refusals_write_nothing():
    L = _L()
    lib = L.lib()
    n, kind = 257, "e"
    F, go, W = _F_all()[:n].contiguous(), _go_all()[:n].contiguous(), _W("jelly", kind, True)
    mlp = L.nm_mlp(L.ptr(W[0]), L.ptr(W[1]), L.ptr(W[2]))
    s = L.stream_ptr(dev())

    def fresh():
        gF = _sentinel_rows(n + PAD)[1]
        gw = [torch.full(w.shape, SENTINEL, dtype=torch.int32, device=dev()).view(torch.float32) for w in W]
        return gF, gw

    def call(nn, gF, gw, flags, ws, nbytes):
        rc = lib.nm_material_bwd_ex(nn, 0, mc.ALPHA, L.ptr(F), C.byref(mlp), L.ptr(go), L.ptr(gF), L.ptr(gw[0]), L.ptr(gw[1]),
                                    L.ptr(gw[2]), flags, L.ptr(ws), nbytes, s)
        torch.cuda.synchronize()
        return rc

    ws, nbytes = _workspace(n)
    # a workspace one byte short
    gF, gw = fresh()
    assert call(n, gF, gw, 0, ws, nbytes - 1) == NM_ERR_WORKSPACE
    assert _untouched(gF) and all(_untouched(g) for g in gw) and b"workspace" in lib.nm_last_error()
    assert call(n, gF, gw, 0, None, nbytes) == NM_ERR_WORKSPACE and _untouched(gF)
    # mixed null weight-gradient pointers
    for mask in ((1, 0, 0), (1, 1, 0), (0, 1, 1), (0, 0, 1), (1, 0, 1)):
        gF, gw = fresh()
        part = [g if m else None for g, m in zip(gw, mask)]
        assert call(n, gF, part, 0, ws, nbytes) == NM_ERR_INVALID, mask
        assert _untouched(gF) and all(_untouched(g) for g in gw), mask
    # n == 0: gw* zeroed - or left alone when they accumulate
    gF, gw = fresh()
    assert call(0, gF, gw, NM_BWD_ACCUMULATE, ws, nbytes) == 0
    assert _untouched(gF) and all(_untouched(g) for g in gw)
    assert call(0, gF, gw, 0, ws, nbytes) == 0
    assert _untouched(gF) and all(bool((g.view(torch.int32) == 0).all()) for g in gw)
    # and the full-size workspace is enough
    gF, gw = fresh()
    assert call(n, gF, gw, 0, ws, nbytes) == 0
    assert _untouched(gF[n:]) and torch.isfinite(gF[:n]).all() and all(torch.isfinite(g).all() for g in gw)
