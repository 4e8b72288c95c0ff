"""GPU: nm_state_loss (csrc/nm_state.hip) against the numpy fp64 statement of its definition, and the autograd operator against
the torch composition.

Bounds (none of them comes from what the kernel gives):
  loss, terms   the kernel sums in fp64 and rounds once to fp32 (the += goes into a zeroed word): relative error <= 2^-23;
  gradients     the fp32 rounding of the fp64 formula, up to fp64 rounding before it: within 1 ulp;
  two calls     accumulate a t + b t with one more fp32 rounding: 2 roundings, <= 2 * 2^-24 relative (positive weights);
  vs torch      torch rounds x - x_gt to fp32 first: 2^-22 on the loss, 2 ulp on the gradients."""
import numpy as np
import pytest
import torch

from gpu_util import dev, measured
from test_state_loss_cpu import masks, reference

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
WX, WV = 0.75, 1.5          # exact in fp32


def sizes():
    from neuma_amd.state_loss import ROWS_PER_SWEEP
    return [1, 2, 63, 64, 65, 255, 256, 257, 4097, ROWS_PER_SWEEP + 5]     # the last: the grid-stride loop runs twice


def ulps(a: np.ndarray, b: np.ndarray) -> int:
    """largest distance in units in the last place between two fp32 arrays (+0 and -0 are the same number)"""
    def key(t):
        i = np.ascontiguousarray(t, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int(np.abs(key(a) - key(b)).max()) if a.size else 0


def inputs(n, seed=0, scale=1.0, spread=1.0):
    rng = np.random.default_rng(seed)
    x = (scale * (1.0 + rng.random((n, 3)))).astype(np.float32)
    v = (scale * rng.standard_normal((n, 3))).astype(np.float32)
    xg = (x + scale * spread * rng.standard_normal((n, 3))).astype(np.float32)
    vg = (v + scale * spread * rng.standard_normal((n, 3))).astype(np.float32)
    return rng, x, v, xg, vg


def gpu(a):
    return None if a is None else torch.tensor(a, device=dev())


def run(x, v, xg, vg, mask, kind, wx=WX, wv=WV, loss=None):
    """one raw call with every output; returns numpy (loss, terms, gx, gv)"""
    from neuma_amd.state_loss import state_loss_raw
    n = x.shape[0]
    tx, tv, txg, tvg, tm = gpu(x), gpu(v), gpu(xg), gpu(vg), gpu(mask)
    terms = torch.full((2,), -7.0, device=dev())
    gx, gv = torch.full((n, 3), 9.0, device=dev()), torch.full((n, 3), 9.0, device=dev())
    out = state_loss_raw(tx, tv, txg, tvg, tm, kind, wx, wv, loss_out=loss, terms_out=terms, dL_dx=gx, dL_dv=gv)
    return out, terms.cpu().numpy(), gx.cpu().numpy(), gv.cpu().numpy()


def relerr(got, ref):
    return abs(float(got) - ref) / abs(ref) if ref != 0.0 else abs(float(got))


@pytest.mark.parametrize("kind", ["l1", "l2"])
@pytest.mark.parametrize("n", sizes())
def test_loss_terms_and_gradients_against_fp64(n, kind):
    rng, x, v, xg, vg = inputs(n, seed=n)
    if kind == "l1":
        x[n // 2] = xg[n // 2]                        # an l1 row with x == x_gt exactly
    for with_v in (False, True):
        for name, mask in masks(n, rng).items():
            ref, tx, tv, gx, gv = reference(x, v, xg, vg if with_v else None, mask, kind, WX, WV)
            loss, terms, hx, hv = run(x, v, xg, vg if with_v else None, mask, kind)
            case = f"n={n} {kind} v={with_v} mask={name}"
            assert measured(relerr(loss, ref), f"loss {case}") <= EPS
            assert measured(relerr(terms[0], tx), f"term_x {case}") <= EPS
            assert measured(relerr(terms[1], tv), f"term_v {case}") <= EPS
            assert measured(ulps(hx, gx.astype(np.float32)), f"dL_dx ulp {case}") <= 1
            assert measured(ulps(hv, gv.astype(np.float32)), f"dL_dv ulp {case}") <= 1
            if mask is not None:
                assert not hx[np.asarray(mask) == 0].any() and not hv[np.asarray(mask) == 0].any()      # dropped rows: exactly 0
            if name == "all-zero":
                assert float(loss) == 0.0 and not hx.any() and not hv.any()
            if not with_v:
                assert not hv.any() and terms[1] == 0.0
            if kind == "l1" and (mask is None or mask[n // 2]):
                assert not hx[n // 2].any()


@pytest.mark.parametrize("kind", ["l1", "l2"])
@pytest.mark.parametrize("scale", [1e-3, 1e3])
def test_cancellation_at_small_and_large_coordinates(kind, scale):
    n = 257
    rng, x, v, xg, vg = inputs(n, seed=5, scale=scale, spread=1e-5)       # differences of a few ulps of the coordinates
    ref, tx, tv, gx, gv = reference(x, v, xg, vg, None, kind, WX, WV)
    loss, terms, hx, hv = run(x, v, xg, vg, None, kind)
    assert measured(relerr(loss, ref), f"loss scale {scale}") <= EPS
    assert measured(relerr(terms[0], tx), f"term_x scale {scale}") <= EPS
    assert measured(ulps(hx, gx.astype(np.float32)), f"dL_dx ulp scale {scale}") <= 1
    assert measured(ulps(hv, gv.astype(np.float32)), f"dL_dv ulp scale {scale}") <= 1


@pytest.mark.parametrize("kind", ["l1", "l2"])
def test_loss_word_accumulates_and_zero_weights_give_zero_gradients(kind):
    n = 4097
    rng, x, v, xg, vg = inputs(n, seed=2)
    a, b = 0.75, 2.5
    _, tx, _, _, _ = reference(x, v, xg, None, None, kind, 1.0, 1.0)
    word = torch.zeros((), device=dev())
    run(x, v, xg, None, None, kind, wx=a, loss=word)
    run(x, v, xg, None, None, kind, wx=b, loss=word)
    assert measured(relerr(word, a * tx + b * tx), "two calls into one word") <= 2 * 2.0 ** -24
    loss, terms, hx, hv = run(x, v, xg, vg, None, kind, wx=0.0, wv=0.0)
    assert float(loss) == 0.0 and not hx.any() and not hv.any()
    assert measured(relerr(terms[0], tx), "terms are unweighted") <= EPS


@pytest.mark.parametrize("n", [257, 4097])
def test_two_calls_are_bitwise_equal(n):
    rng, x, v, xg, vg = inputs(n, seed=9)
    mask = masks(n, rng)["random"]
    for kind in ("l1", "l2"):
        r1, r2 = run(x, v, xg, vg, mask, kind), run(x, v, xg, vg, mask, kind)
        assert torch.equal(r1[0], r2[0])
        for p, q in zip(r1[1:], r2[1:]):
            assert np.array_equal(p.view(np.int32), q.view(np.int32))


@pytest.mark.parametrize("lead", [4, 1])        # rows in front: 4 = 48 bytes (float4 path), 1 = 12 bytes (scalar path)
def test_sentinel_rows_around_the_outputs_stay_untouched(lead):
    from neuma_amd.state_loss import state_loss_raw
    n, tail = 65, 3
    rng, x, v, xg, vg = inputs(n, seed=4)
    bufs = [torch.full((lead + n + tail, 3), 1234.5, device=dev()) for _ in range(2)]
    gx, gv = (b[lead:lead + n] for b in bufs)
    words = torch.full((5,), 1234.5, device=dev())
    words[2] = 0.0
    terms = torch.full((4,), 1234.5, device=dev())
    state_loss_raw(gpu(x), gpu(v), gpu(xg), gpu(vg), None, "l2", WX, WV, loss_out=words[2], terms_out=terms[1:3], dL_dx=gx, dL_dv=gv)
    _, _, _, rx, rv = reference(x, v, xg, vg, None, "l2", WX, WV)
    for b, r in zip(bufs, (rx, rv)):
        assert bool((b[:lead] == 1234.5).all()) and bool((b[lead + n:] == 1234.5).all())
        assert ulps(b[lead:lead + n].cpu().numpy(), r.astype(np.float32)) <= 1
    assert words[[0, 1, 3, 4]].eq(1234.5).all() and terms[[0, 3]].eq(1234.5).all() and float(words[2]) > 0


@pytest.mark.parametrize("kind", ["l1", "l2"])
@pytest.mark.parametrize("n", [5, 257, 4097])
def test_views_offset_by_one_float_equal_aligned_copies_bitwise(n, kind):
    from neuma_amd.state_loss import state_loss_raw
    rng, x, v, xg, vg = inputs(n, seed=7)
    mask = gpu(masks(n, rng)["random"])

    def shifted(a):          # the same values one float off a 16-byte boundary
        flat = torch.zeros(3 * n + 1, device=dev())
        flat[1:] = gpu(a).reshape(-1)
        t = flat[1:].view(n, 3)
        assert t.data_ptr() % 16 == 4
        return t

    aligned = [gpu(a) for a in (x, v, xg, vg)]
    assert all(t.data_ptr() % 16 == 0 for t in aligned)
    outs = []
    for ops, out in ((aligned, lambda: torch.empty(n, 3, device=dev())), ([shifted(a) for a in (x, v, xg, vg)], lambda: shifted(np.zeros((n, 3), np.float32)))):
        gx, gv, terms = out(), out(), torch.zeros(2, device=dev())
        loss = state_loss_raw(*ops, mask, kind, WX, WV, terms_out=terms, dL_dx=gx, dL_dv=gv)
        outs.append((loss.reshape(1), terms, gx, gv))
    for p, q in zip(*outs):
        assert np.array_equal(p.cpu().numpy().view(np.int32), q.cpu().numpy().view(np.int32))


@pytest.mark.parametrize("kind", ["l1", "l2"])
@pytest.mark.parametrize("with_v,masked", [(True, False), (True, True), (False, True)])
def test_autograd_operator_against_the_torch_composition(kind, with_v, masked):
    from neuma_amd.state_loss import state_loss, state_loss_torch
    n = 4097
    rng, x, v, xg, vg = inputs(n, seed=11)
    mask = gpu(masks(n, rng)["random"]) if masked else None
    got = []
    for fn in (state_loss, state_loss_torch):
        tx, tv = gpu(x).requires_grad_(True), gpu(v).requires_grad_(True)
        # unit weights and a power-of-two grad_output: torch then rounds x - x_gt, 2 / (3 m) and their product (up to 1.5 ulp
        # together) and the kernel's gradient once (0.5 ulp) - any further factor in the chain is one more rounding on torch's
        # side that the 2 ulp do not have room for.  The weights' own arithmetic is held to fp64 in the tests above.
        loss = fn(tx, tv, gpu(xg), gpu(vg) if with_v else None, mask, kind=kind, weight_x=1.0, weight_v=1.0)
        (2.0 * loss).backward()                     # (grad_output != 1: backward scales the kept gradients)
        got.append((float(loss.detach()), tx.grad.cpu().numpy(), np.zeros((n, 3), np.float32) if tv.grad is None else tv.grad.cpu().numpy()))
    (l1, gx1, gv1), (l2, gx2, gv2) = got
    assert measured(abs(l1 - l2) / abs(l2), "loss vs torch") <= 2.0 ** -22
    assert measured(ulps(gx1, gx2), "x.grad vs torch (ulp)") <= 2
    assert measured(ulps(gv1, gv2), "v.grad vs torch (ulp)") <= 2


def test_cpu_tensor_raises():
    from neuma_amd import NeumaHipError
    from neuma_amd.state_loss import state_loss
    with pytest.raises(NeumaHipError):
        state_loss(torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4, 3, device=dev()), None)
    with pytest.raises(NeumaHipError):
        state_loss(torch.zeros(4, 3), None, torch.zeros(4, 3))
