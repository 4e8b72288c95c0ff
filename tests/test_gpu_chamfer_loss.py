"""GPU: nm_chamfer_loss (csrc/nm_chamfer_loss.hip) against the numpy fp64 statement of its definition
(neuma_amd/extras/chamfer_loss.py) evaluated on the indices the call returns, the indices themselves against nm_chamfer and brute
force, and the autograd operator against the torch composition.

Bounds (none of them comes from what the kernel gives):
  indices       the fp64 distance of the chosen neighbour <= the row minimum x (1 + 4 x 2^-52): fma contraction may flip an exact
                near-tie, nothing more;
  loss, terms   fp64 sums rounded once to fp32, into a zeroed word: relative error <= 2^-23 (one rounding with a factor 2, the
                bound of test_gpu_state_loss.py);
  gradient      per component |g - g_ref| <= ulp32(g_ref) + 1e-11 S, S = the sum of the absolute values of the component's
                contributions: the single output rounding, plus the fp64 summation-order bound (len - 1) 2^-53 sum|terms|
                <= 2.3e-12 sum|terms| at len = 20 000 taken with a factor ~4;
  two calls     into one word: 2 x 2^-24 relative;
  vs torch      fp64 composition on the same device, grad_output 2: loss 2^-22, gradient twice the bound above."""
import functools

import numpy as np
import pytest
import torch

from gpu_util import dev, measured

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
WXY, WYX = 0.75, 1.5          # exact in fp32
SIZES = [(1, 1), (1, 257), (257, 1), (1, 20000), (63, 65), (64, 64), (255, 257), (256, 256), (1000, 37), (4097, 5003), (20011, 19997)]
BRUTE_MAX = 4_000_000         # n m up to which the brute-force check runs: every case but the two largest sizes


def uniform(rng, n):
    return (0.1 + 0.8 * rng.random((n, 3))).astype(np.float32)


def hub():
    """n = 300, m = 5000: 4000 of the y within 0.01 of x_0, every other x at least 0.2 away - one long segment, many empty"""
    rng = np.random.default_rng(77)
    x = np.empty((300, 3), np.float32)
    x[0] = (0.2, 0.2, 0.2)
    rest = []
    while len(rest) < 299:
        p = uniform(rng, 1)[0]
        if np.linalg.norm(p.astype(np.float64) - x[0]) >= 0.2:
            rest.append(p)
    x[1:] = np.array(rest)
    near = x[0] + (0.01 / np.sqrt(3.0)) * (2.0 * rng.random((4000, 3)) - 1.0) * 0.99
    y = np.concatenate([near.astype(np.float32), uniform(rng, 1000)])
    return x, y[rng.permutation(5000)]


def copies():
    rng = np.random.default_rng(78)
    x, y = uniform(rng, 257), uniform(rng, 300)
    y[50:150] = x[100:200]                          # exact copies: distance 0
    return x, y


def coincident():
    rng = np.random.default_rng(79)
    x, y = uniform(rng, 100), uniform(rng, 400)
    x[7] = x[3]
    return x, y


def scaled(s):
    rng = np.random.default_rng(80)
    return (np.float32(s) * uniform(rng, 255)).astype(np.float32), (np.float32(s) * uniform(rng, 257)).astype(np.float32)


def sized(n, m):
    rng = np.random.default_rng(100000 * n + m)
    return uniform(rng, n), uniform(rng, m)


CASES = {f"{n}x{m}": functools.partial(sized, n, m) for n, m in SIZES}
CASES.update({"hub": hub, "copies": copies, "coincident": coincident, "scale1e-3": functools.partial(scaled, 1e-3),
              "scale1e3": functools.partial(scaled, 1e3)})


def gpu(a):
    return None if a is None else torch.tensor(a, device=dev())


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def run(x, y, mask=None, wxy=WXY, wyx=WYX, loss=None):
    """one raw call with every output, all of them pre-filled with junk; numpy results"""
    from neuma_amd.chamfer_loss import chamfer_loss_raw
    n, m = x.shape[0], y.shape[0]
    terms = torch.full((2,), -7.0, device=dev())
    g = torch.full((n, 3), 9.0, device=dev())
    ixy, iyx = torch.full((n,), 12345, dtype=torch.int64, device=dev()), torch.full((m,), 12345, dtype=torch.int64, device=dev())
    out = chamfer_loss_raw(gpu(x), gpu(y), gpu(mask), wxy, wyx, loss_out=loss, terms_out=terms, dL_dx=g, idx_xy=ixy, idx_yx=iyx)
    return dict(loss=out.cpu().numpy().reshape(1), terms=terms.cpu().numpy(), grad=g.cpu().numpy(), idx_xy=ixy.cpu().numpy(),
                idx_yx=iyx.cpu().numpy())


def same_bits(r1, r2):
    return all(np.array_equal(bits(r1[k]), bits(r2[k])) for k in ("loss", "terms", "grad", "idx_xy", "idx_yx"))


@functools.lru_cache(maxsize=None)
def case(name):
    """(x, y, the unmasked call's outputs, the fp64 reference on the returned indices): computed once, left unchanged"""
    from neuma_amd.extras.chamfer_loss import chamfer_loss_reference
    x, y = CASES[name]()
    got = run(x, y)
    ref = chamfer_loss_reference(x, y, None, WXY, WYX, idx_xy=got["idx_xy"], idx_yx=got["idx_yx"])
    return x, y, got, ref


def relerr(got, ref):
    return abs(float(got) - ref) / abs(ref) if ref != 0.0 else abs(float(got))


def grad_excess(g, ref, factor=1.0, scale=1.0):
    """max over components of |g - g_ref| / (factor (ulp32(g_ref) + 1e-11 S)); g_ref = scale x the reference gradient"""
    g_ref, s = scale * ref["grad"], abs(scale) * ref["abs_sum"]
    bound = factor * (np.spacing(np.abs(g_ref).astype(np.float32)).astype(np.float64) + 1e-11 * s)
    return float((np.abs(g.astype(np.float64) - g_ref) / bound).max())


def in_range(r, n, m):
    return bool(((r["idx_xy"] >= 0) & (r["idx_xy"] < m)).all() and ((r["idx_yx"] >= 0) & (r["idx_yx"] < n)).all())


# ---------------------------------------------------------------- indices

@pytest.mark.parametrize("name", list(CASES))
def test_indices_equal_nm_chamfer_bitwise(name):
    from neuma_amd.particle_metrics import chamfer_native
    x, y, got, _ = case(name)
    _, _, i12, i21 = chamfer_native(gpu(x)[None], gpu(y)[None])
    assert np.array_equal(got["idx_xy"], i12[0].cpu().numpy()) and np.array_equal(got["idx_yx"], i21[0].cpu().numpy())


@pytest.mark.parametrize("name", [k for k, f in CASES.items() if np.prod([a.shape[0] for a in f()]) <= BRUTE_MAX])
def test_indices_against_brute_force(name):
    x, y, got, _ = case(name)
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    d = ((x64[:, None, :] - y64[None, :, :]) ** 2).sum(2)
    assert in_range(got, x.shape[0], y.shape[0])
    slack = 1.0 + 4.0 * 2.0 ** -52
    chosen_xy, chosen_yx = d[np.arange(x.shape[0]), got["idx_xy"]], d[got["idx_yx"], np.arange(y.shape[0])]
    assert (chosen_xy <= d.min(1) * slack).all() and (chosen_yx <= d.min(0) * slack).all()
    if name == "coincident":            # the lower of two coincident rows wins every y
        assert not (got["idx_yx"] == 7).any() and (got["idx_yx"] == 3).any()
    if name == "copies":
        assert (chosen_yx[50:150] == 0.0).all() and (chosen_xy[100:200] == 0.0).all()
    if name == "hub":
        assert int((got["idx_yx"] == 0).sum()) >= 4000 and np.unique(got["idx_yx"]).size < x.shape[0]     # long and empty segments


# ---------------------------------------------------------------- values

@pytest.mark.parametrize("name", list(CASES))
def test_loss_terms_and_gradient_against_fp64_on_the_returned_indices(name):
    x, y, got, ref = case(name)
    assert measured(relerr(got["loss"][0], ref["loss"]), f"loss {name}") <= EPS
    assert measured(relerr(got["terms"][0], ref["term_xy"]), f"term_xy {name}") <= EPS
    assert measured(relerr(got["terms"][1], ref["term_yx"]), f"term_yx {name}") <= EPS
    assert measured(grad_excess(got["grad"], ref), f"dL_dx error / (ulp32 + 1e-11 S) {name}") <= 1.0
    if name == "coincident":            # the higher row keeps only its own term
        from neuma_amd.extras.chamfer_loss import chamfer_loss_reference
        own = chamfer_loss_reference(x, y, None, WXY, 0.0, idx_xy=got["idx_xy"], idx_yx=got["idx_yx"])
        assert measured(grad_excess(got["grad"][7:8], dict(grad=own["grad"][7:8], abs_sum=own["abs_sum"][7:8])), "coincident row 7") <= 1.0


@pytest.mark.parametrize("name", ["1x20000", "hub", "4097x5003"])
@pytest.mark.parametrize("masked", [False, True])
def test_two_calls_are_bitwise_equal(name, masked):
    x, y, got, _ = case(name)
    mask = (np.random.default_rng(1).random(x.shape[0]) < 0.7).astype(np.uint8) if masked else None
    if masked:
        mask[0] = 1
    r1, r2 = run(x, y, mask), run(x, y, mask)
    assert same_bits(r1, r2)
    if not masked:
        assert same_bits(r1, got)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n,m", [(5, 3), (257, 300), (4097, 5003)])
def test_views_offset_by_one_float_equal_aligned_copies_bitwise(n, m, masked):
    from neuma_amd.chamfer_loss import chamfer_loss_raw
    x, y = sized(n, m)
    mask = gpu((np.random.default_rng(2).random(n) < 0.7).astype(np.uint8)) if masked else None

    def shifted(a):          # the same values one float off a 16-byte boundary
        flat = torch.zeros(a.size + 1, device=dev())
        flat[1:] = gpu(a).reshape(-1)
        t = flat[1:].view(a.shape)
        assert t.data_ptr() % 16 == 4
        return t

    outs = []
    for place in (gpu, shifted):
        tx, ty, g = place(x), place(y), place(np.zeros((n, 3), np.float32))
        terms = place(np.zeros(2, np.float32))
        ixy, iyx = torch.zeros(n, dtype=torch.int64, device=dev()), torch.zeros(m, dtype=torch.int64, device=dev())
        loss = chamfer_loss_raw(tx, ty, mask, WXY, WYX, terms_out=terms, dL_dx=g, idx_xy=ixy, idx_yx=iyx)
        outs.append([t.cpu().numpy() for t in (loss.reshape(1), terms, g, ixy, iyx)])
    assert gpu(x).data_ptr() % 16 == 0
    for p, q in zip(*outs):
        assert np.array_equal(bits(p), bits(q))


@pytest.mark.parametrize("mask_name", ["none", "random", "empty"])
def test_sentinel_rows_around_the_outputs_stay_untouched(mask_name):
    from neuma_amd.chamfer_loss import chamfer_loss_raw
    n, m, lead, tail = 65, 70, 1, 3
    x, y = sized(n, m)
    mask = {"none": None, "random": (np.random.default_rng(3).random(n) < 0.7).astype(np.uint8), "empty": np.zeros(n, np.uint8)}[mask_name]
    gbuf = torch.full((lead + n + tail, 3), 1234.5, device=dev())
    ibx, iby = torch.full((lead + n + tail,), 777, dtype=torch.int64, device=dev()), torch.full((lead + m + tail,), 777, dtype=torch.int64, device=dev())
    words, terms = torch.full((5,), 1234.5, device=dev()), torch.full((4,), 1234.5, device=dev())
    words[2] = 0.0
    chamfer_loss_raw(gpu(x), gpu(y), gpu(mask), WXY, WYX, loss_out=words[2], terms_out=terms[1:3], dL_dx=gbuf[lead:lead + n],
                     idx_xy=ibx[lead:lead + n], idx_yx=iby[lead:lead + m])
    assert bool((gbuf[:lead] == 1234.5).all()) and bool((gbuf[lead + n:] == 1234.5).all())
    for buf, rows in ((ibx, n), (iby, m)):
        assert bool((buf[:lead] == 777).all()) and bool((buf[lead + rows:] == 777).all()) and not bool((buf[lead:lead + rows] == 777).any())
    assert words[[0, 1, 3, 4]].eq(1234.5).all() and terms[[0, 3]].eq(1234.5).all() and not terms[1:3].eq(1234.5).any()
    assert not bool((gbuf[lead:lead + n] == 1234.5).any())
    assert (float(words[2]) == 0.0) if mask_name == "empty" else (float(words[2]) > 0.0)


def test_loss_word_accumulates():
    x, y, got, ref = case("4097x5003")
    a, b = 0.75, 2.5
    word = torch.zeros((), device=dev())
    run(x, y, None, a, a, loss=word)
    run(x, y, None, b, b, loss=word)
    total = (a + b) * (ref["term_xy"] + ref["term_yx"])
    assert measured(relerr(word, total), "two calls into one word") <= 2 * 2.0 ** -24


# ---------------------------------------------------------------- mask

def masks(n):
    rng = np.random.default_rng(n)
    single = np.zeros(n, np.uint8)
    single[n // 2] = 1
    return {"random": (rng.random(n) < 0.7).astype(np.uint8), "single": single, "all": np.ones(n, np.uint8), "none-kept": np.zeros(n, np.uint8)}


@pytest.mark.parametrize("mask_name", ["random", "single", "all", "none-kept"])
@pytest.mark.parametrize("name", ["255x257", "hub", "4097x5003"])
def test_mask_equals_the_call_on_the_compacted_cloud_bitwise(name, mask_name):
    x, y, full, _ = case(name)
    n, m = x.shape[0], y.shape[0]
    mask = masks(n)[mask_name]
    keep = mask != 0
    word = torch.full((), 3.5, device=dev())
    got = run(x, y, mask, loss=word)
    assert not got["grad"][~keep].any() and (got["idx_xy"][~keep] == -1).all()          # dropped rows: exactly 0, no neighbour
    if mask_name == "none-kept":
        assert float(got["loss"][0]) == 3.5 and not got["terms"].any() and not got["grad"].any()
        assert (got["idx_xy"] == -1).all() and (got["idx_yx"] == -1).all()
        return
    rows = np.flatnonzero(keep)
    word2 = torch.full((), 3.5, device=dev())
    dense = run(x[rows], y, None, loss=word2)
    assert np.array_equal(bits(got["loss"]), bits(dense["loss"])) and np.array_equal(bits(got["terms"]), bits(dense["terms"]))
    assert np.array_equal(bits(got["grad"][rows]), bits(dense["grad"]))
    assert np.array_equal(got["idx_xy"][rows], dense["idx_xy"])
    assert np.array_equal(got["idx_yx"], rows[dense["idx_yx"]])                             # the original numbering
    if mask_name == "all":
        assert np.array_equal(bits(got["grad"]), bits(full["grad"])) and np.array_equal(got["idx_yx"], full["idx_yx"])
    if mask_name == "single":
        assert (got["idx_yx"] == n // 2).all()                                               # one row collects every observation


# ---------------------------------------------------------------- weights

@pytest.mark.parametrize("name", ["255x257", "hub"])
def test_one_sided_and_zero_weights(name):
    from neuma_amd.extras.chamfer_loss import chamfer_loss_reference
    x, y, full, _ = case(name)
    for wxy, wyx in ((1.0, 0.0), (0.0, 1.0)):
        got = run(x, y, None, wxy, wyx)
        ref = chamfer_loss_reference(x, y, None, wxy, wyx, idx_xy=got["idx_xy"], idx_yx=got["idx_yx"])
        assert measured(relerr(got["loss"][0], ref["loss"]), f"loss {name} w=({wxy},{wyx})") <= EPS
        assert measured(grad_excess(got["grad"], ref), f"dL_dx excess {name} w=({wxy},{wyx})") <= 1.0
        assert np.array_equal(bits(got["terms"]), bits(full["terms"]))                      # both terms always, unweighted
        if wxy == 0.0:                  # the scatter part only: a row nobody chose gets exactly 0
            lonely = np.setdiff1d(np.arange(x.shape[0]), got["idx_yx"])
            assert lonely.size and not got["grad"][lonely].any()
    word = torch.full((), 3.5, device=dev())
    got = run(x, y, None, 0.0, 0.0, loss=word)
    assert float(got["loss"][0]) == 3.5 and not got["grad"].any()
    assert np.array_equal(bits(got["terms"]), bits(full["terms"]))


# ---------------------------------------------------------------- autograd

@pytest.mark.parametrize("n,m,masked", [(1000, 37, False), (255, 257, True), (4097, 5003, True)])
def test_autograd_operator_against_the_torch_composition_in_fp64(n, m, masked):
    from neuma_amd.chamfer_loss import chamfer_loss, chamfer_loss_torch
    from neuma_amd.extras.chamfer_loss import chamfer_loss_reference
    x, y = sized(n, m)
    mask = masks(n)["random"] if masked else None
    tx = gpu(x).requires_grad_(True)
    loss = chamfer_loss(tx, gpu(y), gpu(mask), WXY, WYX)
    (2.0 * loss).backward()                         # (grad_output != 1: backward scales the kept gradient)
    tx64 = gpu(x).double().requires_grad_(True)
    loss64, ixy, iyx = chamfer_loss_torch(tx64, gpu(y).double(), gpu(mask), WXY, WYX, give_id=True)
    (2.0 * loss64).backward()
    assert measured(relerr(loss.detach(), float(loss64.detach())), "loss vs torch fp64") <= 2.0 ** -22
    ref = chamfer_loss_reference(x, y, mask, WXY, WYX, idx_xy=ixy.cpu().numpy(), idx_yx=iyx.cpu().numpy())
    ref["grad"] = tx64.grad.cpu().numpy() / 2.0     # torch's fp64 gradient is the reference; numpy's gives S
    assert measured(grad_excess(tx.grad.cpu().numpy(), ref, factor=2.0, scale=2.0), "x.grad vs torch fp64 / bound") <= 1.0
    if masked:
        assert not bool(tx.grad[gpu(mask) == 0].any())


# ---------------------------------------------------------------- robustness

def test_a_nan_coordinate_gives_a_nan_loss_and_leaves_the_next_call_alone():
    x, y, clean, _ = case("copies")
    bad = x.copy()
    bad[5, 1] = np.nan
    got = run(bad, y)
    assert np.isnan(got["loss"][0]) and np.isnan(got["grad"][5]).any() and in_range(got, x.shape[0], y.shape[0])
    assert same_bits(run(x, y), clean)


def test_cpu_tensor_raises():
    from neuma_amd import NeumaHipError
    from neuma_amd.chamfer_loss import chamfer_loss
    with pytest.raises(NeumaHipError):
        chamfer_loss(torch.zeros(4, 3), torch.zeros(4, 3, device=dev()))
    with pytest.raises(NeumaHipError):
        chamfer_loss(torch.zeros(4, 3, device=dev()), torch.zeros(4, 3))
