"""GPU: the frame-tail kernels of csrc/nm_bind.hip - k_spmm_csr, k_spmm_csr_sum3, k_bind_frame, k_cov_deform, k_pixel_loss -
against fp64 at the edges of their loops (frame_tail_cases.py): empty rows, every tail residue, rows around one and two trips of
the sixteen sharing lanes, every column-count branch, images on both sides of the float4 / scalar, grid-stride and grid-cap rules.

On EXACT data (dyadic grids, every intermediate representable) the fp64 reference rounded to fp32 is the only correct answer
and the comparison is bit for bit: the logged figure is 0, or the largest difference among the words that differ.  On RANDOM
data the logged figure is max |err| / bound with the DERIVED bound (L + c) 2^-24 sum |w| |x| of the row (each test states its
c), held to <= 1.  Every comparison goes through gpu_util.parity."""
import types
from functools import lru_cache

import numpy as np
import pytest
import torch

import frame_tail_cases as fc
from gpu_util import dev, parity

pytestmark = pytest.mark.gpu
SENT = -7777.0                  # what guard rows (and not yet written outputs) hold
LANE_NAMES = [s.name for s in fc.lane_structures()]
BIND_NAMES = [s.name for s in fc.bind_structures()]
PIXEL_IDS = [f"{h}x{w}" for h, w in fc.PIXEL_SHAPES]


# ---------------------------------------------------------------- helpers
def _L():
    from neuma_amd import _lib
    return _lib


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _np(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


@lru_cache(maxsize=None)
def _struct(name, exact=True):
    """(Csr, rowptr, col, val on the device); shared by the tests, never written"""
    s = fc.by_name(fc.lane_structures(exact) + fc.bind_structures(exact))[name]
    return s, _t(s.rowptr), _t(s.col), _t(s.val)


class Guarded(object):
    """an output of `rows` x `width` floats between guard rows that must stay untouched; `shift` floats of misalignment"""

    def __init__(self, rows, width, pad=64, shift=0):
        n = rows * width
        self.buf = torch.full((n + 2 * pad + shift,), SENT, dtype=torch.float32, device=dev())
        self.lo, self.hi = pad + shift, pad + shift + n
        self.view = self.buf[self.lo:self.hi].view(rows, width)

    def intact(self):
        return bool((self.buf[:self.lo] == SENT).all()) and bool((self.buf[self.hi:] == SENT).all())


def _exact_err(got, ref64):
    """0 if `got` (fp32) equals the fp32 rounding of the fp64 reference in every BIT; else the largest difference among the
    words that differ (at least the smallest positive number, so that a wrong sign of zero or a NaN shows too)"""
    got = np.ascontiguousarray(got, dtype=np.float32)
    ref = np.ascontiguousarray(np.asarray(ref64).astype(np.float32))
    assert got.shape == ref.shape, (got.shape, ref.shape)
    bad = got.view(np.int32) != ref.view(np.int32)
    if not bad.any():
        return 0.0
    d = np.abs(got[bad].astype(np.float64) - ref[bad].astype(np.float64))
    return float(max(np.nan_to_num(d, nan=np.inf).max(), np.finfo(np.float64).tiny))


def _exact(case, name, got, ref64):
    parity(case, name, _exact_err(got, ref64), 0.0)


def _within(case, name, got, ref64, bound):
    """max |got - ref| / bound <= 1 (an element whose bound is 0 must be exact)"""
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref64, dtype=np.float64))
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    assert np.isfinite(np.asarray(got)).all()
    parity(case, name + ": abs err / derived bound", float(ratio.max(initial=0.0)), 1.0)


def _last_error():
    return _L().lib().nm_last_error().decode(errors="replace")


def _spmm(sd, D, X, out):
    L = _L()
    s, rowptr, col, val = sd
    return L.lib().nm_spmm_csr(s.rows, D, L.ptr(rowptr), L.ptr(col), L.ptr(val), L.ptr(X), L.ptr(out), L.stream_ptr(dev()))


def _sum3(sd, ins, scale, out):
    L = _L()
    s, rowptr, col, val = sd
    p = [L.ptr(t) for t in ins]
    return L.lib().nm_spmm_csr_sum3(s.rows, L.ptr(rowptr), L.ptr(col), L.ptr(val), p[0], p[1], p[2], p[3], float(scale), L.ptr(out),
                                    L.stream_ptr(dev()))


def _bind_frame(sd, pc, pp, kp, F, cov6, means, cov_out, F_out):
    L = _L()
    s, rowptr, col, val = sd
    return L.lib().nm_bind_frame(s.rows, L.ptr(rowptr), L.ptr(col), L.ptr(val), L.ptr(pc), L.ptr(pp), L.ptr(kp), L.ptr(F), L.ptr(cov6),
                                 L.ptr(means), L.ptr(cov_out), L.ptr(F_out), L.stream_ptr(dev()))


def _bindings_of(s, transposed=False):
    """tune.Bindings of the structure (or of its transpose: then the TRANSPOSED CSR, which the reverse sweep reads, has the
    structure's chosen rows), from raw un-coalesced triples"""
    from neuma_amd.tune import Bindings
    r, c = torch.from_numpy(s.row_of), torch.from_numpy(s.col.astype(np.int64))
    idx, size = (torch.stack([c, r]), (s.ncols, s.rows)) if transposed else (torch.stack([r, c]), (s.rows, s.ncols))
    return Bindings(idx, torch.from_numpy(s.val), size, device=dev())


# ---------------------------------------------------------------- nm_spmm_csr
@pytest.mark.parametrize("name", LANE_NAMES + ["bind_k257"])
def test_spmm_exact_every_column_count(name):
    """every D of fc.SPMM_D (lane sharing D <= 4, a lane per column D <= 16, the second column trip D > 16) on every
    structure: bit-equal to fp64, guard rows untouched"""
    sd = _struct(name)
    s = sd[0]
    assert fc.spmm_margin(s) < fc.EXACT_LIMIT
    rng = np.random.default_rng(11)
    for D in fc.SPMM_D:
        X = fc.exact_values(rng, (s.ncols, D))
        out = Guarded(s.rows, D, pad=2 * D + 1)
        assert _spmm(sd, D, _t(X), out.view) == 0, _last_error()
        _exact(f"nm_spmm_csr, exact data, {name}", f"D={D}", _np(out.view), fc.spmm_ref(s, X))
        assert out.intact(), D


@pytest.mark.parametrize("D", [3, 9, 33])
def test_spmm_random_within_derived_bound(D):
    """c = 1: a row's L products and L - 1 partial sums are at most L roundings per term in any order (the shuffle tree adds
    exact zeros for lanes without entries), none with fma contraction for the products; nothing else is rounded (the store is
    the sum itself).  The 1 covers the second-order terms.  Two calls give the same bits (no atomics, fixed tree)."""
    rng = np.random.default_rng(12)
    for name in LANE_NAMES + BIND_NAMES:
        sd = _struct(name, False)
        s = sd[0]
        X = fc.random_values(rng, (s.ncols, D))
        Xd = _t(X)
        out, again = Guarded(s.rows, D), Guarded(s.rows, D)
        assert _spmm(sd, D, Xd, out.view) == 0 and _spmm(sd, D, Xd, again.view) == 0, _last_error()
        _within(f"nm_spmm_csr, random data, {name}", f"D={D}", _np(out.view), fc.spmm_ref(s, X), fc.dot_bound(s, X, 1))
        _exact(f"nm_spmm_csr, random data, {name}", f"D={D}, second call vs first", _np(again.view), _np(out.view))
        assert out.intact() and again.intact()


def test_spmm_degenerate_calls():
    L = _L()
    sd = _struct("lane_r17")
    s, rowptr, col, val = sd
    X = _t(fc.exact_values(np.random.default_rng(0), (s.ncols, 3)))
    out = Guarded(s.rows, 3)
    st = L.stream_ptr(dev())
    assert L.lib().nm_spmm_csr(0, 3, None, None, None, None, None, st) == 0                     # no rows: nothing to do
    assert L.lib().nm_spmm_csr(s.rows, 0, L.ptr(rowptr), L.ptr(col), L.ptr(val), L.ptr(X), L.ptr(out.view), st) != 0
    assert "bad shape" in _last_error()
    assert L.lib().nm_spmm_csr(-1, 3, L.ptr(rowptr), L.ptr(col), L.ptr(val), L.ptr(X), L.ptr(out.view), st) != 0
    for hole in range(5):
        args = [L.ptr(rowptr), L.ptr(col), L.ptr(val), L.ptr(X), L.ptr(out.view)]
        args[hole] = None
        assert L.lib().nm_spmm_csr(s.rows, 3, *args, st) != 0, hole
        assert "null pointer" in _last_error()
    torch.cuda.synchronize()
    assert bool((out.buf == SENT).all())                                                        # a refused call writes nothing


@pytest.mark.parametrize("name", ["lane_r17", "lane_r257", "bind_k255"])
def test_tune_spmm_wrappers_and_transposed_gradient(name):
    """tune.spmm / compute_bindings_xyz / compute_bindings_F on Bindings built from raw triples: a non-contiguous X, an fp64 X,
    and the gradient through the transposed CSR for D = 3 and D = 9 against fp64 B^T g - with the structure as B (the forward
    product walks the chosen rows) and as B^T (the gradient does).  Exact data: bit-equal."""
    from neuma_amd.tune import spmm, compute_bindings_xyz, compute_bindings_F
    s = _struct(name)[0]
    rng = np.random.default_rng(13)
    for transposed in (False, True):
        A = fc.transpose(s) if transposed else s                # the matrix the Bindings stand for
        b = _bindings_of(s, transposed)
        assert (b.K, b.N) == (A.rows, A.ncols)
        case = f"tune.spmm, exact data, {name}{'^T' if transposed else ''}"
        for D in (3, 9):
            X = fc.exact_values(rng, (A.ncols, D)); G = fc.exact_values(rng, (A.rows, D))
            assert fc.spmm_margin(A) < fc.EXACT_LIMIT and fc.spmm_margin(fc.transpose(A)) < fc.EXACT_LIMIT
            wide = torch.zeros(A.ncols, 2 * D, device=dev())
            wide[:, ::2] = _t(X)
            forms = {"contiguous": _t(X), "non-contiguous": wide[:, ::2], "fp64": _t(X).double()}
            assert not forms["non-contiguous"].is_contiguous()
            for form, Xd in forms.items():
                Xd = Xd.clone().requires_grad_(True) if form != "non-contiguous" else Xd.requires_grad_(True)
                Y = spmm(b, Xd)
                assert Y.dtype == torch.float32 and Y.shape == (A.rows, D)
                _exact(case, f"D={D}, {form} X", _np(Y), fc.spmm_ref(A, X))
                (gX,) = torch.autograd.grad(Y, Xd, _t(G))
                assert gX.shape == Xd.shape
                _exact(case, f"D={D}, {form} X: gradient B^T g", _np(gX.float()), fc.spmm_t_ref(A, G))
        pc, pp, kp = fc.exact_values(rng, (A.ncols, 3)), fc.exact_values(rng, (A.ncols, 3)), fc.exact_values(rng, (A.rows, 3))
        assert fc.bind_frame_margins(A)[0] < fc.EXACT_LIMIT
        pcd = _t(pc).requires_grad_(True)
        k = compute_bindings_xyz(pcd, _t(pp), _t(kp), b)
        _exact(case, "compute_bindings_xyz", _np(k), kp.astype(np.float64) + fc.spmm_ref(A, pc.astype(np.float64) - pp))
        G = fc.exact_values(rng, (A.rows, 3))
        (gp,) = torch.autograd.grad(k, pcd, _t(G))
        _exact(case, "compute_bindings_xyz: dL/dp_curr", _np(gp), fc.spmm_t_ref(A, G))
        F = fc.exact_F(rng, (A.ncols, 3, 3))
        Fk = compute_bindings_F(_t(F), b)
        assert Fk.shape == (A.rows, 3, 3)
        _exact(case, "compute_bindings_F", _np(Fk), fc.spmm_ref(A, F))


# ---------------------------------------------------------------- nm_spmm_csr_sum3
@pytest.mark.parametrize("name", LANE_NAMES)
def test_sum3_exact(name):
    """one to four inputs, scale 1 and 1/4: bit-equal to fp64 scale * A (in0 + ...), guard rows untouched"""
    sd = _struct(name)
    s = sd[0]
    rng = np.random.default_rng(21)
    for n_in in (1, 2, 3, 4):
        assert fc.sum3_margin(s, n_in) < fc.EXACT_LIMIT
        ins = [fc.exact_values(rng, (s.ncols, 3)) for _ in range(n_in)]
        dins = [_t(a) for a in ins] + [None] * (4 - n_in)
        for scale in (1.0, 0.25):
            out = Guarded(s.rows, 3, pad=7)
            assert _sum3(sd, dins, scale, out.view) == 0, _last_error()
            ref = scale * fc.spmm_ref(s, sum(a.astype(np.float64) for a in ins))
            _exact(f"nm_spmm_csr_sum3, exact data, {name}", f"{n_in} inputs, scale {scale}", _np(out.view), ref)
            assert out.intact()


def test_sum3_random_within_derived_bound():
    """c = 5: up to three additions of the inputs (3), the product (1), at most L - 1 partial sums, the scale (1) - L + 4
    roundings per term, and 1 for the second order.  sum_j |in_j| stands for |x| and |scale| in front.  scale = fl32(1/3)."""
    rng = np.random.default_rng(22)
    scale = float(np.float32(1.0 / 3.0))
    for name in LANE_NAMES:
        sd = _struct(name, False)
        s = sd[0]
        for n_in in (1, 2, 3, 4):
            ins = [fc.random_values(rng, (s.ncols, 3)) for _ in range(n_in)]
            out = Guarded(s.rows, 3)
            assert _sum3(sd, [_t(a) for a in ins] + [None] * (4 - n_in), scale, out.view) == 0, _last_error()
            ref = scale * fc.spmm_ref(s, sum(a.astype(np.float64) for a in ins))
            bound = abs(scale) * fc.dot_bound(s, sum(np.abs(a.astype(np.float64)) for a in ins), 5)
            _within(f"nm_spmm_csr_sum3, random data, {name}", f"{n_in} inputs, scale 1/3", _np(out.view), ref, bound)
            assert out.intact()


def test_sum3_refuses_inputs_out_of_order():
    sd = _struct("lane_r17")
    s = sd[0]
    a = _t(fc.exact_values(np.random.default_rng(0), (s.ncols, 3)))
    out = Guarded(s.rows, 3)
    assert _sum3(sd, [a, a, None, a], 1.0, out.view) != 0 and "in3 without in2" in _last_error()
    assert _sum3(sd, [a, None, a, None], 1.0, out.view) != 0 and "in2 without in1" in _last_error()
    assert _sum3(sd, [None, None, None, None], 1.0, out.view) != 0 and "null pointer" in _last_error()
    L = _L()
    assert L.lib().nm_spmm_csr_sum3(0, None, None, None, None, None, None, None, 1.0, None, L.stream_ptr(dev())) == 0
    torch.cuda.synchronize()
    assert bool((out.buf == SENT).all())


@pytest.mark.parametrize("n_outs", [1, 2, 4, 5, 6])
def test_tail_backward_single_launch_and_add_then_launch(n_outs):
    """harness._tail_backward with the jobs' dL/dmeans3D given (outs=): up to four go into ONE nm_spmm_csr_sum3 launch, more are
    added first and launched as one input.  Both equal fp64 scale * B^T sum, bit for bit on exact data."""
    from neuma_amd.harness import _tail_backward
    rng = np.random.default_rng(23 + n_outs)
    for name in ("lane_r17", "lane_r257"):
        s = _struct(name)[0]
        b = _bindings_of(s, transposed=True)                    # B = structure^T: B^T walks the structure's rows
        rt = types.SimpleNamespace(bindings=b, world=1, group=None, device=dev())
        assert fc.sum3_margin(s, n_outs) < fc.EXACT_LIMIT
        outs = [fc.exact_values(rng, (b.K, 3)) for _ in range(n_outs)]
        for scale in (1.0, 0.25):
            dx = Guarded(b.N, 3)
            _tail_backward(rt, None, None, None, dx.view, outs=[_t(a).clone() for a in outs], scale=scale)
            ref = scale * fc.spmm_ref(s, sum(a.astype(np.float64) for a in outs))
            _exact(f"harness._tail_backward, exact data, {name}", f"{n_outs} jobs, scale {scale}", _np(dx.view), ref)
            assert dx.intact()


# ---------------------------------------------------------------- nm_bind_frame
def _bind_inputs(s, exact, seed):
    rng = np.random.default_rng(seed)
    val, Fv = (fc.exact_values, fc.exact_F) if exact else (fc.random_values, fc.random_values)
    return dict(pc=val(rng, (s.ncols, 3)), pp=val(rng, (s.ncols, 3)), kp=val(rng, (s.rows, 3)), F=Fv(rng, (s.ncols, 9)),
                cov6=val(rng, (s.rows, 6)))


def _bind_full(sd, d):
    s = sd[0]
    means, cov, Fo = Guarded(s.rows, 3), Guarded(s.rows, 6), Guarded(s.rows, 9)
    dd = {k: _t(v) for k, v in d.items()}
    assert _bind_frame(sd, dd["pc"], dd["pp"], dd["kp"], dd["F"], dd["cov6"], means.view, cov.view, Fo.view) == 0, _last_error()
    return dd, means, cov, Fo


@pytest.mark.parametrize("name", BIND_NAMES + ["lane_r17"])
def test_bind_frame_exact(name):
    """means and F_k bit-equal to fp64 on every structure and k; an empty row gives exactly k_prev and a zero F_k; the covariance
    within 8 2^-24 |F_k| |S| |F_k|^T of the fp64 push of the kernel's OWN F_k; the calls with optional outputs left out (F = None
    is the form mesh driving uses) give the same bits for what they do produce; nm_spmm_csr gives the same bits."""
    sd = _struct(name)
    s = sd[0]
    case = f"nm_bind_frame, exact data, {name}"
    m_means, m_F = fc.bind_frame_margins(s)
    assert m_means < fc.EXACT_LIMIT and m_F < fc.EXACT_LIMIT
    d = _bind_inputs(s, True, 31)
    dd, means, cov, Fo = _bind_full(sd, d)
    means_ref = d["kp"].astype(np.float64) + fc.spmm_ref(s, d["pc"].astype(np.float64) - d["pp"])
    F_ref = fc.spmm_ref(s, d["F"])
    _exact(case, "means3D", _np(means.view), means_ref)
    _exact(case, "F_k", _np(Fo.view), F_ref)
    empty = s.lengths == 0
    if empty.any():
        _exact(case, "means3D of empty rows == k_prev", _np(means.view)[empty], d["kp"][empty])
        _exact(case, "F_k of empty rows == 0", _np(Fo.view)[empty], np.zeros((int(empty.sum()), 9)))
    cref, cbound = fc.cov_push_ref(d["cov6"], _np(Fo.view))
    _within(case, "cov3D vs fp64 push of the kernel's F_k", _np(cov.view), cref, cbound)
    assert means.intact() and cov.intact() and Fo.intact()
    # optional outputs
    m2 = Guarded(s.rows, 3)
    assert _bind_frame(sd, dd["pc"], dd["pp"], dd["kp"], None, None, m2.view, None, None) == 0, _last_error()
    _exact(case, "F = None: means3D vs the full call", _np(m2.view), _np(means.view))
    m3, F3 = Guarded(s.rows, 3), Guarded(s.rows, 9)
    assert _bind_frame(sd, dd["pc"], dd["pp"], dd["kp"], dd["F"], dd["cov6"], m3.view, None, F3.view) == 0, _last_error()
    _exact(case, "cov6_out = None: means3D vs the full call", _np(m3.view), _np(means.view))
    _exact(case, "cov6_out = None: F_k vs the full call", _np(F3.view), _np(Fo.view))
    m4, c4 = Guarded(s.rows, 3), Guarded(s.rows, 6)
    assert _bind_frame(sd, dd["pc"], dd["pp"], dd["kp"], dd["F"], dd["cov6"], m4.view, c4.view, None) == 0, _last_error()
    _exact(case, "F_out = None: means3D vs the full call", _np(m4.view), _np(means.view))
    _exact(case, "F_out = None: cov3D vs the full call", _np(c4.view), _np(cov.view))
    assert m2.intact() and m3.intact() and F3.intact() and m4.intact() and c4.intact()
    # the autograd form of the same products
    o3, o9 = Guarded(s.rows, 3), Guarded(s.rows, 9)
    assert _spmm(sd, 3, dd["pc"] - dd["pp"], o3.view) == 0 and _spmm(sd, 9, dd["F"], o9.view) == 0, _last_error()
    _exact(case, "means3D vs k_prev + nm_spmm_csr (D=3)", _np(means.view), _np(dd["kp"] + o3.view))
    _exact(case, "F_k vs nm_spmm_csr (D=9)", _np(Fo.view), _np(o9.view))


@pytest.mark.parametrize("name", BIND_NAMES)
def test_bind_frame_random_within_derived_bounds(name):
    """means: c = 3 - the difference p_cur - p_prev (1), the product (1; none where contracted), at most L - 1 partial sums, the
    final k_prev + d (1): L + 2 per term, and 1 for the second order; |k_prev| joins the sum because the last addition rounds
    relative to the result.  F_k: c = 1, as nm_spmm_csr.  Covariance: against the fp64 push of the kernel's own F_k."""
    sd = _struct(name, False)
    s = sd[0]
    case = f"nm_bind_frame, random data, {name}"
    d = _bind_inputs(s, False, 32)
    dd, means, cov, Fo = _bind_full(sd, d)
    dp = d["pc"].astype(np.float64) - d["pp"]
    _within(case, "means3D", _np(means.view), d["kp"] + fc.spmm_ref(s, dp), fc.dot_bound(s, dp, 3, extra=np.abs(d["kp"].astype(np.float64))))
    _within(case, "F_k", _np(Fo.view), fc.spmm_ref(s, d["F"]), fc.dot_bound(s, d["F"], 1))
    cref, cbound = fc.cov_push_ref(d["cov6"], _np(Fo.view))
    _within(case, "cov3D vs fp64 push of the kernel's F_k", _np(cov.view), cref, cbound)
    assert means.intact() and cov.intact() and Fo.intact()


def test_bind_frame_refuses_a_covariance_without_F():
    sd = _struct("bind_k255")
    s = sd[0]
    dd = {k: _t(v) for k, v in _bind_inputs(s, True, 33).items()}
    means, cov = Guarded(s.rows, 3), Guarded(s.rows, 6)
    assert _bind_frame(sd, dd["pc"], dd["pp"], dd["kp"], None, dd["cov6"], means.view, cov.view, None) != 0
    assert "cov6_out needs F" in _last_error()
    assert _bind_frame(sd, dd["pc"], dd["pp"], dd["kp"], dd["F"], None, means.view, cov.view, None) != 0
    assert _bind_frame(sd, dd["pc"], dd["pp"], None, dd["F"], dd["cov6"], means.view, cov.view, None) != 0
    assert "null pointer" in _last_error()
    torch.cuda.synchronize()
    assert bool((means.buf == SENT).all()) and bool((cov.buf == SENT).all())


# ---------------------------------------------------------------- nm_cov_deform
@pytest.mark.parametrize("k", fc.BIND_K)
def test_cov_deform_within_elementwise_bound(k):
    """F S F^T against fp64 of the kernel's own inputs, |err| <= 8 2^-24 (|F| |S| |F|^T) elementwise: random and exact data"""
    L = _L()
    rng = np.random.default_rng(40 + k)
    for kind, cov6, F in (("random", fc.random_values(rng, (k, 6)), fc.random_values(rng, (k, 9))),
                          ("exact", fc.exact_values(rng, (k, 6)), fc.exact_F(rng, (k, 9)))):
        out = Guarded(k, 6)
        assert L.lib().nm_cov_deform(k, L.ptr(_t(cov6)), L.ptr(_t(F)), L.ptr(out.view), L.stream_ptr(dev())) == 0, _last_error()
        ref, bound = fc.cov_push_ref(cov6, F)
        _within(f"nm_cov_deform, {kind} data", f"k={k}", _np(out.view), ref, bound)
        assert out.intact()


# ---------------------------------------------------------------- nm_pixel_loss
def _pixel(kind, weight, h, w, img, gt, grad, row0=0, row1=0, prior=0.0):
    L = _L()
    loss = torch.full((1,), prior, dtype=torch.float32, device=dev())
    rc = L.lib().nm_pixel_loss(kind, float(weight), h, w, row0, row1, L.ptr(img), L.ptr(gt), L.ptr(loss), L.ptr(grad), L.stream_ptr(dev()))
    assert rc == 0, _last_error()
    return _np(loss)


def _misaligned(t):
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=dev())
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


@pytest.mark.parametrize("hw", list(fc.PIXEL_SHAPES), ids=PIXEL_IDS)
@pytest.mark.parametrize("kind", [0, 1], ids=["l1", "l2"])
def test_pixel_loss_exact(kind, hw):
    """Exact data, weight / (3 h w) a power of two.  The loss word is bit-equal to (exact sum) * scale - which also holds the
    restated launch rule's scale to the kernel's - and the gradient to the fp32 expression the kernel states; stripes partition
    the loss and the gradient; row1 <= row0 is the whole image; a null gradient changes nothing; the loss word accumulates;
    pointers one float off 16-byte alignment (the scalar branch on a w % 4 == 0 image) give the same bits."""
    h, w = hw
    case = f"nm_pixel_loss, exact data, {'l1' if kind == 0 else 'l2'}, {h}x{w}"
    weight, scale = fc.pow2_weight(h, w)
    assert fc.pixel_margin(h, w) < fc.EXACT_LIMIT and float(fc.fp32_scale(weight, h, w)) == scale
    a, g = fc.pixel_images(h, w, kind, exact=True)
    ad, gd = _t(a), _t(g)
    assert ad.data_ptr() % 16 == 0 and gd.data_ptr() % 16 == 0
    total = fc.pixel_term_sum(kind, a, g)
    grad = Guarded(3 * h, w)
    assert grad.view.data_ptr() % 16 == 0
    loss = _pixel(kind, weight, h, w, ad, gd, grad.view)
    _exact(case, "loss", loss, [total * scale])
    gref = fc.pixel_grad_fp32(kind, scale, a, g)
    _exact(case, "dL/dimage", _np(grad.view).reshape(3, h, w), gref)
    assert grad.intact()
    _exact(case, "loss, null gradient", _pixel(kind, weight, h, w, ad, gd, None), [total * scale])
    for r0, r1, what in ((2, 2, "row1 == row0"), (h, 1, "row1 < row0")):
        g2 = Guarded(3 * h, w)
        _exact(case, f"loss, {what}: the whole image", _pixel(kind, weight, h, w, ad, gd, g2.view, r0, r1), [total * scale])
        _exact(case, f"dL/dimage, {what}: the whole image", _np(g2.view).reshape(3, h, w), gref)
        assert g2.intact()
    prior = 0.125                                               # a multiple of the granularity scale / 256; the sum stays exact
    assert (prior + total * scale) / (scale / 256.0) < fc.EXACT_LIMIT
    _exact(case, "loss accumulated onto 1/8", _pixel(kind, weight, h, w, ad, gd, None, prior=prior), [prior + total * scale])
    # stripes
    cuts = sorted({0, 1, h // 3, h // 2 + 1, h})
    loss_sum, grad_sum = 0.0, np.zeros((3, h, w), dtype=np.float32)
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        gs = Guarded(3 * h, w)
        ls = _pixel(kind, weight, h, w, ad, gd, gs.view, r0, r1)
        _exact(case, "stripe loss", ls, [fc.pixel_term_sum(kind, a, g, r0, r1) * scale])
        gsn = _np(gs.view).reshape(3, h, w)
        _exact(case, "stripe dL/dimage (zero outside the stripe)", gsn, fc.pixel_grad_fp32(kind, scale, a, g, r0, r1))
        assert gs.intact()
        loss_sum += float(ls[0]); grad_sum += gsn
    _exact(case, "stripe losses add to the full loss", [loss_sum], loss)
    _exact(case, "stripe gradients add to the full gradient", grad_sum, gref)
    # one float off alignment: the scalar branch must give the float4 branch's bits
    if w % 4 == 0:
        for which in ("img", "gt", "grad"):
            gm = Guarded(3 * h, w, shift=1 if which == "grad" else 0)
            assert gm.view.data_ptr() % 16 == (4 if which == "grad" else 0)
            lm = _pixel(kind, weight, h, w, _misaligned(ad) if which == "img" else ad, _misaligned(gd) if which == "gt" else gd, gm.view)
            _exact(case, f"loss, misaligned {which}", lm, [total * scale])
            _exact(case, f"dL/dimage, misaligned {which}", _np(gm.view).reshape(3, h, w), gref)
            assert gm.intact()


@pytest.mark.parametrize("hw", list(fc.PIXEL_SHAPES), ids=PIXEL_IDS)
@pytest.mark.parametrize("kind", [0, 1], ids=["l1", "l2"])
def test_pixel_loss_random(kind, hw):
    """Random images, weight 0.7, against the fp64 mean.  Loss: relative error <= (T + G + 8) 2^-24 with T = terms a thread
    accumulates and G = workgroups, both from the launch rule restated in frame_tail_cases.launch_rule (checked against the
    listed paths on the CPU, its scale against the kernel's in test_pixel_loss_exact).  All terms are positive, so the bound is
    relative to the loss: a term passes at most T roundings in its thread's sum (the difference and the T - 1 additions; 2 more
    for the square of L2), 6 + 3 in the wave and workgroup sums, 1 for the scale, 1 for the division that made the scale and at
    most G - 1 atomic additions: T + G + 10 (L1) or T + G + 12 (L2) in the worst case.  The 8 the test holds is the tighter,
    stated figure - the roundings of a sum of positive terms do not all fall one way.  Gradient: bit-equal to the fp32
    expression with the kernel's fp32 scale."""
    h, w = hw
    case = f"nm_pixel_loss, random data, {'l1' if kind == 0 else 'l2'}, {h}x{w}"
    weight = 0.7
    a, g = fc.pixel_images(h, w, kind, exact=False)
    grad = Guarded(3 * h, w)
    loss = _pixel(kind, weight, h, w, _t(a), _t(g), grad.view)
    rule = fc.launch_rule(h, w)
    ref = fc.pixel_loss_ref(kind, weight, a, g)
    bound = (rule["terms_per_thread"] + rule["grid"] + 8) * fc.U
    parity(case, "loss: relative error vs fp64", abs(float(loss[0]) - ref) / ref, bound)
    _exact(case, "dL/dimage vs its fp32 expression", _np(grad.view).reshape(3, h, w),
           fc.pixel_grad_fp32(kind, fc.fp32_scale(weight, h, w), a, g))
    assert grad.intact()


@pytest.mark.parametrize("hw", [(37, 53), (16, 64)], ids=["37x53", "16x64"])
def test_tune_pixel_losses(hw):
    """tune.l1_loss / l2_loss / pixel_loss_rows: the value within the random-data bound, the autograd gradient (times the
    incoming 2.0, exact) bit-equal to the fp32 expression; an input that does not require grad gives the same value."""
    from neuma_amd.tune import l1_loss, l2_loss, pixel_loss_rows
    h, w = hw
    rule = fc.launch_rule(h, w)
    bound = (rule["terms_per_thread"] + rule["grid"] + 8) * fc.U
    scale = fc.fp32_scale(1.0, h, w)
    for kind, fn in ((0, l1_loss), (1, l2_loss)):
        case = f"tune.{fn.__name__}, random data, {h}x{w}"
        a, g = fc.pixel_images(h, w, kind, exact=False, seed=5)
        ref = fc.pixel_loss_ref(kind, 1.0, a, g)
        ad = _t(a).requires_grad_(True)
        loss = fn(ad, _t(g))
        assert loss.shape == () and loss.dtype == torch.float32
        parity(case, "value: relative error vs fp64", abs(float(loss.detach()) - ref) / ref, bound)
        (ga,) = torch.autograd.grad(2.0 * loss, ad)
        _exact(case, "autograd gradient", _np(ga), 2.0 * fc.pixel_grad_fp32(kind, scale, a, g).astype(np.float64))
        plain = fn(_t(a), _t(g))
        assert not plain.requires_grad
        parity(case, "value, input without grad", abs(float(plain) - ref) / ref, bound)
        r0, r1 = h // 3, h // 3 + 5
        ad2 = _t(a).requires_grad_(True)
        part = pixel_loss_rows(ad2, _t(g), kind, r0, r1)
        pref = fc.pixel_loss_ref(kind, 1.0, a, g, r0, r1)
        parity(case, "pixel_loss_rows, five rows: relative error vs fp64", abs(float(part.detach()) - pref) / pref, bound)
        (gp,) = torch.autograd.grad(part, ad2)
        _exact(case, "pixel_loss_rows: autograd gradient", _np(gp), fc.pixel_grad_fp32(kind, scale, a, g, r0, r1))
        whole = pixel_loss_rows(_t(a), _t(g), kind)
        parity(case, "pixel_loss_rows, all rows: relative error vs fp64", abs(float(whole) - ref) / ref, bound)
