"""CPU: the fp64 statement of LPIPS (neuma_amd/extras/lpips.py) against hand-written numpy loops, its exact zero, the
non-degeneracy of the seeded random weights the GPU tests use, the weight loader and the entry point's flag rule."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import lpips_cases as lc  # noqa: E402

from neuma_amd.extras import lpips as twin  # noqa: E402


def test_twin_convolution_against_a_numpy_loop():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(1, 3, 5, 4, generator=g, dtype=torch.float64)
    w = torch.randn(2, 3, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(2, generator=g, dtype=torch.float64)
    got = twin.conv3x3_relu(x, w, b)[0].numpy()
    want = lc.np_conv3x3_relu(x[0].numpy(), w.numpy(), b.numpy())
    assert (want == 0).any() and (want > 0).any()
    assert np.abs(got - want).max() <= 1e-13


def test_twin_pool_drops_an_odd_last_row_and_column():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(1, 2, 5, 7, generator=g, dtype=torch.float64)
    got = twin.maxpool2(x)[0].numpy()
    assert got.shape == (2, 2, 3)
    assert np.array_equal(got, lc.np_maxpool2(x[0].numpy()))


def test_twin_head_against_a_numpy_loop():
    g = torch.Generator().manual_seed(3)
    ta = lc.post_relu_like((1, 4, 3, 2), g)
    tb = lc.post_relu_like((1, 4, 3, 2), g)
    ta[0, :, 0, 0] = 0          # one vector all zero, then both
    ta[0, :, 1, 1] = 0
    tb[0, :, 1, 1] = 0
    w = torch.rand(4, generator=g)
    got = float(twin.head(ta, tb, w)[0])
    want = lc.np_head(ta[0].numpy(), tb[0].numpy(), w.numpy())
    assert want > 0 and abs(got - want) <= 1e-14 * want


def test_scaling_constants():
    x = torch.tensor([0.0, 0.5, 1.0], dtype=torch.float64).view(1, 1, 3, 1).expand(1, 3, 3, 1)
    y = twin.scale_input(x)
    for c, (sh, sc) in enumerate(zip((-0.030, -0.088, -0.188), (0.458, 0.448, 0.450))):
        want = [(2 * v - 1 - sh) / sc for v in (0.0, 0.5, 1.0)]
        assert np.allclose(y[0, c, :, 0].numpy(), want, rtol=1e-15, atol=0)


def test_identical_images_give_exactly_zero():
    convs, heads = lc.weights()
    a, _ = lc.images(16, 16)
    assert torch.equal(twin.lpips(a, a, convs, heads), torch.zeros(2, dtype=torch.float64))


@pytest.mark.parametrize("h,w", lc.CHAIN_SHAPES)
def test_random_weights_are_not_degenerate(h, w):
    """the GPU chain test means something only if every tap carries signal: values of the size real LPIPS takes, taps about half
    zeros, and every tap contributing at least 1.9e-3 (the smallest is relu5_3 at 16 x 16)"""
    terms = lc.twin_terms(h, w)
    v = terms.sum(0)
    assert terms.shape == (5, 2)
    assert float(v.min()) > 0.10 and float(v.max()) < 0.15, v
    assert float(terms.min()) >= 1.9e-3, terms
    convs, _ = lc.weights()
    a, _ = lc.images(h, w)
    for t in twin.features(a, convs):
        zeros = float((t == 0).double().mean())
        assert 0.25 < zeros < 0.75, zeros


def test_features_refuse_small_images():
    convs, _ = lc.weights()
    with pytest.raises(ValueError, match="16"):
        twin.features(torch.zeros(1, 3, 15, 16), convs)


# ------------------------------------------------------------------ weight loader

def _save(tmp_path, vgg, hd):
    pv, ph = tmp_path / "vgg16.pth", tmp_path / "vgg.pth"
    torch.save(vgg, pv)
    torch.save(hd, ph)
    return pv, ph


def test_loader_reads_good_files_and_the_nested_state_dict(tmp_path):
    from neuma_amd.lpips import load_weights, pack_conv_weight
    convs, heads = lc.weights()
    vgg, hd = lc.state_dicts()
    pv, ph = _save(tmp_path, vgg, hd)
    w = load_weights(pv, ph, "cpu")
    assert len(w.convs) == 13 and len(w.heads) == 5 and w.files == (str(pv), str(ph))
    for (a, b), (c, d) in zip(w.convs, convs):
        assert torch.equal(a, c) and torch.equal(b, d)
    for a, c in zip(w.heads, heads):
        assert torch.equal(a, c)
    # nested under 'state_dict', and the heads under the fall-back key
    torch.save({"state_dict": vgg, "epoch": 3}, pv)
    torch.save({k.replace("model.1", "model.0"): v for k, v in hd.items()}, ph)
    w2 = load_weights(pv, ph, "cpu")
    assert all(torch.equal(a[0], c[0]) for a, c in zip(w2.convs, convs)) and torch.equal(w2.heads[4], heads[4])
    # the packed layouts: [o][tap][c] for cin = 3, [chunk][o][tap][c] otherwise
    p0, p1 = pack_conv_weight(convs[0][0]), pack_conv_weight(convs[1][0])
    assert p0.shape == (64, 9, 3) and p1.shape == (4, 64, 9, 16)
    assert p0[5, 7, 2] == convs[0][0][5, 2, 2, 1] and p1[3, 9, 5, 11] == convs[1][0][9, 59, 1, 2]


def test_loader_names_a_wrong_shape_and_a_missing_key(tmp_path):
    from neuma_amd.lpips import load_weights
    vgg, hd = lc.state_dicts()
    bad = dict(vgg)
    bad["features.7.weight"] = torch.zeros(128, 64, 3, 3)
    pv, ph = _save(tmp_path, bad, hd)
    with pytest.raises(ValueError, match=r"features\.7\.weight"):
        load_weights(pv, ph, "cpu")
    bad = dict(vgg)
    del bad["features.28.bias"]
    pv, ph = _save(tmp_path, bad, hd)
    with pytest.raises(KeyError, match=r"features\.28\.bias"):
        load_weights(pv, ph, "cpu")
    badh = dict(hd)
    badh["lin2.model.1.weight"] = torch.zeros(1, 128, 1, 1)
    pv, ph = _save(tmp_path, vgg, badh)
    with pytest.raises(ValueError, match=r"lin2\.model\.1\.weight"):
        load_weights(pv, ph, "cpu")
    badh = dict(hd)
    del badh["lin4.model.1.weight"]
    pv, ph = _save(tmp_path, vgg, badh)
    with pytest.raises(KeyError, match=r"lin4\.model\.1\.weight"):
        load_weights(pv, ph, "cpu")


def test_cpu_weights_and_cpu_images_are_refused_by_the_native_path(tmp_path):
    from neuma_amd import NeumaHipError
    from neuma_amd.lpips import LpipsWeights, lpips
    convs, heads = lc.weights()
    w = LpipsWeights(convs, heads, "cpu")
    a, b = lc.images(16, 16)
    with pytest.raises(NeumaHipError):
        lpips(a, b, w)


def test_library_refuses_small_images_before_any_device_work():
    """host-only: the workspace size is 0 for sizes nm_lpips refuses, and the call names the reason without touching a device"""
    from neuma_amd import _lib as L
    lib = L.lib()
    assert lib.nm_lpips_workspace(1, 15, 16) == 0 and lib.nm_lpips_workspace(1, 16, 15) == 0 and lib.nm_lpips_workspace(0, 16, 16) == 0
    one, two = int(lib.nm_lpips_workspace(1, 16, 16)), int(lib.nm_lpips_workspace(2, 16, 16))
    assert one >= 2 * 2 * 16 * 16 * 64 * 4 and two > one and one % 256 == 0
    assert lib.nm_lpips(1, 15, 16, None, None, None, None, None, None, 0, None) == -1
    assert b"at least 16" in lib.nm_last_error()
    assert lib.nm_lpips(1, 16, 16, None, None, None, None, None, None, 0, None) == -1
    assert b"null pointer" in lib.nm_last_error()
    assert lib.nm_conv3x3_relu(1, 64, 32, 4, 4, None, None, None, None, None) == -1
    assert b"cout" in lib.nm_last_error()
    assert lib.nm_maxpool2(1, 6, 4, 4, None, None, None) == -1
    assert b"multiple of 4" in lib.nm_last_error()
    assert lib.nm_lpips_head_workspace(2, 4, 4) >= 16 and lib.nm_lpips_head_workspace(0, 4, 4) == 0


# ------------------------------------------------------------------ flags

def test_flags_both_or_neither(capsys):
    from neuma_amd.evaluation import parse_args
    base = ["-p", "x", "-g", "y", "--view", "0"]
    a = parse_args(base)
    assert a.lpips_vgg is None and a.lpips_heads is None
    a = parse_args(base + ["--lpips_vgg", "v.pth", "--lpips_heads", "h.pth"])
    assert (a.lpips_vgg, a.lpips_heads) == ("v.pth", "h.pth")
    with pytest.raises(SystemExit) as e:
        parse_args(base + ["--lpips_vgg", "v.pth"])
    assert e.value.code != 0 and "without --lpips_heads" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        parse_args(base + ["--lpips_heads", "h.pth"])
    assert e.value.code != 0 and "without --lpips_vgg" in capsys.readouterr().err
