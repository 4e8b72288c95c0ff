"""CPU: the torch composition of the particle-state loss against a numpy fp64 statement of its definition, and the presence of
the native entry point in the header and the ctypes table (as tests/test_lib_abi.py checks the others)."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent


def reference(x, v, xg, vg, mask, kind, wx, wv):
    """numpy fp64: (loss, term_x, term_v, dL_dx, dL_dv) of nm_state_loss's definition (include/neuma_hip.h)"""
    n = x.shape[0]
    keep = np.ones(n, bool) if mask is None else (np.asarray(mask) != 0)
    m = int(keep.sum())

    def term(a, b, w):
        d = a.astype(np.float64) - b.astype(np.float64)
        if m == 0:
            return 0.0, np.zeros_like(d)
        e = np.abs(d) if kind == "l1" else d * d
        g = np.sign(d) if kind == "l1" else 2.0 * d
        return float(e[keep].sum() / (3.0 * m)), np.where(keep[:, None], float(w) * g / (3.0 * m), 0.0)

    tx, gx = term(x, xg, wx)
    tv, gv = term(v, vg, wv) if vg is not None else (0.0, np.zeros((n, 3)))
    return float(wx) * tx + (float(wv) * tv if vg is not None else 0.0), tx, tv, gx, gv


def masks(n, rng):
    single = np.zeros(n, np.uint8)
    single[n // 2] = 1
    return {"none": None, "random": (rng.random(n) < 0.6).astype(np.uint8), "all-zero": np.zeros(n, np.uint8), "single": single}


@pytest.mark.parametrize("kind", ["l1", "l2"])
@pytest.mark.parametrize("with_v", [False, True])
@pytest.mark.parametrize("mask_name", ["none", "random", "all-zero", "single"])
def test_torch_composition_equals_the_definition(kind, with_v, mask_name):
    from neuma_amd.state_loss import state_loss_torch
    rng = np.random.default_rng(3)
    n = 37
    x, v, xg, vg = (rng.standard_normal((n, 3)) for _ in range(4))
    x[5] = xg[5]                                            # an exact zero difference: sign gives 0
    mask = masks(n, rng)[mask_name]
    tx_, tv_ = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (x, v))
    loss = state_loss_torch(tx_, tv_, torch.tensor(xg), torch.tensor(vg) if with_v else None,
                            None if mask is None else torch.tensor(mask), kind=kind, weight_x=0.7, weight_v=1.9)
    ref, _, _, gx, gv = reference(x, v, xg, vg if with_v else None, mask, kind, 0.7, 1.9)
    assert abs(float(loss) - ref) <= 1e-14 * max(abs(ref), 1.0)
    if loss.requires_grad:
        loss.backward()
    got_x = np.zeros((n, 3)) if tx_.grad is None else tx_.grad.numpy()
    got_v = np.zeros((n, 3)) if tv_.grad is None else tv_.grad.numpy()
    assert np.abs(got_x - gx).max() <= 1e-15
    assert np.abs(got_v - gv).max() <= 1e-15
    if mask_name == "all-zero":
        assert float(loss) == 0.0


def test_unknown_kind_raises():
    from neuma_amd.state_loss import state_loss_torch
    with pytest.raises(ValueError):
        state_loss_torch(torch.zeros(2, 3), None, torch.zeros(2, 3), kind="huber")


def test_cpu_tensor_is_rejected_by_the_native_operator():
    from neuma_amd import NeumaHipError
    from neuma_amd.state_loss import state_loss
    with pytest.raises(NeumaHipError):
        state_loss(torch.zeros(2, 3), torch.zeros(2, 3), torch.zeros(2, 3), torch.zeros(2, 3))


def test_entry_point_is_declared_exported_and_in_the_ctypes_table():
    from neuma_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "neuma_hip.h").read_text(), flags=re.S)
    lib = _lib.lib()
    for name in ("nm_state_loss_workspace", "nm_state_loss"):
        m = re.search(r"\b" + name + r"\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
        assert m, f"{name} is not declared in neuma_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == len(m.group(1).split(","))
    assert "nm_state.hip" in (ROOT / "neuma_amd" / "csrc" / "Makefile").read_text()
    # host-only behaviour: the workspace size, and the argument checks that come before any device work
    assert lib.nm_state_loss_workspace(1000) >= 2 * 8
    assert lib.nm_state_loss(0, 1, 1.0, 1.0, None, None, None, None, None, None, None, None, None, None, 0, None) == 0      # n == 0
    for args, word in (((4, 2, 1.0, 1.0, None, None, None, None, None, None, None, None, None, None, 0, None), b"kind"),
                       ((4, 1, 1.0, 1.0, None, None, None, None, None, None, None, None, None, None, 0, None), b"null pointer"),
                       ((4, 1, 1.0, 1.0, 16, None, 16, None, None, 16, None, None, None, 16, 8, None), b"workspace too small")):
        assert lib.nm_state_loss(*args) == -1
        assert word in lib.nm_last_error()
