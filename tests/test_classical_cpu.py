"""CPU-side checks of the classical constitutive laws (material/classical.py, csrc/nm_classical.hip): the reference's names
and state_dict layout, the `material.build` factory, and the C ABI's argument checks (no compute without a GPU)."""
import ctypes as C

import numpy as np
import pytest
import torch

NAMES = ["CorotatedElasticity", "StVKElasticity", "VolumeElasticity", "SigmaElasticity", "IdentityPlasticity", "SigmaPlasticity",
         "VonMisesPlasticity", "DruckerPragerPlasticity"]
# fixture -> (class, constructor keys besides `random`)
CASES = {"corotated": "CorotatedElasticity", "stvk": "StVKElasticity", "volume_ziran": "VolumeElasticity",
         "volume_taichi": "VolumeElasticity", "sigma": "SigmaElasticity", "identity": "IdentityPlasticity",
         "sigma_plastic": "SigmaPlasticity", "von_mises": "VonMisesPlasticity", "drucker_prager": "DruckerPragerPlasticity",
         "drucker_prager_cohesion": "DruckerPragerPlasticity"}
NET = dict(layer_widths=[64, 64], norm=None, nonlinearity="gelu", no_bias=True, normalize_input=True, alpha=1e-3)


def fixture_cfg(d, random=False):
    cfg = {k: float(d[k]) for k in ("E", "nu", "sigma_y", "friction_angle", "cohesion") if k in d.files}
    if "mode_id" in d.files:
        cfg["mode"] = ["ziran", "taichi"][int(d["mode_id"])]
    cfg["random"] = random
    return cfg


def test_the_eight_names_import_from_both_modules():
    import neuma_amd.material as m
    import neuma_amd.material.preset as p
    for n in NAMES:
        assert getattr(m, n) is getattr(p, n) and issubclass(getattr(m, n), torch.nn.Module)
    assert p.ComposeMaterial is m.ComposeMaterial


@pytest.mark.parametrize("tag", sorted(CASES))
def test_state_dict_matches_the_reference_modules(golden_dir, tag):
    import neuma_amd.material as m
    d = np.load(golden_dir / "classical" / f"{tag}.npz", allow_pickle=False)
    for prefix, random in (("state.", False), ("state_random.", True)):
        mod = getattr(m, CASES[tag])(fixture_cfg(d, random))
        sd = mod.state_dict()
        want = {k[len(prefix):]: d[k] for k in d.files if k.startswith(prefix)}
        assert sorted(sd) == sorted(want)
        for k, v in sd.items():
            assert tuple(v.shape) == want[k].shape and v.dtype == torch.float32
            assert np.array_equal(v.numpy(), want[k]), (k, random)          # cfg.random scales the learnable ones by 0.8
        assert sorted(n for n, _ in mod.named_parameters()) == sorted(k for k in want if k not in ("nu", "cohesion"))
        mod.load_state_dict({k: torch.tensor(v) for k, v in want.items()})        # a reference state_dict loads (strict)
    if "state.log_E" in d.files:
        assert np.allclose(d["state_random.log_E"], 0.8 * d["state.log_E"])


def test_build_defaults_to_the_neural_class_and_rejects_unknown_names():
    import neuma_amd.material as m
    assert type(m.build(NET)) is m.InvariantFullMetaElasticity
    assert type(m.build(NET, m.InvariantFullMetaPlasticity)) is m.InvariantFullMetaPlasticity
    assert type(m.build(dict(NET, name="InvariantFullMetaPlasticity"))) is m.InvariantFullMetaPlasticity
    assert type(m.build(dict(name="CorotatedElasticity", E=1e5, nu=0.3, random=False))) is m.CorotatedElasticity
    assert type(m.build(dict(name="IdentityPlasticity"))) is m.IdentityPlasticity
    with pytest.raises(ValueError, match="unknown constitutive law"):
        m.build(dict(NET, name="NeoHookeanElasticity"))
    with pytest.raises(ValueError, match="invalid mode"):
        m.VolumeElasticity(dict(E=1e5, nu=0.3, random=False, mode="bogus"))._mode()


def test_cpu_tensors_raise_and_identity_returns_its_input():
    import neuma_amd.material as m
    from neuma_amd import NeumaHipError
    F = torch.eye(3)[None].repeat(4, 1, 1)
    assert m.IdentityPlasticity(None)(F) is F
    for mod in (m.CorotatedElasticity(dict(E=1e5, nu=0.3, random=False)), m.SigmaPlasticity(None)):
        with pytest.raises(NeumaHipError):
            mod(F)


def test_abi_symbols_workspace_query_and_argument_checks():
    from neuma_amd import _lib
    for n in ("nm_classical_fwd", "nm_classical_bwd_workspace", "nm_classical_bwd"):
        assert n in _lib.SIGNATURES
    lib = _lib.lib()
    assert lib.nm_classical_bwd_workspace(0) == 0 and lib.nm_classical_bwd_workspace(-5) == 0
    assert lib.nm_classical_bwd_workspace(100000) >= 2 * 8 and lib.nm_classical_bwd_workspace(2 ** 31 - 1) <= 1 << 20
    p = C.c_void_p(64)              # never dereferenced: every call below fails its argument checks first
    assert lib.nm_classical_fwd(-1, 0, 0, p, p, p, None) == -1 and b"negative n" in lib.nm_last_error()
    assert lib.nm_classical_fwd(8, 8, 0, p, p, p, None) == -1 and b"unknown law" in lib.nm_last_error()
    assert lib.nm_classical_fwd(8, -1, 0, p, p, p, None) == -1
    assert lib.nm_classical_fwd(8, 2, 2, p, p, p, None) == -1 and b"mode" in lib.nm_last_error()
    assert lib.nm_classical_fwd(8, 0, 0, None, p, p, None) == -1 and b"null" in lib.nm_last_error()
    assert lib.nm_classical_fwd(8, 0, 0, p, None, p, None) == -1
    assert lib.nm_classical_fwd(8, 5, 0, None, p, None, None) == -1
    assert lib.nm_classical_bwd(-1, 0, 0, p, p, p, p, p, p, 1 << 20, None) == -1
    assert lib.nm_classical_bwd(8, 9, 0, p, p, p, p, p, p, 1 << 20, None) == -1
    assert lib.nm_classical_bwd(8, 0, 0, p, p, p, p, None, p, 1 << 20, None) == -1
    assert lib.nm_classical_bwd(8, 0, 0, p, p, None, p, p, p, 1 << 20, None) == -1
    assert lib.nm_classical_bwd(8, 0, 0, p, p, p, p, p, None, 0, None) == -1
    assert lib.nm_classical_bwd(8, 0, 0, p, p, p, p, p, p, 8, None) == -1 and b"workspace too small" in lib.nm_last_error()
