"""CPU: the field paint - the fp64 definition (neuma_amd/extras/field_paint.py, also the CPU path of neuma_amd/field_paint.py) against
closed forms, the ABI, and the HOST half of the kernels (nm_particle_field_one and nm_field_color are __host__ __device__):
tests/field_paint_host/field_paint_host_main.hip is built into tmp_path and run as a program; it makes no HIP call and is the target
for a host sanitizer build.

What this does NOT cover: the device path (v_rcp / v_rsq / v_sqrt inside nm_svd3, the device's logf), the CSR walk and the range
reduction, which tests/test_gpu_field_paint.py holds to the same bounds (field_paint_cases.BOUNDS: four times what the host program
measures here)."""
import math
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import field_paint_cases as fc
from neuma_amd import field_paint as fp
from neuma_amd.extras import field_paint as X

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "field_paint_host" / "field_paint_host_main.hip"


@pytest.fixture(scope="module")
def P():
    return fc.particles()


@pytest.fixture(scope="module")
def ref(P):
    """every quantity of the particle case in fp64, once"""
    return {q: X.particle_field(q, **{k: P[k] for k in X.NEEDS[q]}) for q in X.QUANTITIES}


# ---------------------------------------------------------------------------------------------------------------- closed forms

def test_uniaxial_stretch_strain_is_two_thirds_log_lambda(P, ref):
    # e = (L, 0, 0), m = L / 3, sum (e - m)^2 = (4 + 1 + 1) / 9 L^2 = 2/3 L^2, q = sqrt(2/3 * 2/3) |L| = 2/3 |L|
    a, b = fc.BLOCKS["uniaxial"]
    want = math.sqrt(2.0 / 3.0 * (2.0 / 3.0)) * P["lam"].log().abs()
    assert float(P["lam"].min()) < 0.5 and float(P["lam"].max()) > 2.0
    assert float((ref["strain"][a:b] - want).abs().max()) <= 1e-12
    assert float((ref["volume"][a:b] - P["lam"]).abs().max()) <= 1e-12


def test_hydrostatic_stress_has_no_von_mises_and_pressure_p(P):
    a, b = fc.BLOCKS["hydrostatic"]
    F, tau = P["F"][a:b], P["stress_hydro64"]
    assert float(X.particle_field("von_mises", F=F, stress=tau).abs().max()) <= 1e-12 * float(P["p"].abs().max())
    assert float((X.particle_field("pressure", F=F, stress=tau) - P["p"]).abs().max()) <= 1e-12 * float(P["p"].abs().max())
    # a pure shear stress has no pressure, and von Mises sqrt(3) |s|
    I = torch.eye(3, dtype=torch.float64)[None]
    shear = torch.zeros(1, 3, 3, dtype=torch.float64)
    shear[0, 0, 1] = shear[0, 1, 0] = 7.0
    assert float(X.particle_field("pressure", F=I, stress=shear)) == 0.0
    assert abs(float(X.particle_field("von_mises", F=I, stress=shear)) - math.sqrt(3.0) * 7.0) <= 1e-12
    # only the symmetric part of tau counts
    skew = shear.clone()
    skew[0, 0, 1], skew[0, 1, 0] = 14.0, 0.0
    assert abs(float(X.particle_field("von_mises", F=I, stress=skew)) - math.sqrt(3.0) * 7.0) <= 1e-12


def test_identity_has_no_strain_and_unit_volume(ref):
    a, b = fc.BLOCKS["identity"]
    assert float(ref["strain"][a:b].abs().max()) == 0.0
    assert bool((ref["volume"][a:b] == 1.0).all())


def test_inverted_particles_have_no_stress_quantities(P, ref):
    a, b = fc.BLOCKS["reflected"]
    assert bool((ref["volume"][a:b] < 0).all())
    for q in ("pressure", "von_mises"):
        assert bool(torch.isnan(ref[q][a:b]).all())
    assert bool(torch.isfinite(ref["strain"][a:b]).all())                      # |s_i|: a reflection strains like its mirror image
    Z = torch.zeros(2, 3, 3)                                                     # J == 0 too
    assert bool(torch.isnan(X.particle_field("pressure", F=Z, stress=Z)).all())
    assert bool(torch.isfinite(X.particle_field("strain", F=Z)).all())          # the floor under the logarithm


@pytest.mark.parametrize("quantity", X.QUANTITIES)
def test_non_finite_inputs_give_no_data_only_where_they_are_read(ref, quantity):
    bad = torch.zeros(fc.N, dtype=torch.bool)
    bad[fc.bad_rows(quantity)] = True
    if quantity in ("pressure", "von_mises"):
        bad[slice(*fc.BLOCKS["reflected"])] = True
        bad |= ref["volume"].nan_to_num(1.0) <= 0
    assert torch.equal(~torch.isfinite(ref[quantity]), bad)


def test_unknown_names_and_bad_ranges_are_refused():
    v = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="unknown quantity 'vorticity'"):
        fp.particle_field("vorticity", v=v)
    with pytest.raises(ValueError, match="unknown quantity"):
        fp.FieldPainter("vorticity")
    with pytest.raises(ValueError, match="unknown map 'viridis'"):
        fp.paint(torch.zeros(4), None, "viridis")
    with pytest.raises(ValueError, match="unknown map"):
        fp.FieldPainter("speed", "viridis")
    for rng in ((1.0, 1.0), (2.0, 1.0), (0.0, float("inf")), (float("nan"), 1.0), (1.0,)):
        with pytest.raises(ValueError, match="color_range"):
            fp.paint(torch.zeros(4), None, "heat", rng)
        with pytest.raises(ValueError, match="color_range"):
            fp.FieldPainter("speed", None, rng)
    with pytest.raises(ValueError, match="pressure reads stress"):
        fp.particle_field("pressure", F=torch.eye(3)[None])
    with pytest.raises(ValueError, match="knots"):
        X.knots_of([(0, 0, 0)])
    assert fp.FieldPainter("pressure").colormap == "coolwarm" == fp.FieldPainter("volume").colormap
    assert all(fp.FieldPainter(q).colormap == "heat" for q in ("speed", "displacement", "strain", "von_mises"))
    assert fp.QUANTITIES == ("speed", "displacement", "volume", "strain", "pressure", "von_mises")
    assert set(fp.COLORMAPS) == {"heat", "rainbow", "coolwarm", "gray"}


# ---------------------------------------------------------------------------------------------------------------- rows, range, maps

def test_rows_without_data_take_the_no_data_colour():
    c = fc.csr()
    shs, g, rng = X.paint(c["q"], c["rowptr"], c["col"], c["val"], "rainbow")
    nodata = sorted(c["empty"] + c["zero_weight"] + c["touching"])
    assert torch.equal(torch.nonzero(torch.isnan(g)).reshape(-1), torch.tensor(nodata))
    assert float(shs[nodata].abs().max()) == 0.0                               # (0.5 - 0.5) / C0
    rgb = shs[:, 0] * X.C0 + 0.5
    assert float((rgb[nodata] - torch.tensor(X.NODATA, dtype=torch.float64)).abs().max()) == 0.0
    # the mean itself, against a plain loop over one row
    r = next(r for r in range(200, fc.K_CSR) if c["rowptr"][r + 1] - c["rowptr"][r] == 5 and r not in nodata)
    s = slice(int(c["rowptr"][r]), int(c["rowptr"][r + 1]))
    w, qq = c["val"][s].double(), c["q"][c["col"][s].long()].double()
    assert abs(float(g[r]) - float((w * qq).sum() / w.sum())) <= 1e-12
    fin = g[torch.isfinite(g)]
    assert rng == (float(fin.min()), float(fin.max()))
    # the product path on CPU tensors is this path
    shs2, g2 = fp.paint(c["q"], fc.csr_bindings("cpu"), "rainbow")
    assert shs2.dtype == torch.float32 and float((shs2.double() - shs).abs().max()) <= 1e-6 and shs2.shape == (fc.K_CSR, 1, 3)
    assert torch.equal(torch.isnan(g2), torch.isnan(g))
    # a column outside [0, n) is no data, never read
    g3 = X.gaussian_values(torch.ones(4), torch.tensor([0, 1, 2]), torch.tensor([7, 1]), torch.ones(2))
    assert bool(torch.isnan(g3[0])) and float(g3[1]) == 1.0


def test_fp32_row_sums_in_csr_order_against_fp64():
    """What fc.G_BOUND is measured from: the kernel's arithmetic (both sums in fp32, in CSR order, one division) spelled in numpy."""
    b, q = fc.csr_bindings("cpu"), fc.csr()["q"]
    g64 = X.gaussian_values(q, b.rowptr, b.col, b.val)
    rp, col, val, qq = b.rowptr.numpy(), b.col.numpy(), b.val.numpy(), q.numpy()
    g32 = np.full(fc.K_CSR, np.nan, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        for k in range(fc.K_CSR):
            num, den = np.float32(0), np.float32(0)
            for j in range(rp[k], rp[k + 1]):
                num, den = np.float32(num + val[j] * qq[col[j]]), np.float32(den + val[j])
            if rp[k + 1] > rp[k] and den != 0 and np.isfinite(qq[col[rp[k]:rp[k + 1]]]).all():
                g32[k] = num / den
    fin = torch.isfinite(g64)
    assert torch.equal(torch.isfinite(torch.from_numpy(g32)), fin)
    err = float((torch.from_numpy(g32).double()[fin] - g64[fin]).abs().max() / g64[fin].abs().max())
    print(f"g: fp32 sums in CSR order vs fp64, rel to max = {err:.3e} (bound {fc.G_BOUND:.1e})")
    assert err <= fc.G_BOUND <= 1e-5


@pytest.mark.parametrize("name", sorted(X.COLORMAPS))
def test_each_map_returns_its_knots_at_the_knot_positions(name):
    knots = torch.tensor(X.COLORMAPS[name], dtype=torch.float64)
    n = knots.shape[0]
    assert 2 <= n <= X.MAX_KNOTS
    lo, hi = -3.0, 5.0
    g = torch.tensor([lo + (hi - lo) * i / (n - 1) for i in range(n)], dtype=torch.float64)
    assert float((X.colors(g, (lo, hi), name) - knots).abs().max()) <= 1e-15
    out = X.colors(torch.tensor([lo - 1.0, hi + 1.0, float("nan"), float("inf")]), (lo, hi), name)      # clamped; no data
    assert float((out[0] - knots[0]).abs().max()) <= 1e-15 and float((out[1] - knots[-1]).abs().max()) <= 1e-15      # (u = 1: c + 1 (d - c))
    assert torch.equal(out[2:], torch.tensor([X.NODATA, X.NODATA], dtype=torch.float64))
    mid = X.colors(torch.tensor([lo + (hi - lo) * 0.5 / (n - 1)], dtype=torch.float64), (lo, hi), name)[0]
    assert float((mid - 0.5 * (knots[0] + knots[1])).abs().max()) <= 1e-15


def test_built_in_names_and_knots_are_the_documented_ones():
    """The product module and the fp64 yardstick each state the tables themselves: both against the literals."""
    knots = {"heat": [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1)],
             "rainbow": [(0, 0, 1), (0, 1, 1), (0, 1, 0), (1, 1, 0), (1, 0, 0)],
             "coolwarm": [(0.23, 0.30, 0.75), (0.87, 0.87, 0.87), (0.71, 0.02, 0.15)],
             "gray": [(0, 0, 0), (1, 1, 1)]}
    needs = {"speed": ("v",), "displacement": ("x", "x0"), "volume": ("F",), "strain": ("F",), "pressure": ("F", "stress"),
             "von_mises": ("F", "stress")}
    for mod in (fp, X):
        assert {k: [tuple(float(a) for a in c) for c in v] for k, v in mod.COLORMAPS.items()} == \
            {k: [tuple(float(a) for a in c) for c in v] for k, v in knots.items()}
        assert mod.NODATA == (0.5, 0.5, 0.5) and mod.MAX_KNOTS == 8
        assert mod.QUANTITIES == ("speed", "displacement", "volume", "strain", "pressure", "von_mises") and mod.NEEDS == needs
        assert mod.widen(float("inf"), float("-inf")) == (0.0, 1.0) and mod.widen(2.0, 2.0) == (2.0, 3.0)
    assert fp.COLORMAPS is not X.COLORMAPS
    # importing the product module (and the drivers that hold it) does not import the yardstick
    import subprocess, sys
    code = ("import sys, neuma_amd.field_paint, neuma_amd.evaluate, neuma_amd.inference; "
            "sys.exit(1 if 'neuma_amd.extras.field_paint' in sys.modules else 0)")
    assert subprocess.run([sys.executable, "-c", code], cwd=str(ROOT)).returncode == 0


def test_range_widening_rule():
    nan, inf = float("nan"), float("inf")
    assert X.data_range(torch.tensor([3.0, nan, -1.0, inf])) == (-1.0, 3.0)
    assert X.data_range(torch.tensor([2.5, 2.5, nan])) == (2.5, 3.5)
    assert X.data_range(torch.tensor([nan, inf, -inf])) == (0.0, 1.0)
    assert X.data_range(torch.zeros(0)) == (0.0, 1.0)
    assert X.widen(inf, -inf) == (0.0, 1.0) and X.widen(2.0, 2.0) == (2.0, 3.0) and X.widen(-1.0, 4.0) == (-1.0, 4.0)
    # the painter on CPU tensors: per-frame range, overall range over the frames, the line a driver prints
    p = fp.FieldPainter("speed")
    eye = torch.eye(4).to_sparse()
    for scale in (1.0, 3.0, 2.0):
        v = torch.zeros(4, 3)
        v[:, 0] = scale * torch.tensor([1.0, 2.0, 3.0, 4.0])
        shs = p.frame(None, v, None, None, eye)
        assert shs.shape == (4, 1, 3)
        assert float((shs[0, 0] * X.C0 + 0.5).abs().max()) <= 1e-6 and float((shs[3, 0] * X.C0 + 0.5 - 1.0).abs().max()) <= 1e-6
    assert p.overall_range() == (1.0, 12.0)
    assert "--color_range 1 12" in p.summary() and "own range" in p.describe()
    q = fp.FieldPainter("speed", "gray", (0.0, 8.0))
    assert q.summary() is None and q.overall_range() == (0.0, 8.0)


def test_abi_and_build_list_carry_the_paint_calls():
    from neuma_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "neuma_hip.h").read_text(), flags=re.S)
    lib = _lib.lib()
    for name in ("nm_particle_field", "nm_field_range_workspace", "nm_field_range", "nm_field_paint"):
        m = re.search(r"\b" + name + r"\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
        assert m and hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == len(m.group(1).split(","))
    for i, q in enumerate(X.QUANTITIES):
        assert re.search(rf"#define NM_FIELD_{q.upper()} {i}\b", text)
    mk = (ROOT / "neuma_amd" / "csrc" / "Makefile").read_text()
    assert "nm_paint.hip" in mk and "nm_particle_field.h" in mk
    # argument checks come before any device work (the pointers below are never dereferenced)
    p = 4096
    assert lib.nm_field_range_workspace(-1) == 0 and lib.nm_field_range_workspace(70000) >= 2 * 4 * 274
    assert lib.nm_particle_field(0, 0, None, None, None, None, None, None, None) == 0
    for args, word in (((8, 6, p, p, p, p, p, p, None), b"unknown quantity"), ((-1, 0, p, p, p, p, p, p, None), b"n < 0"),
                       ((8, 0, p, None, p, p, p, p, None), b"speed reads v"), ((8, 1, None, p, p, p, p, p, None), b"displacement reads x"),
                       ((8, 1, p, p, p, p, None, p, None), b"displacement reads x0"), ((8, 3, p, p, None, p, p, p, None), b"strain reads F"),
                       ((8, 4, p, p, p, None, p, p, None), b"pressure reads stress"), ((8, 5, p, p, None, p, p, p, None), b"von_mises reads F"),
                       ((8, 2, p, p, p, p, p, None, None), b"q_out")):
        assert lib.nm_particle_field(*args) == -1 and word in lib.nm_last_error(), word
    assert lib.nm_field_range(8, p, p, 2, p, 1 << 20, None) == -1 and b"mode" in lib.nm_last_error()
    assert lib.nm_field_range(8, p, p, 0, p, 8, None) == -1 and b"workspace too small" in lib.nm_last_error()
    assert lib.nm_field_paint(8, 9, None, None, None, p, p, 2, None, None, p, None, None) == -1 and b"k must equal n" in lib.nm_last_error()
    assert lib.nm_field_paint(8, 8, None, None, None, p, p, 2, None, None, None, None, None) == -1 and b"both NULL" in lib.nm_last_error()
    import ctypes
    kn, nd = (ctypes.c_float * 27)(), (ctypes.c_float * 3)()
    assert lib.nm_field_paint(8, 8, None, None, None, p, p, 9, kn, nd, None, p, None) == -1 and b"n_knots" in lib.nm_last_error()
    assert lib.nm_field_paint(8, 8, p, None, p, p, p, 2, kn, nd, None, p, None) == -1 and b"col and val" in lib.nm_last_error()
    # the native path does not take a mix of devices silently: CPU tensors never reach it
    assert fp.particle_field("speed", v=torch.ones(2, 3)).dtype == torch.float32


# ---------------------------------------------------------------------------------------------------------------- host half

def _hipcc():
    return shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else None)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    d = tmp_path_factory.mktemp("field_paint_host")
    exe = d / "field_paint_host_main"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", str(SRC), "-o", str(exe)], check=True)

    def field(quantity, P):
        n = P["x"].shape[0]
        fin, fout = d / "in.bin", d / "out.bin"
        with open(fin, "wb") as fh:
            fh.write(np.array([n, X.QUANTITIES.index(quantity)], dtype=np.int32).tobytes())
            for k in ("x", "v", "F", "stress", "x0"):
                fh.write(P[k].numpy().astype(np.float32).tobytes())
        subprocess.run([str(exe), "field", str(fin), str(fout)], check=True, timeout=60)
        raw = np.fromfile(fout, dtype=np.float32)
        assert raw.size == n
        return torch.from_numpy(raw.copy())

    def color(g, lo, hi, name):
        knots = np.zeros(24, dtype=np.float32)
        kn = np.asarray(X.COLORMAPS[name], dtype=np.float32).reshape(-1)
        knots[:kn.size] = kn
        fin, fout = d / "cin.bin", d / "cout.bin"
        with open(fin, "wb") as fh:
            fh.write(np.array([g.numel(), kn.size // 3], dtype=np.int32).tobytes() + np.array([lo, hi], dtype=np.float32).tobytes())
            fh.write(knots.tobytes() + np.asarray(X.NODATA, dtype=np.float32).tobytes() + g.numpy().astype(np.float32).tobytes())
        subprocess.run([str(exe), "color", str(fin), str(fout)], check=True, timeout=60)
        raw = np.fromfile(fout, dtype=np.float32)
        assert raw.size == 3 * g.numel()
        return torch.from_numpy(raw.copy()).reshape(-1, 3)

    return field, color


@pytest.mark.parametrize("quantity", X.QUANTITIES)
def test_host_body_quantity_against_fp64(host, P, ref, quantity):
    got, want = host[0](quantity, P), ref[quantity]
    fin = torch.isfinite(want)
    assert torch.equal(torch.isfinite(got), fin)                               # no data at the same rows
    err = float((got.double()[fin] - want[fin]).abs().max() / want[fin].abs().max())
    print(f"{quantity}: host fp32 vs fp64, rel to max = {err:.3e} (bound {fc.BOUNDS[quantity]:.1e})")
    assert fc.BOUNDS[quantity] <= 1e-5
    assert err <= fc.BOUNDS[quantity]
    if quantity == "strain":
        a, b = fc.BLOCKS["identity"]
        ident = float(got[a:b].abs().max())
        print(f"strain of the identity block, abs = {ident:.3e}")
        assert ident <= fc.STRAIN_IDENTITY_ABS <= 1e-6


@pytest.mark.parametrize("name", sorted(X.COLORMAPS))
def test_host_body_colours_against_fp64(host, name):
    c = fc.color_case()
    dc = host[1](c["g"], c["lo"], c["hi"], name)
    want = X.colors(c["g"], (c["lo"], c["hi"]), name)
    rgb = dc.double() * X.C0 + 0.5
    err = float((rgb - want).abs().max())
    print(f"{name}: host colours vs fp64, abs = {err:.3e} (bound {fc.COLOR_ABS:.1e})")
    assert err <= fc.COLOR_ABS < 1.0 / 1020.0
    assert float((rgb[c["outside"]] - want[c["outside"]]).abs().max()) <= 1e-7          # clamped onto an end knot
    nod = host[1](torch.tensor([float("nan"), float("inf"), 0.3]), 0.0, 1.0, name)
    assert float(nod[:2].abs().max()) == 0.0 and float(nod[2].abs().max()) > 0
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), (0.0, float("inf")), (float("nan"), 1.0)):  # no range, no data
        assert float(host[1](torch.tensor([0.3, 1.5]), lo, hi, name).abs().max()) == 0.0
