"""extras/gaussian_fill.py, the numpy fp64 statement of the Gaussian fill (and the CPU path of neuma_amd.gaussian_fill):
analytic and topological properties of the field and the six-ray classification, the emission order and layout, the
errors, and prepare_simulation_data(fill=...) end to end on the CPU."""
import numpy as np
import pytest
import torch

from gaussian_fill_scenes import SHELL, shell_scene


def _gf():
    from neuma_amd.extras import gaussian_fill
    return gaussian_fill


def _centres(info):
    return [info["origin"][a] + (np.arange(info["dims"][a]) + 0.5) * info["h"] for a in range(3)]


@pytest.fixture(scope="module")
def shell():
    gf = _gf()
    mu, cv, op = shell_scene()
    origin, h, dims = gf.fill_lattice(mu, cv, SHELL["resolution"], SHELL["cutoff"])
    field, skipped = gf.density_field(mu, cv, op, origin, h, dims, SHELL["cutoff"])
    return dict(mu=mu, cv=cv, op=op, origin=origin, h=h, dims=dims, field=field, skipped=skipped,
                kind=gf.classify_cells(field, dims, SHELL["density_thres"]))


def test_one_isotropic_gaussian_keeps_exactly_the_analytic_ball():
    gf = _gf()
    s, tau, cutoff = 0.2, 0.5, 9.0
    mu = np.array([[0.1, -0.2, 0.3]], np.float32)
    cv = np.array([[s * s, 0, 0, s * s, 0, s * s]], np.float32)
    pts, kind, info = gf.fill_from_gaussians(mu, cv, np.ones(1, np.float32), resolution=21, density_thres=tau, cutoff=cutoff)
    assert info["dims"] == (21, 21, 21) and info["n_enclosed"] == 0 and info["n_skipped"] == 0
    cx, cy, cz = np.meshgrid(*_centres(info), indexing="ij")
    s2 = float(cv[0, 0])
    r2 = (cx - float(mu[0, 0])) ** 2 + (cy - float(mu[0, 1])) ** 2 + (cz - float(mu[0, 2])) ** 2
    assert np.abs(r2 + 2 * s2 * np.log(tau)).min() > 1e-9          # no centre on the sphere itself: the set is unambiguous
    want = (r2 < -2 * s2 * np.log(tau)) & (r2 <= cutoff * s2)
    assert 100 < want.sum() == len(pts) == info["n_shell"] and (kind == 1).all()
    want_pts = np.stack([cx[want], cy[want], cz[want]], 1).astype(np.float32)       # C order = ascending linear index
    assert np.array_equal(pts, want_pts)


def test_hollow_shell_encloses_its_cavity(shell):
    tau, dims = SHELL["density_thres"], tuple(shell["dims"])
    f, kind = shell["field"].reshape(dims), shell["kind"].reshape(dims)
    enc = np.argwhere(kind == 2)
    assert len(enc) > 0 and shell["skipped"] == 0
    assert (f[kind == 2] <= tau).all() and (f[kind == 1] > tau).all()
    assert not (np.abs(shell["field"] - tau) <= 1e-4 * tau).any()      # the scene's promise to the exact GPU comparison
    sh = kind == 1
    for ix, iy, iz in enc:
        assert sh[:ix, iy, iz].any() and sh[ix + 1:, iy, iz].any()
        assert sh[ix, :iy, iz].any() and sh[ix, iy + 1:, iz].any()
        assert sh[ix, iy, :iz].any() and sh[ix, iy, iz + 1:].any()
    # and the six-ray rule marks every such cell: nothing it should have found is missing
    n = 0
    for ix, iy, iz in np.argwhere(~sh):
        n += bool(sh[:ix, iy, iz].any() and sh[ix + 1:, iy, iz].any() and sh[ix, :iy, iz].any() and sh[ix, iy + 1:, iz].any()
                  and sh[ix, iy, :iz].any() and sh[ix, iy, iz + 1:].any())
    assert n == len(enc)


def test_open_bowl_leaves_the_open_column_unmarked(shell):
    gf = _gf()
    low = shell["mu"][:, 2] < 0                                           # the upper half of the shell removed
    mu, cv, op = shell["mu"][low], shell["cv"][low], shell["op"][low]
    origin, h, dims = gf.fill_lattice(mu, cv, SHELL["resolution"], SHELL["cutoff"])
    field, _ = gf.density_field(mu, cv, op, origin, h, dims, SHELL["cutoff"])
    kind = gf.classify_cells(field, dims, SHELL["density_thres"]).reshape(tuple(dims))
    sh = kind == 1
    ix, iy = (int(round((0.0 - origin[a]) / h - 0.5)) for a in range(2))      # the column through the bowl's axis
    col = sh[ix, iy]
    assert col.any()                                                      # the bowl has a bottom here ...
    top = int(np.flatnonzero(col).max())
    assert top < dims[2] - 3 and not col[top + 1:].any()                  # ... and nothing above it
    assert (kind[ix, iy, top + 1:] == 0).all()
    # every cell whose +z ray meets no shell cell is outside, whatever the other five rays meet
    above = np.flip(np.logical_or.accumulate(np.flip(sh, 2), 2), 2)      # a shell cell at this index or higher
    open_up = np.ones_like(sh)
    open_up[:, :, :-1] = ~above[:, :, 1:]
    assert (kind[open_up & ~sh] == 0).all()


def test_emission_order_per_cell_layout_and_no_shell(shell):
    gf = _gf()
    origin, h, dims, kc = shell["origin"], shell["h"], shell["dims"], shell["kind"]
    p1, k1 = gf.emit_points(kc, origin, h, dims, 1, True)
    cells = np.flatnonzero(kc > 0)                                        # ascending linear index
    assert np.array_equal(k1, kc[cells]) and p1.dtype == np.float32 and k1.dtype == np.uint8
    ix, iy, iz = np.unravel_index(cells, tuple(dims))
    for a, i in enumerate((ix, iy, iz)):
        assert np.array_equal(p1[:, a], (origin[a] + (i + 0.5) * h).astype(np.float32))
    p2, k2 = gf.emit_points(kc, origin, h, dims, 2, True)
    assert p2.shape == (8 * len(cells), 3) and np.array_equal(k2, np.repeat(k1, 8))
    q = 0
    for c in (0, len(cells) // 2, len(cells) - 1):
        for sx in range(2):
            for sy in range(2):
                for sz in range(2):
                    q = 8 * c + (sx * 2 + sy) * 2 + sz                    # s nested x, y, z
                    want = [np.float32(origin[a] + (i[c] + (s + 0.5) / 2) * h) for a, (i, s) in enumerate(((ix, sx), (iy, sy), (iz, sz)))]
                    assert p2[q].tolist() == [float(w) for w in want]
    p3, k3 = gf.emit_points(kc, origin, h, dims, 1, False)
    assert (k3 == 2).all() and np.array_equal(p3, p1[k1 == 2]) and len(p3) == (kc == 2).sum()
    pts, kind, info = gf.fill_from_gaussians(shell["mu"], shell["cv"], shell["op"], include_shell=False, **SHELL)
    assert np.array_equal(pts, p3) and info["n_shell"] == (kc == 1).sum() and info["n_enclosed"] == len(p3)
    empty, ke, info = gf.fill_from_gaussians(shell["mu"], shell["cv"], shell["op"], resolution=32, density_thres=1e3)
    assert empty.shape == (0, 3) and ke.shape == (0,) and info["n_shell"] == 0


def test_fp32_evaluation_stays_close_to_fp64(shell):
    gf = _gf()
    f32, _ = gf.density_field(shell["mu"], shell["cv"], shell["op"], shell["origin"], shell["h"], shell["dims"], SHELL["cutoff"],
                              dtype=np.float32)
    assert f32.dtype == np.float32
    m = shell["field"] > 0.05 * SHELL["density_thres"]
    assert (np.abs(f32[m] - shell["field"][m]) / shell["field"][m]).max() < 1e-5


def test_value_errors():
    gf = _gf()
    mu, cv, op = shell_scene(K=8)
    with pytest.raises(ValueError, match="K = 0"):
        gf.fill_from_gaussians(mu[:0], cv[:0], op[:0])
    for bad in (np.nan, np.inf):
        for which in range(3):
            a = [mu.copy(), cv.copy(), op.copy()]
            a[which].reshape(-1)[3] = bad
            with pytest.raises(ValueError, match="non-finite"):
                gf.fill_from_gaussians(*a)
    with pytest.raises(ValueError, match="2\\^27"):
        gf.fill_from_gaussians(mu, cv, op, resolution=1024)
    with pytest.raises(ValueError, match="resolution"):
        gf.fill_lattice(mu, cv, 0)
    with pytest.raises(ValueError, match="per_cell"):
        gf.fill_from_gaussians(mu, cv, op, per_cell=0)
    # 1100 Gaussians that each cover the whole 500^3 lattice: 1100 x 125^3 (Gaussian, block) pairs > 2^31
    big = np.tile(np.array([[1, 0, 0, 1, 0, 1]], np.float32), (1100, 1))
    with pytest.raises(ValueError, match="pairs"):
        gf.fill_lattice(np.zeros((1100, 3), np.float32), big, 500)


def test_degenerate_covariance_is_skipped_and_counted(shell):
    gf = _gf()
    mu, cv, op = shell["mu"], shell["cv"], shell["op"]
    flat = np.array([[0.01, 0, 0, 0.01, 0, 0.0], [0.01, 0.02, 0, 0.01, 0, 0.01]], np.float32)     # det = 0, det < 0
    mu2 = np.concatenate([mu, np.zeros((2, 3), np.float32)])
    cv2 = np.concatenate([cv, flat])
    op2 = np.concatenate([op, np.ones(2, np.float32)])
    origin, h, dims = shell["origin"], shell["h"], shell["dims"]
    for dt in (np.float64, np.float32):
        f, skipped = gf.density_field(mu2, cv2, op2, origin, h, dims, SHELL["cutoff"], dtype=dt)
        ref, _ = gf.density_field(mu, cv, op, origin, h, dims, SHELL["cutoff"], dtype=dt)
        assert skipped == 2 and np.array_equal(f, ref)
    assert gf.fill_from_gaussians(mu2, cv2, op2, **SHELL)[2]["n_skipped"] == 2


def test_prepare_simulation_data_fills_on_the_cpu(tmp_path):
    from neuma_amd import io as nio
    from neuma_amd.prepare import prepare_simulation_data
    from neuma_amd.render.gaussian_model import GaussianModel
    mu, _, op, quat, scales = shell_scene(K=96, return_raw=True)
    K = len(mu)
    gm = GaussianModel(0)
    t = lambda a: torch.tensor(np.asarray(a, np.float32))
    logit = np.log(op / (1 - op))
    logit[:5] = -6.0                                                       # five Gaussians below opacity_thres: pruned
    gm.set_params(t(mu), torch.zeros(K, 1, 3), torch.zeros(K, 0, 3), t(np.log(scales)), t(quat), t(logit[:, None]))
    nio.save_gaussians_ply(gm, tmp_path / "point_cloud.ply")
    out = tmp_path / "assets"
    with pytest.raises(ValueError, match="particles_path"):
        prepare_simulation_data(out, tmp_path / "point_cloud.ply", sh_degree=0, device="cpu")
    fill = dict(resolution=24, density_thres=0.3)
    prepare_simulation_data(out, tmp_path / "point_cloud.ply", sh_degree=0, device="cpu", fill=fill)
    assert all((out / n).is_file() for n in ("kernels.ply", "particles.ply", "bindings.pt"))
    kept = nio.load_gaussians_ply(out / "kernels.ply", 0)
    assert kept.get_xyz.shape[0] == K - 5
    pts, _, _ = _gf().fill_from_gaussians(kept.get_xyz.numpy(), kept.get_covariance().numpy(), kept.get_opacity.squeeze(-1).numpy(), **fill)
    particles = nio.load_particles_ply(out / "particles.ply")
    assert len(pts) > 100 and len(particles) >= len(pts) and np.array_equal(particles[:len(pts)].astype(np.float32), pts)
    _, n_particles = nio.load_bindings(out / "bindings.pt")
    assert n_particles.shape[0] == K - 5 and int(n_particles.min()) >= 1
