"""Shared lattice fields of the surface-mesh tests (tests/test_surface_mesh_cpu.py, tests/test_gpu_surface_mesh.py): the
smallest shapes at which the extraction can go wrong.  Every field is fp32 with values in [0, 1] and is extracted at
ISO = 0.5.  That range is what the position bound of the GPU tests rests on: on a crossed edge each of iso - f_a and
f_b - f_a is either exact in fp32 (operands within a factor of two of each other: Sterbenz) or |f_b - f_a| >= 2^-4 - the
random case by rejection, the others because an inexact difference needs one end below ISO / 2 (a ring sample's 0, for one)
while the other is at or above ISO."""
import numpy as np

ISO = 0.5


def _centres(dims, origin, h):
    ax = [origin[a] + (np.arange(dims[a], dtype=np.float64) + 0.5) * h for a in range(3)]
    return np.meshgrid(*ax, indexing="ij")


def _case(field, dims, origin=(0.0, 0.0, 0.0), h=0.1):
    f = np.ascontiguousarray(np.asarray(field, dtype=np.float32).reshape(-1))
    assert f.size == int(np.prod(dims)) and f.min() >= 0.0 and f.max() <= 1.0
    return dict(field=f, dims=tuple(int(d) for d in dims), origin=np.asarray(origin, dtype=np.float64), h=float(h), iso=ISO)


def random_field(dims, seed):
    """Uniform in [0, 1]; any value within 2^-4 of ISO is drawn again, so every crossed edge has |f_b - f_a| >= 2^-4."""
    rng = np.random.default_rng(seed)
    f = rng.random(int(np.prod(dims)))
    while True:
        bad = np.abs(f.astype(np.float32).astype(np.float64) - ISO) < 2.0 ** -4
        if not bad.any():
            return f
        f[bad] = rng.random(int(bad.sum()))


def sphere_field(n, centre=None, R=1.8, h=None, origin=(-0.3, 0.2, 0.1)):
    """1 - |x - c| / R on n^3 over a box of edge 2: the level ISO is a sphere of radius R / 2 = 0.9 inside the box."""
    h = 2.0 / n if h is None else h
    c = np.asarray(origin) + 1.0 + np.array([0.013, -0.021, 0.008]) if centre is None else np.asarray(centre)
    X, Y, Z = _centres((n, n, n), origin, h)
    r = np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2)
    return _case(1.0 - r / R, (n, n, n), origin, h), c, R * (1.0 - ISO)


def torus_field(dims=(22, 22, 10), h=0.1):
    X, Y, Z = _centres(dims, (0.0, 0.0, 0.0), h)
    c = np.array([dims[0], dims[1], dims[2]]) * h / 2 + np.array([0.011, -0.007, 0.004])
    ring = np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2) - 0.65        # major radius 0.65, tube radius 0.25 at ISO
    r = np.sqrt(ring ** 2 + (Z - c[2]) ** 2)
    return _case(np.clip(1.0 - r / 0.5, 0.0, 1.0), dims, (0.0, 0.0, 0.0), h)


def two_spheres_field(dims=(24, 12, 12), h=0.1):
    X, Y, Z = _centres(dims, (0.0, 0.0, 0.0), h)
    f = np.zeros(dims)
    for cx in (0.62, 1.79):
        r = np.sqrt((X - cx) ** 2 + (Y - 0.61) ** 2 + (Z - 0.58) ** 2)
        f = np.maximum(f, 1.0 - r / 0.8)                              # radius 0.4 at ISO; centres 1.17 apart
    return _case(np.clip(f, 0.0, 1.0), dims, (0.0, 0.0, 0.0), h)


def touching_field(dims=(7, 6, 5), h=0.1):
    """A ball larger than the lattice in every direction but its corners: the inside region reaches all six faces."""
    X, Y, Z = _centres(dims, (0.0, 0.0, 0.0), h)
    c = np.array(dims) * h / 2
    r = np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2)
    return _case(np.clip(1.0 - r / 0.84, 0.0, 1.0), dims, (0.0, 0.0, 0.0), h)


def ties_field(dims=(8, 7, 6)):
    """A plateau of samples equal to ISO exactly (inside, by f >= iso) around a core of 0.75, in a sea of 0.25."""
    f = np.full(dims, 0.25)
    f[1:-1, 1:-2, 1:-1] = ISO
    f[3:5, 2:4, 2:4] = 0.75
    f[2, 2, 2] = 0.25                     # a dent in the plateau: ties on both sides of crossed edges
    return _case(f, dims, (1.0, -2.0, 0.5), 0.25)


def all_cases():
    """name -> case (field, dims, origin, h, iso); every one has a non-empty closed surface."""
    cases = {
        "one_cell": _case(np.full((1, 1, 1), 0.75), (1, 1, 1), (0.3, -0.2, 0.1), 0.5),
        "odd_9x8x7": _case(random_field((9, 8, 7), 1), (9, 8, 7), (-0.4, 0.3, 1.0), 0.125),
        "flat_5x1x6": _case(random_field((5, 1, 6), 2), (5, 1, 6), (0.0, 0.0, 0.0), 0.3),
        "random_12": _case(random_field((12, 12, 12), 3), (12, 12, 12), (2.0, -1.0, 0.5), 0.05),
        "touching": touching_field(),
        "sphere_20": sphere_field(20)[0],
        "torus": torus_field(),
        "two_spheres": two_spheres_field(),
        "ties": ties_field(),
    }
    return cases


def attrs_for(case, A=3, seed=7):
    """(A, ncells) fp32 attributes in [0, 1]."""
    rng = np.random.default_rng(seed)
    return rng.random((A, case["field"].size)).astype(np.float32)
