"""The clouds of the EMD tests (tests/test_emd_cpu.py, tests/test_gpu_emd.py): each case is a function returning fp32 (a, b) of n
points each.  CASES maps a name to (function, n); POWERS are the two cost exponents.  The twin's round counts over CASES x POWERS
are the statistics behind the default round limit (neuma_amd/extras/emd.py)."""
import functools

import numpy as np

POWERS = (1, 2)


def _rng(seed):
    return np.random.default_rng(seed)


def uniform(n, seed=0):
    r = _rng(100 + seed + n)
    return r.random((n, 3), dtype=np.float32), r.random((n, 3), dtype=np.float32)


def permuted_jitter(n=256):
    r = _rng(1)
    a = r.random((n, 3), dtype=np.float32)
    return a, a[r.permutation(n)] + np.float32(0.01) * r.standard_normal((n, 3)).astype(np.float32)


def clusters(n=1024, split=700 / 1024):
    """two clusters, a 700/324 split of a against 324/700 of b (scaled with n): the surplus of each cluster has to cross over,
    and the persons of the crowded cluster fight a long price war first"""
    r = _rng(2)
    k = int(round(n * split))
    c0, c1 = np.float32([0.2, 0.2, 0.2]), np.float32([0.8, 0.7, 0.6])

    def cloud(n0):
        p = np.float32(0.05) * r.standard_normal((n, 3)).astype(np.float32)
        p[:n0] += c0
        p[n0:] += c1
        return p

    return cloud(k), cloud(n - k)


def ties(n=1024, distinct=16):
    """`distinct` points each repeated n / distinct times in both clouds (different points in a and b): massive exact ties"""
    r = _rng(3)
    pa, pb = r.random((distinct, 3), dtype=np.float32), r.random((distinct, 3), dtype=np.float32)
    return np.repeat(pa, n // distinct, 0), np.repeat(pb, n // distinct, 0)[r.permutation(n)]


def exact_permutation(n=512):
    r = _rng(4)
    a = r.random((n, 3), dtype=np.float32)
    return a, a[r.permutation(n)].copy()


def identical(n=100):
    p = np.float32([0.3, -1.5, 2.25])
    return np.tile(p, (n, 1)), np.tile(p, (n, 1))


def collinear(n=256):
    r = _rng(5)
    d, o = np.float32([1.0, 2.0, -0.5]), np.float32([0.1, 0.2, 0.3])
    return o + r.random((n, 1), dtype=np.float32) * d, o + r.random((n, 1), dtype=np.float32) * d


def coplanar(n=256):
    r = _rng(6)
    a, b = r.random((n, 3), dtype=np.float32), r.random((n, 3), dtype=np.float32)
    a[:, 2] = 0.5
    b[:, 2] = 0.5
    return a, b


def offset(n=256):
    r = _rng(7)
    return np.float32(1e3) + r.random((n, 3), dtype=np.float32), np.float32(1e3) + r.random((n, 3), dtype=np.float32)


CASES = {f"uniform{n}": (functools.partial(uniform, n), n) for n in (1, 2, 63, 64, 65, 256, 1000)}
CASES.update({
    "permuted_jitter256": (permuted_jitter, 256),
    "clusters1024": (clusters, 1024),
    "ties1024": (ties, 1024),
    "exact_permutation512": (exact_permutation, 512),
    "identical100": (identical, 100),
    "collinear256": (collinear, 256),
    "coplanar256": (coplanar, 256),
    "offset256": (offset, 256),
})


@functools.lru_cache(maxsize=None)
def case(name):
    """(a, b) of a case, built once; read-only"""
    a, b = CASES[name][0]()
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape == (CASES[name][1], 3)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def twin(name, power):
    """neuma_amd.extras.emd.solve of a case (computed once per process, shared by the tests that need it) plus C"""
    from neuma_amd.extras import emd as E
    a, b = case(name)
    res = E.solve(a, b, power, max_rounds=10 ** 7)
    res["C"] = E.quantised_costs(a, b, power)[0]
    return res
