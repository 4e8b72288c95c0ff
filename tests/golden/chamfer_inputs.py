"""Inputs of the Chamfer fixtures (tests/golden/chamfer/*.npz), rebuilt from seeded np.random.Generator(PCG64) draws for the
generator (gen_chamfer_golden.py) and the tests alike, so that they are never stored.  Every case is a pair of fp32 clouds
(B, N, 3) and (B, M, 3) of at most about 2 000 points in all."""
import numpy as np


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _lattice_ball(n, G, rng):
    """the synth.py particle layout: a jittered lattice of spacing dx/2 (dx = 1/G), the n points nearest (0.5, 0.5, 0.5),
    jitter U(-dx/8, dx/8)"""
    dx = 1.0 / G
    h = dx / 2
    m = int(np.ceil((3 * n / (4 * np.pi)) ** (1 / 3) * 1.15 + 2))
    ax = (np.arange(-m, m + 1) + 0.25) * h
    X = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    X = X[np.argsort((X ** 2).sum(1), kind="stable")[:n]] + 0.5
    return X + rng.uniform(-dx / 8, dx / 8, size=X.shape)


def uniform():
    """uniform clouds in the unit cube, N != M, B = 2"""
    r = _rng(1)
    return r.uniform(0, 1, (2, 600, 3)).astype(np.float32), r.uniform(0, 1, (2, 400, 3)).astype(np.float32)


def lattice():
    """a jittered lattice at the synth.py layout (G = 32) against a smoothly deformed copy of itself"""
    r = _rng(2)
    x = _lattice_ball(900, 32, r)
    y = x + 0.03 * np.sin(2 * np.pi * x[:, [1, 2, 0]]) + r.normal(0, 2e-3, x.shape)
    return x[None].astype(np.float32), y[None].astype(np.float32)


def clusters():
    """two tight clusters 10 apart in each cloud: most grid cells between them are empty"""
    r = _rng(3)
    c = np.array([[0.0, 0.0, 0.0], [10.0, 10.0, 10.0]])
    a = np.concatenate([c[0] + r.normal(0, 0.02, (350, 3)), c[1] + r.normal(0, 0.02, (250, 3))])
    b = np.concatenate([c[0] + r.normal(0, 0.02, (200, 3)), c[1] + r.normal(0, 0.02, (300, 3))])
    return a[None].astype(np.float32), b[None].astype(np.float32)


def outside():
    """queries drawn from three times the targets' box, so that most of them lie outside it"""
    r = _rng(4)
    return r.uniform(-1, 2, (1, 500, 3)).astype(np.float32), r.uniform(0, 1, (1, 600, 3)).astype(np.float32)


def duplicates():
    """targets made of 150 points each repeated four times (exact distance ties between copies)"""
    r = _rng(5)
    t = np.repeat(r.uniform(0, 1, (150, 3)), 4, axis=0)
    t = t[r.permutation(len(t))]
    return r.uniform(0, 1, (1, 500, 3)).astype(np.float32), t[None].astype(np.float32)


def naive():
    """N = M (chamfer_distance_naive's assertion), B = 2"""
    r = _rng(6)
    return r.normal(0, 1, (2, 400, 3)).astype(np.float32), r.normal(0.1, 1, (2, 400, 3)).astype(np.float32)


KDTREE_CASES = {"uniform": uniform, "lattice": lattice, "clusters": clusters, "outside": outside, "duplicates": duplicates}
NAIVE_CASES = {"naive": naive}
