"""Scenes shared by tests/test_gaussian_fill_cpu.py and tests/test_gpu_gaussian_fill.py (no tests here)."""
import numpy as np


def cov6_from(quat, scales):
    """cov6 (K, 6) fp32 = R diag(s^2) R^T in fp64 from quaternions (r, x, y, z) and per-axis scales."""
    q = np.asarray(quat, np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    r, x, y, z = q.T
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], -1),
                  np.stack([2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)], -1),
                  np.stack([2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1)], -2)
    L = R * np.asarray(scales, np.float64)[:, None, :]
    S = L @ L.transpose(0, 2, 1)
    return np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], -1).astype(np.float32)


def shell_scene(seed=17, K=384, return_raw=False):
    """The hollow ellipsoidal shell: K Gaussians centred on unit directions x 0.5 x (1, 0.8, 0.6), random rotations, scales
    log-uniform in [0.04, 0.12], opacity uniform in [0.3, 0.95].  (means, cov6, opacity) fp32 [+ (quat, scales)].  Seed 17:
    with this draw order seed 7 leaves one cell 6e-6 tau from the threshold at resolution 32, and the exact end-to-end
    comparison needs a scene with no cell within 1e-4 tau of it (seed 17: the nearest is 1e-3 tau away)."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(K, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    means = (d * 0.5 * np.array([1.0, 0.8, 0.6])).astype(np.float32)
    quat = rng.normal(size=(K, 4))
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    scales = np.exp(rng.uniform(np.log(0.04), np.log(0.12), size=(K, 3)))
    opacity = rng.uniform(0.3, 0.95, size=K).astype(np.float32)
    out = (means, cov6_from(quat, scales), opacity)
    return out + (quat, scales) if return_raw else out


SHELL = dict(resolution=32, density_thres=0.5, cutoff=9.0)


def random_cloud(seed, K, extent, smin, smax):
    """K random anisotropic Gaussians with centres uniform in +-extent (3,) and scales log-uniform in [smin, smax]."""
    rng = np.random.default_rng(seed)
    means = (rng.uniform(-1, 1, size=(K, 3)) * np.asarray(extent, float)).astype(np.float32)
    quat = rng.normal(size=(K, 4))
    scales = np.exp(rng.uniform(np.log(smin), np.log(smax), size=(K, 3)))
    return means, cov6_from(quat, scales), rng.uniform(0.3, 0.95, size=K).astype(np.float32)
