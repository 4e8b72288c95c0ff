"""Particle -> Gaussian binding in numpy: the CPU path of neuma_amd/binding.py `build_bindings` (csrc/nm_bindbuild.hip), for
asset preparation on a machine without a GPU (`prepare_simulation_data(device="cpu")`).  The same rule in the same fp32
arithmetic: particle j binds to Gaussian k iff p = (x_j - mu_k)^T inv(Sigma_k) (x_j - mu_k) <= threshold, the inverse by
cofactors; at most max_particles per Gaussian, the ones with the smallest p (ties by index), columns ascending.  Dense
K x N in chunks of Gaussians: meant for the small scenes a CPU run prepares, not for the hot path."""
import numpy as np


def build_bindings(means, cov6, particles, threshold: float, max_particles: int):
    """-> (counts (K,) int32, n_inside (K,) int32, cols (K, max_particles) int32 [-1 padded], pvals (K, max_particles) fp32)."""
    m = np.asarray(means, dtype=np.float32).reshape(-1, 3)
    s = np.asarray(cov6, dtype=np.float32).reshape(-1, 6)
    x = np.asarray(particles, dtype=np.float32).reshape(-1, 3)
    K, N, P = len(m), len(x), int(max_particles)
    s00, s01, s02, s11, s12, s22 = (s[:, i] for i in range(6))
    with np.errstate(all="ignore"):
        c = np.stack([s11 * s22 - s12 * s12, s12 * s02 - s01 * s22, s01 * s12 - s11 * s02,
                      s00 * s22 - s02 * s02, s01 * s02 - s00 * s12, s00 * s11 - s01 * s01], 1)
        det = s00 * c[:, 0] + s01 * c[:, 1] + s02 * c[:, 2]
        idet = np.float32(1) / det
        A = c * idet[:, None]
    ok = np.isfinite(idet) & (det != 0)
    counts, inside = np.zeros(K, np.int32), np.zeros(K, np.int32)
    cols, pvals = np.full((K, P), -1, np.int32), np.zeros((K, P), np.float32)
    thr = np.float32(threshold)
    step = max(1, (1 << 22) // max(N, 1))
    for k0 in range(0, K if N else 0, step):
        k1 = min(k0 + step, K)
        d = x[None, :, :] - m[k0:k1, None, :]                                   # (k, N, 3)
        a = A[k0:k1, None, :]
        p1 = d[..., 0] * a[..., 0] + d[..., 1] * a[..., 1] + d[..., 2] * a[..., 2]
        p2 = d[..., 0] * a[..., 1] + d[..., 1] * a[..., 3] + d[..., 2] * a[..., 4]
        p3 = d[..., 0] * a[..., 2] + d[..., 1] * a[..., 4] + d[..., 2] * a[..., 5]
        with np.errstate(all="ignore"):
            p = p1 * d[..., 0] + p2 * d[..., 1] + p3 * d[..., 2]
        hit = (p <= thr) & ok[k0:k1, None]
        inside[k0:k1] = hit.sum(1)
        for k in np.flatnonzero(inside[k0:k1]):
            j = np.flatnonzero(hit[k])
            best = np.sort(j[np.lexsort((j, p[k, j]))[:P]])
            counts[k0 + k] = len(best)
            cols[k0 + k, :len(best)] = best
            pvals[k0 + k, :len(best)] = p[k, best]
    return counts, inside, cols, pvals
