"""Inputs of the registration / SSIM fixtures (tests/golden/regist/*.npz), rebuilt wherever they are needed instead of being
stored: the generator (gen_regist_golden.py) and the tests call the same functions.

Every value comes from a splitmix64 integer hash (numpy uint64 arithmetic, wrapping) turned into a 24-bit uniform, then only
element-wise +, -, *, /, sqrt and floor in float64 (no reductions) and one cast to float32 - correctly rounded IEEE operations,
no libm calls - so the arrays are bit-identical on every machine.  The fixtures hold only what the reference's code computed from them."""
import numpy as np

K_TRANSFORM = 4096
ROW_STRIDE = 16            # per-Gaussian outputs are stored for rows 0, 16, 32, ... (every category of inputs is hit)


def uniform(n: int, stream: int) -> np.ndarray:
    """n values in [0, 1), float64, multiples of 2^-24."""
    with np.errstate(over="ignore"):
        z = np.arange(n, dtype=np.uint64) + np.uint64(stream) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x632BE59BD9B4E019)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(np.float64) / float(1 << 24)


def _u(shape, stream):
    return uniform(int(np.prod(shape)), stream).reshape(shape)


def transform_inputs(K: int = K_TRANSFORM) -> dict:
    """Per-Gaussian inputs shared by both transform cases: positions, quaternions as loaded (not normalised, norms 0.3 .. 3),
    log-scales (rows [0, K/8) large 0.5 .. 2.5, [K/8, K/4) tiny -12 .. -9, the rest -7 .. -2) and seeded upstream gradients."""
    xyz = 0.3 + 0.4 * _u((K, 3), 1)
    q = _u((K, 4), 2) - 0.5
    n2 = q[:, 0:1] * q[:, 0:1] + q[:, 1:2] * q[:, 1:2] + q[:, 2:3] * q[:, 2:3] + q[:, 3:4] * q[:, 3:4]
    q = q / np.sqrt(n2 + 1e-3) * (0.3 + 2.7 * _u((K, 1), 3))
    ls = -7.0 + 5.0 * _u((K, 3), 4)
    ls[: K // 8] = 0.5 + 2.0 * _u((K // 8, 3), 5)
    ls[K // 8: K // 4] = -12.0 + 3.0 * _u((K // 8, 3), 6)
    gm = 4.0 * (_u((K, 3), 7) - 0.5)
    gc = 40.0 * (_u((K, 6), 8) - 0.5)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return dict(xyz=f(xyz), rot=f(q), log_scales=f(ls), dL_dmeans3D=f(gm), dL_dcov6=f(gc))


def transform_case(case: int) -> dict:
    """Global parameters of case 0 (s < 1, scaling_modifier 1.0) and case 1 (s > 1, 1.2): r6 (float64), t, s, modifier."""
    r6 = 2.0 * (_u((6,), 20 + case) - 0.5)
    t = 0.6 * (_u((3,), 30 + case) - 0.5)
    return dict(r6=r6, t=np.asarray(t, np.float32), s=np.float32((0.63, 1.47)[case]), scaling_modifier=np.float32((1.0, 1.2)[case]))


def pcd_points(n: int = 200) -> np.ndarray:
    return _u((n, 3), 40) - 0.5


SSIM_SIZES = ((16, 16), (37, 53), (135, 240))


def ssim_images(h: int, w: int):
    """(img1, img2) (3,h,w) float32 in [0,1]: a smooth triangle-wave pattern plus hashed noise, and a noisy copy of it."""
    stream = 100 + h * 7 + w
    yy = np.arange(h, dtype=np.float64)[None, :, None] / h
    xx = np.arange(w, dtype=np.float64)[None, None, :] / w
    ch = np.arange(3, dtype=np.float64)[:, None, None]
    ph = 3.0 * xx + 2.0 * yy + 0.25 * ch
    tri = 2.0 * np.abs(ph - np.floor(ph) - 0.5)                       # triangle wave in [0, 1]
    a = 0.6 * (0.1 + 0.8 * tri) + 0.4 * _u((3, h, w), stream)
    b = np.clip(a + 0.3 * (_u((3, h, w), stream + 1) - 0.5), 0.0, 1.0)
    return np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)


def ssim_rows(h: int) -> np.ndarray:
    """Image rows whose gradient the fixture stores: all rows of images up to 16 rows, else three bands of three (top border,
    middle, bottom border)."""
    if h <= 16:
        return np.arange(h)
    m = h // 2
    return np.array([0, 1, 2, m - 1, m, m + 1, h - 3, h - 2, h - 1])
