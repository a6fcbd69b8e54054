"""
Yardsticks of the image-quality metrics, all on the host: the documented skimage formula of the 3-D
SSIM evaluated in fp64 with scipy.ndimage.gaussian_filter and cropped by 5, a second, independent fp64 evaluation with
torch.nn.functional.conv3d on "valid" windows, a plain fp32 evaluation (what an un-pivoted fp32 kernel computes: it
sets the accuracy bound of the GPU tests), numpy fp64 error moments, and the seeded phantom the tests run on.
Helper module of tests/test_metrics_cpu.py and tests/test_gpu_metrics.py.
"""

import numpy as np
import scipy.ndimage
import torch
import torch.nn.functional as F

RADIUS = 5
SIGMA = 1.5
SHAPES = [(48, 64, 64), (40, 96, 96), (23, 37, 61)]      # three different extents; 23 x 37 x 61 fits no tile
NOISES = (0.02, 0.1)


def taps():
    """the 11 window taps in fp64: exp(-0.5 (j - 5)^2 / sigma^2), normalised to sum 1"""
    j = np.arange(-RADIUS, RADIUS + 1, dtype=np.float64)
    g = np.exp(-0.5 * j * j / (SIGMA * SIGMA))
    return g / g.sum()


def scipy_taps():
    """the taps scipy.ndimage.gaussian_filter(., 1.5, truncate=3.5) applies: its response to a unit impulse"""
    delta = np.zeros(4 * RADIUS + 1)
    delta[2 * RADIUS] = 1.0
    return scipy.ndimage.gaussian_filter(delta, SIGMA, truncate=3.5)[RADIUS:3 * RADIUS + 1]


def constants(L):
    return (0.01 * L) ** 2, (0.03 * L) ** 2


def _crop(a):
    return a[RADIUS:-RADIUS, RADIUS:-RADIUS, RADIUS:-RADIUS]


def _combine(ux, uy, uxx, uyy, uxy, L):
    c1, c2 = constants(L)
    vx, vy, vxy = uxx - ux * ux, uyy - uy * uy, uxy - ux * uy
    return ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))


def interior_mask(mask):
    return None if mask is None else _crop(np.asarray(mask) != 0)


def masked_mean(smap, mask):
    """mean of the map over the interior voxels the mask counts, in fp64"""
    smap = np.asarray(smap, dtype=np.float64)
    return float(smap.mean()) if mask is None else float(smap[interior_mask(mask)].mean())


def ssim_map(x, y, L):
    """THE yardstick: fp64, scipy's Gaussian filter (the border mode never reaches the cropped interior)"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    f = lambda a: _crop(scipy.ndimage.gaussian_filter(a, SIGMA, truncate=3.5))
    return _combine(f(x), f(y), f(x * x), f(y * y), f(x * y), L)


def ssim(x, y, L, mask=None):
    return masked_mean(ssim_map(x, y, L), mask)


def ssim_map_conv3d(x, y, L):
    """the cross-check: one dense 11 x 11 x 11 fp64 window through conv3d, no padding"""
    w = torch.from_numpy(taps())
    k = (w[:, None, None] * w[None, :, None] * w[None, None, :])[None, None]
    x, y = (torch.from_numpy(np.asarray(a, dtype=np.float64))[None, None] for a in (x, y))
    f = lambda a: F.conv3d(a, k)[0, 0]
    return _combine(f(x), f(y), f(x * x), f(y * y), f(x * y), L).numpy()


def ssim_map_fp32(x, y, L):
    """the same formula in plain fp32 (separable conv3d, fp32 taps, E[x^2] - mu^2 without a pivot)"""
    w = torch.from_numpy(taps()).to(torch.float32)
    x, y = (torch.from_numpy(np.asarray(a, dtype=np.float32))[None, None] for a in (x, y))

    def f(a):
        a = F.conv3d(a, w.view(1, 1, -1, 1, 1))
        a = F.conv3d(a, w.view(1, 1, 1, -1, 1))
        return F.conv3d(a, w.view(1, 1, 1, 1, -1))[0, 0]

    c1, c2 = (torch.tensor(c, dtype=torch.float32) for c in constants(L))
    ux, uy, uxx, uyy, uxy = f(x), f(y), f(x * x), f(y * y), f(x * y)
    vx, vy, vxy = uxx - ux * ux, uyy - uy * uy, uxy - ux * uy
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    assert s.dtype == torch.float32
    return s.numpy()


def constant_ssim(a, b, L):
    """S of two constant volumes x = a, y = b: the variances vanish and C2 cancels"""
    c1, _ = constants(L)
    return (2 * a * b + c1) / (a * a + b * b + c1)


def moments(x, y, mask=None, std=None):
    """error moments over the counted voxels, every term and sum in numpy fp64"""
    x, y = np.asarray(x, dtype=np.float64).ravel(), np.asarray(y, dtype=np.float64).ravel()
    on = np.ones(x.shape, dtype=bool) if mask is None else np.asarray(mask).ravel() != 0
    e, t = (x - y)[on], y[on]
    res = dict(n=int(on.sum()), mse=float((e * e).sum() / e.size), mae=float(np.abs(e).sum() / e.size),
               bias=float(e.sum() / e.size), target_sq_mean=float((t * t).sum() / e.size),
               target_mean=float(t.sum() / e.size), target_min=float(t.min()), target_max=float(t.max()),
               target_abs_mean=float(np.abs(t).sum() / e.size))
    if std is not None:
        s = np.asarray(std, dtype=np.float64).ravel()[on]
        res["cover_1"], res["cover_2"] = int((np.abs(e) <= s).sum()), int((np.abs(e) <= 2.0 * s).sum())
    return res


def phantom(shape, seed=0):
    """A seeded PET-like target in [0, 1], float32 (D, H, W): an ellipsoid body at 0.25 (about a quarter of the box),
    a dozen spheres of higher uptake inside it, blurred with sigma 1, clipped."""
    rng = np.random.default_rng(1000 + seed)
    D, H, W = shape
    z, yy, xx = np.meshgrid(*(np.linspace(-1.0, 1.0, n) for n in shape), indexing="ij")
    body = (z / 0.9) ** 2 + (yy / 0.8) ** 2 + (xx / 0.65) ** 2 <= 1.0
    vol = np.where(body, 0.25, 0.0)
    for _ in range(12):
        c = rng.uniform(-0.5, 0.5, size=3)
        r = rng.uniform(0.08, 0.2)
        uptake = rng.uniform(0.5, 1.0)
        vol[((z - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2 <= r * r) & body] = uptake
    vol = scipy.ndimage.gaussian_filter(vol, 1.0)
    return np.clip(vol, 0.0, 1.0).astype(np.float32)


def noisy(target, sigma, seed=0):
    rng = np.random.default_rng(2000 + seed)
    return (target + sigma * rng.standard_normal(target.shape)).astype(np.float32)


def body_mask(target, threshold=0.1):
    return (target > threshold * target.max()).astype(np.uint8)


def pairs():
    """every (shape, noise) case: (name, estimate, target)"""
    for i, shape in enumerate(SHAPES):
        y = phantom(shape, seed=i)
        for j, sigma in enumerate(NOISES):
            yield "%dx%dx%d/noise%g" % (shape + (sigma,)), noisy(y, sigma, seed=10 * i + j), y
