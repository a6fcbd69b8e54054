"""
Yardsticks of the multi-scale 3-D SSIM, all on the host: the 2 x 2 x 2 pooling in numpy fp32 in the
documented order of additions and the 4-of-8 mask rule, the per-scale CS and S maps in fp64 with
scipy.ndimage.gaussian_filter cropped by 5 (as metrics_ref.ssim_map does it), a second, independent evaluation with
torch.nn.functional.avg_pool3d and conv3d in fp64 throughout, a plain fp32 evaluation of the maps (it sets the
accuracy bound of the GPU tests), and the cases the tests run on.  Helper module of tests/test_msssim_cpu.py and
tests/test_gpu_msssim.py.
"""

import functools
import math

import numpy as np
import scipy.ndimage
import torch
import torch.nn.functional as F

import metrics_ref as R

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MAX_SCALES = 5
# (shape, scales): even extents throughout; odd extents dropped at both levels and a last scale one plane deep;
# a shape that fits no tile; a last scale of a single interior voxel
CASES = [((48, 64, 64), 3), ((45, 50, 91), 3), ((23, 37, 61), 2), ((22, 22, 22), 2)]
NOISES = (0.02, 0.1)


def weights(scales):
    w = WEIGHTS[:scales]
    total = math.fsum(w)
    return [v / total for v in w]


# ------------------------------------------------------------------------------------------------ pooling
def pool2(x):
    """(..., D, H, W) -> (..., D // 2, H // 2, W // 2) in fp32: ((v000 + v001) + (v010 + v011)) + ((v100 + v101) +
    (v110 + v111)), index order dz dy dx, times 0.125"""
    x = np.asarray(x)
    assert x.dtype == np.float32
    D, H, W = (n // 2 for n in x.shape[-3:])
    v = lambda dz, dy, dx: x[..., dz:2 * D:2, dy:2 * H:2, dx:2 * W:2]
    s = ((v(0, 0, 0) + v(0, 0, 1)) + (v(0, 1, 0) + v(0, 1, 1))) + ((v(1, 0, 0) + v(1, 0, 1)) + (v(1, 1, 0) + v(1, 1, 1)))
    out = s * np.float32(0.125)
    assert out.dtype == np.float32
    return np.ascontiguousarray(out)


def pool2_mask(mask):
    """a pooled voxel is counted iff at least 4 of its 8 inputs are"""
    m = (np.asarray(mask) != 0).astype(np.int32)
    D, H, W = (n // 2 for n in m.shape)
    n = sum(m[dz:2 * D:2, dy:2 * H:2, dx:2 * W:2] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1))
    return (n >= 4).astype(np.uint8)


def pyramid(x, y, mask, scales):
    """[(x_j, y_j, mask_j)] for j = 0 .. scales - 1, pooled in fp32"""
    x, y = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
    levels = [(x, y, mask)]
    for _ in range(scales - 1):
        x, y, mask = pool2(x), pool2(y), None if mask is None else pool2_mask(mask)
        levels.append((x, y, mask))
    return levels


# ----------------------------------------------------------------------------------------------- the maps
def _terms(ux, uy, uxx, uyy, uxy, L):
    c1, c2 = R.constants(L)
    vx, vy, vxy = uxx - ux * ux, uyy - uy * uy, uxy - ux * uy
    cs = (2 * vxy + c2) / (vx + vy + c2)
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    return cs, s


def maps(x, y, L):
    """THE yardstick of one scale: (CS map, S map) in fp64, scipy's Gaussian filter, cropped by 5"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    f = lambda a: R._crop(scipy.ndimage.gaussian_filter(a, R.SIGMA, truncate=3.5))
    return _terms(f(x), f(y), f(x * x), f(y * y), f(x * y), L)


def maps_conv3d(x, y, L):
    """the cross-check: one dense 11 x 11 x 11 fp64 window through conv3d, no padding; x, y fp64 tensors or arrays"""
    w = torch.from_numpy(R.taps())
    k = (w[:, None, None] * w[None, :, None] * w[None, None, :])[None, None]
    x, y = (torch.as_tensor(np.asarray(a, dtype=np.float64))[None, None] for a in (x, y))
    f = lambda a: F.conv3d(a, k)[0, 0]
    cs, s = _terms(f(x), f(y), f(x * x), f(y * y), f(x * y), L)
    return cs.numpy(), s.numpy()


def maps_fp32(x, y, L):
    """the same formulas in plain fp32 (separable conv3d, fp32 taps, E[x^2] - mu^2 without a pivot)"""
    w = torch.from_numpy(R.taps()).to(torch.float32)
    x, y = (torch.from_numpy(np.asarray(a, dtype=np.float32))[None, None] for a in (x, y))

    def f(a):
        a = F.conv3d(a, w.view(1, 1, -1, 1, 1))
        a = F.conv3d(a, w.view(1, 1, 1, -1, 1))
        return F.conv3d(a, w.view(1, 1, 1, 1, -1))[0, 0]

    c1, c2 = (torch.tensor(c, dtype=torch.float32) for c in R.constants(L))
    ux, uy, uxx, uyy, uxy = f(x), f(y), f(x * x), f(y * y), f(x * y)
    vx, vy, vxy = uxx - ux * ux, uyy - uy * uy, uxy - ux * uy
    cs = (2 * vxy + c2) / (vx + vy + c2)
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    assert cs.dtype == s.dtype == torch.float32
    return cs.numpy(), s.numpy()


# ------------------------------------------------------------------------------------------ the combination
def combine(terms, w):
    """prod max(t_j, 0) ** w_j in fp64; 0.0 when a term is <= 0"""
    assert len(terms) == len(w)
    if any(not t > 0 for t in terms):
        return 0.0
    return math.prod(float(t) ** float(e) for t, e in zip(terms, w))


def scale_means(levels, L, evaluate=maps):
    """[(CS_j, S_j)]: the means over the counted interior voxels of every level of a pyramid"""
    out = []
    for x, y, mask in levels:
        cs, s = evaluate(x, y, L)
        out.append((R.masked_mean(cs, mask), R.masked_mean(s, mask)))
    return out


def msssim(x, y, L, scales, mask=None, w=None):
    """THE yardstick -> (value, terms): terms = [CS_0 .. CS_{M-2}, S_{M-1}]"""
    means = scale_means(pyramid(x, y, mask, scales), L)
    terms = [m[0] for m in means[:-1]] + [means[-1][1]]
    return combine(terms, weights(scales) if w is None else w), terms


def msssim_torch(x, y, L, scales, mask=None, w=None):
    """the independent evaluation: avg_pool3d and conv3d, fp64 throughout (the pooling is not rounded to fp32)"""
    x, y = (torch.from_numpy(np.asarray(a, dtype=np.float64))[None, None] for a in (x, y))
    m = None if mask is None else torch.from_numpy((np.asarray(mask) != 0).astype(np.float64))[None, None]
    terms = []
    for j in range(scales):
        cs, s = maps_conv3d(x[0, 0].numpy(), y[0, 0].numpy(), L)
        on = None if m is None else (m[0, 0].numpy() != 0).astype(np.uint8)
        terms.append(R.masked_mean(cs if j < scales - 1 else s, on))
        if j < scales - 1:
            x, y = F.avg_pool3d(x, 2), F.avg_pool3d(y, 2)
            m = None if m is None else (F.avg_pool3d(m, 2) >= 0.5).to(torch.float64)
    return combine(terms, weights(scales) if w is None else w), terms


def e32_per_scale(levels, L):
    """per scale the largest per-voxel deviation of the plain fp32 CS and S maps from the fp64 ones"""
    out = []
    for x, y, _ in levels:
        cs, s = maps(x, y, L)
        cs32, s32 = maps_fp32(x, y, L)
        out.append(float(max(np.abs(cs32 - cs).max(), np.abs(s32 - s).max())))
    return out


# -------------------------------------------------------------------------------------------------- cases
@functools.lru_cache(maxsize=None)
def case(i, k):
    """Case i of CASES with noise k of NOISES, computed once: a dict with name, scales, x (estimate), y (target), mask
    (the body mask of the target), levels (the pyramid of (x_j, y_j, mask_j)), e32 (per scale), and per mask choice
    (False, True) value[...] and terms[...] of the yardstick.  The arrays are shared: do not write to them."""
    shape, scales = CASES[i]
    y = R.phantom(shape, seed=i)
    x = R.noisy(y, NOISES[k], seed=10 * i + k)
    mask = R.body_mask(y)
    levels = pyramid(x, y, mask, scales)
    value, terms = {}, {}
    for masked in (False, True):
        means = scale_means([(a, b, m if masked else None) for a, b, m in levels], 1.0)
        terms[masked] = [m[0] for m in means[:-1]] + [means[-1][1]]
        value[masked] = combine(terms[masked], weights(scales))
    return dict(name="%dx%dx%d/M%d/noise%g" % (shape + (scales, NOISES[k])), shape=shape, scales=scales, x=x, y=y,
                mask=mask, levels=levels, e32=e32_per_scale(levels, 1.0), value=value, terms=terms)


def case_ids():
    return [(i, k) for i in range(len(CASES)) for k in range(len(NOISES))]


def case_name(ik):
    shape, scales = CASES[ik[0]]
    return "%dx%dx%d-M%d-noise%g" % (shape + (scales, NOISES[ik[1]]))


def first_order_bound(value, terms, w, e):
    """the first-order propagation of a per-term error e through the product: value * sum_j w_j e / v_j"""
    return value * sum(wj * e / v for wj, v in zip(w, terms))
