"""
Yardstick of the sphere-mean map and of SUVpeak / MTV / TLG, on the host in fp64.  The footprint is
found by brute force over the integer box, straight from its definition and without the run table of
metrics.sphere_footprint; the mean is scipy.ndimage.correlate of the kept values over the correlate of the kept
flags, zeros beyond the faces; `bound` is the arithmetic contract of ddpm3d_sphere_mean (include/ddpm3d.h).
"""

import functools
import math

import numpy as np
from scipy import ndimage

U = 2.0 ** -24           # the unit roundoff of fp32


def radius_mm(volume_mm3=1000.0):
    return (3.0 * volume_mm3 / (4.0 * math.pi)) ** (1.0 / 3.0)


def footprint(spacing, volume_mm3=1000.0):
    """bool array (2 b0 + 1, 2 b1 + 1, 2 b2 + 1), centred, b = ceil(r / s) + 1 per axis: True where the voxel centre
    lies in the sphere"""
    r = radius_mm(volume_mm3)
    box = [int(math.ceil(r / s)) + 1 for s in spacing]
    grids = np.meshgrid(*[np.arange(-b, b + 1, dtype=np.float64) * s for b, s in zip(box, spacing)], indexing="ij")
    return grids[0] ** 2 + grids[1] ** 2 + grids[2] ** 2 <= r * r


def margin_mm(spacing, volume_mm3=1000.0):
    """the distance in mm from the sphere's surface to the nearest lattice point (how far a case is from a tie)"""
    r = radius_mm(volume_mm3)
    box = [int(math.ceil(r / s)) + 1 for s in spacing]
    grids = np.meshgrid(*[np.arange(-b, b + 1, dtype=np.float64) * s for b, s in zip(box, spacing)], indexing="ij")
    return float(np.abs(np.sqrt(grids[0] ** 2 + grids[1] ** 2 + grids[2] ** 2) - r).min())


def trimmed(fp):
    """the footprint without its all-False outer planes -> (array, radii)"""
    at = np.argwhere(fp)
    centre = np.array(fp.shape) // 2
    radii = np.abs(at - centre).max(axis=0)
    cut = tuple(slice(c - r, c + r + 1) for c, r in zip(centre, radii))
    return fp[cut], tuple(int(v) for v in radii)


def expand(radii, half_w):
    """the run table of metrics.sphere_footprint as a bool array of shape (2 r0 + 1, 2 r1 + 1, 2 r2 + 1)"""
    r0, r1, r2 = radii
    out = np.zeros((2 * r0 + 1, 2 * r1 + 1, 2 * r2 + 1), dtype=bool)
    assert len(half_w) == 2 * r0 + 1 and all(len(row) == 2 * r1 + 1 for row in half_w)
    for i, row in enumerate(half_w):
        for j, w in enumerate(row):
            assert -1 <= w <= r2
            if w >= 0:
                out[i, j, r2 - w:r2 + w + 1] = True
    return out


def sphere_mean(x, fp, keep=None):
    """-> (mean fp64, n int64, bound fp64) per voxel of x (D, H, W): the mean of x over the footprint voxels inside
    the volume with keep != 0, 0 where there is none; their number; and (n + 2) 2^-24 (sum |x_i| / n), 0 where n = 0"""
    x = np.asarray(x, dtype=np.float64)
    kept = np.ones(x.shape, dtype=np.float64) if keep is None else (np.asarray(keep) != 0).astype(np.float64)
    w = trimmed(fp)[0].astype(np.float64)
    xk = np.where(kept != 0, x, 0.0)
    total = ndimage.correlate(xk, w, mode="constant", cval=0.0)
    mag = ndimage.correlate(np.abs(xk), w, mode="constant", cval=0.0)
    n = np.rint(ndimage.correlate(kept, w, mode="constant", cval=0.0)).astype(np.int64)
    safe = np.maximum(n, 1)
    mean = np.where(n > 0, total / safe, 0.0)
    bound = np.where(n > 0, (n + 2) * U * mag / safe, 0.0)
    return mean, n, bound


def region_peaks(mean, bound, labels, values, keep=None):
    """per label value: (the largest mean over the region's kept voxels, the largest bound there).  A maximum of
    values each within its bound of the yardstick's lies within the largest such bound of the yardstick's maximum."""
    out = []
    for v in values:
        at = labels == v
        if keep is not None:
            at &= np.asarray(keep) != 0
        out.append((float(mean[at].max()), float(bound[at].max())))
    return out


def figures(x, labels, value, spacing, keep=None):
    """n, mean (fp64), volume_ml and tlg of one region"""
    at = labels == value
    if keep is not None:
        at &= np.asarray(keep) != 0
    n = int(at.sum())
    mean = float(np.asarray(x, dtype=np.float64)[at].sum() / n)
    volume_ml = n * float(spacing[0]) * float(spacing[1]) * float(spacing[2]) / 1000.0
    return {"n": n, "mean": mean, "volume_ml": volume_ml, "tlg": volume_ml * mean}


def data(shape, seed, offset=0.0, batch=None):
    """fp32 noise of both signs (standard normal) on an offset"""
    rng = np.random.default_rng(seed)
    full = shape if batch is None else (batch,) + tuple(shape)
    return (rng.standard_normal(full) + offset).astype(np.float32)


def keep_mask(shape, radii, seed):
    """uint8: 60 % of the voxels at random, and a block of zeros at the origin corner that is larger than the
    footprint (r + 2 per axis, or the whole extent), so that the voxels next to the corner count nothing"""
    rng = np.random.default_rng(seed)
    keep = (rng.random(shape) < 0.6).astype(np.uint8)
    keep[tuple(slice(0, r + 2) for r in radii)] = 0
    return keep


@functools.lru_cache(maxsize=None)
def case(shape, spacing, offset, masked, batch=None, seed=0):
    """one shared, read-only reference: (x, keep or None, [(mean, n, bound) per volume])"""
    fp = footprint(spacing)
    x = data(shape, seed + 7, offset, batch)
    keep = keep_mask(shape, trimmed(fp)[1], seed + 11) if masked else None
    ref = [sphere_mean(v, fp, keep) for v in (x if batch else [x])]
    for a in (x, keep) + tuple(r for t in ref for r in t):
        if a is not None:
            a.setflags(write=False)
    return x, keep, ref
