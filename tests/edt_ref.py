"""
Yardstick of the distance transform and the lesion boundary figures, numpy + scipy on the host:
distance_sq is scipy.ndimage.distance_transform_edt on the fp32-rounded spacings, squared, in fp64; brute is the fp64
all-pairs minimum that pins it without scipy; emulate restates the three fp32 passes of include/ddpm3d.h with full
(unpruned) minima, which is what the 5-rounding bound is about; surface, boundary and edge_profile restate the
definitions of guided_diffusion/metrics.py with scipy.ndimage.binary_erosion and numpy.percentile.  Nothing here is
shared with the code under test.
"""

import math

import numpy as np
from scipy import ndimage

U = 2.0 ** -24
BOUND = (1.0 + U) ** 5 - 1.0            # relative, of every finite squared distance (include/ddpm3d.h)
# of a distance in mm as the consumers form it, and of their means and percentiles: the root of a square within
# (1 + u)^5 lies within (1 + u)^2.5, the fp32 root rounds once more, and half a unit is left for the fp64 sums and the
# interpolation, whose roundings are 2^-29 of that
BOUND_MM = (1.0 + U) ** 4 - 1.0
SPACINGS = ((3.27, 2.0, 2.0), (0.7, 1.3, 2.9), (5.0, 1.0, 1.0))


def rounded(spacing):
    """the spacings as the kernel sees them: fp32 values, as fp64 numbers"""
    return tuple(float(np.float32(s)) for s in spacing)


def foreground(mask, invert=False):
    return (np.asarray(mask) != 0) != bool(invert)


def distance_sq(mask, spacing, invert=False):
    """fp64 squared distance in mm^2 to the nearest background voxel; +inf everywhere without one.  scipy names the
    nearest background voxel; the squared distance to it is formed here, without scipy's root in between, so that it is
    the exact integer at unit spacing"""
    fg = foreground(mask, invert)
    if fg.all():
        return np.full(fg.shape, np.inf)
    s = rounded(spacing)
    nearest = ndimage.distance_transform_edt(fg, sampling=s, return_distances=False, return_indices=True)
    grid = np.indices(fg.shape)
    return sum(((nearest[a] - grid[a]) * s[a]) ** 2 for a in range(3))


def brute(mask, spacing, invert=False):
    """the same by the definition: the minimum over all background voxels, in fp64; for a few thousand voxels"""
    fg = foreground(mask, invert)
    s = np.array(rounded(spacing))
    at = np.argwhere(fg) * s
    to = np.argwhere(~fg) * s
    out = np.zeros(fg.shape)
    if len(to) == 0:
        out[...] = np.inf
    elif len(at):
        out[fg] = ((at[:, None, :] - to[None, :, :]) ** 2).sum(axis=2).min(axis=1)
    return out


def _line_pass(f, axis, s):
    """f1(y) = min over y' of fma(a, a, f(y')), a = s * (float)(y - y'), along `axis`; the fma in fp64 rounded once
    (a * a is exact in fp64, the sum of two fp64 numbers rounds to fp64 first: a double rounding that can differ from
    a true fma in the last fp32 bit only in a tie, which the bound does not notice)"""
    f = np.moveaxis(f, axis, 0)
    n = f.shape[0]
    out = np.full(f.shape, np.inf, dtype=np.float32)
    for y in range(n):
        for y2 in range(n):
            a = np.float32(s) * np.float32(y - y2)
            with np.errstate(over="ignore"):
                cand = (np.float64(a) * np.float64(a) + f[y2].astype(np.float64)).astype(np.float32)
            out[y] = np.minimum(out[y], cand)
    return np.moveaxis(out, 0, axis)


def emulate(mask, spacing, invert=False):
    """the three passes of include/ddpm3d.h in fp32, every minimum taken over the whole line -> float32"""
    fg = foreground(mask, invert)
    s = [np.float32(v) for v in spacing]
    D, H, W = fg.shape
    x = np.arange(W)
    f0 = np.full(fg.shape, np.inf, dtype=np.float32)
    for d in range(D):
        for h in range(H):
            bg = np.nonzero(~fg[d, h])[0]
            if len(bg):
                n = np.abs(x[:, None] - bg[None, :]).min(axis=1)
                t = s[2] * n.astype(np.float32)
                f0[d, h] = t * t
    return _line_pass(_line_pass(f0, 1, s[1]), 0, s[0])


def random_mask(shape, density, seed):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def share_of_bound(got, want):
    """the largest relative error of the finite outputs in units of BOUND; infinities and zeros must agree exactly"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    assert np.array_equal(np.isinf(got), np.isinf(want)) and np.array_equal(got == 0, want == 0)
    assert not np.isnan(got).any()
    live = np.isfinite(want) & (want > 0)
    if not live.any():
        return 0.0
    return float((np.abs(got[live] - want[live]) / want[live]).max() / BOUND)


# ------------------------------------------------------------------------------------------ the consumers
def surface(mask):
    m = np.asarray(mask) != 0
    return m & ~ndimage.binary_erosion(m, border_value=0)


def _to_surface(surf, spacing):
    """mm from every voxel to the nearest voxel of `surf`; +inf without one"""
    return np.sqrt(distance_sq(surf, spacing, invert=True))


def boundary(target_labels, estimate_labels, spacing):
    """-> (figures as metrics.boundary returns them, the two directed value sets {"t": ..., "e": ...} for the tests)"""
    t, e = np.asarray(target_labels), np.asarray(estimate_labels)
    tf, ef = t > 0, e > 0
    ts, es = surface(tf), surface(ef)
    n_t, n_e, both = int(tf.sum()), int(ef.sum()), int((tf & ef).sum())
    out = {"dice": 2.0 * both / (n_t + n_e), "jaccard": both / (n_t + n_e - both), "hd_mm": None, "hd95_mm": None,
           "assd_mm": None, "n_surface_target": int(ts.sum()), "n_surface_estimate": int(es.sum()), "regions": {}}
    labels = [int(v) for v in np.unique(t) if v > 0]
    if n_e == 0:
        for v in labels:
            out["regions"][v] = {"surface_mean_mm": None, "surface_p95_mm": None, "surface_max_mm": None}
        return out, {"t": np.zeros(0), "e": np.zeros(0)}
    to_e, to_t = _to_surface(es, spacing), _to_surface(ts, spacing)
    dt, de = to_e[ts], to_t[es]                 # target -> estimate, estimate -> target
    out["hd_mm"] = float(max(dt.max(), de.max()))
    out["hd95_mm"] = float(max(np.percentile(dt, 95, method="linear"), np.percentile(de, 95, method="linear")))
    out["assd_mm"] = float((math.fsum(dt) + math.fsum(de)) / (len(dt) + len(de)))
    for v in labels:
        d = to_e[ts & (t == v)]
        out["regions"][v] = {"surface_mean_mm": float(math.fsum(d) / len(d)),
                             "surface_p95_mm": float(np.percentile(d, 95, method="linear")),
                             "surface_max_mm": float(d.max())}
    return out, {"t": dt, "e": de}


def shells(labels, spacing, width, inside, outside):
    """-> (shell number per voxel: 1 .. inside + outside from the innermost outward, 0 for none; the smallest relative
    gap between a distance and a shell edge it is compared with)"""
    fg = np.asarray(labels) > 0
    d_in, d_out = np.sqrt(distance_sq(fg, spacing)), np.sqrt(distance_sq(fg, spacing, invert=True))
    out = np.zeros(fg.shape, dtype=np.int32)
    gap = np.inf
    for d, count, number in ((d_in, inside, lambda i: inside - i), (d_out, outside, lambda o: inside + 1 + o)):
        for i in range(count):
            out[(d > i * width) & (d <= (i + 1) * width)] = number(i)
        live = d[np.isfinite(d) & (d > 0)]
        for edge in range(1, count + 1):
            if len(live):
                gap = min(gap, float((np.abs(live - edge * width) / (edge * width)).min()))
    return out, gap


def edge_profile(volumes, labels, spacing, width, inside=3, outside=5, keep=None):
    number, _ = shells(labels, spacing, width, inside, outside)
    if keep is not None:
        number = np.where(np.asarray(keep) != 0, number, 0)
    rows = []
    for j in range(1, inside + outside + 1):
        at = number == j
        n = int(at.sum())
        rows.append({"distance_mm": (j - inside - 0.5) * width, "n": n,
                     "mean": {name: (math.fsum(np.asarray(v, dtype=np.float64)[at]) / n if n else None)
                              for name, v in volumes.items()}})
    return {"width_mm": float(width), "inside": inside, "outside": outside, "rows": rows}


def blobs(shape=(20, 26, 36)):
    """(target labels, estimate labels, target volume, estimate volume): a ball and an ellipsoid; the
    estimate misses the first and has the second shifted by one voxel along H"""
    z, y, x = np.indices(shape)
    t = np.zeros(shape, dtype=np.int32)
    e = np.zeros(shape, dtype=np.int32)
    t[(z - 5) ** 2 + (y - 6) ** 2 + (x - 7) ** 2 <= 9] = 1
    big = (z - 11) ** 2 / 25.0 + (y - 15) ** 2 / 36.0 + (x - 22) ** 2 / 64.0 <= 1.0
    t[big] = 2
    e[np.roll(big, 1, axis=1)] = 1
    return t, e, np.where(t > 0, 4.0, 1.0).astype(np.float32), np.where(e > 0, 3.5, 1.0).astype(np.float32)


def phantom_rows(seed=4):
    """the 24 x 40 x 40 phantom's clean, noisy and Gaussian-filtered volumes (the README's table)"""
    import metrics_ref
    clean = metrics_ref.phantom((24, 40, 40), seed=seed)
    low = metrics_ref.noisy(clean, 0.1, seed=seed)
    return clean, low, ndimage.gaussian_filter(low.astype(np.float64), 1.0).astype(np.float32)
