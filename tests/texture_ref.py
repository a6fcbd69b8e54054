"""
A numpy restatement of the per-region texture definition of include/ddpm3d.h (ddpm3d_roi_texture),
written from the definition and not from the kernel: the fp32 binning expression, 13 shifted slice pairs and
np.add.at for the co-occurrence matrix, and Haralick's figures as IBSI defines them in fp64.  figures() returns, beside
every figure, the sum of the absolute values of the terms it was summed from: what an error bound on another
summation order of the same terms is a multiple of.
"""

import itertools
import math

import numpy as np

# the offsets (dz, dy, dx) in {-1, 0, 1}^3 lexicographically above (0, 0, 0): distance 1, half the 26-neighbourhood
DIRECTIONS = [d for d in itertools.product((-1, 0, 1), repeat=3) if d > (0, 0, 0)]
N, BELOW, ABOVE, PAIRS, REC = range(5)


def grey_levels(x, lo, inv_w, levels):
    """-> (g, counted, below, above) of a float32 array: g = min(max(floor((x - lo) * inv_w), 0), levels - 1) with the
    subtraction and the product each rounded to fp32; a NaN product is not counted; below / above flag the counted
    values whose unclamped bin is < 0 / >= levels (decided on the floored float, so +-inf is safe)"""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (x - np.float32(lo)).astype(np.float32) * np.float32(inv_w)
    assert t.dtype == np.float32
    counted = ~np.isnan(t)
    f = np.floor(np.where(counted, t, np.float32(0)))
    below = counted & (f < 0)
    above = counted & (f >= levels)
    g = np.where(below, 0, np.where(above, levels - 1, np.where(below | above, 0, f))).astype(np.int64)
    return g, counted, below, above


def _pair(n, d):
    """slices (lower voxel, its neighbour at +d) along an axis of length n"""
    if d == 0:
        return slice(0, n), slice(0, n)
    if d == 1:
        return slice(0, n - 1), slice(1, n)
    return slice(1, n), slice(0, n - 1)


def region_texture(vol, member, lo, inv_w, levels):
    """(glcm [levels, levels], hist [levels], counts [REC]) int64 of the voxels of `vol` where `member` is True"""
    g, counted, below, above = grey_levels(vol, lo, inv_w, levels)
    use = counted & member
    glcm = np.zeros((levels, levels), dtype=np.int64)
    pairs = 0
    for d in DIRECTIONS:
        a, b = zip(*[_pair(n, dd) for n, dd in zip(vol.shape, d)])
        both = use[a] & use[b]
        ga, gb = g[a][both], g[b][both]
        np.add.at(glcm, (ga, gb), 1)
        np.add.at(glcm, (gb, ga), 1)
        pairs += int(both.sum())
    hist = np.bincount(g[use], minlength=levels).astype(np.int64)
    counts = np.array([use.sum(), (below & member).sum(), (above & member).sum(), pairs], dtype=np.int64)
    return glcm, hist, counts


def roi_texture(est, labels, lo, inv_w, levels, found=None):
    """est (D, H, W) or (B, D, H, W) float32, labels (D, H, W) ints (0 = none; regions are the values of `found`,
    default the distinct positive labels in ascending order), lo and inv_w [B][R] -> glcm [B, R, levels, levels],
    hist [B, R, levels], counts [B, R, REC], int64"""
    est = np.asarray(est, dtype=np.float32)
    est = est[None] if est.ndim == 3 else est
    found = [int(v) for v in np.unique(labels[labels > 0])] if found is None else list(found)
    B, R = est.shape[0], len(found)
    lo = np.broadcast_to(np.asarray(lo, dtype=np.float32), (B, R))
    inv_w = np.broadcast_to(np.asarray(inv_w, dtype=np.float32), (B, R))
    glcm = np.zeros((B, R, levels, levels), dtype=np.int64)
    hist = np.zeros((B, R, levels), dtype=np.int64)
    counts = np.zeros((B, R, REC), dtype=np.int64)
    for b in range(B):
        for r, label in enumerate(found):
            glcm[b, r], hist[b, r], counts[b, r] = region_texture(est[b], labels == label, lo[b, r], inv_w[b, r],
                                                                  levels)
    return glcm, hist, counts


FIGURES = ("joint_entropy", "angular_second_moment", "contrast", "dissimilarity", "inverse_difference",
           "inverse_difference_moment", "joint_average", "joint_variance", "correlation", "hist_entropy",
           "hist_uniformity", "p10", "p50", "p90", "clamped")


def figures(glcm, hist, counts, lo, inv_w):
    """-> (figures, sums): the figures of one region in fp64 from its integer matrices, None for each when the region
    has no pair, and per figure the sum of |terms| (see the module docstring)"""
    levels = glcm.shape[0]
    n, pairs = int(counts[N]), int(counts[PAIRS])
    out, mag = {"n": n, "pairs": pairs}, {"n": 0.0, "pairs": 0.0}
    if pairs == 0:
        out.update({k: None for k in FIGURES})
        return out, mag
    total = int(glcm.sum())
    assert total == 2 * pairs
    terms = {k: [] for k in FIGURES}
    mu = math.fsum(i * int(glcm[i, j]) / total for i in range(levels) for j in range(levels))
    for i in range(levels):
        for j in range(levels):
            p = int(glcm[i, j]) / total
            if p > 0:
                terms["joint_entropy"].append(-p * math.log2(p))
            terms["angular_second_moment"].append(p * p)
            terms["contrast"].append((i - j) ** 2 * p)
            terms["dissimilarity"].append(abs(i - j) * p)
            terms["inverse_difference"].append(p / (1 + abs(i - j)))
            terms["inverse_difference_moment"].append(p / (1 + (i - j) ** 2))
            terms["joint_average"].append(i * p)
            terms["joint_variance"].append((i - mu) ** 2 * p)
            terms["correlation"].append(i * j * p)
    for g in range(levels):
        q = int(hist[g]) / n
        if q > 0:
            terms["hist_entropy"].append(-q * math.log2(q))
        terms["hist_uniformity"].append(q * q)
    for k in ("joint_entropy", "angular_second_moment", "contrast", "dissimilarity", "inverse_difference",
              "inverse_difference_moment", "joint_average", "joint_variance", "hist_entropy", "hist_uniformity"):
        out[k], mag[k] = math.fsum(terms[k]), math.fsum(abs(t) for t in terms[k])
    var, sij = out["joint_variance"], math.fsum(terms["correlation"])
    if var == 0:
        out["correlation"], mag["correlation"] = None, 0.0
    else:
        # the numerator's two parts each carry a relative error (the square of mu twice its own), and so does var
        out["correlation"] = (sij - mu * mu) / var
        mag["correlation"] = (sij + 2 * mu * mu) / var + abs(out["correlation"])
    cum = 0
    want = [10, 50, 90]
    for g in range(levels):
        cum += int(hist[g])
        while want and cum * 100 >= want[0] * n:
            pct = want.pop(0)
            if float(inv_w) == 0:
                out["p%d" % pct], mag["p%d" % pct] = None, 0.0
            else:
                out["p%d" % pct] = float(lo) + (g + 0.5) / float(inv_w)
                mag["p%d" % pct] = abs(float(lo)) + (g + 0.5) / float(inv_w)
    out["clamped"] = (int(counts[BELOW]) + int(counts[ABOVE])) / n
    mag["clamped"] = out["clamped"]
    return out, mag


def phantom(seed=0):
    """the 24 x 40 x 40 phantom of the feature's motivation: a Gaussian blob of amplitude 0.3 on 0.5, the same with
    noise of sigma 0.1, and the box region [6:18, 10:30, 10:30] -> (clean, noisy, labels)"""
    z, y, x = np.meshgrid(np.arange(24), np.arange(40), np.arange(40), indexing="ij")
    clean = (0.5 + 0.3 * np.exp(-((z - 12) ** 2 + (y - 20) ** 2 + (x - 20) ** 2) / (2 * 5.0 ** 2))).astype(np.float32)
    noisy = (clean + 0.1 * np.random.default_rng(seed).standard_normal(clean.shape)).astype(np.float32)
    labels = np.zeros(clean.shape, dtype=np.int32)
    labels[6:18, 10:30, 10:30] = 1
    return clean, noisy, labels
