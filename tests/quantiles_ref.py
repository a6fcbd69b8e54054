"""
numpy fp64 restatement of ddpm3d_draw_quantiles (include/ddpm3d.h): the per-voxel quantiles of K draws with
numpy.quantile's method "linear" and the rank of a target among them.  The draws are the fp32 values the kernel sorts:
acc[d] / wsum as one correctly rounded fp32 division (numpy's), or the plain stack.
"""

import numpy as np

NOT_COUNTED = 255


def draws_of(acc, weight=None):
    """(K, n) fp32 accumulators [/ (n,) fp32 weight] -> the (K, n) fp32 draws; a voxel of weight <= 0 keeps its
    accumulators (it is not counted)"""
    acc = np.asarray(acc, dtype=np.float32)
    if weight is None:
        return acc
    w = np.where(weight > 0, weight, np.float32(1)).astype(np.float32)
    return (acc / w[None]).astype(np.float32)


def quantiles(acc, levels, weight=None):
    """-> (nq, n) fp64: np.quantile(method="linear") over the draw axis; 0 where the weight is <= 0, NaN where a draw
    is NaN"""
    x = draws_of(acc, weight).astype(np.float64)
    with np.errstate(invalid="ignore"):
        out = np.quantile(x, np.asarray(levels, dtype=np.float64), axis=0, method="linear")
    if weight is not None:
        out[:, ~(weight > 0)] = 0.0
    return out


def neighbours(acc, levels, weight=None):
    """-> (s_lo, s_hi, frac), each (nq, n): the two order statistics quantile i interpolates between and its fp64
    fraction (s_hi = s_lo where frac == 0)"""
    x = np.sort(draws_of(acc, weight).astype(np.float64), axis=0)
    K = x.shape[0]
    lo, hi, fr = [], [], []
    for q in levels:
        h = float(q) * (K - 1)
        j = min(int(np.floor(h)), K - 1)
        f = h - j
        lo.append(x[j])
        hi.append(x[min(j + 1, K - 1)] if f else x[j])
        fr.append(np.full(x.shape[1], f))
    return np.stack(lo), np.stack(hi), np.stack(fr)


def ranks(acc, target, weight=None):
    """-> (below, equal) uint8 (n,): #{d : x_d < t}, #{d : x_d == t}; 255 in both where the weight is <= 0, a draw is
    NaN or the target is NaN"""
    x = draws_of(acc, weight)
    t = np.asarray(target, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        below = (x < t[None]).sum(axis=0)
        equal = (x == t[None]).sum(axis=0)
    out = np.isnan(x).any(axis=0) | np.isnan(t)
    if weight is not None:
        out |= ~(weight > 0)
    below[out] = NOT_COUNTED
    equal[out] = NOT_COUNTED
    return below.astype(np.uint8), equal.astype(np.uint8)


def rank_histogram(below, equal, K, mask=None):
    """np.bincount of the untied counted voxels' ranks -> {"counts", "ties", "n"}"""
    counted = below != NOT_COUNTED
    if mask is not None:
        counted &= mask != 0
    tied = counted & (equal > 0)
    counts = np.bincount(below[counted & ~tied].astype(np.int64), minlength=K + 1)
    return {"counts": [int(c) for c in counts], "ties": int(tied.sum()), "n": int(counts.sum() + tied.sum())}
