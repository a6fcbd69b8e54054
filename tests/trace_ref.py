"""
The numpy fp64 yardstick of the per-step convergence trace (include/ddpm3d.h has the columns):
ddpm3d_trace_moments' records with every term formed as the kernel forms it (the fp32 values widened to double,
e = x - y, d = x - p, w * (e * e): at most three roundings per term) and summed by numpy, together with the sum
of |term| per column that the GPU tier's bound is taken from:

    |got - ref| <= (n + 8) * 2^-52 * sum |term|,   n = the number of counted voxels,

which holds for any two summation orders of terms that carry at most three roundings each.  No GPU is touched here.
"""

import numpy as np

(W, N, SUM_E, SUM_ABS_E, SUM_SQ_E, SUM_SQ_Y, SUM_X, SUM_SQ_X, SUM_SQ_D, CLIPPED, REC) = range(11)
NEEDS_TARGET = (SUM_E, SUM_ABS_E, SUM_SQ_E, SUM_SQ_Y)


def moments(est, prev=None, target=None, weight=None):
    """est (B, voxels) fp32; prev (B, voxels) or None; target / weight (voxels,) shared, (B, voxels) own, or None.
    -> (records (B, REC) fp64, magnitudes (B, REC) fp64: the sum of |term| of every column).  Only voxels with
    weight > 0 enter a term, so whatever the others hold (NaN, inf) is never touched."""
    est = np.asarray(est)
    assert est.ndim == 2 and est.dtype == np.float32
    B, voxels = est.shape
    rec, mag = np.zeros((B, REC)), np.zeros((B, REC))

    def row(a, b):
        if a is None:
            return None
        a = np.asarray(a)
        assert a.dtype == np.float32 and a.shape in ((voxels,), (B, voxels))
        return a if a.ndim == 1 else a[b]

    for b in range(B):
        w = row(weight, b)
        on = np.ones(voxels, dtype=bool) if w is None else w > 0
        wd = np.ones(int(on.sum())) if w is None else w[on].astype(np.float64)
        x = est[b][on].astype(np.float64)
        terms = {W: wd, N: np.ones_like(wd), SUM_X: wd * x, SUM_SQ_X: wd * (x * x),
                 CLIPPED: np.where(np.abs(x) >= 1.0, wd, 0.0)}
        y = row(target, b)
        if y is not None:
            y = y[on].astype(np.float64)
            e = x - y
            terms.update({SUM_E: wd * e, SUM_ABS_E: wd * np.abs(e), SUM_SQ_E: wd * (e * e), SUM_SQ_Y: wd * (y * y)})
        if prev is not None:
            d = x - np.asarray(prev)[b][on].astype(np.float64)
            terms[SUM_SQ_D] = wd * (d * d)
        for k, v in terms.items():
            rec[b, k] = v.sum()
            mag[b, k] = np.abs(v).sum()
    return rec, mag


def bound(rec, mag):
    """the GPU tier's per-column bound for records of these magnitudes"""
    return (rec[:, N:N + 1] + 8.0) * 2.0 ** -52 * mag


def make_case(B, voxels, seed, own_target=True, own_weight=True):
    """seeded inputs of one case: estimates around a target in [-1.2, 1.2] (some |x| >= 1), a previous estimate,
    weights in (0, 1] with about a third exact zeros, and NaN / inf in est, prev and target at weight-0 voxels."""
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    target = f32(rng.uniform(-1.2, 1.2, (B, voxels) if own_target else (voxels,)))
    est = f32(target + 0.1 * rng.standard_normal((B, voxels)))
    prev = f32(est + 0.05 * rng.standard_normal((B, voxels)))
    weight = f32(rng.uniform(0.01, 1.0, (B, voxels) if own_weight else (voxels,)))
    weight[rng.random(weight.shape) < 1.0 / 3.0] = 0.0
    return est, prev, target, weight


def poison(est, prev, target, weight):
    """copies with NaN / inf wherever every estimate's weight is 0"""
    est, prev, target = est.copy(), prev.copy(), target.copy()
    off = weight == 0
    off_all = off if off.ndim == 2 else np.broadcast_to(off, est.shape)
    est[off_all] = np.nan
    prev[off_all] = np.inf
    if target.ndim == 2:
        target[off_all] = -np.inf
    elif off.ndim == 1:
        target[off] = np.nan
    else:
        target[off.all(axis=0)] = np.nan
    return est, prev, target
