"""
Host yardstick of the per-region moments: the fp64 terms ddpm3d_roi_moments forms -- (double)x,
x * x (exact in fp64 for an fp32 x), e = (double)x - (double)y, |e| and e * e (one IEEE rounding each, the same on
both sides) -- summed exactly with math.fsum.  The
kernel's terms are these bit for bit; only its order of summation differs, so a sum column of n terms may deviate by
at most n * 2^-53 * sum |term| (bound()): derived, not measured.  N, MIN_X and MAX_X must be equal.
"""

import math

import numpy as np

N, SUM_X, SUM_SQ_X, MIN_X, MAX_X, SUM_E, SUM_ABS_E, SUM_SQ_E, REC = range(9)
SUMS = (SUM_X, SUM_SQ_X, SUM_E, SUM_ABS_E, SUM_SQ_E)
CHUNK = 4096
SHAPE = (24, 20, 28)                   # 13 440 voxels, odd extents against the 256-thread passes
SIZES = {1: 1, 2: 1, 7: 4095, 300: 4096, 4000: 4097}      # label: voxels; one below, at and above a chunk


def region_lists(labels, keep=None):
    """(ascending positive labels, per label the ascending flat indices of its voxels) as np.nonzero finds them"""
    flat = np.asarray(labels).reshape(-1)
    if keep is not None:
        flat = np.where(np.asarray(keep).reshape(-1) != 0, flat, 0)
    found = [int(v) for v in np.unique(flat) if v > 0]
    return found, [np.nonzero(flat == v)[0].astype(np.int64) for v in found]


def _terms(x, at, y):
    xs = np.asarray(x, dtype=np.float32).reshape(-1)[at].astype(np.float64)
    cols = {SUM_X: xs, SUM_SQ_X: xs * xs}
    if y is not None:
        e = xs - np.asarray(y, dtype=np.float32).reshape(-1)[at].astype(np.float64)
        cols.update({SUM_E: e, SUM_ABS_E: np.abs(e), SUM_SQ_E: e * e})
    return xs, cols


def moments(x, lists, y=None):
    """the R records of one estimate: exact sums of the kernel's own fp64 terms"""
    out = []
    for at in lists:
        xs, cols = _terms(x, at, y)
        rec = [0.0] * REC
        rec[N] = float(len(at))
        rec[MIN_X] = float(xs.min()) if len(at) else math.inf
        rec[MAX_X] = float(xs.max()) if len(at) else -math.inf
        for k, t in cols.items():
            rec[k] = math.fsum(t.tolist())
        out.append(rec)
    return out


def bound(x, lists, y=None):
    """per region and sum column: n * 2^-53 * sum |term|"""
    out = []
    for at in lists:
        _, cols = _terms(x, at, y)
        b = [0.0] * REC
        for k, t in cols.items():
            b[k] = len(at) * 2.0 ** -53 * math.fsum(np.abs(t).tolist())
        out.append(b)
    return out


def check(got, want, bounds):
    """records of one estimate against the yardstick's: counts and extremes equal, sums within their bound"""
    assert len(got) == len(want) == len(bounds)
    for r, (g, w, b) in enumerate(zip(got, want, bounds)):
        assert g[N] == w[N] and g[MIN_X] == w[MIN_X] and g[MAX_X] == w[MAX_X], (r, g, w)
        for k in SUMS:
            assert abs(g[k] - w[k]) <= b[k], (r, k, g[k], w[k], b[k])


def stats(rec):
    """n, mean, population std, min, max of one record"""
    n = int(rec[N])
    mean = rec[SUM_X] / n
    return n, mean, math.sqrt(max(rec[SUM_SQ_X] / n - mean * mean, 0.0)), rec[MIN_X], rec[MAX_X]


def labels_volume(scattered, seed=5):
    """SHAPE labels with SIZES: label 1 is flat index 0, label 2 the last voxel, the others either contiguous runs of
    flat indices or a seeded permutation of them (a scattered gather)"""
    n = int(np.prod(SHAPE))
    flat = np.zeros(n, dtype=np.int32)
    flat[0], flat[n - 1] = 1, 2
    free = np.arange(1, n - 1)
    if scattered:
        free = np.random.default_rng(seed).permutation(free)
    start = 0
    for label in (7, 300, 4000):
        flat[free[start:start + SIZES[label]]] = label
        start += SIZES[label] + (0 if scattered else 3)
    assert start <= free.size
    return flat.reshape(SHAPE)


def volumes(offset=0.0, seed=1):
    """three estimates and a target on SHAPE, fp32, terms of both signs unless on an offset"""
    rng = np.random.default_rng(seed)
    y = (rng.standard_normal(SHAPE) + offset).astype(np.float32)
    xs = np.stack([(y + s * rng.standard_normal(SHAPE)).astype(np.float32) for s in (0.05, 0.2, 0.7)])
    return xs, y


def report_volumes(labels, seed=2):
    """PET-like data for the figures: a positive target with an uptake per region (label 7 a hot lesion, 300 the
    reference organ), three estimates with noise and a bias of 0.1, 0.2 and 0.3 of their own"""
    rng = np.random.default_rng(seed)
    uptake = np.select([labels == 7, labels == 300, labels == 4000, labels == 1, labels == 2], [6.0, 2.0, 3.5, 4.0, 1.0],
                       1.0)
    y = (uptake * (1.0 + 0.1 * rng.standard_normal(SHAPE))).astype(np.float32)
    xs = np.stack([(y + 0.1 * (i + 1) + s * rng.standard_normal(SHAPE)).astype(np.float32)
                   for i, s in enumerate((0.05, 0.2, 0.4))])
    return xs, y
