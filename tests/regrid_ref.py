"""
The fp64 yardstick of volume regridding, written apart from guided_diffusion/regrid.py: the tap
tables of one axis from their definition, the regridding of a volume pass by pass (W, H, D) on the fp32-rounded
weights, the composed rounding bound of the device's fma chains, and what the tables predict for a NaN and for a mask
of counted voxels.

Per pass, for an output with n counted taps, |y - sum w x| <= gamma_n sum |w| |x| with gamma_n = n u / (1 - n u),
u = 2^-24 (one rounding for the product, one per fma).  Across passes, with m_j the exact chain and e_j the bound on
the device's distance from it after pass j (e_0 = 0: the input is fp32),
    e_j = |W_j| e_{j-1} + gamma_{n_j} |W_j| (|m_{j-1}| + e_{j-1})
evaluated numerically by applying |W_j| to the absolute values.
"""

import math

import numpy as np

U = 2.0 ** -24
SUPPORT = {"linear": 1, "cubic": 2}
MAX_TAPS = 18


def gamma(n):
    n = np.asarray(n, dtype=np.float64)
    return n * U / (1.0 - n * U)


def kernel(mode, x):
    x = abs(x)
    if mode == "linear":
        return 1.0 - x if x < 1.0 else 0.0
    if mode != "cubic":
        raise ValueError(mode)
    a = -0.5
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    if x < 2.0:
        return (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return 0.0


def table(Li, Lo, mode):
    """(first [Lo], count [Lo], rows: Lo lists of fp64 weights that sum to 1) of the axis Li -> Lo; None for Li == Lo"""
    if Li == Lo:
        return None
    S = SUPPORT[mode]
    scale = Li / Lo
    fs = max(1.0, scale)
    first, count, rows = [], [], []
    for o in range(Lo):
        c = (o + 0.5) * scale
        lo = max(0, int(c - S * fs + 0.5))
        hi = min(Li, int(c + S * fs + 0.5))
        w = [kernel(mode, (k + 0.5 - c) / fs) for k in range(lo, hi)]
        total = math.fsum(w)
        first.append(lo), count.append(hi - lo), rows.append([v / total for v in w])
    return first, count, rows


def matrix(Li, Lo, mode, rounded=True):
    """The axis map as a dense [Lo][Li] fp64 matrix (weights rounded once to fp32 first unless rounded=False), and the
    counted taps per row"""
    t = table(Li, Lo, mode)
    if t is None:
        return np.eye(Li), np.ones(Lo, dtype=np.int64)
    first, count, rows = t
    M = np.zeros((Lo, Li), dtype=np.float64)
    for o in range(Lo):
        w = np.asarray(rows[o], dtype=np.float64)
        M[o, first[o]:first[o] + count[o]] = w.astype(np.float32).astype(np.float64) if rounded else w
    return M, np.asarray(count, dtype=np.int64)


def _along(M, x, axis):
    return np.moveaxis(np.tensordot(M, x, axes=([1], [axis])), 0, axis)


def apply(x, shape_out, mode="linear", rounded=True):
    """x (..., D, H, W) on shape_out, in fp64, passes W, H, D -> (m, bound) with bound the composed e of the head"""
    m = np.asarray(x, dtype=np.float64)
    e = np.zeros_like(m)
    for axis, Lo in ((-1, shape_out[2]), (-2, shape_out[1]), (-3, shape_out[0])):
        Li = m.shape[axis]
        if Li == Lo:
            continue
        M, n = matrix(Li, Lo, mode, rounded)
        A = np.abs(M)
        g = gamma(n).reshape([-1 if a == axis % m.ndim else 1 for a in range(m.ndim)])
        mag = np.abs(m) + e
        e = _along(A, e, axis) + g * _along(A, mag, axis)
        m = _along(M, m, axis)
    return m, e


def counted(Li, Lo, mode):
    """[Lo][Li] bool: input k is one of output o's counted taps (zero weights included: 0 * NaN is NaN)"""
    t = table(Li, Lo, mode)
    if t is None:
        return np.eye(Li, dtype=bool)
    first, count, _ = t
    C = np.zeros((Lo, Li), dtype=bool)
    for o in range(Lo):
        C[o, first[o]:first[o] + count[o]] = True
    return C


def _spread(mask, shape_out, mode, reach):
    m = np.asarray(mask, dtype=np.float64)
    for axis, Lo in ((-1, shape_out[2]), (-2, shape_out[1]), (-3, shape_out[0])):
        m = (_along(reach(m.shape[axis], Lo, mode).astype(np.float64), m, axis) > 0).astype(np.float64)
    return m > 0


def nonfinite_after(bad, shape_out, mode):
    """bool (D, H, W) of non-finite inputs -> the outputs that read at least one of them"""
    return _spread(bad, shape_out, mode, counted)


def nonzero(Li, Lo, mode):
    """[Lo][Li] bool: input k enters output o with a non-zero fp32 tap"""
    return matrix(Li, Lo, mode)[0] != 0


def keep_after(keep, shape_out, mode):
    """uint8 (D, H, W) mask of counted voxels -> the mask on shape_out: an output is counted iff every input that
    enters it with a non-zero tap is"""
    return (~_spread(np.asarray(keep) == 0, shape_out, mode, nonzero)).astype(np.uint8)


def data(shape, seed, offset=0.0):
    rng = np.random.default_rng(seed)
    return (rng.random(shape, dtype=np.float32) + np.float32(offset)).astype(np.float32)
