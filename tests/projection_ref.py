"""
The yardstick of ddpm3d_project (include/ddpm3d.h): a numpy fp64 restatement of the definition,
evaluated from the fp32 table the kernel reads.  Per output it returns the value, the header's error bound and the
"ambiguous" flag: an output one of whose samples has a rounded coordinate within max(2^-12 voxel, its error) of a face
of the counting box, so that the device may count it where the yardstick does not, or the reverse.
"""

import numpy as np

U32 = 2.0 ** -24
AMBIGUOUS = 2.0 ** -12


def _exact_f32(x):
    """where the fp64 values are fp32 numbers (an fma whose exact result is one does not round)"""
    return x.astype(np.float32).astype(np.float64) == x


def _coordinate(coef3, u, j):
    """origin, per-u and per-j increment (fp32) -> the fp64 coordinate (U, R), the device's error bound e on it
    (0 where neither fma rounds) and the flag `rounded`"""
    o, du, dj = (float(np.float32(v)) for v in coef3)
    t = j[None, :] * dj + o                      # an integer below 2^12 times an fp32 number is exact in fp64
    c = u[:, None] * du + t
    exact = _exact_f32(t) & _exact_f32(c)
    e = np.where(exact, 0.0, U32 * (np.abs(t) + np.abs(c)) * (1.0 + U32))
    return c, e, ~exact


def _neighbourhood_max(a, axis_h, axis_w):
    """the largest entry of `a` over index offsets -1..1 along both named axes (edges replicate)"""
    out = a
    for axis in (axis_h, axis_w):
        n = out.shape[axis]
        idx = np.arange(n)
        lo = np.take(out, np.maximum(idx - 1, 0), axis=axis)
        hi = np.take(out, np.minimum(idx + 1, n - 1), axis=axis)
        out = np.maximum(out, np.maximum(lo, hi))
    return out


def _cell_tables(vol):
    """per cell (y, x) of every slice, over the cell's corners and those of the cells that touch it: G_h, G_w (the
    largest |difference| of two voxels adjacent along H, W) and A (the largest |voxel|); (..., H, W) each, with the
    upper index clamped as the kernel clamps it"""
    H, W = vol.shape[-2:]
    y1 = np.minimum(np.arange(H) + 1, H - 1)
    x1 = np.minimum(np.arange(W) + 1, W - 1)
    v = np.abs(vol)
    dh = np.abs(vol[..., y1, :] - vol)                               # between rows y and y + 1, at column x
    dw = np.abs(vol[..., :, x1] - vol)                               # between columns x and x + 1, at row y
    # a cell's own corners: columns x, x + 1 of dh; rows y, y + 1 of dw; the four voxels
    g_h = np.maximum(dh, dh[..., :, x1])
    g_w = np.maximum(dw, dw[..., y1, :])
    a = np.maximum(np.maximum(v, v[..., :, x1]), np.maximum(v[..., y1, :], v[..., y1, :][..., :, x1]))
    return tuple(_neighbourhood_max(t, t.ndim - 2, t.ndim - 1) for t in (g_h, g_w, a))


def project(vol, coef, bins, samples, step, mode):
    """vol: (B, D, H, W) array; coef: (A, 6) fp32 {h0, hu, hj, w0, wu, wj}; step: the table's fp32 step.
    -> (out, bound, ambiguous), each (B, A, D, U): the fp64 projection, the header's bound on |device - out| and the
    flag of the outputs the bound does not cover.  NaN voxels give NaN outputs (and a NaN bound)."""
    vol = np.asarray(vol, dtype=np.float64)
    B, D, H, W = vol.shape
    coef = np.asarray(coef, dtype=np.float32)
    A = coef.shape[0]
    step = float(np.float32(step))
    u, j = np.arange(bins, dtype=np.float64), np.arange(samples, dtype=np.float64)
    g_h, g_w, a_max = _cell_tables(np.nan_to_num(vol, nan=0.0))
    out = np.zeros((B, A, D, bins))
    bound = np.zeros((B, A, D, bins))
    ambiguous = np.zeros((B, A, D, bins), dtype=bool)
    y1 = np.minimum(np.arange(H) + 1, H - 1)
    x1 = np.minimum(np.arange(W) + 1, W - 1)
    for k in range(A):
        hc, e_h, rounded_h = _coordinate(coef[k, 0:3], u, j)
        wc, e_w, rounded_w = _coordinate(coef[k, 3:6], u, j)
        counts = (hc >= 0) & (hc <= H - 1) & (wc >= 0) & (wc <= W - 1)                # (U, R)
        near = lambda c, e, top: (np.abs(c) <= np.maximum(AMBIGUOUS, e)) | (np.abs(c - top) <= np.maximum(AMBIGUOUS, e))
        # a rounded coordinate near a face decides nothing while the other coordinate is clearly outside the box
        clear_out = lambda c, e, top: (c < -np.maximum(AMBIGUOUS, e)) | (c > top + np.maximum(AMBIGUOUS, e))
        doubt = ((rounded_h & near(hc, e_h, H - 1) & ~clear_out(wc, e_w, W - 1)) |
                 (rounded_w & near(wc, e_w, W - 1) & ~clear_out(hc, e_h, H - 1)))
        ambiguous[:, k] = doubt.any(axis=1)[None, None, :]
        y = np.clip(np.floor(hc), 0, H - 1).astype(np.int64)
        x = np.clip(np.floor(wc), 0, W - 1).astype(np.int64)
        fy, fx = hc - np.floor(hc), wc - np.floor(wc)
        v00, v01 = vol[:, :, y, x], vol[:, :, y, x1[x]]                                 # (B, D, U, R)
        v10, v11 = vol[:, :, y1[y], x], vol[:, :, y1[y], x1[x]]
        top = v00 + fx * (v01 - v00)
        bot = v10 + fx * (v11 - v10)
        val = top + fy * (bot - top)
        err = (e_h * g_h[:, :, y, x] + e_w * g_w[:, :, y, x] + 6.0 * U32 * a_max[:, :, y, x]) * (1.0 + 2.0 ** -20)
        cnt = np.broadcast_to(counts, val.shape)
        if mode == "max":
            has_nan = np.isnan(np.where(cnt, val, 0.0)).any(axis=-1)
            best = np.where(cnt, np.nan_to_num(val, nan=-np.inf), -np.inf).max(axis=-1)
            r = np.where(counts.any(axis=1)[None, None, :], best, 0.0)
            out[:, k] = np.where(has_nan, np.nan, r)
            bound[:, k] = np.where(has_nan, np.nan, np.where(cnt, err, 0.0).max(axis=-1))
        else:
            n = counts.sum(axis=1).astype(np.float64)[None, None, :]
            g = n * U32 / (1.0 - n * U32)
            total = np.where(cnt, val, 0.0).sum(axis=-1)                                # NaN stays NaN
            out[:, k] = step * total
            bound[:, k] = step * ((1.0 + g) * np.where(cnt, err, 0.0).sum(axis=-1)
                                  + g * np.where(cnt, np.abs(val), 0.0).sum(axis=-1)) * (1.0 + 2.0 ** -20)
    return out, bound, ambiguous


def nan_reach(coef, bins, samples, shape_hw, voxel):
    """for one NaN voxel (y, x) of a slice: (must, may) boolean (A, U).  must: the ray has a sample that counts beyond
    doubt (at least 2^-12 inside every face) within 1 - 2^-12 of the voxel in both coordinates, so the voxel is one of
    its corners; may: some sample lies within 1 + 2^-12 in both, so it could be."""
    H, W = shape_hw
    coef = np.asarray(coef, dtype=np.float32)
    u, j = np.arange(bins, dtype=np.float64), np.arange(samples, dtype=np.float64)
    must = np.zeros((coef.shape[0], bins), dtype=bool)
    may = np.zeros((coef.shape[0], bins), dtype=bool)
    for k in range(coef.shape[0]):
        hc, e_h, _ = _coordinate(coef[k, 0:3], u, j)
        wc, e_w, _ = _coordinate(coef[k, 3:6], u, j)
        mh, mw = np.maximum(AMBIGUOUS, e_h), np.maximum(AMBIGUOUS, e_w)
        inside = (hc >= mh) & (hc <= H - 1 - mh) & (wc >= mw) & (wc <= W - 1 - mw)
        dy, dx = np.abs(hc - voxel[0]), np.abs(wc - voxel[1])
        must[k] = (inside & (dy <= 1 - AMBIGUOUS) & (dx <= 1 - AMBIGUOUS)).any(axis=1)
        may[k] = ((dy <= 1 + AMBIGUOUS) & (dx <= 1 + AMBIGUOUS)).any(axis=1)
    return must, may
