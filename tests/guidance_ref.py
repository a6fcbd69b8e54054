"""
Yardstick of the low-pass data-consistency pull (include/ddpm3d.h, ddpm3d_xstart_pull) and of the
three guided steps, on the host.

fp32, one rounding at a time in the kernels' order: pull() and the steps p_sample_step / ddim_step /
dpm_solver_step, in torch on the CPU.  The fma of the Gaussian's tap chain is formed in fp64 with the sum rounded to
odd, so that the final rounding to fp32 is the fused operation's single rounding.  pull() is also what the golden
maker hands the reference as denoised_fn (tests/golden/make_golden_guidance.py).

fp64: pull64() -> the exact operator on the same fp32 inputs and the per-voxel bound of the entry's contract.
"""

import numpy as np
import torch

from baseline_ref import gauss_pass

U = 2.0 ** -24           # the unit roundoff of fp32


def _f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def fma32(t, x, acc):
    """fl32(t * x + acc) of fp32 arrays with ONE rounding: the product is exact in fp64, the fp64 sum is rounded to odd
    (TwoSum tells whether it was exact), and 53 >= 24 + 2 bits make the second rounding the only one that counts."""
    p = np.float64(t) * x.astype(np.float64)
    a = acc.astype(np.float64)
    s = p + a
    bb = s - p
    e = (p - (s - bb)) + (a - bb)
    even = (s.view(np.int64) & 1) == 0
    fix = (e != 0) & even & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def smooth_pass32(x, taps, axis):
    """ddpm3d_gauss_smooth's per-pass rule along `axis` of an fp32 (D, H, W) array: the counted taps ascending, the
    first as a product and the others by fma, over the fp64 sum of the counted taps rounded once."""
    t = _f32(taps)
    r, L = len(t) // 2, x.shape[axis]
    prefix = np.concatenate([[0.0], np.cumsum(t.astype(np.float64))])
    xm = np.moveaxis(x, axis, 0)
    out = np.empty_like(xm)
    for c in range(L):
        lo, hi = max(-r, -c), min(r, L - 1 - c)
        acc = t[lo + r] * xm[c + lo]
        for j in range(lo + 1, hi + 1):
            acc = fma32(t[j + r], xm[c + j], acc)
        out[c] = acc / np.float32(prefix[hi + r + 1] - prefix[lo + r])
    return np.ascontiguousarray(np.moveaxis(out, 0, axis))


def smooth32(x, taps):
    """the separable Gaussian of one fp32 (D, H, W) array: passes along W, H, D, a pass with radius 0 skipped"""
    x = _f32(x)
    for axis in (2, 1, 0):
        if len(taps[axis]) > 1:
            x = smooth_pass32(x, taps[axis], axis)
    return x


def pull(x0_raw, y, taps, w):
    """x0_raw + w * G(y - x0_raw) before the clip, in fp32: (N, 1, D, H, W) torch tensors on the CPU, taps = three
    sequences along (D, H, W).  This is the reference's denoised_fn."""
    d = (y - x0_raw).numpy()                                  # one fp32 subtraction
    g = np.stack([smooth32(d[n, 0], taps)[None] for n in range(d.shape[0])])
    wg = torch.from_numpy(g) * torch.tensor(np.float32(w))    # one rounding
    return x0_raw + wg                                        # and one more


def _rows(tab, t, x):
    b = (-1,) + (1,) * (x.dim() - 1)
    return [torch.from_numpy(np.ascontiguousarray(tab[:, j]))[t].reshape(b) for j in range(tab.shape[1])]


def x0_raw(coef, model_out, x, t, predict_xstart):
    """the step's x_start prediction before the clip; coef: the package's [T][8] fp32 table"""
    C = x.shape[1]
    c_recip, c_recipm1 = _rows(coef, t, x)[:2]
    e = model_out[:, :C]
    return e if predict_xstart else c_recip * x - c_recipm1 * e


def pulled_x0(coef, model_out, x, t, y, taps, w, predict_xstart, clip):
    x0 = pull(x0_raw(coef, model_out, x, t, predict_xstart), y, taps, w)
    return x0.clamp(-1, 1) if clip else x0


def p_sample_step(coef, model_out, x, t, noise, x0, learn_sigma):
    """ddpm3d_p_sample_step_x0: the posterior mean from the finished x0, then the draw (:216-219, :438)"""
    C = x.shape[1]
    _, _, c1, c2, min_log, max_log = _rows(coef, t, x)[:6]
    if learn_sigma:
        frac = (model_out[:, C:] + 1.0) / 2.0
        logvar = frac * max_log + (1.0 - frac) * min_log
    else:
        logvar = min_log.expand(x.shape)
    mean = c1 * x0 + c2 * x
    mask = (t != 0).float().reshape((-1,) + (1,) * (x.dim() - 1))
    return mean + mask * torch.exp(0.5 * logvar) * noise


def ddim_step(coef, x, t, noise, x0, eta):
    """ddpm3d_ddim_step_x0: eps re-derived from the finished x0 (:566), then :570-584"""
    r = _rows(coef, t, x)
    c_recip, c_recipm1, ab, ab_prev = r[0], r[1], r[6], r[7]
    eps = (c_recip * x - x0) / c_recipm1
    sigma = eta * torch.sqrt((1.0 - ab_prev) / (1.0 - ab)) * torch.sqrt(1.0 - ab / ab_prev)
    mean_pred = x0 * torch.sqrt(ab_prev) + torch.sqrt(1.0 - ab_prev - sigma * sigma) * eps
    mask = (t != 0).float().reshape((-1,) + (1,) * (x.dim() - 1))
    return mean_pred + mask * sigma * noise


def dpm_solver_step(scoef, x, t, x0, m1, m2, z, order):
    """ddpm3d_dpm_solver_step_x0: c_x x + w0 x0 (+ w1 m1) (+ w2 m2) (+ c_z z), summed in that order"""
    c_x, w0, w1, w2, c_z = _rows(scoef, t, x)[:5]
    out = c_x * x + w0 * x0
    if order >= 2:
        out = out + w1 * m1
    if order >= 3:
        out = out + w2 * m2
    if z is not None:
        out = out + c_z * z
    return out


def pull64(x0_raw32, y32, taps, w):
    """fp64 on the same fp32 inputs -> (x0_raw + w m before the clip, bound):
    u |x0_raw + w m| + w ((1 + u)^3 prod_a (1 + c_a u) - 1) M, with m / M the exact filter of (|)y - x0_raw(|) and
    c_a = n_a + 2 for a pass that runs, 0 for a skipped one.  Arrays (N, 1, D, H, W); w the fp32 weight."""
    x0 = np.asarray(x0_raw32, dtype=np.float64)
    d = np.asarray(y32, dtype=np.float64) - x0
    m, mag, factor = d.copy(), np.abs(d), np.ones(d.shape)
    for n in range(d.shape[0]):
        for axis in (2, 1, 0):
            if len(taps[axis]) > 1:
                m[n, 0], cnt = gauss_pass(m[n, 0], _f32(taps[axis]), axis)
                mag[n, 0], _ = gauss_pass(mag[n, 0], _f32(taps[axis]), axis)
                factor[n, 0] = factor[n, 0] * (1.0 + (cnt + 2) * U)
    w = float(np.float32(w))
    exact = x0 + w * m
    return exact, U * np.abs(exact) + w * ((1.0 + U) ** 3 * factor - 1.0) * mag


def taps_for(radii):
    """the tap tables of the tests and the golden file for radii along (D, H, W): exp(-j^2 / 2 sigma^2) with
    sigma = r / 2 (one unit tap for r = 0), formed in fp64 and rounded to fp32"""
    out = []
    for r in radii:
        j = np.arange(-r, r + 1, dtype=np.float64)
        out.append(np.exp(-0.5 * j * j / (max(r, 1) / 2.0) ** 2).astype(np.float32))
    return out
