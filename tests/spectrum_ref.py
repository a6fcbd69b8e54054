"""
numpy fp64 restatement of the radial spectra and the Fourier shell correlation: windows, DFT tables,
q tables, shell numbers, the per-shell records taken from numpy.fft.fftn of the FULL spectrum (so the half-spectrum
twin weights of the kernel are checked against something that has none), and the figures.
"""

import math

import numpy as np

N, XX, YY, XY, EE, REC = 0, 1, 2, 3, 4, 6
THRESHOLDS = (("0.5", 0.5), ("0.143", 1.0 / 7.0))


def window(name, n):
    x = np.arange(n, dtype=np.float64)
    if name == "hann":
        return np.sin(np.pi * (x + 0.5) / n) ** 2
    assert name == "none"
    return np.ones(n)


def windows(name, shape):
    return [window(name, n) for n in shape]


def weight(name, shape):
    w = windows(name, shape)
    return w[0][:, None, None] * w[1][None, :, None] * w[2][None, None, :]


def tables(n, rows, w):
    """C[k][x] = w[x] cos(2 pi ((k x) mod n) / n), S[k][x] = -w[x] sin(...), fp64"""
    c, s = np.empty((rows, n)), np.empty((rows, n))
    for k in range(rows):
        for x in range(n):
            a = 2.0 * math.pi * ((k * x) % n) / n
            c[k, x], s[k, x] = w[x] * math.cos(a), -w[x] * math.sin(a)
    return c, s


def default_width(shape, spacing):
    return 1.0 / max(n * s for n, s in zip(shape, spacing))


def q_table(n, spacing, width, half=False):
    k = np.arange(n // 2 + 1 if half else n)
    folded = np.where(2 * k <= n, k, k - n).astype(np.float64)
    return (folded / (n * spacing * width)) ** 2


def shell_of(r2):
    """the largest integer s with s * s <= r2, by a search among the exact squares"""
    squares = np.arange(0, 8193, dtype=np.float64) ** 2
    return np.searchsorted(squares, r2, side="right") - 1


def shell_numbers(shape, spacing, width=None, half=False):
    width = default_width(shape, spacing) if width is None else width
    q = [q_table(n, s, width, half and a == 2) for a, (n, s) in enumerate(zip(shape, spacing))]
    r2 = (q[0][:, None, None] + q[1][None, :, None]) + q[2][None, None, :]
    return shell_of(r2)


def pivot(v, name):
    w = weight(name, v.shape)
    return float((w * v.astype(np.float64)).sum() / w.sum())


def transform(v, name, p=0.0):
    """the full unnormalised spectrum of w (v - p), the difference formed in fp32 as the kernel forms it"""
    d = (v.astype(np.float32) - np.float32(p)).astype(np.float64)
    return np.fft.fftn(weight(name, v.shape) * d)


def records(X, Y, shells, S):
    """(S, REC) records of full spectra X (and Y or None) over the full-spectrum shell numbers"""
    out = np.zeros((S, REC))
    flat = shells.reshape(-1)
    x = X.reshape(-1)
    out[:, N] = np.bincount(flat, minlength=S)
    out[:, XX] = np.bincount(flat, weights=np.abs(x) ** 2, minlength=S)
    if Y is not None:
        y = Y.reshape(-1)
        out[:, YY] = np.bincount(flat, weights=np.abs(y) ** 2, minlength=S)
        out[:, XY] = np.bincount(flat, weights=(x * np.conj(y)).real, minlength=S)
        out[:, EE] = np.bincount(flat, weights=np.abs(x - y) ** 2, minlength=S)
    return out


def shell_records(est, target, spacing, name, width=None):
    """est (K, D, H, W), target (D, H, W) or None -> (K, S, REC), pivots the window-weighted means"""
    shape = est.shape[1:]
    sh = shell_numbers(shape, spacing, width)
    S = int(sh.max()) + 1
    Y = None if target is None else transform(target, name, np.float32(pivot(target, name)))
    return np.stack([records(transform(e, name, np.float32(pivot(e, name))), Y, sh, S) for e in est])


def crossing(curve, thr, freq):
    for s in range(1, len(curve)):
        if curve[s] is None:
            return None, False
        if curve[s] < thr:
            if s == 1:
                return 1.0 / freq[s], False
            a, b = curve[s - 1], curve[s]
            return 1.0 / (freq[s - 1] + (a - thr) / (a - b) * (freq[s] - freq[s - 1])), False
    return None, True


def figures(rec, shape, spacing, name, width=None):
    width = default_width(shape, spacing) if width is None else width
    nyq = min(1.0 / (2.0 * s) for s in spacing)
    n_rep = sum(1 for s in range(rec.shape[0]) if (s + 1) * width <= nyq)
    norm = float(np.prod(shape)) * float((weight(name, shape) ** 2).sum())
    r = rec[:n_rep]
    freq = [(s + 0.5) * width for s in range(n_rep)]
    div = lambda a, b: None if b == 0 or not (math.isfinite(a) and math.isfinite(b)) else a / b
    fig = {"frequency": freq, "n": [int(v) for v in r[:, N]],
           "power": [v / norm for v in r[:, XX]], "power_target": [v / norm for v in r[:, YY]],
           "power_error": [v / norm for v in r[:, EE]],
           "fsc": [div(v[XY], math.sqrt(v[XX] * v[YY])) for v in r],
           "ratio": [div(v[XX], v[YY]) for v in r], "error_rel": [div(v[EE], v[YY]) for v in r]}
    res, never = {}, False
    for key, thr in THRESHOLDS:
        res[key], n = crossing(fig["fsc"], thr, freq)
        never = never or n
    res["to_nyquist"] = never
    fig["fsc_resolution_mm"] = res
    fig["ratio_half_mm"] = crossing(fig["ratio"], 0.25, freq)[0]
    return fig


def phantom_rows(seed=4):
    """the 24 x 40 x 40 phantom's clean, noisy and Gaussian-filtered volumes (the README's table)"""
    import metrics_ref
    from scipy.ndimage import gaussian_filter
    clean = metrics_ref.phantom((24, 40, 40), seed=seed)
    low = metrics_ref.noisy(clean, 0.1, seed=seed)
    return clean, low, gaussian_filter(low.astype(np.float64), 1.0).astype(np.float32)
