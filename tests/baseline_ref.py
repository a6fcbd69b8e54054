"""
Yardstick of the two baseline denoisers, on the host in fp64: the separable Gaussian with taps
renormalised at the faces and non-local means, each a direct restatement of its definition in include/ddpm3d.h as
plain loops over offsets, with the per-voxel bound of the entry's arithmetic contract.
"""

import functools
import itertools
import math

import numpy as np

from peak_ref import data

U = 2.0 ** -24           # the unit roundoff of fp32
CUTOFF = 80.0            # DDPM3D_NLM_CUTOFF
EXP_E = 2.0              # expf is within 1 ulp = 2 u


# ------------------------------------------------------------------------------------------ Gaussian
def taps_of(sigma, radius):
    """exp(-j^2 / 2 sigma^2), j = -r..r, formed in fp64 and rounded to fp32"""
    j = np.arange(-radius, radius + 1, dtype=np.float64)
    return np.exp(-0.5 * j * j / (sigma * sigma)).astype(np.float32)


def gauss_pass(x, taps, axis):
    """one axis: y[i] = sum_j t[j] x[i + j] / sum_j t[j] over the j with i + j inside -> (y, n counted taps)"""
    t = np.asarray(taps, dtype=np.float64)
    r, L = len(t) // 2, x.shape[axis]
    num, den, n = np.zeros(x.shape), np.zeros(x.shape), np.zeros(x.shape, dtype=np.int64)
    at = lambda lo, hi: tuple(slice(lo, hi) if a == axis else slice(None) for a in range(3))
    for j in range(-r, r + 1):
        lo, hi = max(0, -j), min(L, L - j)                   # the i with 0 <= i + j < L
        if lo >= hi:
            continue
        num[at(lo, hi)] += t[j + r] * x[at(lo + j, hi + j)]
        den[at(lo, hi)] += t[j + r]
        n[at(lo, hi)] += 1
    return num / den, n


def gaussian(x, taps):
    """x (D, H, W), taps = three fp32 arrays along (D, H, W); passes along W, H, D -> (m, bound): the exact filter
    and ((1 + c_0 u)(1 + c_1 u)(1 + c_2 u) - 1) M, c_a = n_a + 2, M the exact filter of |x|"""
    m, mag = np.asarray(x, dtype=np.float64), np.abs(np.asarray(x, dtype=np.float64))
    factor = np.ones(m.shape)
    for axis in (2, 1, 0):
        m, n = gauss_pass(m, taps[axis], axis)
        mag, _ = gauss_pass(mag, taps[axis], axis)
        factor = factor * (1.0 + (n + 2) * U)
    return m, (factor - 1.0) * mag


# ------------------------------------------------------------------------------------------ non-local means
def _padded(x, search, patch):
    """x with replicate padding of s_a + p_a per side, and the function that reads x[c(v + d)] for every v at once"""
    x = np.asarray(x, dtype=np.float64)
    R = [s + p for s, p in zip(search, patch)]
    xp = np.pad(x, [(r, r) for r in R], mode="edge")
    shifted = lambda d: xp[tuple(slice(r + o, r + o + n) for r, o, n in zip(R, d, x.shape))]
    return x, shifted


def _offsets(radii):
    """the box |o_a| <= r_a in raster order"""
    return list(itertools.product(*[range(-r, r + 1) for r in radii]))


def _inside(shape, s):
    """bool (D, H, W): v + s lies inside the volume"""
    axes = [(np.arange(n) + o >= 0) & (np.arange(n) + o < n) for n, o in zip(shape, s)]
    return axes[0][:, None, None] & axes[1][None, :, None] & axes[2][None, None, :]


def patch_distance(shifted, s, patch):
    """d2(v, s) = (1 / n_p) sum_p (x[c(v + p)] - x[c(v + s + p)])^2 for every v"""
    ps = _offsets(patch)
    d2 = 0.0
    for p in ps:
        d = shifted(p) - shifted(tuple(a + b for a, b in zip(s, p)))
        d2 = d2 + d * d
    return d2 / len(ps)


def distances(x, search, patch):
    """[(s, d2(., s))] for the candidates in raster order: formed once, shared by median_distance and nlm"""
    _, shifted = _padded(x, search, patch)
    return [(s, patch_distance(shifted, s, patch)) for s in _offsets(search)]


def median_distance(x, search, patch, dist=None):
    """the median of sqrt(d2) over every voxel's candidates inside the volume, the voxel itself left out"""
    dist = distances(x, search, patch) if dist is None else dist
    found = [np.sqrt(d2)[_inside(np.shape(x), s)] for s, d2 in dist if s != (0, 0, 0)]
    return float(np.median(np.concatenate(found))) if found else 1.0


def nlm(x, search, patch, h, sigma=0.0, dist=None):
    """-> (m, bound, wx, info): out[v] = sum_s w x[v + s] / sum_s w; the bound c u wx with wx = sum w |x| / sum w and
    c = 2 (80 (n_p + 4) + E) + N_s + 2 (the form for sigma = 0, which asks no less with sigma > 0), plus, for every
    candidate whose exponent lies within (n_p + 4) u of the cutoff, e^-79.9 (|x[v + s]| + |m|) / sum w; info counts
    the weights of candidates other than the voxel itself above 0.5 and exactly 0, and the borderline candidates"""
    x, shifted = _padded(x, search, patch)
    n_p = len(_offsets(patch))
    num, den, mag, edge_x, edge_n = (np.zeros(x.shape) for _ in range(5))
    n_s = np.zeros(x.shape, dtype=np.int64)
    info = {"above_half": 0, "zero": 0, "borderline": 0}
    delta = (n_p + 4) * U
    for s, d2 in (distances(x, search, patch) if dist is None else dist):
        inside = _inside(x.shape, s)
        a = np.maximum(d2 - 2.0 * sigma * sigma, 0.0) / (h * h)
        w = np.where(a <= CUTOFF, np.exp(-np.minimum(a, CUTOFF)), 0.0)
        if s == (0, 0, 0):
            w = np.ones(x.shape)
        else:
            info["above_half"] += int((w[inside] > 0.5).sum())
            info["zero"] += int((w[inside] == 0.0).sum())
            edge = inside & (np.abs(a - CUTOFF) <= CUTOFF * delta)
            info["borderline"] += int(edge.sum())
            edge_x += np.where(edge, np.abs(shifted(s)), 0.0)
            edge_n += edge
        w = np.where(inside, w, 0.0)
        num += w * shifted(s)
        den += w
        mag += w * np.abs(shifted(s))
        n_s += inside
    m, wx = num / den, mag / den
    c = 2.0 * (CUTOFF * (n_p + 4) + EXP_E) + n_s + 2
    bound = c * U * wx + math.exp(-79.9) * (edge_x + edge_n * np.abs(m)) / den
    return m, bound, wx, info


def box_mean(x, search):
    """the mean over the candidates inside the volume: what NLM tends to as h grows"""
    x, shifted = _padded(x, search, (0, 0, 0))
    num, n = np.zeros(x.shape), np.zeros(x.shape)
    for s in _offsets(search):
        inside = _inside(x.shape, s)
        num += np.where(inside, shifted(s), 0.0)
        n += inside
    return num / n


def spiked(shape, seed, offset=0.0, height=300.0):
    """peak_ref.data's noise with one voxel in a thousand (at least one, the last voxel among them) raised by
    `height`: patches that hold a spike lie beyond the cutoff of those that do not at h = the median distance, so
    that the weights span the whole range from 1 to exactly 0"""
    x = data(shape, seed, offset).copy()
    flat = x.reshape(-1)
    n = max(1, flat.size // 1000)
    at = np.random.default_rng(seed + 1).choice(flat.size - 1, size=n - 1, replace=False) if n > 1 else []
    flat[np.concatenate([np.asarray(at, dtype=np.int64), [flat.size - 1]])] += np.float32(height)
    return x


@functools.lru_cache(maxsize=None)
def gauss_case(shape, radii, offset, seed=0):
    """one shared, read-only reference: (x fp32, taps, m, bound); sigma_a = r_a / 3 (a single tap of 1 for r_a = 0)"""
    x = data(shape, seed + 21, offset)
    taps = tuple(taps_of(max(r, 1) / 3.0, r) for r in radii)
    m, bound = gaussian(x, taps)
    for a in (x, m, bound) + taps:
        a.setflags(write=False)
    return x, taps, m, bound


@functools.lru_cache(maxsize=None)
def nlm_case(shape, search, patch, offset, sigma=0.0, seed=0):
    """one shared, read-only reference with h = the median patch distance: (x fp32, h, m, bound, wx, info)"""
    x = spiked(shape, seed + 31, offset)
    dist = distances(x, search, patch)
    h = float(np.float32(median_distance(x, search, patch, dist)))
    m, bound, wx, info = nlm(x, search, patch, h, sigma, dist)
    for a in (x, m, bound, wx):
        a.setflags(write=False)
    return x, h, m, bound, wx, info


def noise_gain(taps):
    """the factor by which the separable filter lowers the std of white noise, away from the faces"""
    return math.prod(math.sqrt(float((np.float64(t) ** 2).sum())) / float(np.float64(t).sum()) for t in taps)


@functools.lru_cache(maxsize=None)
def hot_case(shape=(11, 15, 66), height=50.0, seed=5):
    """Unit noise with one hot voxel of `height` at the centre; NLM with the default windows at h = 2 noise stds,
    and the isotropic Gaussian (scipy's radius rule at truncate 3) whose gain on white noise equals the ratio by
    which NLM lowered the std of the voxels out of the hot voxel's reach.  A filter's `kept` is the share of the hot
    voxel's height above the background mean that survives it.  -> dict"""
    x = data(shape, seed, 0.0).copy()
    at = tuple(n // 2 for n in shape)
    x[at] += np.float32(height)
    search, patch, h = (3, 3, 3), (1, 1, 1), 2.0
    m, bound, _, _ = nlm(x, search, patch, h)
    grids = np.meshgrid(*[np.abs(np.arange(n) - c) for n, c in zip(shape, at)], indexing="ij")
    far = np.maximum(np.maximum(grids[0], grids[1]), grids[2]) > 5
    x64 = x.astype(np.float64)
    background = float(x64[far].mean())
    ratio = float(m[far].std() / x64[far].std())
    taps_at = lambda sigma: (taps_of(sigma, int(3.0 * sigma + 0.5)),) * 3
    lo, hi = 0.2, 5.0                                        # the gain falls as sigma grows
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if noise_gain(taps_at(mid)) > ratio else (lo, mid)
    taps = taps_at(hi)
    g, g_bound = gaussian(x, taps)
    kept = lambda y: (float(y[at]) - background) / (float(x64[at]) - background)
    return {"x": x, "at": at, "far": far, "h": h, "search": search, "patch": patch, "nlm": m, "nlm_bound": bound,
            "ratio": ratio, "sigma": hi, "taps": taps, "gaussian": g, "gaussian_bound": g_bound,
            "background": background, "kept": kept}
