"""
Per-voxel uncertainty maps: mean and sample standard deviation (ddof = 1) of K
independent reverse-diffusion draws of the same low-dose volume, the second
output the paper reports for every denoised volume (reference README.md:44).

Draw d of the volume is the Hann-weighted overlap-add of the d-th draw of
every patch, with exactly patches.stitch_patches' arithmetic; the std is taken
over the K stitched volumes (not a blend of per-patch maps), so it is what K
runs of the single-draw script with different noise followed by
np.std(ddof=1) give.  Both steps run on HIP kernels (csrc/uncertainty.hip,
ddpm3d_draw_stitch / ddpm3d_draw_moments); there is no host fallback.

The same K values per voxel also give the distribution-free maps (DESIGN.md
3.18, csrc/quantiles.hip, ddpm3d_draw_quantiles): per-voxel quantiles with
numpy's "linear" interpolation (median, credible interval) and the rank of a
target value among the draws, whose histogram over the volume is the ensemble's
calibration check (rank_histogram).
"""

import ctypes
import math

import numpy as np
import torch

from . import _hip as H
from . import patches


def _check_draws(K, what):
    if not (isinstance(K, int) and 2 <= K <= H.MAX_DRAWS):
        raise ValueError("%s: needs 2..%d draws, got %r" % (what, H.MAX_DRAWS, K))


def draw_moments(draws):
    """(K, ...) float32 CUDA tensor of K draws -> (mean, std) of shape draws.shape[1:], the sample std with
    ddof = 1, both accumulated in fp64 per voxel."""
    H.require_device(draws, "draws")
    _check_draws(int(draws.shape[0]) if draws.dim() > 0 else 0, "draw_moments")
    K = int(draws.shape[0])
    mean = torch.empty(draws.shape[1:], dtype=torch.float32, device=draws.device)
    std = torch.empty_like(mean)
    with torch.cuda.device(draws.device):
        H.check(H.load().ddpm3d_draw_moments(H.ptr(draws), None, K, mean.numel(), H.ptr(mean), H.ptr(std),
                                             H.stream()))
    return mean, std


def quantile_positions(levels, K):
    """Where numpy.quantile(method="linear") reads K sorted values for each level q: h = q (K - 1) in fp64, split into
    lower = floor(h) and frac = h - lower, so that the quantile is s[lower] + frac * (s[lower + 1] - s[lower]).
    levels: 1..MAX_QUANTILES numbers in [0, 1], strictly ascending.  -> (lower: list of int, frac: list of float)"""
    _check_draws(K, "quantile_positions")
    levels = [float(q) for q in levels]
    if not 1 <= len(levels) <= H.MAX_QUANTILES:
        raise ValueError("quantile_positions: needs 1..%d levels, got %d" % (H.MAX_QUANTILES, len(levels)))
    if not all(0.0 <= q <= 1.0 for q in levels):                # NaN fails the comparison too
        raise ValueError("quantile_positions: every level must lie in [0, 1], got %r" % (levels,))
    if any(b <= a for a, b in zip(levels, levels[1:])):
        raise ValueError("quantile_positions: levels must be strictly ascending, got %r" % (levels,))
    lower, frac = [], []
    for q in levels:
        h = q * (K - 1)
        lo = min(int(math.floor(h)), K - 1)
        lower.append(lo)
        frac.append(h - lo)
    return lower, frac


def _launch_quantiles(acc, wsum, K, shape, levels, target):
    """ddpm3d_draw_quantiles on acc (K, *shape) [/ wsum] -> quant (nq, *shape) or None, below, equal (uint8) or None"""
    nq = len(levels)
    if nq == 0 and target is None:
        raise ValueError("draw_quantiles: no level and no target: nothing to compute")
    lower, frac = quantile_positions(levels, K) if nq else ([], [])
    # the kernel interpolates in fp32: a frac that rounds up to 1 would step past the neighbour, keep it below
    frac32 = np.minimum(np.asarray(frac, dtype=np.float64).astype(np.float32),
                        np.nextafter(np.float32(1), np.float32(0)))
    if target is not None:
        H.require_device(target, "target")
        if tuple(target.shape) != tuple(shape) or target.device != acc.device:
            raise ValueError("draw_quantiles: target of shape %s on %s, the draws are %s on %s"
                             % (tuple(target.shape), target.device, tuple(shape), acc.device))
    quant = torch.empty((nq,) + tuple(shape), dtype=torch.float32, device=acc.device) if nq else None
    below = equal = None
    if target is not None:
        below = torch.empty(tuple(shape), dtype=torch.uint8, device=acc.device)
        equal = torch.empty_like(below)
    n = 1
    for v in shape:
        n *= int(v)
    with torch.cuda.device(acc.device):
        H.check(H.load().ddpm3d_draw_quantiles(
            H.ptr(acc), H.ptr(wsum), K, n, nq, (ctypes.c_int * max(nq, 1))(*lower),
            (ctypes.c_float * max(nq, 1))(*[float(f) for f in frac32]), H.ptr(target), H.ptr(quant), H.ptr(below),
            H.ptr(equal), H.stream()))
    return quant, below, equal


def draw_quantiles(draws, levels, weight=None, target=None):
    """(K, ...) float32 CUDA tensor of K draws -> quant (len(levels), ...): the per-voxel quantiles at `levels`
    (numpy.quantile's method "linear"; levels as quantile_positions takes them).  weight (...): every draw is divided
    by it first, as VolumeStitcher's accumulators are; voxels of weight <= 0 get 0.  With target (...) also
    -> (quant, below, equal): uint8 maps of how many draws lie below and how many equal the target's value, 255 where
    the voxel is not counted (weight <= 0, a NaN draw or a NaN target); levels=() then gives (None, below, equal).
    A voxel with a NaN draw has NaN quantiles."""
    H.require_device(draws, "draws")
    _check_draws(int(draws.shape[0]) if draws.dim() > 0 else 0, "draw_quantiles")
    shape = tuple(draws.shape[1:])
    if weight is not None:
        H.require_device(weight, "weight")
        if tuple(weight.shape) != shape:
            raise ValueError("draw_quantiles: weight of shape %s, the draws are %s" % (tuple(weight.shape), shape))
    quant, below, equal = _launch_quantiles(draws, weight, int(draws.shape[0]), shape, tuple(levels), target)
    return quant if target is None else (quant, below, equal)


def rank_histogram(below, equal, K, mask=None):
    """The rank histogram (Talagrand diagram) of a target among K draws from draw_quantiles' below / equal maps:
    {"counts": K + 1 ints, counts[r] = voxels with r draws below the target and none equal to it, "ties": voxels with
    a draw equal to the target (left out of counts: their rank is not defined), "n": counts' sum + ties}.  Voxels
    marked 255 or where mask is 0 are not counted.  torch ops on the device, one copy to the host."""
    _check_draws(K, "rank_histogram")
    counted = below != 255
    if mask is not None:
        counted = counted & (mask.reshape(below.shape) != 0)
    b, e = below[counted].long(), equal[counted]
    tied = e > 0
    # one bincount: ranks 0..K of the untied voxels, bin K + 1 for the tied ones
    host = torch.bincount(torch.where(tied, torch.full_like(b, K + 1), b), minlength=K + 2).cpu().tolist()
    counts, ties = host[:K + 1], int(sum(host[K + 1:]))
    return {"counts": [int(c) for c in counts], "ties": ties, "n": int(sum(counts)) + ties}


class VolumeStitcher:
    """K >= 1 full-volume accumulators and one weight sum on the device, (K + 1) * H * W * D * 4 bytes: the one-shot
    Hann blend of patches.stitch_patches, patch by patch as the patches arrive, so that no rank holds all patches.

    add(global_index, samples_kcdhw, origin) blends one patch origin's K draws, as the sampler returns them
    ((K, 1, res, res, res) NCDHW float32), at origin = (x_start, y_start, z_start) of the patch grid;
    patches must come in ascending global index (the order patches.stitch_patches sums in).
    finish() (K >= 2) -> (mean, std, weight), each (H, W, D) float32 on the device (the reference's (H, W, Z)
    layout); voxels of weight 0 are 0 in mean and std.
    finish_single() (K = 1) -> (volume, weight), (H, W, D) float32 host arrays: patches.stitch_patches' result bit
    for bit.  The sums are the device's; the one division per voxel is numpy's on the host, as in stitch_patches."""

    _MIN_DRAWS = 1

    def __init__(self, shape_dhw, resolution, num_draws, device):
        if not (isinstance(num_draws, int) and self._MIN_DRAWS <= num_draws <= H.MAX_DRAWS):
            raise ValueError("%s: needs %d..%d draws, got %r"
                             % (type(self).__name__, self._MIN_DRAWS, H.MAX_DRAWS, num_draws))
        D, Hh, W = (int(v) for v in shape_dhw)
        self.shape_hwd = (Hh, W, D)
        self.res = int(resolution)
        self.K = int(num_draws)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("%s runs on HIP kernels only (got device %s)" % (type(self).__name__, self.device))
        self.acc = torch.zeros((self.K,) + self.shape_hwd, dtype=torch.float32, device=self.device)
        self.wsum = torch.zeros(self.shape_hwd, dtype=torch.float32, device=self.device)
        self.window = torch.from_numpy(np.ascontiguousarray(patches.hann_window_3d(self.res))).to(self.device)
        self._last = -1

    def add(self, global_index, samples_kcdhw, origin):
        if global_index <= self._last:
            raise ValueError("%s.add: patch %d after patch %d -- patches must come in ascending order"
                             % (type(self).__name__, global_index, self._last))
        r = self.res
        if tuple(samples_kcdhw.shape) != (self.K, 1, r, r, r):
            raise ValueError("%s.add: samples of shape %s, expected %s"
                             % (type(self).__name__, tuple(samples_kcdhw.shape), (self.K, 1, r, r, r)))
        H.require_device(samples_kcdhw, "samples")
        xs, ys, zs = (int(v) for v in origin)
        Hh, W, D = self.shape_hwd
        with torch.cuda.device(self.device):
            H.check(H.load().ddpm3d_draw_stitch(H.ptr(samples_kcdhw), self.K, r, H.ptr(self.window), xs, ys, zs, Hh,
                                                W, D, H.ptr(self.acc), H.ptr(self.wsum), H.stream()))
        self._last = global_index

    def finish(self):
        _check_draws(self.K, type(self).__name__ + ".finish")
        mean = torch.empty(self.shape_hwd, dtype=torch.float32, device=self.device)
        std = torch.empty_like(mean)
        with torch.cuda.device(self.device):
            H.check(H.load().ddpm3d_draw_moments(H.ptr(self.acc), H.ptr(self.wsum), self.K, mean.numel(), H.ptr(mean),
                                                 H.ptr(std), H.stream()))
        return mean, std, self.wsum

    def draw(self, k):
        """Stitched draw k as finish() averages it: acc[k] / wsum in fp32, 0 where the weight is 0; (H, W, D) on the
        device, one temporary volume."""
        return torch.where(self.wsum > 0, self.acc[k] / self.wsum, torch.zeros_like(self.wsum))

    def quantiles(self, levels, target=None):
        """draw_quantiles of the K stitched draws (K >= 2), straight from the accumulators and the weight sum: no
        K-volume temporary.  -> quant (len(levels), H, W, D), or (quant, below, equal) with a target (H, W, D)."""
        _check_draws(self.K, type(self).__name__ + ".quantiles")
        quant, below, equal = _launch_quantiles(self.acc, self.wsum, self.K, self.shape_hwd, tuple(levels), target)
        return quant if target is None else (quant, below, equal)

    def finish_single(self):
        if self.K != 1:
            raise ValueError("%s.finish_single: one draw only, this stitcher holds %d (use finish())"
                             % (type(self).__name__, self.K))
        acc, wsum = self.acc[0].cpu().numpy(), self.wsum.cpu().numpy()
        return np.divide(acc, wsum, out=acc.copy(), where=wsum > 0), wsum


class DrawStitcher(VolumeStitcher):
    """VolumeStitcher for the uncertainty maps: K >= 2 draws."""

    _MIN_DRAWS = 2
