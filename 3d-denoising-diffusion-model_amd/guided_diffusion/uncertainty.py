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
"""

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

    def finish_single(self):
        if self.K != 1:
            raise ValueError("%s.finish_single: one draw only, this stitcher holds %d (use finish())"
                             % (type(self).__name__, self.K))
        acc, wsum = self.acc[0].cpu().numpy(), self.wsum.cpu().numpy()
        return np.divide(acc, wsum, out=acc.copy(), where=wsum > 0), wsum


class DrawStitcher(VolumeStitcher):
    """VolumeStitcher for the uncertainty maps: K >= 2 draws."""

    _MIN_DRAWS = 2
