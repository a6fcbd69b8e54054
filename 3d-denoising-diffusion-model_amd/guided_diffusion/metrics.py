"""
Image quality of a denoised volume against a full-dose target: error moments (PSNR, NRMSE, MAE, bias, coverage of
the per-voxel std map) and the 3-D SSIM of Wang et al. 2004 in the form
skimage.metrics.structural_similarity(gaussian_weights=True, sigma=1.5, use_sample_covariance=False) takes for 3-D
input (include/ddpm3d.h has the definitions, DESIGN.md 3.8 the kernels).  The volumes stay on the device: both
metrics are one pass of a HIP kernel (csrc/metrics.hip, ddpm3d_error_moments / ddpm3d_ssim3d) over K estimates
against one shared target, and only the K small records come back, in one copy.  There is no host fallback.

All of it is isotropic: (D, H, W) canvases and the inference script's (H, W, Z) volumes alike.
"""

import math

import torch

from . import _hip as H

SSIM_RADIUS = 5         # 11 taps per axis; the map covers the voxels at least this far from every face


def _stack(estimate, target, what):
    """estimate (D, H, W) or (K, D, H, W) against target (D, H, W) -> (K, batched)"""
    H.require_device(estimate, "estimate")
    H.require_device(target, "target")
    if estimate.device != target.device:
        raise ValueError("%s: estimate on %s, target on %s" % (what, estimate.device, target.device))
    if target.dim() != 3 or estimate.dim() not in (3, 4) or tuple(estimate.shape[-3:]) != tuple(target.shape):
        raise ValueError("%s: estimate of shape %s against a target of shape %s (want (D, H, W) or (K, D, H, W) "
                         "against (D, H, W))" % (what, tuple(estimate.shape), tuple(target.shape)))
    K = int(estimate.shape[0]) if estimate.dim() == 4 else 1
    if not 1 <= K <= H.MAX_DRAWS:
        raise ValueError("%s: %d estimates (1..%d)" % (what, K, H.MAX_DRAWS))
    return K, estimate.dim() == 4


def _check_mask(mask, target, what):
    if mask is None:
        return
    if not (isinstance(mask, torch.Tensor) and mask.is_cuda):
        raise RuntimeError("mask must live on the GPU: this package runs on HIP kernels only "
                           "(got %s)" % getattr(mask, "device", type(mask)))
    if mask.dtype != torch.uint8 or not mask.is_contiguous() or tuple(mask.shape) != tuple(target.shape):
        raise ValueError("%s: mask must be contiguous uint8 of the target's shape %s" % (what, tuple(target.shape)))


def _unbatch(d, batched):
    return d if batched else {k: v[0] for k, v in d.items()}


def error_moments(estimate, target, mask=None, std=None):
    """Moments of e = estimate - target over the voxels the mask counts (all without one), every term in fp64:
    a dict with n, mse, mae, bias, target_sq_mean, target_mean, target_min, target_max and, with the per-voxel
    `std` volume of --num_draws, coverage_1 / coverage_2 (and their integer counts cover_1 / cover_2): the share of
    counted voxels with |e| <= k std.  Values are Python floats (n: int), or lists of K for a (K, D, H, W) estimate."""
    K, batched = _stack(estimate, target, "error_moments")
    _check_mask(mask, target, "error_moments")
    if std is not None:
        H.require_device(std, "std")
        if tuple(std.shape) != tuple(target.shape):
            raise ValueError("error_moments: std of shape %s, target of shape %s" % (tuple(std.shape),
                                                                                    tuple(target.shape)))
    lib = H.load()
    voxels = target.numel()
    need = lib.ddpm3d_error_moments_workspace_bytes(K, voxels)
    with torch.cuda.device(target.device):
        ws = torch.empty(max(need, 16) // 8, dtype=torch.float64, device=target.device)
        out = torch.empty((K, H.EM_REC), dtype=torch.float64, device=target.device)
        H.check(lib.ddpm3d_error_moments(H.ptr(estimate), H.ptr(target), H.ptr(mask), H.ptr(std), K, voxels,
                                         H.ptr(ws), ws.numel() * 8, H.ptr(out), H.stream()))
        rec = out.cpu().tolist()                       # the one device-to-host copy (it waits for the stream)
    keys = ["n", "mse", "mae", "bias", "target_sq_mean", "target_mean", "target_min", "target_max"]
    if std is not None:
        keys += ["cover_1", "cover_2", "coverage_1", "coverage_2"]
    res = {k: [] for k in keys}
    for r in rec:
        n = int(r[H.EM_N])
        if n == 0:
            raise ValueError("error_moments: the mask counts no voxel")
        res["n"].append(n)
        res["mse"].append(r[H.EM_SUM_SQ_E] / n)
        res["mae"].append(r[H.EM_SUM_ABS_E] / n)
        res["bias"].append(r[H.EM_SUM_E] / n)
        res["target_sq_mean"].append(r[H.EM_SUM_SQ_Y] / n)
        res["target_mean"].append(r[H.EM_SUM_Y] / n)
        res["target_min"].append(r[H.EM_MIN_Y])
        res["target_max"].append(r[H.EM_MAX_Y])
        if std is not None:
            res["cover_1"].append(int(r[H.EM_COVER_1]))
            res["cover_2"].append(int(r[H.EM_COVER_2]))
            res["coverage_1"].append(r[H.EM_COVER_1] / n)
            res["coverage_2"].append(r[H.EM_COVER_2] / n)
    return _unbatch(res, batched)


def psnr(mse, data_range):
    """10 log10(L^2 / mse); inf for mse = 0."""
    if not data_range > 0 or mse < 0:
        raise ValueError("psnr: needs data_range > 0 and mse >= 0 (got %r, %r)" % (data_range, mse))
    return math.inf if mse == 0 else 10.0 * math.log10(data_range * data_range / mse)


def nrmse(mse, target_sq_mean):
    """sqrt(mse / mean(target^2)): skimage's normalized_root_mse with the "euclidean" normalisation."""
    if not target_sq_mean > 0 or mse < 0:
        raise ValueError("nrmse: needs mean(target^2) > 0 and mse >= 0 (got %r, %r)" % (target_sq_mean, mse))
    return math.sqrt(mse / target_sq_mean)


def ssim3d(estimate, target, data_range, mask=None, full=False):
    """Mean structural similarity over the interior voxels (at least 5 from every face) that the mask counts; the
    window itself reads all voxels.  Every extent must be at least 11.  -> float (list of K for a (K, D, H, W)
    estimate); with full=True also the map, a float32 device tensor of shape ([K,] D - 10, H - 10, W - 10)."""
    K, batched = _stack(estimate, target, "ssim3d")
    _check_mask(mask, target, "ssim3d")
    if not (isinstance(data_range, (int, float)) and math.isfinite(data_range) and data_range > 0):
        raise ValueError("ssim3d: data_range must be a positive finite number (got %r)" % (data_range,))
    D, Hh, W = (int(v) for v in target.shape)
    n = 2 * SSIM_RADIUS + 1
    if min(D, Hh, W) < n:
        raise ValueError("ssim3d: every extent must be at least %d (got %s)" % (n, (D, Hh, W)))
    lib = H.load()
    need = lib.ddpm3d_ssim3d_workspace_bytes(K, D, Hh, W)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    with torch.cuda.device(target.device):
        ws = torch.empty(max(need, 16) // 8, dtype=torch.float64, device=target.device)
        out = torch.empty((K, 2), dtype=torch.float64, device=target.device)
        smap = None
        if full:
            smap = torch.empty((K, D - n + 1, Hh - n + 1, W - n + 1), dtype=torch.float32, device=target.device)
        H.check(lib.ddpm3d_ssim3d(H.ptr(estimate), H.ptr(target), H.ptr(mask), K, D, Hh, W, c1, c2, H.ptr(ws),
                                  ws.numel() * 8, H.ptr(smap), H.ptr(out), H.stream()))
        rec = out.cpu().tolist()
    if any(r[1] == 0 for r in rec):
        raise ValueError("ssim3d: the mask counts no interior voxel")
    mean = [r[0] / r[1] for r in rec]
    if not batched:
        mean, smap = mean[0], (smap[0] if full else None)
    return (mean, smap) if full else mean


def evaluate(estimate, target, data_range=None, mask=None, std=None):
    """All figures of one estimate (or K of them) against the target: psnr, nrmse, mae, bias, ssim, data_range,
    n_voxels and, with `std`, coverage_1 / coverage_2.  data_range None: max - min of the target over the counted
    voxels.  Python floats, or lists of K; data_range and n_voxels are the same for every estimate."""
    m = error_moments(estimate, target, mask=mask, std=std)
    batched = isinstance(m["n"], list)
    first = (lambda v: v[0]) if batched else (lambda v: v)
    if data_range is None or data_range == 0:
        data_range = first(m["target_max"]) - first(m["target_min"])
    data_range = float(data_range)
    if not data_range > 0:
        raise ValueError("evaluate: data range %r (a constant target needs an explicit data_range)" % data_range)
    each = (lambda f, *cols: [f(*a) for a in zip(*cols)]) if batched else (lambda f, *cols: f(*cols))
    res = {
        "psnr": each(lambda mse: psnr(mse, data_range), m["mse"]),
        "nrmse": each(nrmse, m["mse"], m["target_sq_mean"]),
        "mae": m["mae"],
        "bias": m["bias"],
        "ssim": ssim3d(estimate, target, data_range, mask=mask),
        "data_range": data_range,
        "n_voxels": first(m["n"]),
    }
    if std is not None:
        res["coverage_1"], res["coverage_2"] = m["coverage_1"], m["coverage_2"]
    return res
