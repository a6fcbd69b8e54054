"""
Image quality of a denoised volume against a full-dose target: error moments (PSNR, NRMSE, MAE, bias, coverage of
the per-voxel std map) and the 3-D SSIM of Wang et al. 2004 in the form
skimage.metrics.structural_similarity(gaussian_weights=True, sigma=1.5, use_sample_covariance=False) takes for 3-D
input (include/ddpm3d.h has the definitions, DESIGN.md 3.8 the kernels).  The volumes stay on the device: both
metrics are one pass of a HIP kernel (csrc/metrics.hip, ddpm3d_error_moments / ddpm3d_ssim3d) over K estimates
against one shared target, and only the K small records come back, in one copy.  There is no host fallback.

All of it is isotropic: (D, H, W) canvases and the inference script's (H, W, Z) volumes alike.

Per-region (lesion / organ) statistics: roi_index turns a label volume into a region index on the
device, roi_moments is one launch of ddpm3d_roi_moments (csrc/roi.hip) over it, roi_figures turns the records into
SUVmean / SUVmax bias, contrast recovery, CNR, CoV and the spread of a region mean over draws, roi_report puts them
together.

Lesion segmentation: label_components thresholds a volume and labels its connected components with
ddpm3d_label_components (csrc/ccl.hip), segment drops the specks, detection compares two segmentations (lesions
found and missed, false positives).  Their labels feed roi_index.

SUVpeak, MTV and TLG: sphere_footprint turns a voxel spacing into PERCIST's 1 cm^3 sphere in run
form, sphere_mean is one launch of ddpm3d_sphere_mean (csrc/peak.hip) that writes the sphere mean around every voxel,
roi_peak is roi_moments' MAX_X of that map; with a spacing roi_figures adds volume_ml and tlg, roi_report the peaks.

Baseline denoisers, to score beside the written volume: gaussian_taps turns a FWHM in mm and a voxel
spacing into the taps of the clinic's Gaussian post-filter, gaussian_smooth applies them with ddpm3d_gauss_smooth
(csrc/smooth.hip), nlm is non-local means in one launch of ddpm3d_nlm (csrc/nlm.hip).

Multi-scale SSIM: pool2 is the 2 x 2 x 2 mean pooling of ddpm3d_pool2, msssim3d one call of
ddpm3d_msssim3d (csrc/msssim.hip) over up to five scales and the product of the per-scale means on the host;
evaluate(..., msssim_scales=M) adds it to the figures.

Per-step convergence trace: a StepTrace handed to a sampling loop as trace= records, per reverse
step and sample, the weighted moments of that step's pred_xstart against a target and against the previous step's
pred_xstart, one call of ddpm3d_trace_moments (csrc/trace.hip) per step and no host synchronisation before
records(); trace_figures turns pooled records into PSNR, NRMSE, MAE, bias, mean, std, delta_rms and clipped per step
on the host.

Per-region texture: roi_texture is one call of ddpm3d_roi_texture (csrc/texture.hip) that builds the
grey-level co-occurrence matrix, the grey-level histogram and the side counters of every region of a region index,
texture_figures takes Haralick's figures from them on the host as IBSI defines them (contrast, joint entropy, inverse
difference moment, ...), roi_report(..., texture=...) adds them to both of its blocks.

Radial spectra and Fourier shell correlation: spectrum_plan builds the per-axis DFT tables (window
folded in) and the frequency shells of a volume shape and spacing on the host and, on first use, the shell index on
the device; dft3 is ddpm3d_dft3 (csrc/spectrum.hip: three MFMA GEMM passes), shell_spectrum one call of
ddpm3d_shell_spectrum and one copy of its per-shell records, spectrum_figures turns them into power spectra, the FSC,
the power ratio and the resolutions at FSC = 0.5 and 1/7 on the host.  evaluate does not take a plan: its parameter list is pinned as it is.

Rotating maximum-intensity and ray-sum projections: projection_plan folds a slice geometry, a
detector and a list of angles into the six fp32 numbers per angle ddpm3d_project reads (ddpm3d_project_table_fill, on
the host), project is one launch of ddpm3d_project (csrc/project.hip) over a volume or a stack: the MIP ("max") or
the line integral ("sum") of every ray through every slice, rotated about the D axis.

Distances and lesion boundaries: distance_sq is one call of ddpm3d_distance_sq (csrc/edt.hip), the
exact squared Euclidean distance transform on anisotropic voxels; surface, boundary_target and boundary turn two such
transforms into Dice, Hausdorff, HD95 and ASSD figures of an estimate's segmentation against the target's, whole and
per target region, with one device-to-host copy; edge_profile reduces every volume over shells of a given width
inside and outside the labelled regions' boundary (roi_index, roi_moments).

Splitting touching lesions: basins is one call of ddpm3d_basins (csrc/watershed.hip): every voxel
of a labelled component climbs a height volume to a peak under the total order (height, -index); basin_saddles is
ddpm3d_basin_saddles plus a reduction with torch sorts to the saddle graph between the basins; merge_basins merges
basins by peak prominence on the host; split_components puts them together and relabels on the device.

Credible intervals: interval_figures scores two per-voxel quantile maps of
uncertainty.draw_quantiles against the target: the share of voxels the interval covers and its mean width.
"""

import ctypes
import math

import numpy as np
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


# ----------------------------------------------------------------- multi-scale SSIM
MSSSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)      # Wang, Simoncelli, Bovik 2003, scales 0..4


def _check_scales(scales, what):
    if isinstance(scales, bool) or not isinstance(scales, int) or not 1 <= scales <= H.MSSSIM_MAX_SCALES:
        raise ValueError("%s: scales must be an int in 1..%d (got %r)" % (what, H.MSSSIM_MAX_SCALES, scales))
    return scales


def msssim_weights(scales):
    """The default exponents of msssim3d: the first `scales` of MSSSIM_WEIGHTS divided by their sum (the published
    weights for 5 scales, (1.0,) for one).  -> a tuple of floats"""
    w = MSSSIM_WEIGHTS[:_check_scales(scales, "msssim_weights")]
    total = math.fsum(w)
    return tuple(v / total for v in w)


def msssim_max_scales(shape):
    """The most scales a volume of this shape allows: every extent >> (M - 1) must be at least 11; 0 if none."""
    n = 2 * SSIM_RADIUS + 1
    return max([m for m in range(1, H.MSSSIM_MAX_SCALES + 1) if min(int(v) for v in shape) >> (m - 1) >= n],
               default=0)


def pool2(volume, mask=None):
    """2 x 2 x 2 mean pooling of a device float32 (D, H, W) or (K, D, H, W) tensor: one call of ddpm3d_pool2
    (csrc/msssim.hip), no host copy.  The extents halve (an odd trailing plane, row or column is dropped); the eight
    values are summed in fp32 in one fixed order.  With mask (a device uint8 (D, H, W) tensor shared by the K
    volumes) also the pooled mask: 1 where at least 4 of the 8 inputs are non-zero.  -> pooled, or (pooled, mask)."""
    H.require_device(volume, "volume")
    if volume.dim() not in (3, 4):
        raise ValueError("pool2: volume of shape %s (want (D, H, W) or (K, D, H, W))" % (tuple(volume.shape),))
    D, Hh, W = (int(v) for v in volume.shape[-3:])
    if min(D, Hh, W) < 2:
        raise ValueError("pool2: every extent must be at least 2 (got %s)" % ((D, Hh, W),))
    K = int(volume.shape[0]) if volume.dim() == 4 else 1
    if not 1 <= K <= H.MAX_DRAWS:
        raise ValueError("pool2: %d volumes (1..%d)" % (K, H.MAX_DRAWS))
    if mask is not None and not (isinstance(mask, torch.Tensor) and mask.is_cuda and mask.dtype == torch.uint8
                                 and mask.is_contiguous() and tuple(mask.shape) == (D, Hh, W)
                                 and mask.device == volume.device):
        raise ValueError("pool2: mask must be a contiguous device uint8 tensor of the volume's shape %s"
                         % ((D, Hh, W),))
    lib = H.load()
    with torch.cuda.device(volume.device):
        out = torch.empty(tuple(volume.shape[:-3]) + (D // 2, Hh // 2, W // 2), dtype=torch.float32,
                          device=volume.device)
        mask_out = None if mask is None else torch.empty((D // 2, Hh // 2, W // 2), dtype=torch.uint8,
                                                         device=volume.device)
        H.check(lib.ddpm3d_pool2(H.ptr(volume), H.ptr(mask), K, D, Hh, W, H.ptr(out), H.ptr(mask_out), H.stream()))
    return out if mask is None else (out, mask_out)


def msssim3d(estimate, target, data_range, scales, weights=None, mask=None, parts=False):
    """Multi-scale structural similarity (include/ddpm3d.h has the definition): the product over the scales
    j < scales - 1 of max(CS_j, 0) ** w_j, times max(S_last, 0) ** w_last, where scale j + 1 is scale j pooled by
    2 x 2 x 2 means (estimate, target and mask alike), CS_j and S_j are the means of the contrast-structure term and
    of the SSIM over the interior voxels that scale's mask counts, and w = weights, default msssim_weights(scales).
    A mean that is not positive makes the result 0.0.  One call of ddpm3d_msssim3d and one device-to-host copy.
    scales = 1 is ssim3d.  -> float (list of K for a (K, D, H, W) estimate); with parts=True also {"cs": the
    scales - 1 values CS_j, "ssim": S_last} (a list of K such dicts)."""
    K, batched = _stack(estimate, target, "msssim3d")
    _check_mask(mask, target, "msssim3d")
    if not (isinstance(data_range, (int, float)) and math.isfinite(data_range) and data_range > 0):
        raise ValueError("msssim3d: data_range must be a positive finite number (got %r)" % (data_range,))
    M = _check_scales(scales, "msssim3d")
    D, Hh, W = (int(v) for v in target.shape)
    most = msssim_max_scales((D, Hh, W))
    if M > most:
        raise ValueError("msssim3d: a volume of %s is too small for %d scales: every extent must be at least %d after "
                         "%d halvings; it allows at most %d" % ((D, Hh, W), M, 2 * SSIM_RADIUS + 1, M - 1, most))
    if weights is None:
        w = msssim_weights(M)
    else:
        try:
            w = tuple(math.nan if isinstance(v, (bool, str)) else float(v) for v in weights)
        except (TypeError, ValueError):
            w = ()
        if len(w) != M or not all(math.isfinite(v) and v >= 0 for v in w):
            raise ValueError("msssim3d: weights must be %d finite numbers, none negative (got %r)" % (M, weights))
    lib = H.load()
    need = lib.ddpm3d_msssim3d_workspace_bytes(K, D, Hh, W, M)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    with torch.cuda.device(target.device):
        ws = torch.empty(max(need, 16) // 8, dtype=torch.float64, device=target.device)
        out = torch.empty((K, M, 3), dtype=torch.float64, device=target.device)
        H.check(lib.ddpm3d_msssim3d(H.ptr(estimate), H.ptr(target), H.ptr(mask), K, D, Hh, W, M, c1, c2, H.ptr(ws),
                                    ws.numel() * 8, H.ptr(out), H.stream()))
        rec = out.cpu().tolist()                       # the one device-to-host copy (it waits for the stream)
    values, details = [], []
    for r in rec:
        for j, (_, _, n) in enumerate(r):
            if n == 0:
                raise ValueError("msssim3d: the mask counts no interior voxel at scale %d" % j)
        cs = [r[j][1] / r[j][2] for j in range(M - 1)]
        last = r[M - 1][0] / r[M - 1][2]
        terms = cs + [last]
        value = 0.0 if any(not t > 0 for t in terms) else math.prod(t ** e for t, e in zip(terms, w))
        values.append(value)
        details.append({"cs": cs, "ssim": last})
    if not batched:
        values, details = values[0], details[0]
    return (values, details) if parts else values


def evaluate(estimate, target, data_range=None, mask=None, std=None, msssim_scales=0):
    """All figures of one estimate (or K of them) against the target: psnr, nrmse, mae, bias, ssim, data_range,
    n_voxels and, with `std`, coverage_1 / coverage_2; msssim_scales M > 0 adds msssim = msssim3d over M scales with
    the default weights.  data_range None: max - min of the target over the counted voxels.  Python floats, or lists
    of K; data_range and n_voxels are the same for every estimate."""
    if isinstance(msssim_scales, bool) or not isinstance(msssim_scales, int) or msssim_scales < 0:
        raise ValueError("evaluate: msssim_scales must be an int, 0 (none) or 1..%d (got %r)"
                         % (H.MSSSIM_MAX_SCALES, msssim_scales))
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
    if msssim_scales:
        res["msssim"] = msssim3d(estimate, target, data_range, msssim_scales, mask=mask)
    return res


def interval_figures(q_lo, q_hi, target, mask=None):
    """A per-voxel credible interval [q_lo, q_hi] (two quantile maps of uncertainty.draw_quantiles) against the target,
    over the voxels the mask counts (all without one): {"coverage": the share with q_lo <= target <= q_hi, an integer
    count over n_voxels, "mean_width": the fp64 mean of q_hi - q_lo, "n_voxels"}.  A voxel with a NaN bound is not
    covered.  torch reductions on the device, one copy to the host."""
    for t, what in ((q_lo, "q_lo"), (q_hi, "q_hi"), (target, "target")):
        H.require_device(t, what)
    if not tuple(q_lo.shape) == tuple(q_hi.shape) == tuple(target.shape):
        raise ValueError("interval_figures: q_lo %s, q_hi %s and target %s must share one shape"
                         % (tuple(q_lo.shape), tuple(q_hi.shape), tuple(target.shape)))
    inside = (q_lo <= target) & (target <= q_hi)
    width = q_hi.double() - q_lo.double()
    if mask is not None:
        if not (isinstance(mask, torch.Tensor) and mask.is_cuda and tuple(mask.shape) == tuple(target.shape)):
            raise ValueError("interval_figures: mask must be a GPU tensor of the target's shape %s"
                             % (tuple(target.shape),))
        counted = mask != 0
        n = counted.sum()
        inside, width = inside & counted, torch.where(counted, width, torch.zeros_like(width))
    else:
        n = torch.tensor(target.numel(), device=target.device)
    n, covered, total = torch.stack([n.double(), inside.sum().double(), width.sum()]).cpu().tolist()
    n, covered = int(n), int(covered)
    if n == 0:
        raise ValueError("interval_figures: the mask counts no voxel")
    return {"coverage": covered / n, "mean_width": total / n, "n_voxels": n}


# ----------------------------------------------------------------- per-step convergence trace
class StepTrace:
    """The trace= argument of a sampling loop: per reverse step k and sample b, one ddpm3d_trace_moments record of
    that step's pred_xstart x (include/ddpm3d.h has the columns): its weighted moments against `target`, against the
    previous step's pred_xstart and on its own.

    target, weight  optional device float32 tensors of the loop's x shape (every sample has its own target and
                    weights) or of one sample's shape (shared by all samples).  Only voxels with weight > 0 count;
                    no weight counts every voxel with weight 1.
    The first step allocates a (T, N, REC) float64 table and the workspace on x's device; every step writes row k with
    one call.  Nothing waits for the device until records().  `t` lists the original timestep of each row.  One
    StepTrace serves one run of one loop."""

    def __init__(self, target=None, weight=None):
        for name, v in (("target", target), ("weight", weight)):
            if v is not None:
                H.require_device(v, name)
        self.target, self.weight = target, weight
        self.t = []
        self._table = self._ws = None

    def _stride(self, v, est, name):
        if v is None:
            return 0
        if v.device != est.device:
            raise ValueError("StepTrace: %s on %s, the loop's x on %s" % (name, v.device, est.device))
        if tuple(v.shape) == tuple(est.shape):
            return est[0].numel()
        if tuple(v.shape) == tuple(est.shape[1:]):
            return 0
        raise ValueError("StepTrace: %s of shape %s; the loop's x has shape %s (want that, or one sample's %s)"
                         % (name, tuple(v.shape), tuple(est.shape), tuple(est.shape[1:])))

    def add(self, est, prev, t, steps):
        """Called by the loops: row len(self.t) of `steps` <- the records of est (N, ...) against prev (the previous
        step's est, None on the first step); t is the step's original timestep.  Enqueue-only."""
        H.require_device(est, "pred_xstart")
        N, voxels = int(est.shape[0]), est[0].numel()
        k = len(self.t)
        lib = H.load()
        if self._table is None:
            if not 1 <= N <= H.TRACE_MAX_BATCH:
                raise ValueError("StepTrace: %d samples per step (1..%d)" % (N, H.TRACE_MAX_BATCH))
            self._strides = self._stride(self.target, est, "target"), self._stride(self.weight, est, "weight")
            need = lib.ddpm3d_trace_moments_workspace_bytes(N, voxels)
            self._ws = torch.empty(max(need, 16) // 8, dtype=torch.float64, device=est.device)
            self._table = torch.zeros((int(steps), N, H.TR_REC), dtype=torch.float64, device=est.device)
            self._shape = tuple(est.shape)
        if k >= self._table.shape[0] or tuple(est.shape) != self._shape:
            raise ValueError("StepTrace: step %d of shape %s does not fit the trace begun with %d steps of shape %s "
                             "(one StepTrace serves one run of one loop)"
                             % (k, tuple(est.shape), self._table.shape[0], self._shape))
        if prev is not None:
            H.require_device(prev, "previous pred_xstart")
            assert prev.shape == est.shape
        H.check(lib.ddpm3d_trace_moments(H.ptr(est), H.ptr(prev), H.ptr(self.target), H.ptr(self.weight), N, voxels,
                                         self._strides[0], self._strides[1], H.ptr(self._ws), self._ws.numel() * 8,
                                         H.ptr(self._table[k]), H.stream()))
        self.t.append(int(t))

    def device_records(self):
        """The (T, N, REC) float64 table on the device, no copy and no wait: rows not yet written are 0."""
        if self._table is None:
            raise ValueError("StepTrace: no step was traced")
        return self._table

    def records(self):
        """The rows written so far as a float64 numpy array (T, N, REC): the one device-to-host copy (it waits for
        the stream)."""
        if self._table is None:
            raise ValueError("StepTrace: no step was traced")
        return self._table[:len(self.t)].cpu().numpy()

    def figures(self, data_range=None):
        """trace_figures of records(), pooled over the samples."""
        return trace_figures(self.records(), data_range=data_range, has_target=self.target is not None)


def trace_figures(records, data_range=None, has_target=True):
    """Host only.  records: (T, M, REC) ddpm3d_trace_moments records (or (T, REC)), pooled per step by summing the M
    records in index order.  -> a list of T dicts: psnr = 10 log10(L^2 / mse) with L = data_range and
    mse = SUM_SQ_E / W, nrmse = sqrt(SUM_SQ_E / SUM_SQ_Y), mae, bias, mean = SUM_X / W,
    std = sqrt(max(SUM_SQ_X / W - mean^2, 0)), delta_rms = sqrt(SUM_SQ_D / W) (None on the first step),
    clipped = CLIPPED / W, weight = W, and mse itself.  A figure is None when its denominator is 0, psnr also when
    data_range is None, and psnr, nrmse, mae, bias and mse when no target was given (has_target=False)."""
    rec = np.asarray(records, dtype=np.float64)
    if rec.ndim == 2:
        rec = rec[:, None, :]
    if rec.ndim != 3 or rec.shape[2] != H.TR_REC:
        raise ValueError("trace_figures: records of shape %s (want (T, M, %d) or (T, %d))"
                         % (rec.shape, H.TR_REC, H.TR_REC))
    if data_range is not None and not (isinstance(data_range, (int, float)) and math.isfinite(data_range)
                                       and data_range > 0):
        raise ValueError("trace_figures: data_range must be a positive finite number or None (got %r)"
                         % (data_range,))
    pooled = np.zeros((rec.shape[0], H.TR_REC), dtype=np.float64)
    for m in range(rec.shape[1]):                   # a fixed order: the same bits however the records were batched
        pooled += rec[:, m]
    rows = []
    for k, r in enumerate(pooled.tolist()):
        W = r[H.TR_W]
        over = (lambda v: v / W) if W > 0 else (lambda v: None)
        err = has_target and W > 0
        mse = r[H.TR_SUM_SQ_E] / W if err else None
        mean = over(r[H.TR_SUM_X])
        rows.append({
            "psnr": psnr(mse, data_range) if err and data_range is not None else None,
            "nrmse": math.sqrt(r[H.TR_SUM_SQ_E] / r[H.TR_SUM_SQ_Y]) if err and r[H.TR_SUM_SQ_Y] > 0 else None,
            "mae": r[H.TR_SUM_ABS_E] / W if err else None,
            "bias": r[H.TR_SUM_E] / W if err else None,
            "mse": mse,
            "mean": mean,
            "std": None if mean is None else math.sqrt(max(r[H.TR_SUM_SQ_X] / W - mean * mean, 0.0)),
            "delta_rms": None if k == 0 or not W > 0 else math.sqrt(r[H.TR_SUM_SQ_D] / W),
            "clipped": over(r[H.TR_CLIPPED]),
            "weight": W,
        })
    return rows


# ----------------------------------------------------------------- per-region statistics
class RoiIndex:
    """A labelled volume as a region index (roi_index): `labels` (ascending positive ints), `counts` and host
    `offsets` per region, the sorted flat voxel indices on the device, and the ddpm3d_roi_index descriptor."""

    def __init__(self, shape, labels, counts, index):
        self.shape = tuple(int(v) for v in shape)
        self.voxels = int(math.prod(self.shape))
        self.labels = [int(v) for v in labels]
        self.counts = [int(v) for v in counts]
        self.index = index                                        # device int64 [entries]
        self.device = index.device
        offsets = [0]
        for n in self.counts:
            offsets.append(offsets[-1] + n)
        chunks = [0]
        for n in self.counts:
            chunks.append(chunks[-1] + (n + H.ROI_CHUNK - 1) // H.ROI_CHUNK)
        self.offsets = offsets
        self._host = (ctypes.c_int64 * len(offsets))(*offsets)
        self._dev = torch.tensor([offsets, chunks], dtype=torch.int64).to(self.device)
        self.desc = H.RoiIndex(len(self.labels), offsets[-1], self._host, H.ptr(self._dev[0]), H.ptr(self._dev[1]),
                               H.ptr(index))
        self._region_of = None

    def __len__(self):
        return len(self.labels)

    def region_of(self):
        """The dense map ddpm3d_roi_texture reads: a device int16 tensor of the volume's shape holding ordinal + 1 of
        the voxel's region in this index, 0 for a voxel of none.  Built on first use with torch ops from `index` and
        `counts` and cached: it costs 2 bytes per voxel for as long as the index lives."""
        if self._region_of is None:
            with torch.cuda.device(self.device):
                ordinal = torch.repeat_interleave(
                    torch.arange(1, len(self.labels) + 1, dtype=torch.int16, device=self.device),
                    torch.tensor(self.counts, dtype=torch.int64, device=self.device))
                dense = torch.zeros(self.voxels, dtype=torch.int16, device=self.device)
                dense[self.index] = ordinal
                self._region_of = dense.view(self.shape)
        return self._region_of


def roi_index(labels, keep=None):
    """The region index of a device integer tensor (D, H, W): 0 is unlabelled, every distinct positive value is a
    region, in ascending order; voxels with keep == 0 (an optional uint8 tensor of the same shape) are dropped.
    Built on the device with torch ops, once, and reused for every estimate."""
    if not (isinstance(labels, torch.Tensor) and labels.is_cuda):
        raise RuntimeError("labels must live on the GPU: this package runs on HIP kernels only "
                           "(got %s)" % getattr(labels, "device", type(labels)))
    if labels.dtype not in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64) or labels.dim() != 3:
        raise ValueError("roi_index: labels must be an integer tensor (D, H, W), got %s of shape %s"
                         % (labels.dtype, tuple(labels.shape)))
    flat = labels.reshape(-1)
    if keep is not None:
        if not (isinstance(keep, torch.Tensor) and keep.is_cuda and keep.dtype == torch.uint8
                and tuple(keep.shape) == tuple(labels.shape)):
            raise ValueError("roi_index: keep must be a device uint8 tensor of the labels' shape %s"
                             % (tuple(labels.shape),))
        flat = torch.where(keep.reshape(-1) != 0, flat, torch.zeros_like(flat))
    with torch.cuda.device(labels.device):
        if int(flat.min()) < 0:
            raise ValueError("roi_index: negative labels")
        at = torch.nonzero(flat).squeeze(1)                        # ascending flat indices, int64
        if at.numel() == 0:
            raise ValueError("roi_index: no labelled voxel")
        values, order = torch.sort(flat[at].to(torch.int64), stable=True)
        found, counts = torch.unique_consecutive(values, return_counts=True)
        if found.numel() > H.ROI_MAX_REGIONS:
            raise ValueError("roi_index: %d regions (at most %d)" % (found.numel(), H.ROI_MAX_REGIONS))
        return RoiIndex(labels.shape, found.tolist(), counts.tolist(), at[order].contiguous())


def _roi_moments_device(estimate, index, target=None):
    """roi_moments' checks and launch: the (K, R, H.ROI_REC) fp64 records, still on the device"""
    H.require_device(estimate, "estimate")
    if estimate.dim() not in (3, 4) or tuple(estimate.shape[-3:]) != index.shape or estimate.device != index.device:
        raise ValueError("roi_moments: estimate of shape %s on %s against an index of a %s volume on %s"
                         % (tuple(estimate.shape), estimate.device, index.shape, index.device))
    if target is not None:
        H.require_device(target, "target")
        if tuple(target.shape) != index.shape or target.device != index.device:
            raise ValueError("roi_moments: target of shape %s, index of a %s volume" % (tuple(target.shape),
                                                                                      index.shape))
    K = int(estimate.shape[0]) if estimate.dim() == 4 else 1
    if not 1 <= K <= H.MAX_DRAWS:
        raise ValueError("roi_moments: %d estimates (1..%d)" % (K, H.MAX_DRAWS))
    lib = H.load()
    need = lib.ddpm3d_roi_moments_workspace_bytes(K, index.desc)
    with torch.cuda.device(index.device):
        ws = torch.empty(max(need, 16) // 8, dtype=torch.float64, device=index.device)
        out = torch.empty((K, len(index), H.ROI_REC), dtype=torch.float64, device=index.device)
        H.check(lib.ddpm3d_roi_moments(H.ptr(estimate), H.ptr(target), K, index.voxels, index.desc, H.ptr(ws),
                                       ws.numel() * 8, H.ptr(out), H.stream()))
    return out


def roi_moments(estimate, index, target=None):
    """ddpm3d_roi_moments of a (D, H, W) or (K, D, H, W) estimate over a region index: one launch, one
    device-to-host copy.  -> the R records of the regions, each a list of H.ROI_REC floats (columns H.ROI_*; the
    three error columns are 0 without a target); a list of K such lists for a (K, D, H, W) estimate."""
    rec = _roi_moments_device(estimate, index, target).cpu().tolist()   # the one device-to-host copy (it waits)
    return rec if estimate.dim() == 4 else rec[0]


def _ratio(a, b):
    return None if a is None or b is None or b == 0 else a / b


def _region(rec):
    """n, mean, std (population), min, max, cov of one record"""
    n = int(rec[H.ROI_N])
    mean = _ratio(rec[H.ROI_SUM_X], n)
    std = None if mean is None else math.sqrt(max(rec[H.ROI_SUM_SQ_X] / n - mean * mean, 0.0))
    return {"n": n, "mean": mean, "std": std, "min": rec[H.ROI_MIN_X] if n else None,
            "max": rec[H.ROI_MAX_X] if n else None, "cov": _ratio(std, mean)}


def roi_figures(records, target_records=None, labels=None, background=None, draw_records=None, *, spacing=None,
                peaks=None, target_peaks=None, draw_peaks=None, texture=None, target_texture=None, draw_texture=None):
    """Records to figures, on the host: {label: figures} for the R records of one estimate (roi_moments' return).
    Per region n, mean, std (population), min, max, cov = std / mean.  With target_records, the target's own records
    (roi_moments(target, index)) beside records taken against that target: mean_bias, mean_bias_rel, max_bias_rel,
    rmse, mae.  With a background label g, for every other region contrast = mean_r / mean_g - 1, cnr =
    (mean_r - mean_g) / std_g and, with target_records, crc = contrast / the target's contrast.  With draw_records
    (K >= 2 lists of R records): draw_means, mean_std (sample std of the K region means, ddof = 1) and, with
    target_records, mean_z = (mean of the draw means - target mean) / mean_std.  A figure whose denominator is 0 is
    None.  labels default to 0..R-1.  The keyword-only arguments add figures and change none: spacing (mm per voxel,
    three numbers): volume_ml = n s0 s1 s2 / 1000 (the MTV of a lesion), tlg = volume_ml * mean and, with
    target_records, tlg_bias_rel; peaks (R values, roi_peak's return): peak and, with target_peaks, peak_bias_rel =
    (peak - target peak) / target peak; draw_peaks (K >= 2 lists of R values): draw_peaks and peak_std (sample std,
    ddof = 1); texture (R dicts, texture_figures' return): texture and, with target_texture (the target's own R
    dicts), texture_rel = (f - target's f) / target's f per figure, None where either is None or the denominator is
    0; draw_texture (K >= 2 lists of R dicts): draw_texture and texture_std (sample std per figure, ddof = 1, over
    the draws where it is defined)."""
    R = len(records)
    labels = list(range(R)) if labels is None else [int(v) for v in labels]
    if len(labels) != R or (target_records is not None and len(target_records) != R):
        raise ValueError("roi_figures: %d records, %d labels, %s target records"
                         % (R, len(labels), None if target_records is None else len(target_records)))
    if draw_records is not None and (len(draw_records) < 2 or any(len(d) != R for d in draw_records)):
        raise ValueError("roi_figures: draw_records must be K >= 2 lists of %d records" % R)
    if background is not None and background not in labels:
        raise ValueError("roi_figures: background label %r is not a region (%s)" % (background, labels))
    if any(p is not None and len(p) != R for p in (peaks, target_peaks)):
        raise ValueError("roi_figures: peaks and target_peaks must hold %d values" % R)
    if draw_peaks is not None and (len(draw_peaks) < 2 or any(len(d) != R for d in draw_peaks)):
        raise ValueError("roi_figures: draw_peaks must be K >= 2 lists of %d values" % R)
    if any(t is not None and len(t) != R for t in (texture, target_texture)):
        raise ValueError("roi_figures: texture and target_texture must hold %d dicts" % R)
    if draw_texture is not None and (len(draw_texture) < 2 or any(len(d) != R for d in draw_texture)):
        raise ValueError("roi_figures: draw_texture must be K >= 2 lists of %d dicts" % R)
    voxel_ml = None if spacing is None else math.prod(_check_spacing(spacing, "roi_figures")) / 1000.0
    figs = [_region(r) for r in records]
    tfigs = None if target_records is None else [_region(r) for r in target_records]
    g = None if background is None else labels.index(background)
    out = {}
    for i, (label, rec, f) in enumerate(zip(labels, records, figs)):
        n = f["n"]
        if tfigs is not None:
            t = tfigs[i]
            f["mean_bias"] = None if f["mean"] is None or t["mean"] is None else f["mean"] - t["mean"]
            f["mean_bias_rel"] = _ratio(f["mean_bias"], t["mean"])
            f["max_bias_rel"] = None if not n or t["max"] is None else _ratio(f["max"] - t["max"], t["max"])
            f["rmse"] = math.sqrt(rec[H.ROI_SUM_SQ_E] / n) if n else None
            f["mae"] = _ratio(rec[H.ROI_SUM_ABS_E], n)
        if g is not None and i != g:
            bg = figs[g]
            ratio = _ratio(f["mean"], bg["mean"])
            f["contrast"] = None if ratio is None else ratio - 1.0
            if tfigs is not None:
                tr = _ratio(tfigs[i]["mean"], tfigs[g]["mean"])
                f["crc"] = _ratio(f["contrast"], None if tr is None else tr - 1.0)
            f["cnr"] = None if f["mean"] is None or bg["mean"] is None else _ratio(f["mean"] - bg["mean"], bg["std"])
        if draw_records is not None:
            means = [_ratio(d[i][H.ROI_SUM_X], int(d[i][H.ROI_N])) for d in draw_records]
            f["draw_means"] = means
            f["mean_std"] = f["mean_z"] = None
            if n:
                K = len(means)
                centre = math.fsum(means) / K
                f["mean_std"] = math.sqrt(math.fsum((m - centre) ** 2 for m in means) / (K - 1))
                if tfigs is not None:
                    f["mean_z"] = _ratio(centre - tfigs[i]["mean"], f["mean_std"])
        if voxel_ml is not None:
            f["volume_ml"] = n * voxel_ml
            f["tlg"] = None if f["mean"] is None else f["volume_ml"] * f["mean"]
            if tfigs is not None:
                t = tfigs[i]
                t_tlg = None if t["mean"] is None else t["n"] * voxel_ml * t["mean"]
                f["tlg_bias_rel"] = None if f["tlg"] is None or t_tlg is None else _ratio(f["tlg"] - t_tlg, t_tlg)
        if peaks is not None:
            f["peak"] = peaks[i] if n else None
            if target_peaks is not None:
                tp = target_peaks[i] if n else None
                f["peak_bias_rel"] = None if tp is None else _ratio(f["peak"] - tp, tp)
        if draw_peaks is not None:
            f["draw_peaks"] = [d[i] if n else None for d in draw_peaks]
            f["peak_std"] = None
            if n:
                K = len(draw_peaks)
                centre = math.fsum(f["draw_peaks"]) / K
                f["peak_std"] = math.sqrt(math.fsum((v - centre) ** 2 for v in f["draw_peaks"]) / (K - 1))
        if texture is not None:
            f["texture"] = texture[i]
            if target_texture is not None:
                f["texture_rel"] = _texture_rel(texture[i], target_texture[i])
        if draw_texture is not None:
            f["draw_texture"] = [d[i] for d in draw_texture]
            f["texture_std"] = _texture_std(f["draw_texture"])
        out[label] = f
    return out


def roi_report(estimate, target, index, labels=None, background=None, draws=None, *, spacing=None, volume_mm3=None,
               keep=None, draw_peaks=None, footprint=None, target_peaks=None, texture=None, draw_texture=None,
               target_texture=None):
    """Region figures of one (D, H, W) estimate against the target: {label: {"n", "target": the target's own n,
    mean, std, min, max, cov, "estimate": roi_figures of the estimate}}.  labels names the regions (default: the
    index's own labels); draws is a (K, D, H, W) device tensor of K >= 2 posterior draws or their K lists of records
    (roi_moments of each draw).  The target's own statistics come from one roi_moments(target, index) call.
    With spacing (mm per voxel along the tensors' three axes) both blocks gain volume_ml, tlg and peak (roi_peak over
    the sphere of volume_mm3, default 1000; keep as in sphere_mean) and the estimate tlg_bias_rel and peak_bias_rel;
    draws given as a tensor, or draw_peaks (K lists of roi_peak's values, for draws given as records), add draw_peaks
    and peak_std.  A caller that reports several estimates against one target passes the footprint it already has
    (sphere_footprint of the same spacing; volume_mm3 is then not given) and the target's peaks (roi_peak(target,
    ...)) so that neither is computed again.
    With texture = {"bin_width": w, "levels": 64, "lower": 0.0} (fixed bin size: the same bins for the target and every
    estimate, so that their figures are comparable; levels and lower are optional) both blocks gain "texture"
    (texture_figures of roi_texture) and the estimate "texture_rel" against the target's; draws given as a tensor, or
    draw_texture (K lists of texture_figures' R dicts, for draws given as records), add draw_texture and texture_std;
    target_texture passes the target's own figures when the caller has them already.  Without texture the return is
    what it was."""
    labels = index.labels if labels is None else labels
    if texture is None and not (draw_texture is None and target_texture is None):
        raise ValueError("roi_report: draw_texture and target_texture need texture")
    if texture is not None:
        if not isinstance(texture, dict) or set(texture) - {"levels", "bin_width", "lower"} or \
                texture.get("bin_width") is None:
            raise ValueError("roi_report: texture must be a dict with bin_width and optionally levels and lower "
                             "(got %r)" % (texture,))
        _check_texture("roi_report", texture.get("levels", 64), texture["bin_width"], texture.get("lower", 0.0))
    if spacing is None and not (volume_mm3 is None and keep is None and draw_peaks is None and footprint is None
                                and target_peaks is None):
        raise ValueError("roi_report: volume_mm3, keep, draw_peaks, footprint and target_peaks need a spacing")
    more, tmore = {}, {}
    if spacing is not None:
        if footprint is None:
            footprint = sphere_footprint(spacing, 1000.0 if volume_mm3 is None else volume_mm3)
        elif volume_mm3 is not None or footprint.spacing != _check_spacing(spacing, "roi_report"):
            raise ValueError("roi_report: the footprint given is its own volume_mm3 and must be of the spacing %r"
                             % (spacing,))
        tpeaks = roi_peak(target, index, footprint, keep=keep) if target_peaks is None else target_peaks
        if draw_peaks is None and isinstance(draws, torch.Tensor):
            draw_peaks = roi_peak(draws, index, footprint, keep=keep)
        tmore = dict(spacing=spacing, peaks=tpeaks)
        more = dict(spacing=spacing, peaks=roi_peak(estimate, index, footprint, keep=keep), target_peaks=tpeaks,
                    draw_peaks=draw_peaks)
    if texture is not None:
        ttex = texture_figures(roi_texture(target, index, **texture)) if target_texture is None else target_texture
        if draw_texture is None and isinstance(draws, torch.Tensor):
            draw_texture = texture_figures(roi_texture(draws, index, **texture))
        tmore = dict(tmore, texture=ttex)
        more = dict(more, texture=texture_figures(roi_texture(estimate, index, **texture)), target_texture=ttex,
                    draw_texture=draw_texture)
    trec = roi_moments(target, index)
    if isinstance(draws, torch.Tensor):
        draws = roi_moments(draws, index)
    est = roi_figures(roi_moments(estimate, index, target=target), target_records=trec, labels=labels,
                      background=background, draw_records=draws, **more)
    tgt = roi_figures(trec, labels=labels, **tmore)
    return {label: {"n": tgt[label]["n"], "target": tgt[label], "estimate": est[label]} for label in labels}


# ----------------------------------------------------------------- per-region texture
TEXTURE_DIRECTIONS = 13
# what keeps the region's maximum inside the top bin of fixed-bin-number discretisation: with inv_w = levels (1 - 8 u)
# / (max - min) rounded to fp32 (u = 2^-24), the fp32 product (max - min) * inv_w is at most levels (1 - 8 u)(1 + u)^2 <
# levels (1 - 2 u), which lies below the fp32 predecessor of `levels`
_FBN_SHRINK = 1.0 - 2.0 ** -21


class RoiTexture:
    """roi_texture's return: the integer matrices of ddpm3d_roi_texture as numpy int64 arrays, `glcm` (K, R, levels,
    levels), `hist` (K, R, levels) and `counts` (K, R, H.TEX_REC; columns H.TEX_*), the discretisation `lo` and
    `inv_w` (K, R) float32, `levels`, the index's `labels`, and `batched`: whether the estimate was a (K, D, H, W)
    stack (K = 1 otherwise)."""

    def __init__(self, glcm, hist, counts, lo, inv_w, levels, labels, batched):
        self.glcm, self.hist, self.counts, self.lo, self.inv_w = glcm, hist, counts, lo, inv_w
        self.levels, self.labels, self.batched = levels, labels, batched


def _check_texture(what, levels, bin_width, lower):
    """(levels, bin_width or None, lower) of a texture request, refused on the host"""
    if isinstance(levels, bool) or not isinstance(levels, int) or not 2 <= levels <= H.TEX_MAX_LEVELS:
        raise ValueError("%s: levels must be an integer in 2..%d (got %r)" % (what, H.TEX_MAX_LEVELS, levels))
    number = lambda v: (not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating))
                        and math.isfinite(v))
    if bin_width is not None and not (number(bin_width) and bin_width > 0 and 1.0 / float(bin_width) < 3.0e38):
        raise ValueError("%s: bin_width must be a positive finite number or None (got %r)" % (what, bin_width))
    if not number(lower):
        raise ValueError("%s: lower must be a finite number (got %r)" % (what, lower))
    return levels, None if bin_width is None else float(bin_width), float(lower)


def roi_texture(estimate, index, *, levels=64, bin_width=None, lower=0.0):
    """The grey-level co-occurrence matrices, grey-level histograms and side counters of every region of the index
    in a (D, H, W) or (K, D, H, W) estimate: one call of ddpm3d_roi_texture (csrc/texture.hip; include/ddpm3d.h has
    the definition: 13 directions at distance 1, merged, symmetric) and one device-to-host copy.  A value x of region
    r gets the grey level min(max(floor((x - lo) * inv_w), 0), levels - 1) in fp32.  With bin_width (fixed bin size,
    what IBSI recommends for SUV) lo = lower and inv_w = 1 / bin_width for every region and estimate, so that the
    figures of several volumes are comparable.  Without it (fixed bin number) lo is the region's own minimum in that
    estimate and inv_w = levels (1 - 2^-21) / (max - min), 0 for a flat region, both from one ddpm3d_roi_moments
    launch and kept on the device: the factor keeps the maximum inside the top bin instead of on its upper edge.
    Uses index.region_of().  -> RoiTexture"""
    levels, bin_width, lower = _check_texture("roi_texture", levels, bin_width, lower)
    H.require_device(estimate, "estimate")
    if estimate.dim() not in (3, 4) or tuple(estimate.shape[-3:]) != index.shape or estimate.device != index.device:
        raise ValueError("roi_texture: estimate of shape %s on %s against an index of a %s volume on %s"
                         % (tuple(estimate.shape), estimate.device, index.shape, index.device))
    K = int(estimate.shape[0]) if estimate.dim() == 4 else 1
    if not 1 <= K <= H.MAX_DRAWS:
        raise ValueError("roi_texture: %d estimates (1..%d)" % (K, H.MAX_DRAWS))
    if max(index.shape) > 65535 or index.voxels > 2 ** 31 - 1:
        raise ValueError("roi_texture: a volume of %s (every extent at most 65535, at most 2^31 - 1 voxels)"
                         % (index.shape,))
    lib = H.load()
    R, D, Hh, W = len(index), index.shape[0], index.shape[1], index.shape[2]
    sizes = [K * R * levels * levels, K * R * levels, K * R * H.TEX_REC, K * R]
    with torch.cuda.device(index.device):
        # one buffer, so that one copy brings everything back: the three outputs, then lo and inv_w as 2 K R floats
        buf = torch.empty(sum(sizes), dtype=torch.int64, device=index.device)
        glcm, hist, counts, tail = torch.split(buf, sizes)
        params = tail.view(torch.float32).view(2, K, R)
        if bin_width is not None:
            params[0] = float(np.float32(lower))
            params[1] = float(np.float32(1.0 / bin_width))
        else:
            rec = _roi_moments_device(estimate, index)
            mn, mx = rec[..., H.ROI_MIN_X], rec[..., H.ROI_MAX_X]
            some = mx > mn
            params[0] = torch.where(rec[..., H.ROI_N] > 0, mn, torch.zeros_like(mn)).to(torch.float32)
            params[1] = torch.where(some, (levels * _FBN_SHRINK) / torch.where(some, mx - mn, torch.ones_like(mn)),
                                    torch.zeros_like(mn)).to(torch.float32)
        H.check(lib.ddpm3d_roi_texture(H.ptr(estimate), K, D, Hh, W, index.desc, H.ptr(index.region_of()),
                                       H.ptr(params[0]), H.ptr(params[1]), levels, H.ptr(glcm), H.ptr(hist),
                                       H.ptr(counts), H.stream()))
        host = buf.cpu().numpy()                       # the one device-to-host copy (it waits for the stream)
    glcm, hist, counts, tail = np.split(host, np.cumsum(sizes)[:-1])
    params = tail.view(np.float32).reshape(2, K, R)
    return RoiTexture(glcm.reshape(K, R, levels, levels), hist.reshape(K, R, levels), counts.reshape(K, R, H.TEX_REC),
                      params[0].copy(), params[1].copy(), levels, list(index.labels), estimate.dim() == 4)


TEXTURE_FIGURES = ("joint_entropy", "angular_second_moment", "contrast", "dissimilarity", "inverse_difference",
                   "inverse_difference_moment", "joint_average", "joint_variance", "correlation", "hist_entropy",
                   "hist_uniformity", "p10", "p50", "p90", "clamped")


def _texture_region(glcm, hist, counts, lo, inv_w, levels):
    """The figures of one region from its integer matrices, in fp64 (p = C / sum C, i and j 0-based)"""
    n, pairs = int(counts[H.TEX_N]), int(counts[H.TEX_PAIRS])
    out = {"n": n, "pairs": pairs}
    if pairs == 0:
        out.update({k: None for k in TEXTURE_FIGURES})
        return out
    p = glcm.astype(np.float64) / float(glcm.sum())
    i = np.arange(levels, dtype=np.float64)[:, None]
    j = np.arange(levels, dtype=np.float64)[None, :]
    d = np.abs(i - j)
    some = p > 0
    out["joint_entropy"] = float(-np.sum(p[some] * np.log2(p[some])))
    out["angular_second_moment"] = float(np.sum(p * p))
    out["contrast"] = float(np.sum(d * d * p))
    out["dissimilarity"] = float(np.sum(d * p))
    out["inverse_difference"] = float(np.sum(p / (1.0 + d)))
    out["inverse_difference_moment"] = float(np.sum(p / (1.0 + d * d)))
    mu = float(np.sum(i * p))
    var = float(np.sum((i - mu) ** 2 * p))
    out["joint_average"], out["joint_variance"] = mu, var
    out["correlation"] = None if var == 0 else (float(np.sum(i * j * p)) - mu * mu) / var
    q = hist.astype(np.float64) / n
    out["hist_entropy"] = float(-np.sum(q[q > 0] * np.log2(q[q > 0])))
    out["hist_uniformity"] = float(np.sum(q * q))
    cum = np.cumsum(hist.astype(np.int64))
    for pct in (10, 50, 90):                           # the first bin whose cumulative count reaches pct % of n
        g = int(np.argmax(cum * 100 >= pct * n))
        out["p%d" % pct] = None if inv_w == 0 else float(lo) + (g + 0.5) / float(inv_w)
    out["clamped"] = (int(counts[H.TEX_BELOW]) + int(counts[H.TEX_ABOVE])) / n
    return out


def texture_figures(result):
    """Haralick's figures as IBSI defines them, from roi_texture's integer matrices, on the host in fp64: per region a
    dict with n (counted voxels), pairs, and from p = C / sum C: joint_entropy = -sum p log2 p,
    angular_second_moment = sum p^2, contrast = sum (i - j)^2 p, dissimilarity = sum |i - j| p, inverse_difference =
    sum p / (1 + |i - j|), inverse_difference_moment = sum p / (1 + (i - j)^2), joint_average mu = sum i p,
    joint_variance = sum (i - mu)^2 p, correlation = (sum i j p - mu^2) / variance (None for variance 0); from the
    histogram q = hist / n: hist_entropy, hist_uniformity = sum q^2 and p10, p50, p90 in the volume's units (lo +
    (g + 0.5) / inv_w for the first bin g whose cumulative count reaches that share of n; None for inv_w = 0); and
    clamped, the share of counted voxels outside the bins.  Every figure of a region without pairs is None.  -> a list
    of R dicts, K such lists for a (K, D, H, W) estimate."""
    rows = [[_texture_region(result.glcm[k, r], result.hist[k, r], result.counts[k, r], result.lo[k, r],
                             result.inv_w[k, r], result.levels) for r in range(result.glcm.shape[1])]
            for k in range(result.glcm.shape[0])]
    return rows if result.batched else rows[0]


def _texture_rel(f, t):
    """(f - t) / t per figure; None where either is None or t is 0"""
    return {k: None if f[k] is None or t[k] is None else _ratio(f[k] - t[k], t[k]) for k in f}


def _texture_std(draws):
    """the sample std (ddof = 1) per figure over the draws where it is defined; None with fewer than two"""
    out = {}
    for k in draws[0]:
        v = [d[k] for d in draws if d[k] is not None]
        centre = math.fsum(v) / len(v) if v else 0.0
        out[k] = math.sqrt(math.fsum((x - centre) ** 2 for x in v) / (len(v) - 1)) if len(v) >= 2 else None
    return out


# ----------------------------------------------------------------- SUVpeak, MTV, TLG
def _check_spacing(spacing, what):
    try:
        values = [float(v) for v in spacing]
    except (TypeError, ValueError):
        values = []
    if len(values) != 3 or not all(math.isfinite(v) and v > 0 for v in values):
        raise ValueError("%s: the voxel spacing must be three positive finite numbers, in mm (got %r)"
                         % (what, spacing))
    return tuple(values)


class SphereFootprint:
    """sphere_footprint's return: `spacing` and `volume_mm3` as given, `radius_mm`, the per-axis `radii` (r0, r1, r2)
    in voxels, `half_w`, a (2 r0 + 1) x (2 r1 + 1) tuple of tuples (-1: the row is absent, w: it covers dx in -w..w)
    and the tap count `taps`."""

    def __init__(self, spacing, volume_mm3, radius_mm, radii, half_w):
        self.spacing, self.volume_mm3, self.radius_mm, self.radii = spacing, volume_mm3, radius_mm, radii
        self.half_w = tuple(tuple(row) for row in half_w)
        self.taps = sum(2 * w + 1 for row in self.half_w for w in row if w >= 0)
        flat = [w for row in self.half_w for w in row]
        self.table = (ctypes.c_int32 * len(flat))(*flat)            # what ddpm3d_sphere_mean reads, on the host


def sphere_footprint(spacing, volume_mm3=1000.0):
    """The binary sphere of volume_mm3 (PERCIST's SUVpeak: 1 cm^3) on a grid of `spacing` = (s0, s1, s2) mm per voxel,
    in the axis order of the tensor it will be applied to.  r = (3 V / 4 pi)^(1/3) in fp64 (6.2035 mm for 1000);
    offset (dz, dy, dx) belongs iff (dz s0)^2 + (dy s1)^2 + (dx s2)^2 <= r^2: the voxel centre decides, no partial
    volumes.  A spacing coarser than r on every axis gives the single voxel (the peak is then the maximum).  Refuses a
    spacing that is not three positive finite numbers, a volume that is not positive and finite, and a radius above
    DDPM3D_PEAK_MAX_RADIUS voxels on any axis.  Host arithmetic only.  -> SphereFootprint"""
    s = _check_spacing(spacing, "sphere_footprint")
    try:
        volume = math.nan if isinstance(volume_mm3, (bool, str)) else float(volume_mm3)
    except (TypeError, ValueError):
        volume = math.nan
    if not (math.isfinite(volume) and volume > 0):
        raise ValueError("sphere_footprint: the volume must be a positive finite number of mm^3 (got %r)"
                         % (volume_mm3,))
    volume_mm3 = volume
    r = (3.0 * volume / (4.0 * math.pi)) ** (1.0 / 3.0)
    if any(r / v >= H.PEAK_MAX_RADIUS + 1 for v in s):
        raise ValueError("sphere_footprint: a sphere of %g mm^3 (radius %.4f mm) spans more than %d voxels from its "
                         "centre at a spacing of %s mm: the radius is limited to DDPM3D_PEAK_MAX_RADIUS = %d voxels "
                         "per axis" % (volume_mm3, r, H.PEAK_MAX_RADIUS, s, H.PEAK_MAX_RADIUS))
    inside = lambda dz, dy, dx: (dz * s[0]) ** 2 + (dy * s[1]) ** 2 + (dx * s[2]) ** 2 <= r * r
    reach = lambda axis: max(d for d in range(H.PEAK_MAX_RADIUS + 1) if inside(*[d if a == axis else 0 for a in range(3)]))
    r0, r1, r2 = reach(0), reach(1), reach(2)
    half_w = [[max((dx for dx in range(r2 + 1) if inside(dz, dy, dx)), default=-1) for dy in range(-r1, r1 + 1)]
              for dz in range(-r0, r0 + 1)]
    return SphereFootprint(s, float(volume_mm3), r, (r0, r1, r2), half_w)


def sphere_mean(volume, footprint, keep=None):
    """The mean over the footprint around every voxel of a device float32 (D, H, W) or (K, D, H, W) tensor: one call
    of ddpm3d_sphere_mean (csrc/peak.hip), no host copy.  Only the footprint voxels inside the volume and, with keep
    (a device uint8 tensor (D, H, W), shared by the K volumes), with keep != 0 are counted; a voxel none of whose
    footprint counts gets 0.  keep does not blank the voxel itself.  -> a tensor of the volume's shape."""
    H.require_device(volume, "volume")
    if volume.dim() not in (3, 4):
        raise ValueError("sphere_mean: volume of shape %s (want (D, H, W) or (K, D, H, W))" % (tuple(volume.shape),))
    if not isinstance(footprint, SphereFootprint):
        raise ValueError("sphere_mean: footprint must be sphere_footprint's return (got %r)" % (footprint,))
    shape = tuple(int(v) for v in volume.shape[-3:])
    if keep is not None and not (isinstance(keep, torch.Tensor) and keep.is_cuda and keep.dtype == torch.uint8
                                 and keep.is_contiguous() and tuple(keep.shape) == shape
                                 and keep.device == volume.device):
        raise ValueError("sphere_mean: keep must be a contiguous device uint8 tensor of the volume's shape %s"
                         % (shape,))
    K = int(volume.shape[0]) if volume.dim() == 4 else 1
    if not 1 <= K <= H.MAX_DRAWS:
        raise ValueError("sphere_mean: %d volumes (1..%d)" % (K, H.MAX_DRAWS))
    voxels = shape[0] * shape[1] * shape[2]
    if voxels == 0 or voxels > 2 ** 31 - 1:
        raise ValueError("sphere_mean: %d voxels (1..2^31 - 1)" % voxels)
    lib = H.load()
    with torch.cuda.device(volume.device):
        out = torch.empty_like(volume)
        H.check(lib.ddpm3d_sphere_mean(H.ptr(volume), H.ptr(keep), K, shape[0], shape[1], shape[2],
                                       footprint.radii[0], footprint.radii[1], footprint.table, H.ptr(out),
                                       H.stream()))
    return out


def roi_peak(volume, index, footprint, keep=None):
    """SUVpeak of every region of the index: the largest sphere mean centred on a voxel of the region, i.e. column
    MAX_X of roi_moments(sphere_mean(volume, footprint, keep), index).  -> a list of R floats for a (D, H, W) volume,
    K such lists for a (K, D, H, W) stack."""
    rec = roi_moments(sphere_mean(volume, footprint, keep=keep), index)
    if volume.dim() == 4:
        return [[r[H.ROI_MAX_X] for r in draw] for draw in rec]
    return [r[H.ROI_MAX_X] for r in rec]


# ----------------------------------------------------------------- baseline denoisers
FWHM_PER_SIGMA = 2.0 * math.sqrt(2.0 * math.log(2.0))


class GaussianTaps:
    """gaussian_taps' return: `fwhm_mm` (three values) and `spacing` as given, the per-axis `sigma_voxels`, `radii`
    and `taps`: three tuples of 2 r + 1 fp32 values, exp(-j^2 / 2 sigma^2) for j = -r..r."""

    def __init__(self, fwhm_mm, spacing, sigma_voxels, radii, taps):
        self.fwhm_mm, self.spacing, self.sigma_voxels, self.radii = fwhm_mm, spacing, sigma_voxels, radii
        self.taps = tuple(tuple(t) for t in taps)
        self.tables = tuple((ctypes.c_float * len(t))(*t) for t in self.taps)   # what ddpm3d_gauss_smooth reads


def _positive(value, what):
    try:
        v = math.nan if isinstance(value, (bool, str)) else float(value)
    except (TypeError, ValueError):
        v = math.nan
    if not (math.isfinite(v) and v > 0):
        raise ValueError("%s must be a positive finite number (got %r)" % (what, value))
    return v


def gaussian_taps(fwhm_mm, spacing, truncate=3.0):
    """The taps of a Gaussian post-filter of `fwhm_mm` (one number or three, in mm) on a grid of `spacing` mm per
    voxel, in the axis order of the tensor: per axis sigma = fwhm / (2 sqrt(2 ln 2)) / spacing voxels and the radius
    int(truncate sigma + 0.5), scipy.ndimage.gaussian_filter's rule, so that away from the faces gaussian_smooth
    equals scipy.ndimage.gaussian_filter(x, sigma, truncate=truncate).  The taps are formed in fp64 and rounded to
    fp32.  Refuses a radius above DDPM3D_SMOOTH_MAX_RADIUS voxels and names the axis.  Host arithmetic only.
    -> GaussianTaps"""
    s = _check_spacing(spacing, "gaussian_taps")
    if isinstance(fwhm_mm, (list, tuple)):
        if len(fwhm_mm) != 3:
            raise ValueError("gaussian_taps: the FWHM is one number or three, in mm (got %r)" % (fwhm_mm,))
        fwhm = tuple(_positive(f, "gaussian_taps: the FWHM") for f in fwhm_mm)
    else:
        fwhm = (_positive(fwhm_mm, "gaussian_taps: the FWHM"),) * 3
    truncate = _positive(truncate, "gaussian_taps: truncate")
    sigma = tuple(f / FWHM_PER_SIGMA / v for f, v in zip(fwhm, s))
    radii = tuple(int(truncate * sg + 0.5) for sg in sigma)
    for axis, r in enumerate(radii):
        if r > H.SMOOTH_MAX_RADIUS:
            raise ValueError("gaussian_taps: a FWHM of %g mm at a spacing of %g mm needs a radius of %d voxels along "
                             "axis %d: the radius is limited to DDPM3D_SMOOTH_MAX_RADIUS = %d voxels per axis"
                             % (fwhm[axis], s[axis], r, axis, H.SMOOTH_MAX_RADIUS))
    as_fp32 = lambda v: ctypes.c_float(v).value
    taps = [[as_fp32(math.exp(-0.5 * j * j / (sg * sg))) for j in range(-r, r + 1)] for sg, r in zip(sigma, radii)]
    for axis, t in enumerate(taps):
        if not all(v > 0 for v in t):
            raise ValueError("gaussian_taps: a tap along axis %d underflows fp32 (truncate = %g)" % (axis, truncate))
    return GaussianTaps(fwhm, s, sigma, radii, taps)


def _one_volume(volume, what):
    H.require_device(volume, "volume")
    if volume.dim() != 3:
        raise ValueError("%s: volume of shape %s (want (D, H, W))" % (what, tuple(volume.shape)))
    shape = tuple(int(v) for v in volume.shape)
    voxels = shape[0] * shape[1] * shape[2]
    if voxels == 0 or voxels > 2 ** 31 - 1:
        raise ValueError("%s: %d voxels (1..2^31 - 1)" % (what, voxels))
    return shape


def gaussian_smooth(volume, taps):
    """The separable Gaussian of a device float32 (D, H, W) tensor with gaussian_taps' taps: ddpm3d_gauss_smooth
    (csrc/smooth.hip), no host copy.  Taps beyond a face do not count and the rest are renormalised.  -> a device
    tensor of the volume's shape."""
    if not isinstance(taps, GaussianTaps):
        raise ValueError("gaussian_smooth: taps must be gaussian_taps' return (got %r)" % (taps,))
    shape = _one_volume(volume, "gaussian_smooth")
    lib = H.load()
    with torch.cuda.device(volume.device):
        out = torch.empty_like(volume)
        need = lib.ddpm3d_gauss_smooth_workspace_bytes(*shape)
        ws = torch.empty(max(need, 16) // 4, dtype=torch.float32, device=volume.device)
        H.check(lib.ddpm3d_gauss_smooth(H.ptr(volume), shape[0], shape[1], shape[2], taps.radii[0], taps.radii[1],
                                        taps.radii[2], taps.tables[0], taps.tables[1], taps.tables[2], H.ptr(out),
                                        H.ptr(ws), ws.numel() * 4, H.stream()))
    return out


def _radii(value, limit, what):
    """an int for all three axes, or three ints, each in 0..limit"""
    values = [value] * 3 if isinstance(value, int) and not isinstance(value, bool) else value
    try:
        values = tuple(values)
    except TypeError:
        values = ()
    if len(values) != 3 or not all(isinstance(v, int) and not isinstance(v, bool) and 0 <= v <= limit for v in values):
        raise ValueError("%s must be an int or three ints in 0..%d (got %r)" % (what, limit, value))
    return values


def nlm_check(h, search=(3, 3, 3), patch=(1, 1, 1), sigma=0.0):
    """nlm's refusals of its parameters, on the host.  -> (h, search, patch, sigma) as nlm passes them on"""
    search = _radii(search, H.NLM_MAX_SEARCH, "nlm: the search radius")
    patch = _radii(patch, H.NLM_MAX_PATCH, "nlm: the patch radius")
    h = ctypes.c_float(_positive(h, "nlm: h")).value
    try:
        sigma = math.nan if isinstance(sigma, (bool, str)) else float(sigma)
    except (TypeError, ValueError):
        sigma = math.nan
    if not (math.isfinite(sigma) and sigma >= 0):
        raise ValueError("nlm: sigma must be a finite number, 0 or more (got %r)" % (sigma,))
    sigma = ctypes.c_float(sigma).value
    fp32_max = 3.4028234663852886e38
    n_p = (2 * patch[0] + 1) * (2 * patch[1] + 1) * (2 * patch[2] + 1)
    if h == 0 or math.isinf(h) or math.isinf(sigma):
        raise ValueError("nlm: h and sigma must be finite in fp32, h above 0 (got %r, %r)" % (h, sigma))
    if 1.0 / n_p / h / h > fp32_max or 2.0 * (sigma / h) ** 2 > fp32_max:
        raise ValueError("nlm: h = %r is too small: 1 / (n_p h^2) and 2 sigma^2 / h^2 must be finite in fp32" % (h,))
    return h, search, patch, sigma


def nlm(volume, h, search=(3, 3, 3), patch=(1, 1, 1), sigma=0.0):
    """Non-local means of a device float32 (D, H, W) tensor: ddpm3d_nlm (csrc/nlm.hip), one launch, no host copy.
    Every voxel becomes the weighted mean of the voxels within `search` (radii per axis, or one int for all) that lie
    inside the volume, with the weight exp(-max(d2 - 2 sigma^2, 0) / h^2) of the mean squared difference d2 of the
    patches of radius `patch` around the two (replicate padding), exactly 0 beyond an exponent of 80, and 1 for the
    voxel itself.  -> a device tensor of the volume's shape."""
    h, search, patch, sigma = nlm_check(h, search, patch, sigma)
    shape = _one_volume(volume, "nlm")
    lib = H.load()
    with torch.cuda.device(volume.device):
        out = torch.empty_like(volume)
        H.check(lib.ddpm3d_nlm(H.ptr(volume), shape[0], shape[1], shape[2], search[0], search[1], search[2],
                               patch[0], patch[1], patch[2], h, sigma, H.ptr(out), H.stream()))
    return out


# ----------------------------------------------------------------- lesion segmentation
def _check_labels(labels, what):
    if not (isinstance(labels, torch.Tensor) and labels.is_cuda):
        raise RuntimeError("%s must live on the GPU: this package runs on HIP kernels only "
                           "(got %s)" % (what, getattr(labels, "device", type(labels))))
    if labels.dtype not in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64) or labels.dim() != 3:
        raise ValueError("%s must be an integer tensor (D, H, W), got %s of shape %s"
                         % (what, labels.dtype, tuple(labels.shape)))


def _forest_call(what, noun, shape, device, call, then=None):
    """One call of the entry ddpm3d_<what> over a (D, H, W) volume on `device` (csrc/voxel_forest.h's status
    protocol): allocates its workspace and status, runs call(lib, ws, ws_bytes, status, stream) -> return code, then
    then() if given (device work queued behind the entry), then makes the one device-to-host copy, of status.
    -> (status[1], what then() gave); RuntimeError if the cap flag is set: the `noun` are not valid."""
    lib = H.load()
    need = getattr(lib, "ddpm3d_%s_workspace_bytes" % what)(*shape)
    with torch.cuda.device(device):
        ws = torch.empty(max(need, 16) // 4, dtype=torch.int32, device=device)
        status = torch.empty(2, dtype=torch.int32, device=device)
        H.check(call(lib, H.ptr(ws), ws.numel() * 4, H.ptr(status), H.stream()))
        rest = then() if then is not None else None
        overrun, count = status.cpu().tolist()
    if overrun:
        raise RuntimeError("%s: a device loop hit its iteration cap; the %s are not valid" % (what, noun))
    return int(count), rest


def label_components(volume, threshold, connectivity=26, keep=None):
    """Connected components of volume > threshold (and keep != 0, an optional device uint8 tensor of the same shape)
    of a device float32 (D, H, W) tensor, connectivity 6, 18 or 26: one call of ddpm3d_label_components
    (csrc/ccl.hip), then the roots are ranked with torch ops.  -> (labels, n): int32 (D, H, W) on the device, 0 for
    background and 1..n in raster order of each component's first voxel (scipy.ndimage.label's numbering)."""
    H.require_device(volume, "volume")
    if volume.dim() != 3:
        raise ValueError("label_components: volume of shape %s (want (D, H, W))" % (tuple(volume.shape),))
    if connectivity not in (6, 18, 26):
        raise ValueError("label_components: connectivity %r (6, 18 or 26)" % (connectivity,))
    threshold = float(threshold)
    if math.isnan(threshold):
        raise ValueError("label_components: the threshold is NaN")
    if keep is not None and not (isinstance(keep, torch.Tensor) and keep.is_cuda and keep.dtype == torch.uint8
                                 and keep.is_contiguous() and tuple(keep.shape) == tuple(volume.shape)
                                 and keep.device == volume.device):
        raise ValueError("label_components: keep must be a contiguous device uint8 tensor of the volume's shape %s"
                         % (tuple(volume.shape),))
    D, Hh, W = (int(v) for v in volume.shape)
    if volume.numel() == 0 or volume.numel() > 2 ** 31 - 1:
        raise ValueError("label_components: %d voxels (1..2^31 - 1)" % volume.numel())
    roots = torch.empty((D, Hh, W), dtype=torch.int32, device=volume.device)

    def ranked():                                                  # queued behind the entry, before the status copy
        flat = roots.reshape(-1)
        is_root = flat == torch.arange(flat.numel(), dtype=torch.int32, device=volume.device)
        rank = torch.cumsum(is_root, 0, dtype=torch.int32)         # rank[root] = its 1-based number, in raster order
        labels = torch.where(flat >= 0, rank.index_select(0, flat.clamp(min=0)), torch.zeros_like(flat))
        return labels.reshape(D, Hh, W)

    n, labels = _forest_call(
        "label_components", "labels", (D, Hh, W), volume.device,
        lambda lib, *ws_status_stream: lib.ddpm3d_label_components(
            H.ptr(volume), H.ptr(keep), threshold, connectivity, D, Hh, W, H.ptr(roots), *ws_status_stream),
        then=ranked)
    return labels, n


def segment(volume, threshold, connectivity=26, min_voxels=1, keep=None):
    """label_components with the components of fewer than min_voxels voxels set to 0 and the rest renumbered 1..n in
    raster order of their first voxel; torch ops on the device.  -> (labels int32 (D, H, W) on the device, n)."""
    if int(min_voxels) != min_voxels or min_voxels < 1:
        raise ValueError("segment: min_voxels must be an integer of at least 1 (got %r)" % (min_voxels,))
    labels, n = label_components(volume, threshold, connectivity=connectivity, keep=keep)
    if min_voxels == 1 or n == 0:
        return labels, n
    with torch.cuda.device(volume.device):
        # sizes by sorting the foreground's labels, not by bincount: a histogram's atomics would all land on one word
        # for the background and for a component of millions of voxels
        flat = labels.reshape(-1)
        _, counts = torch.unique_consecutive(torch.sort(flat[flat > 0]).values, return_counts=True)   # numbers 1..n
        kept = counts >= int(min_voxels)
        remap = torch.zeros(n + 1, dtype=torch.int32, device=volume.device)   # old number -> new number, 0 = dropped
        remap[1:] = torch.cumsum(kept, 0) * kept
        return remap.index_select(0, flat).reshape(labels.shape), int(kept.sum())


def detection(target_labels, estimate_labels):
    """Lesion detectability of an estimate's segmentation against the target's, both device integer label volumes
    (D, H, W) as segment returns them (0 = background; target numbers in 1..DDPM3D_ROI_MAX_REGIONS, estimate numbers
    1..n all in use, any n).  A target region is found iff at least one of its voxels is foreground in the estimate;
    an estimate component is a false positive iff none of its voxels is foreground in the target.  torch ops only and
    one device-to-host copy.  -> {"n_target", "n_estimate", "found": [bool per target region], "overlap": [voxels of
    the region that are foreground in the estimate], "n_found", "n_missed", "false_positives", "sensitivity":
    n_found / n_target, None without a target region}."""
    _check_labels(target_labels, "target_labels")
    _check_labels(estimate_labels, "estimate_labels")
    if tuple(target_labels.shape) != tuple(estimate_labels.shape) or target_labels.device != estimate_labels.device:
        raise ValueError("detection: target labels of shape %s on %s, estimate labels of shape %s on %s"
                         % (tuple(target_labels.shape), target_labels.device, tuple(estimate_labels.shape),
                            estimate_labels.device))
    cap, spread = H.ROI_MAX_REGIONS, 4096
    with torch.cuda.device(target_labels.device):
        t = target_labels.reshape(-1).long()
        e = estimate_labels.reshape(-1).long()
        both = (t > 0) & (e > 0)
        # overlap[r], r in 1..cap (cap + 1 collects any larger number): voxels of both go to their region's bin, all
        # others add 0 to one of `spread` spare bins, so that no single word takes every atomic
        spare = cap + 2 + (torch.arange(t.numel(), device=t.device) & (spread - 1))
        overlap = torch.zeros(cap + 2 + spread, dtype=torch.int64, device=t.device)
        overlap.scatter_add_(0, torch.where(both, t.clamp(max=cap + 1), spare), both.long())
        # hit[c] = 1 for every estimate component c with a voxel in the target's foreground (plain stores of one
        # value; slot 0 takes the rest)
        hit = torch.zeros(t.numel() + 1, dtype=torch.uint8, device=t.device)
        hit.scatter_(0, torch.where(both, e, torch.zeros_like(e)), 1)
        head = torch.stack([t.max(), e.max(), hit[1:].sum(dtype=torch.int64)])
        rec = torch.cat([head, overlap[1:cap + 1]]).cpu().tolist()  # the one device-to-host copy
    n_target, n_estimate, n_hit = (int(v) for v in rec[:3])
    if n_target > cap:
        raise ValueError("detection: %d target regions (at most %d)" % (n_target, cap))
    over = [int(v) for v in rec[3:3 + n_target]]
    found = [v > 0 for v in over]
    n_found = sum(found)
    return {"n_target": n_target, "n_estimate": n_estimate, "found": found, "overlap": over, "n_found": n_found,
            "n_missed": n_target - n_found, "false_positives": n_estimate - n_hit,
            "sensitivity": n_found / n_target if n_target else None}


# ----------------------------------------------------------------- radial spectra, shell correlation
SPECTRUM_WINDOWS = ("hann", "none")
FSC_THRESHOLDS = (("0.5", 0.5), ("0.143", 1.0 / 7.0))
RATIO_HALF = 0.25           # the power ratio at which the amplitude ratio is 1/2


def _window(name, n):
    x = np.arange(n, dtype=np.float64)
    return np.sin(np.pi * (x + 0.5) / n) ** 2 if name == "hann" else np.ones(n)


def _dft_tables(n, rows, w):
    """(C, S) in fp64: C[k][x] = w[x] cos(2 pi ((k x) mod n) / n), S[k][x] = -w[x] sin(same); the integer mod keeps
    the argument reduction exact"""
    kx = (np.arange(rows, dtype=np.int64)[:, None] * np.arange(n, dtype=np.int64)[None, :]) % n
    ang = 2.0 * np.pi * kx.astype(np.float64) / n
    return w[None, :] * np.cos(ang), -w[None, :] * np.sin(ang)


def _shell_of(r2, xp):
    """the largest integer s with s^2 <= r2 (fp64 array of numpy or torch, xp): the sqrt only proposes, the integer
    comparisons decide (s^2 is exact in fp64 for every s a plan allows)"""
    s = xp.floor(xp.sqrt(r2))
    s = xp.where((s + 1.0) * (s + 1.0) <= r2, s + 1.0, s)
    return xp.where(s * s > r2, s - 1.0, s)


class SpectrumPlan:
    """spectrum_plan's return.  Host side (numpy, fp64 unless noted): `shape` (D, H, W), `spacing`, `window`,
    `shell_width` (cycles/mm), `windows` (three vectors), `cos` / `sin` (the fp32 tables per axis, as uploaded), `q`
    (three tables), `shells` S, `n_reported`, `frequency` (the S shell centres, cycles/mm), `weight_sq` = sum of w^2
    over the volume.  The device side (tables, shell index, window vectors) is built on first use per device."""

    def __init__(self, shape, spacing, window, shell_width, windows, q, shells, n_reported):
        self.shape, self.spacing, self.window, self.shell_width = shape, spacing, window, shell_width
        self.windows, self.q, self.shells, self.n_reported = windows, q, shells, n_reported
        self.rows = (shape[0], shape[1], shape[2] // 2 + 1)
        tables = [_dft_tables(n, r, w) for n, r, w in zip(shape, self.rows, windows)]
        self.cos = [np.ascontiguousarray(c, dtype=np.float32) for c, _ in tables]
        self.sin = [np.ascontiguousarray(s, dtype=np.float32) for _, s in tables]
        self.frequency = (np.arange(shells, dtype=np.float64) + 0.5) * shell_width
        self.weight_sq = float(np.prod([np.sum(w * w) for w in windows]))
        self.voxels = int(math.prod(shape))
        self.coeffs = shape[0] * shape[1] * self.rows[2]
        self._device = {}

    def shell_numbers(self):
        """the shell of every half-spectrum coefficient, numpy int64 (D, H, W / 2 + 1)"""
        r2 = (self.q[0][:, None, None] + self.q[1][None, :, None]) + self.q[2][None, None, :]
        return _shell_of(r2, np).astype(np.int64)

    def on(self, device):
        """the device side for `device`: (axes descriptor array, shell RoiIndex, [wD, wH, wW] fp64 tensors)"""
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("a spectrum plan's tables live on the GPU: this package runs on HIP kernels only "
                               "(got %s)" % device)
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        if key not in self._device:
            with torch.cuda.device(device):
                keep = [torch.from_numpy(np.stack([c, s])).to(device) for c, s in zip(self.cos, self.sin)]
                axes = (H.DftAxis * 3)(*[H.DftAxis(n, r, H.ptr(t[0]), H.ptr(t[1]))
                                         for n, r, t in zip(self.shape, self.rows, keep)])
                q = [torch.from_numpy(v).to(device) for v in self.q]
                r2 = (q[0][:, None, None] + q[1][None, :, None]) + q[2][None, None, :]
                found = roi_index((_shell_of(r2, torch) + 1.0).to(torch.int64))
                counts = [0] * self.shells                      # a shell no coefficient falls into stays, empty
                for label, n in zip(found.labels, found.counts):
                    counts[label - 1] = n
                index = RoiIndex(r2.shape, range(1, self.shells + 1), counts, found.index)
                wins = [torch.from_numpy(w).to(device) for w in self.windows]
            self._device[key] = (axes, index, wins, keep)
        return self._device[key][:3]

    def pivot(self, volume):
        """the window-weighted mean sum w v / sum w of each (K, D, H, W) volume: a device fp32 tensor (K), no sync"""
        wins = self.on(volume.device)[2]
        t = torch.matmul(volume, wins[2].to(torch.float32)).to(torch.float64)      # (K, D, H)
        t = torch.matmul(torch.matmul(t, wins[1]), wins[0])
        return (t / float(np.prod([w.sum() for w in self.windows]))).to(torch.float32).contiguous()


def spectrum_plan(shape, spacing, window="hann", shell_width=None):
    """The plan of dft3 / shell_spectrum for (D, H, W) volumes of `spacing` mm per voxel (same order): the per-axis
    window (`hann`: sin^2(pi (x + 1/2) / n), never 0; `none`), the DFT tables with the window folded in, and the
    radial shells of width `shell_width` cycles/mm (default 1 / the longest edge in mm).  All of it is built on the
    host in fp64; nothing touches a device before the plan is first used."""
    try:
        shape = tuple(int(v) for v in shape)
    except (TypeError, ValueError):
        shape = ()
    if len(shape) != 3 or not all(2 <= n <= H.SPEC_MAX_EXTENT for n in shape):
        raise ValueError("spectrum_plan: the shape must be three extents in 2..%d (got %r)" % (H.SPEC_MAX_EXTENT, shape))
    spacing = _check_spacing(spacing, "spectrum_plan")
    if window not in SPECTRUM_WINDOWS:
        raise ValueError("spectrum_plan: window %r (one of %s)" % (window, ", ".join(SPECTRUM_WINDOWS)))
    edges = [n * s for n, s in zip(shape, spacing)]
    if shell_width is None:
        shell_width = 1.0 / max(edges)
    shell_width = float(shell_width)
    if not (math.isfinite(shell_width) and shell_width > 0):
        raise ValueError("spectrum_plan: the shell width must be positive and finite, in cycles/mm (got %r)"
                         % shell_width)
    q = []
    for a, (n, edge) in enumerate(zip(shape, edges)):
        k = np.arange(n // 2 + 1 if a == 2 else n, dtype=np.int64)
        folded = np.where(2 * k <= n, k, k - n).astype(np.float64)         # k folded to (-n/2, n/2]
        q.append((folded / (edge * shell_width)) ** 2)
    top = (q[0].max() + q[1].max()) + q[2].max()
    if not top < float(2 * H.ROI_MAX_REGIONS) ** 2:
        raise ValueError("spectrum_plan: a shell width of %g cycles/mm gives more than %d shells"
                         % (shell_width, H.ROI_MAX_REGIONS))
    shells = int(_shell_of(np.float64(top), np)) + 1
    if shells > H.ROI_MAX_REGIONS:
        raise ValueError("spectrum_plan: a shell width of %g cycles/mm gives %d shells (at most %d)"
                         % (shell_width, shells, H.ROI_MAX_REGIONS))
    nyquist = min(1.0 / (2.0 * s) for s in spacing)
    n_reported = sum(1 for s in range(shells) if (s + 1) * shell_width <= nyquist)
    return SpectrumPlan(shape, spacing, window, shell_width, [_window(window, n) for n in shape], q, shells,
                        n_reported)


def _spectrum_stack(volume, plan, what):
    H.require_device(volume, what)
    if volume.dim() not in (3, 4) or tuple(volume.shape[-3:]) != plan.shape:
        raise ValueError("%s of shape %s against a plan for %s volumes" % (what, tuple(volume.shape), plan.shape))
    K = int(volume.shape[0]) if volume.dim() == 4 else 1
    if not 1 <= K <= H.MAX_DRAWS:
        raise ValueError("%s: %d volumes (1..%d)" % (what, K, H.MAX_DRAWS))
    return K


def dft3(volume, plan, pivot=None):
    """ddpm3d_dft3 of a (D, H, W) or (K, D, H, W) device volume: numpy.fft.rfftn(w (v - pivot)) with the plan's
    window, as two fp32 device tensors (re, im) of shape (..., D, H, W / 2 + 1).  pivot: None (0) or a device fp32
    tensor of K values."""
    K = _spectrum_stack(volume, plan, "volume")
    if pivot is not None:
        H.require_device(pivot, "pivot")
        if pivot.numel() != K or pivot.device != volume.device:
            raise ValueError("dft3: a pivot of %d values for %d volumes" % (pivot.numel(), K))
    axes = plan.on(volume.device)[0]
    lib = H.load()
    D, Hh, W = plan.shape
    need = lib.ddpm3d_dft3_workspace_bytes(K, D, Hh, W)
    with torch.cuda.device(volume.device):
        ws = torch.empty(max(need, 16) // 4, dtype=torch.float32, device=volume.device)
        out = torch.empty((2,) + tuple(volume.shape[:-1]) + (plan.rows[2],), dtype=torch.float32,
                          device=volume.device)
        H.check(lib.ddpm3d_dft3(H.ptr(volume), H.ptr(pivot), K, D, Hh, W, axes, H.ptr(ws), ws.numel() * 4,
                                H.ptr(out[0]), H.ptr(out[1]), H.stream()))
    return out[0], out[1]


def _shell_spectrum_device(estimate, plan, target=None):
    K = _spectrum_stack(estimate, plan, "estimate")
    if target is not None:
        H.require_device(target, "target")
        if tuple(target.shape) != plan.shape or target.device != estimate.device:
            raise ValueError("shell_spectrum: target of shape %s on %s, estimate on %s, plan for %s"
                             % (tuple(target.shape), target.device, estimate.device, plan.shape))
    axes, index, _ = plan.on(estimate.device)
    lib = H.load()
    D, Hh, W = plan.shape
    need = lib.ddpm3d_shell_spectrum_workspace_bytes(K, D, Hh, W, index.desc, int(target is not None))
    with torch.cuda.device(estimate.device):
        pe = plan.pivot(estimate.reshape((K,) + plan.shape))
        pt = None if target is None else plan.pivot(target[None])
        ws = torch.empty(max(need, 16) // 8, dtype=torch.float64, device=estimate.device)
        out = torch.empty((K, plan.shells, H.SP_REC), dtype=torch.float64, device=estimate.device)
        H.check(lib.ddpm3d_shell_spectrum(H.ptr(estimate), H.ptr(pe), H.ptr(target), H.ptr(pt), K, D, Hh, W, axes,
                                          index.desc, H.ptr(ws), ws.numel() * 8, H.ptr(out), H.stream()))
    return out


def shell_spectrum(estimate, plan, target=None):
    """The per-shell records of a (D, H, W) or (K, D, H, W) estimate (and of a (D, H, W) target): one call of
    ddpm3d_shell_spectrum and one device-to-host copy.  The pivots are the window-weighted means.  -> a numpy float64
    array (K, S, H.SP_REC), columns H.SP_* (the Y, XY and EE columns are 0 without a target)."""
    return _shell_spectrum_device(estimate, plan, target).cpu().numpy()   # the one device-to-host copy (it waits)


def _first_crossing(curve, threshold, frequency):
    """1 / f where `curve` first falls below the threshold among shells >= 1, linear between shell centres; (None,
    True) if it never does, (None, False) if an undefined shell comes first"""
    for s in range(1, len(curve)):
        if curve[s] is None:
            return None, False
        if curve[s] < threshold:
            if s == 1 or curve[s - 1] is None:
                return 1.0 / frequency[s], False
            a, b = curve[s - 1], curve[s]
            f = frequency[s - 1] + (a - threshold) / (a - b) * (frequency[s] - frequency[s - 1])
            return 1.0 / f, False
    return None, True


def spectrum_figures(records, plan):
    """The figures of shell records (K, S, H.SP_REC) or (S, H.SP_REC), on the host in fp64, over the plan's reported
    shells (those wholly below the smallest axis Nyquist): per estimate a dict of lists `frequency` (cycles/mm), `n`,
    `power`, `power_target`, `power_error` (sum / (V sum w^2)), `fsc` = XY / sqrt(XX YY), `ratio` = XX / YY,
    `error_rel` = EE / YY (None for a zero denominator or a non-finite sum), and the summaries `fsc_resolution_mm`
    {"0.5", "0.143", "to_nyquist"} (1 / f at the first crossing below the threshold among shells >= 1, linear between
    shell centres; None, with to_nyquist true, for a curve that never crosses) and `ratio_half_mm` (the first crossing
    of `ratio` below 0.25).  A list of K dicts for three-dimensional records."""
    rec = np.asarray(records, dtype=np.float64)
    if rec.ndim not in (2, 3) or rec.shape[-2:] != (plan.shells, H.SP_REC):
        raise ValueError("spectrum_figures: records of shape %s for a plan of %d shells" % (rec.shape, plan.shells))
    norm = plan.voxels * plan.weight_sq
    freq = [float(f) for f in plan.frequency[:plan.n_reported]]

    def div(a, b):
        return None if not (math.isfinite(a) and math.isfinite(b)) or b == 0 else a / b

    def one(r):
        r = r[:plan.n_reported].tolist()
        fig = {"frequency": freq, "n": [int(v[H.SP_N]) for v in r]}
        for key, col in (("power", H.SP_SUM_XX), ("power_target", H.SP_SUM_YY), ("power_error", H.SP_SUM_EE)):
            fig[key] = [v[col] / norm if math.isfinite(v[col]) else None for v in r]
        fig["fsc"] = [None if not (math.isfinite(v[H.SP_SUM_XX]) and math.isfinite(v[H.SP_SUM_YY]))
                      else div(v[H.SP_SUM_XY], math.sqrt(v[H.SP_SUM_XX] * v[H.SP_SUM_YY])) for v in r]
        fig["ratio"] = [div(v[H.SP_SUM_XX], v[H.SP_SUM_YY]) for v in r]
        fig["error_rel"] = [div(v[H.SP_SUM_EE], v[H.SP_SUM_YY]) for v in r]
        res, open_end = {}, False
        for name, thr in FSC_THRESHOLDS:
            res[name], never = _first_crossing(fig["fsc"], thr, freq)
            open_end = open_end or never
        res["to_nyquist"] = open_end
        fig["fsc_resolution_mm"] = res
        fig["ratio_half_mm"] = _first_crossing(fig["ratio"], RATIO_HALF, freq)[0]
        return fig

    return one(rec) if rec.ndim == 2 else [one(r) for r in rec]


# ----------------------------------------------------------------- rotating MIP and ray sums
PROJECTION_MODES = {"max": H.PROJECT_MAX, "sum": H.PROJECT_SUM}


class ProjectionPlan:
    """projection_plan's return: `shape` (D, H, W), `spacing`, `angles_deg` (a tuple), `pitch` and `step` (mm),
    `bins` U and `samples` R, `table` (the H.ProjectTable ddpm3d_project reads, on the host) and `coef`, its angles
    as a numpy float32 array (A, 6): h0, hu, hj, w0, wu, wj."""

    def __init__(self, shape, spacing, angles_deg, pitch, bins, step, samples, table):
        self.shape, self.spacing, self.angles_deg = shape, spacing, angles_deg
        self.pitch, self.bins, self.step, self.samples, self.table = pitch, bins, step, samples, table
        self.coef = np.ctypeslib.as_array(table.coef)[:len(angles_deg)].astype(np.float32)


def _count(value, what):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not 1 <= value <= H.PROJECT_MAX_BINS:
        raise ValueError("projection_plan: %s must be an integer in 1..%d (got %r)" % (what, H.PROJECT_MAX_BINS, value))
    return int(value)


def projection_default_bins(shape, spacing, pitch=None):
    """the bin (and sample) count projection_plan chooses for a (D, H, W) shape: ceil(hypot(H s1, W s2) / pitch), the
    slice's diagonal, so that no angle clips it; pitch defaults to min(s1, s2)"""
    pitch = min(spacing[1], spacing[2]) if pitch is None else pitch
    return int(math.ceil(math.hypot(shape[1] * spacing[1], shape[2] * spacing[2]) / pitch))


def projection_plan(shape, spacing, angles_deg, pitch=None, bins=None, step=None, samples=None):
    """The plan of project for (D, H, W) volumes of `spacing` = (s0, s1, s2) mm per voxel (same order): parallel rays
    through every (H, W) slice, rotated about the D axis by each of `angles_deg` (1..64 of them), `bins` detector bins
    `pitch` mm apart and `samples` samples `step` mm apart per ray, all centred on the slice.  The defaults are
    pitch = step = min(s1, s2) and bins = samples = ceil(hypot(H s1, W s2) / pitch), so that no angle clips the
    slice.  ddpm3d_project_table_fill folds it into six fp32 numbers per angle on the host; nothing touches a device.
    -> ProjectionPlan"""
    try:
        shape = tuple(int(v) for v in shape)
    except (TypeError, ValueError):
        shape = ()
    if len(shape) != 3 or not all(n >= 1 for n in shape):
        raise ValueError("projection_plan: the shape must be three extents of 1 or more (got %r)" % (shape,))
    spacing = _check_spacing(spacing, "projection_plan")
    try:
        angles = tuple(float(a) for a in angles_deg)
    except (TypeError, ValueError):
        angles = ()
    if not 1 <= len(angles) <= H.PROJECT_MAX_ANGLES or not all(math.isfinite(a) for a in angles):
        raise ValueError("projection_plan: angles_deg must be 1..%d finite angles in degrees (got %r)"
                         % (H.PROJECT_MAX_ANGLES, angles_deg))
    pitch = min(spacing[1], spacing[2]) if pitch is None else _positive(pitch, "projection_plan: the pitch")
    step = min(spacing[1], spacing[2]) if step is None else _positive(step, "projection_plan: the step")
    if bins is None or samples is None:
        default = projection_default_bins(shape, spacing, pitch)
        if default > H.PROJECT_MAX_BINS:
            raise ValueError("projection_plan: the diagonal of a %d x %d slice at %g x %g mm is %d bins of %g mm: bins "
                             "and samples are limited to %d" % (shape[1], shape[2], spacing[1], spacing[2], default,
                                                                pitch, H.PROJECT_MAX_BINS))
        bins = default if bins is None else bins
        samples = default if samples is None else samples
    bins, samples = _count(bins, "bins"), _count(samples, "samples")
    table = H.ProjectTable()
    H.check(H.load().ddpm3d_project_table_fill(shape[1], shape[2], spacing[1], spacing[2], pitch, bins, step, samples,
                                               (ctypes.c_double * len(angles))(*angles), len(angles),
                                               ctypes.byref(table)))
    return ProjectionPlan(shape, spacing, angles, pitch, bins, step, samples, table)


def project(volume, plan, mode="max"):
    """The projections of a device float32 (D, H, W) or (K, D, H, W) tensor along the plan's rays: one call of
    ddpm3d_project (csrc/project.hip), no host copy.  mode "max": the largest bilinear sample along each ray, 0 where
    the ray misses the slice (the rotating MIP); "sum": step times the sum of the samples, the line integral in
    value * mm.  -> a device tensor (A, D, U) or (K, A, D, U)."""
    if not isinstance(plan, ProjectionPlan):
        raise ValueError("project: plan must be projection_plan's return (got %r)" % (plan,))
    if mode not in PROJECTION_MODES:
        raise ValueError("project: mode %r (one of %s)" % (mode, ", ".join(PROJECTION_MODES)))
    K = _spectrum_stack(volume, plan, "volume")
    D, Hh, W = plan.shape
    A = len(plan.angles_deg)
    if K * D * Hh * W > 2 ** 31 - 1 or K * A * D * plan.bins > 2 ** 31 - 1:
        raise ValueError("project: %d voxels in and %d out (at most 2^31 - 1 each)"
                         % (K * D * Hh * W, K * A * D * plan.bins))
    with torch.cuda.device(volume.device):
        out = torch.empty(tuple(volume.shape[:-3]) + (A, D, plan.bins), dtype=torch.float32, device=volume.device)
        H.check(H.load().ddpm3d_project(H.ptr(volume), K, D, Hh, W, ctypes.byref(plan.table),
                                        PROJECTION_MODES[mode], H.ptr(out), H.stream()))
    return out


# ----------------------------------------------------------------- distances, lesion boundaries
PERCENTILE = 0.95           # of hd95_mm and surface_p95_mm
EDGE_MAX_SHELLS = 64        # inside + outside of edge_profile


def _mask_u8(mask, what):
    """a device uint8 or bool tensor (D, H, W) or (K, D, H, W) -> contiguous uint8 (a bool tensor's bytes are 0 / 1)"""
    if not (isinstance(mask, torch.Tensor) and mask.is_cuda):
        raise RuntimeError("%s must live on the GPU: this package runs on HIP kernels only "
                           "(got %s)" % (what, getattr(mask, "device", type(mask))))
    if mask.dtype not in (torch.uint8, torch.bool) or mask.dim() not in (3, 4):
        raise ValueError("%s must be a uint8 or bool tensor (D, H, W) or (K, D, H, W), got %s of shape %s"
                         % (what, mask.dtype, tuple(mask.shape)))
    mask = mask.contiguous()
    return mask.view(torch.uint8) if mask.dtype == torch.bool else mask


def distance_sq(mask, spacing, invert=False):
    """The squared distance in mm^2 from every foreground voxel of a device uint8 or bool tensor (D, H, W) or
    (K, D, H, W) to the nearest background voxel of its volume, 0 on the background and +inf in a volume without
    background: scipy.ndimage.distance_transform_edt(mask, sampling=spacing) ** 2.  Foreground is mask != 0, or
    mask == 0 with invert.  `spacing` = (s0, s1, s2) mm along D, H, W.  One call of ddpm3d_distance_sq
    (csrc/edt.hip), no host copy.  -> a device float32 tensor of the mask's shape."""
    spacing = _check_spacing(spacing, "distance_sq")
    m = _mask_u8(mask, "distance_sq: mask")
    K = int(m.shape[0]) if m.dim() == 4 else 1
    D, Hh, W = (int(v) for v in m.shape[-3:])
    if max(D, Hh, W) > H.EDT_MAX_EXTENT:
        raise ValueError("distance_sq: a %d x %d x %d volume (every extent is at most %d)"
                         % (D, Hh, W, H.EDT_MAX_EXTENT))
    with torch.cuda.device(m.device):
        out = torch.empty(tuple(m.shape), dtype=torch.float32, device=m.device)
        H.check(H.load().ddpm3d_distance_sq(H.ptr(m), K, D, Hh, W, 1 if invert else 0, spacing[0], spacing[1],
                                            spacing[2], H.ptr(out), H.stream()))
    return out


def surface(mask):
    """The voxels of a device uint8 or bool mask (D, H, W) with at least one of the 6 face neighbours outside the mask;
    a neighbour beyond the volume counts as outside: mask & ~scipy.ndimage.binary_erosion(mask) with the default
    structure and border_value=0.  torch ops on the device.  -> a device bool tensor (D, H, W)."""
    m = _mask_u8(mask, "surface: mask")
    if m.dim() != 3:
        raise ValueError("surface: mask of shape %s (want (D, H, W))" % (tuple(m.shape),))
    with torch.cuda.device(m.device):
        m = (m != 0).to(torch.uint8)
        p = torch.nn.functional.pad(m, (1, 1, 1, 1, 1, 1))
        inner = (p[:-2, 1:-1, 1:-1] & p[2:, 1:-1, 1:-1] & p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1]
                 & p[1:-1, 1:-1, :-2] & p[1:-1, 1:-1, 2:])
        return (m & ~inner & 1).bool()


def _percentile_at(n):
    """numpy.percentile's method "linear" at PERCENTILE over n sorted values -> (lo, hi, t): lerp of v[lo], v[hi]"""
    pos = PERCENTILE * (n - 1)
    lo = int(math.floor(pos))
    return lo, min(lo + 1, n - 1), pos - lo


def _lerp(a, b, t):
    """numpy's _lerp: a + (b - a) t, from the far end for t >= 0.5"""
    return b - (b - a) * (1.0 - t) if t >= 0.5 else a + (b - a) * t


class BoundaryTarget:
    """boundary_target's return, the target's side of boundary: `spacing`, the foreground `fg` (device bool) and its
    voxel count `n_fg`, `dist` (device fp32: mm from every voxel to the target's nearest surface voxel), `roi` (the
    RoiIndex of the surface voxels, labelled by region) and `n_surface`."""

    def __init__(self, spacing, fg, n_fg, dist, roi):
        self.spacing, self.fg, self.n_fg, self.dist, self.roi = spacing, fg, n_fg, dist, roi
        self.n_surface = roi.offsets[-1]
        self.where = [_percentile_at(self.n_surface)] + [_percentile_at(n) for n in roi.counts]
        starts = [0] + roi.offsets[:-1]                                     # of the whole set, then of every region
        at = [s + w[0] for s, w in zip(starts, self.where)] + [s + w[1] for s, w in zip(starts, self.where)]
        dev = roi.device
        self._at = torch.tensor(at, dtype=torch.int64).to(dev)
        self._ordinal = torch.repeat_interleave(torch.arange(len(roi), dtype=torch.int64, device=dev),
                                                torch.tensor(roi.counts, dtype=torch.int64).to(dev))


def boundary_target(target_labels, spacing):
    """The part of boundary that depends on the target alone, for a caller that scores several estimates: the surface
    of target_labels > 0, one distance_sq call on its complement, and the region index of the surface voxels.
    -> BoundaryTarget"""
    _check_labels(target_labels, "target_labels")
    spacing = _check_spacing(spacing, "boundary")
    with torch.cuda.device(target_labels.device):
        fg = target_labels > 0
        n_fg = int(fg.sum())
        if n_fg == 0:
            raise ValueError("boundary: the target has no foreground")
        surf = surface(fg)
        dist = distance_sq(surf, spacing, invert=True).sqrt_()
        roi = roi_index(torch.where(surf, target_labels, torch.zeros_like(target_labels)))
    return BoundaryTarget(spacing, fg, n_fg, dist, roi)


def boundary(target_labels, estimate_labels, spacing, index=None):
    """Where the estimate's segmentation put the lesion boundaries against the target's, both device integer label
    volumes (D, H, W) as segment returns them.  Surfaces are surface() of labels > 0; a directed distance is the
    distance in mm from a surface voxel of one to the nearest surface voxel of the other (two distance_sq calls, on
    the complement of each surface; `index` = boundary_target(target_labels, spacing) hands the target's in).  Given
    the index, the rest is torch ops, roi_moments over the target's surface voxels and ONE device-to-host copy.
    -> {"dice", "jaccard" (of the foregrounds), "hd_mm" (the larger of the two directed maxima), "hd95_mm" (the larger
    of the two directed 95th percentiles, numpy's method "linear"), "assd_mm" (the sum of all directed distances over
    the count of both surfaces), "n_surface_target", "n_surface_estimate", "regions": {target label: {"surface_mean_mm",
    "surface_p95_mm", "surface_max_mm"}}}.  A region's figures are DIRECTED: from that lesion's surface voxels to the
    estimate's surface of ANY component, not only of the component that overlaps it.  When the estimate has no
    foreground, dice and jaccard are 0 and every distance is None (decided on the host from the counts in the copy)."""
    tgt = boundary_target(target_labels, spacing) if index is None else index
    if not isinstance(tgt, BoundaryTarget):
        raise ValueError("boundary: index must be boundary_target's return (got %r)" % (index,))
    _check_labels(target_labels, "target_labels")
    _check_labels(estimate_labels, "estimate_labels")
    spacing = _check_spacing(spacing, "boundary")
    if (tuple(estimate_labels.shape) != tgt.roi.shape or tuple(target_labels.shape) != tgt.roi.shape
            or estimate_labels.device != tgt.roi.device or spacing != tgt.spacing):
        raise ValueError("boundary: estimate labels of shape %s on %s at %s mm against a target of shape %s on %s at "
                         "%s mm" % (tuple(estimate_labels.shape), estimate_labels.device, spacing, tgt.roi.shape,
                                    tgt.roi.device, tgt.spacing))
    R = len(tgt.roi)
    with torch.cuda.device(tgt.roi.device):
        e_fg = estimate_labels > 0
        e_surf = surface(e_fg)
        to_e = distance_sq(e_surf, spacing, invert=True).sqrt_()         # +inf everywhere without an estimate surface
        # target -> estimate: the values at the target's surface voxels, sorted as a whole and within each region
        v = to_e.reshape(-1).index_select(0, tgt.roi.index)
        whole, order = torch.sort(v)
        by_region = whole.index_select(0, torch.sort(tgt._ordinal.index_select(0, order), stable=True).indices)
        n_pick = 1 + R
        at = tgt._at
        picks_t = torch.cat([whole.index_select(0, at[0:1]), by_region.index_select(0, at[1:n_pick]),
                             whole.index_select(0, at[n_pick:n_pick + 1]),
                             by_region.index_select(0, at[n_pick + 1:])]).double()
        rec = _roi_moments_device(to_e, tgt.roi)[0]                      # (R, H.ROI_REC) fp64, fixed-order sums
        # estimate -> target: the estimate's surface count stays on the device, so the whole volume is sorted
        n_e = e_surf.sum()
        last = (n_e - 1).clamp(min=0)
        pos = PERCENTILE * last.double()
        lo = pos.floor().long()
        ranked = torch.sort(tgt.dist.masked_fill(~e_surf, math.inf).reshape(-1)).values
        picks_e = ranked.index_select(0, torch.stack([lo, torch.minimum(lo + 1, last), last])).double()
        sum_e = tgt.dist.masked_fill(~e_surf, 0.0).sum(dtype=torch.float64)
        head = torch.stack([e_fg.sum(), (e_fg & tgt.fg).sum(), n_e]).double()
        got = torch.cat([head, sum_e.reshape(1), picks_e, picks_t,
                         rec[:, H.ROI_SUM_X], rec[:, H.ROI_MAX_X]]).cpu().tolist()   # the one device-to-host copy
    n_efg, both, n_es = (int(x) for x in got[:3])
    sum_e, e_lo, e_hi, e_max = got[3:7]
    t = got[7:7 + 2 * n_pick]
    sums, maxima = got[7 + 2 * n_pick:7 + 2 * n_pick + R], got[7 + 2 * n_pick + R:]
    out = {"dice": 2.0 * both / (tgt.n_fg + n_efg), "jaccard": both / (tgt.n_fg + n_efg - both),
           "hd_mm": None, "hd95_mm": None, "assd_mm": None, "n_surface_target": tgt.n_surface,
           "n_surface_estimate": n_es, "regions": {}}
    p95 = [_lerp(t[i], t[n_pick + i], tgt.where[i][2]) for i in range(n_pick)]
    for r, label in enumerate(tgt.roi.labels):
        out["regions"][label] = ({"surface_mean_mm": sums[r] / tgt.roi.counts[r], "surface_p95_mm": p95[1 + r],
                                  "surface_max_mm": maxima[r]} if n_efg else
                                 {"surface_mean_mm": None, "surface_p95_mm": None, "surface_max_mm": None})
    if n_efg:
        pos = PERCENTILE * (n_es - 1)
        out["hd_mm"] = max(max(maxima), e_max)
        out["hd95_mm"] = max(p95[0], _lerp(e_lo, e_hi, pos - math.floor(pos)))
        out["assd_mm"] = (math.fsum(sums) + sum_e) / (tgt.n_surface + n_es)
    return out


def edge_profile(volumes, labels, spacing, width_mm, inside=3, outside=5, keep=None):
    """The mean of every volume in shells of width_mm around the boundary of labels > 0 (a device integer (D, H, W)
    tensor): the activity profile across the lesion edge, which shows spill-out.  `volumes` is a dict of name ->
    device float32 (D, H, W) tensor.  d_in = sqrt(distance_sq(fg)) and d_out = sqrt(distance_sq(fg, invert=True));
    inside shell i (0 .. inside - 1) holds the foreground voxels with i W < d_in <= (i + 1) W, outside shell o the
    background voxels with o W < d_out <= (o + 1) W; voxels with keep == 0 (an optional device uint8 tensor) are
    dropped.  The shells become a label volume, and roi_index and one roi_moments call reduce every volume over it.
    -> {"width_mm", "inside", "outside", "rows": [{"distance_mm" (the shell's centre, negative inside), "n", "mean":
    {name: mean or None}}]}, rows from the innermost shell outward."""
    _check_labels(labels, "labels")
    spacing = _check_spacing(spacing, "edge_profile")
    width = _positive(width_mm, "edge_profile: width_mm")
    for name, v in (("inside", inside), ("outside", outside)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
            raise ValueError("edge_profile: %s must be an integer of 0 or more (got %r)" % (name, v))
    inside, outside = int(inside), int(outside)
    if not 1 <= inside + outside <= EDGE_MAX_SHELLS:
        raise ValueError("edge_profile: inside + outside = %d shells (1..%d)" % (inside + outside, EDGE_MAX_SHELLS))
    if not isinstance(volumes, dict) or not volumes:
        raise ValueError("edge_profile: volumes must be a dict of name -> device float32 (D, H, W) tensor")
    names = list(volumes)
    for name in names:
        H.require_device(volumes[name], "edge_profile: volume %r" % (name,))
        if tuple(volumes[name].shape) != tuple(labels.shape) or volumes[name].device != labels.device:
            raise ValueError("edge_profile: volume %r of shape %s, labels of shape %s"
                             % (name, tuple(volumes[name].shape), tuple(labels.shape)))
    with torch.cuda.device(labels.device):
        fg = labels > 0
        edges = torch.arange(max(inside, outside) + 1, dtype=torch.float64, device=labels.device) * width
        b_in = torch.bucketize(distance_sq(fg, spacing).double().sqrt_(), edges)      # i + 1 in shell i, 0 at d = 0
        b_out = torch.bucketize(distance_sq(fg, spacing, invert=True).double().sqrt_(), edges)
        zero = torch.zeros_like(b_in)
        shells = (torch.where((b_in >= 1) & (b_in <= inside), inside + 1 - b_in, zero)
                  + torch.where((b_out >= 1) & (b_out <= outside), inside + b_out, zero)).int()
        try:
            index = roi_index(shells, keep=keep)
        except ValueError as e:
            if "no labelled voxel" not in str(e):
                raise
            index = None
        rec = [] if index is None else roi_moments(torch.stack([volumes[n] for n in names]), index)
    at = {} if index is None else {label: r for r, label in enumerate(index.labels)}
    rows = []
    for j in range(1, inside + outside + 1):
        r = at.get(j)
        n = 0 if r is None else int(rec[0][r][H.ROI_N])
        rows.append({"distance_mm": (j - inside - 0.5) * width, "n": n,
                     "mean": {name: (rec[k][r][H.ROI_SUM_X] / n if n else None) for k, name in enumerate(names)}})
    return {"width_mm": width, "inside": inside, "outside": outside, "rows": rows}


# ------------------------------------------------------------------------------------------------ watershed split
def _check_watershed(what, height, labels, connectivity, peaks=None):
    """the argument checks of basins / basin_saddles / split_components: ValueError before any launch"""
    for name, t, dtype in (("height", height, torch.float32), ("labels", labels, torch.int32),
                           ("peaks", peaks, torch.int32)):
        if name == "peaks" and t is None:
            continue
        if not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise ValueError("%s: %s must live on the GPU: this package runs on HIP kernels only (got %s)"
                             % (what, name, getattr(t, "device", type(t))))
        if t.dtype != dtype or t.dim() != 3 or not t.is_contiguous():
            raise ValueError("%s: %s must be a contiguous %s tensor (D, H, W), got %s of shape %s"
                             % (what, name, dtype, t.dtype, tuple(t.shape)))
        if tuple(t.shape) != tuple(height.shape) or t.device != height.device:
            raise ValueError("%s: %s of shape %s on %s against a height of shape %s on %s"
                             % (what, name, tuple(t.shape), t.device, tuple(height.shape), height.device))
    if connectivity not in (6, 18, 26):
        raise ValueError("%s: connectivity %r (6, 18 or 26)" % (what, connectivity))
    if height.numel() == 0 or height.numel() > 2 ** 31 - 1:
        raise ValueError("%s: %d voxels (1..2^31 - 1)" % (what, height.numel()))
    return tuple(int(v) for v in height.shape)


def basins(height, labels, connectivity=26):
    """The watershed basins of a device float32 height (D, H, W) inside the components of a device int32 label volume
    of the same shape (0 = background; a NaN height is background too): every voxel climbs to the neighbour of
    greatest key (height, -flat index) of its own label until it stands on a peak.  One call of ddpm3d_basins
    (csrc/watershed.hip) and one copy of its status.  -> (peaks, n_basins): int32 (D, H, W) on the device, the flat
    index of each voxel's peak and -1 on the background."""
    D, Hh, W = _check_watershed("basins", height, labels, connectivity)
    peaks = torch.empty((D, Hh, W), dtype=torch.int32, device=height.device)
    n, _ = _forest_call("basins", "peaks", (D, Hh, W), height.device,
                        lambda lib, *ws_status_stream: lib.ddpm3d_basins(
                            H.ptr(height), H.ptr(labels), connectivity, D, Hh, W, H.ptr(peaks), *ws_status_stream))
    return peaks, n


def _saddle_records(height, labels, peaks, connectivity, cap):
    """one call of ddpm3d_basin_saddles with room for cap records -> (pairs, saddle, records needed)"""
    D, Hh, W = (int(v) for v in height.shape)
    pairs = torch.empty((cap, 2), dtype=torch.int32, device=height.device)
    saddle = torch.empty(cap, dtype=torch.float32, device=height.device)
    needed, _ = _forest_call("basin_saddles", "records", (D, Hh, W), height.device,
                             lambda lib, *ws_status_stream: lib.ddpm3d_basin_saddles(
                                 H.ptr(height), H.ptr(labels), H.ptr(peaks), connectivity, D, Hh, W, cap,
                                 H.ptr(pairs), H.ptr(saddle), *ws_status_stream))
    return pairs, saddle, needed


def reduce_saddles(pairs, saddle):
    """A multiset of device records (pairs (E, 2) int32 with a < b, saddle (E,) float32) -> the unique pairs in
    ascending order of (a, b), each with the maximum of its saddles; torch ops on the device."""
    if pairs.shape[0] == 0:
        return pairs.reshape(0, 2), saddle.reshape(0)
    key = pairs[:, 0].to(torch.int64) << 32 | pairs[:, 1].to(torch.int64)
    by_saddle = torch.sort(saddle, stable=True).indices
    by_key = torch.sort(key.index_select(0, by_saddle), stable=True)          # within a pair the saddles ascend
    order = by_saddle.index_select(0, by_key.indices)
    _, counts = torch.unique_consecutive(by_key.values, return_counts=True)
    last = order.index_select(0, torch.cumsum(counts, 0) - 1)                 # a pair's last record holds its maximum
    return pairs.index_select(0, last).contiguous(), saddle.index_select(0, last).contiguous()


def basin_saddles(height, labels, peaks, connectivity=26, capacity=None):
    """The saddle graph of basins(): for every two basins a < b (peak indices) with neighbouring voxels p, q of one
    label, the maximum over such pairs of min(height[p], height[q]).  ddpm3d_basin_saddles (csrc/watershed.hip) writes
    a multiset of records, reduce_saddles makes it the graph.  The first call has room for `capacity` records (default:
    an eighth of the voxels, at least 4096); if it reports a larger need, one more call has exactly that; never a
    third.  -> (pairs (E, 2) int32, saddle (E,) float32) on the device, the pairs unique and ascending."""
    _check_watershed("basin_saddles", height, labels, connectivity, peaks)
    n = height.numel()
    cap = max(n // 8, 4096) if capacity is None else int(capacity)
    if not 0 <= cap <= 2 ** 31 - 1:
        raise ValueError("basin_saddles: capacity %r (0..2^31 - 1 records)" % (capacity,))
    with torch.cuda.device(height.device):
        pairs, saddle, needed = _saddle_records(height, labels, peaks, connectivity, cap)
        if needed > cap:
            if needed >= 2 ** 31 - 1:
                raise ValueError("basin_saddles: 2^31 - 1 or more records; smooth the height first")
            cap = needed
            pairs, saddle, needed = _saddle_records(height, labels, peaks, connectivity, cap)
            if needed > cap:
                raise RuntimeError("basin_saddles: the second call needs %d records, the first asked for %d"
                                   % (needed, cap))
        return reduce_saddles(pairs[:needed], saddle[:needed])


def _check_prominence(what, prominence):
    prominence = float(prominence)
    if math.isnan(prominence) or prominence < 0:
        raise ValueError("%s: prominence %r (0 or more; inf gives back the components)" % (what, prominence))
    return prominence


def merge_basins(peak_index, peak_height, pairs, saddle, prominence, first_voxel=None):
    """Merges basins across their saddles by peak prominence, on the host in fp64.  peak_index: the basins' peaks
    (flat indices, ascending); peak_height: their heights; pairs (E, 2), saddle (E,): the reduced saddle graph in
    peak indices.  The edges are taken by saddle descending, then a and b ascending; a cluster's peak is its member
    of greatest key (height, -index); an edge between two clusters unites them unless the lesser peak stands
    `prominence` or more above the saddle (a NaN difference, inf - inf, unites).  Pieces are numbered 1..n in
    ascending order of their lowest first_voxel (a basin's lowest voxel; default: its peak).
    -> (piece, n): int32 per basin."""
    prominence = _check_prominence("merge_basins", prominence)
    index = np.asarray(peak_index, dtype=np.int64).reshape(-1)
    height = np.asarray(peak_height, dtype=np.float64).reshape(-1)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    saddle = np.asarray(saddle, dtype=np.float64).reshape(-1)
    first = index if first_voxel is None else np.asarray(first_voxel, dtype=np.int64).reshape(-1)
    nb = index.size
    if height.size != nb or first.size != nb or saddle.size != pairs.shape[0]:
        raise ValueError("merge_basins: %d peaks, %d heights, %d first voxels; %d pairs, %d saddles"
                         % (nb, height.size, first.size, pairs.shape[0], saddle.size))
    if nb > 1 and not (np.diff(index) > 0).all():
        raise ValueError("merge_basins: peak_index must ascend")
    a = np.searchsorted(index, pairs[:, 0])
    b = np.searchsorted(index, pairs[:, 1])
    if pairs.size and not (np.array_equal(index[np.minimum(a, nb - 1)], pairs[:, 0])
                           and np.array_equal(index[np.minimum(b, nb - 1)], pairs[:, 1])):
        raise ValueError("merge_basins: a pair names a voxel that is no peak")
    with np.errstate(invalid="ignore"):
        order = np.lexsort((b, a, -saddle))
    root = list(range(nb))
    top = list(range(nb))                                 # a cluster's peak, kept at its root
    hl, sl = height.tolist(), saddle.tolist()
    al, bl = a.tolist(), b.tolist()

    def find(i):
        r = i
        while root[r] != r:
            r = root[r]
        while root[i] != r:
            root[i], i = r, root[i]
        return r

    for e in order.tolist():
        ra, rb = find(al[e]), find(bl[e])
        if ra == rb:
            continue
        pa, pb = top[ra], top[rb]
        a_greater = hl[pa] > hl[pb] or (hl[pa] == hl[pb] and pa < pb)       # basins ascend with their peak's index
        hi, lo = (ra, rb) if a_greater else (rb, ra)
        with np.errstate(invalid="ignore"):
            stands = np.float64(hl[top[lo]]) - np.float64(sl[e]) >= prominence
        if not stands:
            root[lo] = hi
    cluster = np.fromiter((find(i) for i in range(nb)), dtype=np.int64, count=nb)
    lowest = np.full(nb, np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(lowest, cluster, first)
    roots = np.flatnonzero(lowest != np.iinfo(np.int64).max)
    number = np.zeros(nb, dtype=np.int32)
    number[roots[np.argsort(lowest[roots], kind="stable")]] = np.arange(1, roots.size + 1, dtype=np.int32)
    return number[cluster], int(roots.size)


def split_components(labels, height, prominence, connectivity=26, max_basins=1 << 20):
    """Splits the components of a device int32 label volume (D, H, W) along the watershed of a device float32 height
    of the same shape: basins() and basin_saddles() on the device, merge_basins on the host, and a relabelling through
    a rank table and index_select.  prominence = 0 keeps every basin, inf gives back the components' voxels.
    -> (labels int32 (D, H, W) on the device, n, info), the pieces numbered 1..n in raster order of their first voxel;
    info = {"n_before", "n_basins", "n_edges", "n_after", "parent": the old label of each new piece}."""
    prominence = _check_prominence("split_components", prominence)
    if int(max_basins) != max_basins or max_basins < 1:
        raise ValueError("split_components: max_basins must be an integer of at least 1 (got %r)" % (max_basins,))
    _check_watershed("split_components", height, labels, connectivity)
    peaks, n_basins = basins(height, labels, connectivity)
    if n_basins > max_basins:
        raise ValueError("split_components: %d basins, more than max_basins = %d: smooth the height first "
                         "(pre-smoothing removes the noise's peaks) or, if the count is wanted, raise max_basins; a "
                         "larger prominence merges them but does not lower this count" % (n_basins, max_basins))
    with torch.cuda.device(height.device):
        pairs, saddle = basin_saddles(height, labels, peaks, connectivity)
        flat = peaks.reshape(-1)
        is_peak = flat == torch.arange(flat.numel(), dtype=torch.int32, device=flat.device)
        rank = torch.cumsum(is_peak, 0, dtype=torch.int32) - 1     # rank[peak] = its basin, in ascending peak index
        voxels = torch.nonzero(flat >= 0).reshape(-1)
        basin = rank.index_select(0, flat.index_select(0, voxels).to(torch.int64)).to(torch.int64)
        peak_index = torch.nonzero(is_peak).reshape(-1)
        # a basin's first voxel: the stable sort keeps the voxels of a basin in ascending order
        by_basin = torch.sort(basin, stable=True)
        _, counts = torch.unique_consecutive(by_basin.values, return_counts=True)
        first = voxels.index_select(0, by_basin.indices.index_select(0, torch.cumsum(counts, 0) - counts))
        old = labels.reshape(-1).index_select(0, peak_index)
        peak_height = height.reshape(-1).index_select(0, peak_index)
        n_before = int(labels.max()) if labels.numel() else 0
        piece, n_after = merge_basins(peak_index.cpu().numpy(), peak_height.cpu().numpy(), pairs.cpu().numpy(),
                                      saddle.cpu().numpy(), prominence, first_voxel=first.cpu().numpy())
        parent = np.zeros(n_after, dtype=np.int64)
        parent[piece - 1] = old.cpu().numpy()
        table = torch.from_numpy(piece).to(flat.device)
        out = torch.zeros_like(flat)
        out[voxels] = table.index_select(0, basin)
    info = {"n_before": n_before, "n_basins": int(n_basins), "n_edges": int(pairs.shape[0]), "n_after": int(n_after),
            "parent": [int(p) for p in parent]}
    return out.reshape(labels.shape), int(n_after), info
