"""
Low-pass data-consistency guidance of the samplers (an extension).

The reference applies `denoised_fn` to a step's x_start prediction before the clip and before the posterior mean
(gaussian_diffusion.py:293-314).  LowPassPull is one operator for that position, evaluated on the GPU by
ddpm3d_xstart_pull (csrc/guide.hip):

    x0 = clip(x0_raw + w * G(y - x0_raw))

with y a measurement in x's units (by default the low-dose conditioning volume), G the package's separable Gaussian
with renormalised faces (metrics.gaussian_taps / ddpm3d_gauss_smooth's rule) and w in [0, 1]: the sample's local means
are corrected towards the measurement's, its detail above the filter's band is left alone.  This is the low-pass
correction of ILVR (Choi et al. 2021, arXiv:2108.02938) and the range-space correction of DDNM (Wang et al. 2022,
arXiv:2212.00490) with G as the measurement operator.  Every loop takes it as `guide=`; the step then runs on the
ddpm3d_*_step_x0 entries, which take the pulled x0 in place of the model output's first half.  `denoised_fn` and
`cond_fn` themselves stay refused.
"""

import ctypes
import math

import numpy as np
import torch as th

from . import _hip as H
from . import metrics


def _number(value, what):
    try:
        v = math.nan if isinstance(value, (bool, str)) else float(value)
    except (TypeError, ValueError):
        v = math.nan
    if not math.isfinite(v):
        raise ValueError("%s must be a finite number (got %r)" % (what, value))
    return v


def pull_taps(fwhm_mm, spacing):
    """The taps of the pull's Gaussian: metrics.gaussian_taps(fwhm_mm, spacing) for a positive FWHM; a FWHM of 0 is the
    pointwise pull, radii (0, 0, 0) with one unit tap per axis, and needs no spacing.  -> metrics.GaussianTaps"""
    fwhm = _number(fwhm_mm, "LowPassPull: fwhm_mm")
    if fwhm < 0:
        raise ValueError("LowPassPull: fwhm_mm must be 0 (pointwise) or positive, got %r" % (fwhm_mm,))
    if fwhm == 0:
        return metrics.GaussianTaps((0.0,) * 3, None if spacing is None else tuple(spacing), (0.0,) * 3, (0,) * 3,
                                    ((1.0,),) * 3)
    if spacing is None:
        raise ValueError("LowPassPull: a positive fwhm_mm needs the voxel spacing in mm")
    return metrics.gaussian_taps(fwhm, spacing)


class LowPassPull:
    """guide= of the sampling loops: x0 = clip(x0_raw + weight * G(measurement - x0_raw)) on the steps whose original
    timestep is >= stop_t.

    fwhm_mm, spacing  the Gaussian, as metrics.gaussian_taps takes them (built once, here, on the host); fwhm_mm = 0 is
                      the pointwise pull and needs no spacing
    weight            a float in [0, 1]; 0 never launches anything in a loop
    stop_t            the guide is active on steps whose original timestep (through timestep_map under respacing) is
                      >= stop_t; 0: every step
    measurement       an (N, 1, D, H, W) float32 device tensor in x's units, or None: model_kwargs["low_res"], which
                      must then exist and have x's shape."""

    def __init__(self, fwhm_mm, spacing, weight=1.0, stop_t=0, measurement=None):
        self.taps = pull_taps(fwhm_mm, spacing)
        w = _number(weight, "LowPassPull: weight")
        if not 0.0 <= w <= 1.0:
            raise ValueError("LowPassPull: weight must lie in [0, 1], got %r" % (weight,))
        self.weight = ctypes.c_float(w).value
        if isinstance(stop_t, bool) or not isinstance(stop_t, (int, np.integer)) or stop_t < 0:
            raise ValueError("LowPassPull: stop_t must be a non-negative integer, got %r" % (stop_t,))
        self.stop_t = int(stop_t)
        if measurement is not None and not isinstance(measurement, th.Tensor):
            raise ValueError("LowPassPull: measurement must be a tensor or None, got %r" % type(measurement))
        self.measurement = measurement

    @property
    def radii(self):
        return self.taps.radii

    def active(self, diffusion, i):
        """Whether the step at index i of `diffusion` is pulled: weight > 0 and its original timestep >= stop_t."""
        tmap = getattr(diffusion, "timestep_map", None)
        return self.weight > 0.0 and (i if tmap is None else tmap[i]) >= self.stop_t

    @staticmethod
    def _checked(y, shape, device):
        if not isinstance(y, th.Tensor) or tuple(y.shape) != tuple(shape):
            raise ValueError("guide: the measurement has shape %s, the sample %s"
                             % (tuple(getattr(y, "shape", ())), tuple(shape)))
        if len(shape) != 5 or shape[1] != 1:
            raise ValueError("guide: LowPassPull works on (N, 1, D, H, W) samples, got %s" % (tuple(shape),))
        if device is not None and y.device != th.device(device):
            y = y.to(device)
        if y.dtype != th.float32 or not y.is_contiguous():
            y = y.to(th.float32).contiguous()
        return y

    def resolve(self, shape, model_kwargs, device=None):
        """The measurement of a loop on batches of `shape`, checked before the model runs: the pull's own, else
        model_kwargs["low_res"]."""
        y = self.measurement
        if y is None:
            y = (model_kwargs or {}).get("low_res")
            if y is None:
                raise ValueError("guide: LowPassPull has no measurement and model_kwargs has no \"low_res\" to take "
                                 "its place")
        return self._checked(y, shape, device)

    def apply(self, model_output, x, t, flags, diffusion, measurement=None, out=None):
        """The single-call form: the pulled x0 of one step, a tensor of x's shape.  model_output: the network's output
        for (x, t); t: (N,) step indices of `diffusion`, whose coefficient table the kernel reads; flags: the step's
        (diffusion._flags(clip_denoised)); measurement: defaults to the pull's own."""
        y = self.measurement if measurement is None else measurement
        if y is None:
            raise ValueError("LowPassPull.apply: no measurement (give measurement=, or build the pull with one)")
        H.require_device(x, "x")
        y = self._checked(y, x.shape, x.device)
        H.require_device(y, "measurement")
        diffusion._model_step_output(model_output, x, flags)
        N, _, D, Hh, W = x.shape
        lib = H.load()
        need = lib.ddpm3d_xstart_pull_workspace_bytes(N, D, Hh, W)
        if need == 0:
            raise ValueError("LowPassPull.apply: a batch of shape %s is beyond ddpm3d_xstart_pull (N <= 65535, "
                             "N * D * H * W <= 2^31 - 1)" % (tuple(x.shape),))
        with th.cuda.device(x.device):
            t = t.to(device=x.device, dtype=th.int64).contiguous()
            if out is None:
                out = th.empty_like(x)
            H.require_device(out, "out")
            ws = th.empty(need // 4, dtype=th.float32, device=x.device)
            tp = self.taps
            H.check(lib.ddpm3d_xstart_pull(H.ptr(model_output), H.ptr(x), H.ptr(y),
                                           H.ptr(diffusion._device_state(x.device)["coef"]), H.ptr(t), N, D, Hh, W,
                                           diffusion.num_timesteps, flags, self.weight, tp.radii[0], tp.radii[1],
                                           tp.radii[2], tp.tables[0], tp.tables[1], tp.tables[2], H.ptr(out),
                                           H.ptr(ws), need, H.stream()))
        return out


def check_guide(guide):
    if guide is not None and not isinstance(guide, LowPassPull):
        raise ValueError("guide must be a guidance.LowPassPull or None, got %r" % type(guide))
