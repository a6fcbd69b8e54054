"""
Volume regridding between a scanner's voxel spacing and the spacing the model was trained at (DESIGN.md 3.17;
include/ddpm3d.h has the definitions).  Separable: one banded linear map per axis, built here on the host in fp64,
rounded once to fp32 and applied on the device by one call of ddpm3d_regrid (csrc/regrid.hip): one launch per axis
whose extent changes, in the order W, H, D.  There is no host fallback.

For an axis of input extent Li and output extent Lo: scale = Li / Lo, fs = max(1, scale) (the kernel is widened when
shrinking: the anti-aliasing), and for output index o

    c     = (o + 0.5) * scale                       half-voxel centres, the volumes' faces aligned
    first = max(0,  int(c - S * fs + 0.5))
    end   = min(Li, int(c + S * fs + 0.5))
    w_k   = f((k + 0.5 - c) / fs),  k = first .. end - 1,   divided by their sum

with f the triangle (S = 1, mode "linear") or Keys' cubic with a = -0.5 (S = 2, mode "cubic").  Taps beyond a face are
not counted and the rest are renormalised, so faces do not darken.  Cubic weights are negative in places: the output
can undershoot below 0 and is not clamped.  An axis with Li == Lo is the identity and is skipped.

grid_shape turns two spacings into the output shape, plan builds the tables (and keeps their device copies), apply
regrids a (D, H, W) volume or a (K, D, H, W) stack, keep_after carries a mask of counted voxels across a plan.
"""

import math

import numpy as np
import torch

from . import _hip as H

MODES = {"linear": 1, "cubic": 2}       # mode -> support S of its kernel
MIN_RATIO, MAX_RATIO = 0.25, 4.0        # Li / Lo per axis: at most 2 S fs + 1 = 17 taps (cubic at ratio 4)
AXES = "DHW"


def _kernel(mode, x):
    x = np.abs(x)
    if mode == "linear":
        return np.where(x < 1.0, 1.0 - x, 0.0)
    a = -0.5
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    far = (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


class AxisTable:
    """The banded map of one axis: in_len, out_len, scale = in_len / out_len, taps (the largest count; 0 for the
    identity), first and count ([out_len] int32) and the weights as [out_len][taps] arrays, zero beyond count: weights64
    as formed and normalised in fp64, weights their one rounding to fp32."""

    def __init__(self, in_len, out_len, taps, first, count, weights64):
        self.in_len, self.out_len, self.taps = int(in_len), int(out_len), int(taps)
        self.scale = self.in_len / self.out_len
        self.first, self.count, self.weights64 = first, count, weights64
        self.weights = weights64.astype(np.float32)

    @property
    def identity(self):
        return self.taps == 0


def axis_table(in_len, out_len, mode="linear"):
    """The AxisTable from in_len to out_len (see the module's head); the identity when they are equal."""
    if mode not in MODES:
        raise ValueError("regrid: unknown mode %r (one of %s)" % (mode, ", ".join(sorted(MODES))))
    Li, Lo = int(in_len), int(out_len)
    if Li == Lo:
        return AxisTable(Li, Lo, 0, np.zeros(Lo, np.int32), np.zeros(Lo, np.int32), np.zeros((Lo, 0), np.float64))
    S = MODES[mode]
    scale = Li / Lo
    fs = max(1.0, scale)
    first, count, rows = np.zeros(Lo, np.int32), np.zeros(Lo, np.int32), []
    for o in range(Lo):
        c = (o + 0.5) * scale
        lo, hi = max(0, int(c - S * fs + 0.5)), min(Li, int(c + S * fs + 0.5))
        w = _kernel(mode, (np.arange(lo, hi, dtype=np.float64) + 0.5 - c) / fs)
        rows.append(w / math.fsum(w))
        first[o], count[o] = lo, hi - lo
    taps = int(count.max())
    if taps > H.REGRID_MAX_TAPS:
        raise ValueError("regrid: %d taps from %d to %d (at most DDPM3D_REGRID_MAX_TAPS = %d)"
                         % (taps, Li, Lo, H.REGRID_MAX_TAPS))
    weights = np.zeros((Lo, taps), np.float64)
    for o, w in enumerate(rows):
        weights[o, :w.size] = w
    return AxisTable(Li, Lo, taps, first, count, weights)


def _shape3(shape, what):
    try:
        s = () if isinstance(shape, str) else tuple(int(v) for v in shape)
        ok = len(s) == 3 and all(v >= 1 for v in s) and all(float(v) == int(v) for v in shape)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("regrid: %s must be three extents of at least 1 (got %r)" % (what, shape))
    if s[0] * s[1] * s[2] > 2 ** 31 - 1:
        raise ValueError("regrid: %s %s has more than 2^31 - 1 voxels" % (what, s))
    return s


def _spacing3(spacing, what):
    try:
        s = () if isinstance(spacing, str) else tuple(float(v) for v in spacing)
        ok = len(s) == 3 and all(math.isfinite(v) and v > 0 for v in s)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("regrid: %s must be three positive finite numbers (got %r)" % (what, spacing))
    return s


def grid_shape(shape, spacing, model_spacing):
    """The shape of a volume of `shape` voxels of `spacing` mm on a grid of `model_spacing` mm: per axis
    max(1, floor(L * s / m + 0.5)), so that the physical extent is kept as nearly as whole voxels allow."""
    shape = _shape3(shape, "shape")
    s, m = _spacing3(spacing, "spacing"), _spacing3(model_spacing, "model_spacing")
    return tuple(max(1, int(math.floor(L * a / b + 0.5))) for L, a, b in zip(shape, s, m))


class RegridPlan:
    """plan()'s return: shape_in, shape_out, mode, axes (three AxisTables, D, H, W), scale (in / out per axis); the
    device copies of the tables are made once per device on first use."""

    def __init__(self, shape_in, shape_out, mode, axes):
        self.shape_in, self.shape_out, self.mode, self.axes = tuple(shape_in), tuple(shape_out), mode, tuple(axes)
        self.scale = tuple(a.scale for a in self.axes)
        self._device = {}
        self._inverse = self._absolute = None

    @property
    def identity(self):
        return all(a.identity for a in self.axes)

    def inverse(self):
        """The plan from shape_out back to shape_in, in the same mode (not the inverse map: regridding loses what the
        coarser grid cannot hold)."""
        if self._inverse is None:
            self._inverse = plan(self.shape_out, self.shape_in, self.mode)
            self._inverse._inverse = self
        return self._inverse

    def absolute(self):
        """The same plan with |w| as weights (fp64 and fp32 alike): what bounds the rounding error, and what tells
        which inputs enter an output with a non-zero tap."""
        if self._absolute is None:
            axes = []
            for a in self.axes:
                t = AxisTable(a.in_len, a.out_len, a.taps, a.first, a.count, np.abs(a.weights64))
                t.weights = np.abs(a.weights)
                axes.append(t)
            self._absolute = RegridPlan(self.shape_in, self.shape_out, self.mode, axes)
        return self._absolute

    def device_axes(self, device):
        """(the ctypes array of three ddpm3d_regrid_axis, the tensors it points into) on `device`"""
        key = str(device)
        if key not in self._device:
            arr, keep = (H.RegridAxis * 3)(), []
            for i, a in enumerate(self.axes):
                arr[i].in_len, arr[i].out_len, arr[i].taps = a.in_len, a.out_len, a.taps
                if a.taps:
                    t = [torch.from_numpy(np.ascontiguousarray(v)).to(device)
                         for v in (a.first, a.count, a.weights.T)]                 # weights as [tap][out_len]
                    arr[i].first, arr[i].count, arr[i].weights = (H.ptr(v) for v in t)
                    keep.append(t)
            self._device[key] = (arr, keep)
        return self._device[key]


def plan(shape_in, shape_out, mode="linear"):
    """The RegridPlan from shape_in to shape_out, both (D, H, W).  Host arithmetic only."""
    if mode not in MODES:
        raise ValueError("regrid: unknown mode %r (one of %s)" % (mode, ", ".join(sorted(MODES))))
    shape_in, shape_out = _shape3(shape_in, "shape_in"), _shape3(shape_out, "shape_out")
    for name, Li, Lo in zip(AXES, shape_in, shape_out):
        if not MIN_RATIO <= Li / Lo <= MAX_RATIO:
            raise ValueError("regrid: axis %s: %d -> %d voxels is a ratio of %g, outside [1/4, 4]"
                             % (name, Li, Lo, Li / Lo))
    return RegridPlan(shape_in, shape_out, mode, [axis_table(Li, Lo, mode) for Li, Lo in zip(shape_in, shape_out)])


def apply(volume, plan):
    """A device float32 (D, H, W) volume or (K, D, H, W) stack of plan.shape_in on plan.shape_out: one call of
    ddpm3d_regrid, nothing copied to the host, a new tensor.  The volumes of a stack do not see each other."""
    if not isinstance(plan, RegridPlan):
        raise ValueError("regrid.apply: plan must be regrid.plan's return (got %s)" % type(plan).__name__)
    if not (isinstance(volume, torch.Tensor) and volume.is_cuda):
        raise ValueError("regrid.apply: volume must live on the GPU: this package runs on HIP kernels only (got %s)"
                         % getattr(volume, "device", type(volume)))
    if volume.dtype != torch.float32 or not volume.is_contiguous():
        raise ValueError("regrid.apply: volume must be contiguous float32")
    if volume.dim() not in (3, 4) or tuple(volume.shape[-3:]) != plan.shape_in:
        raise ValueError("regrid.apply: volume of shape %s, the plan takes %s or (K,) + %s"
                         % (tuple(volume.shape), plan.shape_in, plan.shape_in))
    K = int(volume.shape[0]) if volume.dim() == 4 else 1
    if not 1 <= K <= H.MAX_DRAWS:
        raise ValueError("regrid.apply: %d volumes (1..%d)" % (K, H.MAX_DRAWS))
    lib = H.load()
    need = lib.ddpm3d_regrid_workspace_bytes(K, *plan.shape_in, *plan.shape_out)
    if need == 0:
        raise ValueError("regrid.apply: %s -> %s has more than 2^31 - 1 voxels per volume after one of its passes"
                         % (plan.shape_in, plan.shape_out))
    with torch.cuda.device(volume.device):
        axes, _ = plan.device_axes(volume.device)
        out = torch.empty(tuple(volume.shape[:-3]) + plan.shape_out, dtype=torch.float32, device=volume.device)
        ws = torch.empty(need // 4, dtype=torch.float32, device=volume.device)
        H.check(lib.ddpm3d_regrid(H.ptr(volume), K, *plan.shape_in, axes, H.ptr(out), H.ptr(ws), need, H.stream()))
    return out


def keep_after(keep, plan):
    """A device uint8 (D, H, W) mask of counted voxels on the plan's input grid -> the mask on its output grid: an
    output voxel is counted iff every input voxel that enters it with a non-zero tap is counted.  Exact: the voxels
    left out, regridded with |w|, give a sum of non-negative terms, which is 0 iff each term is."""
    if not (isinstance(keep, torch.Tensor) and keep.is_cuda):
        raise ValueError("regrid.keep_after: keep must live on the GPU (got %s)" % getattr(keep, "device", type(keep)))
    if not isinstance(plan, RegridPlan):
        raise ValueError("regrid.keep_after: plan must be regrid.plan's return (got %s)" % type(plan).__name__)
    if keep.dtype != torch.uint8 or not keep.is_contiguous() or tuple(keep.shape) != plan.shape_in:
        raise ValueError("regrid.keep_after: keep must be contiguous uint8 of the plan's input shape %s"
                         % (plan.shape_in,))
    left_out = (keep == 0).to(torch.float32).contiguous()
    return (apply(left_out, plan.absolute()) == 0).to(torch.uint8).contiguous()
