"""
CPU tier of the per-step convergence trace: the two C entries are declared, exported and bound within
ABI 13 and refuse bad arguments on the host before any HIP call, the workspace query answers 0 for what the entry
refuses, patches.blend_shares is the one-shot Hann blend's share of every patch (it sums to 1 exactly where
stitch_patches has a weight), the yardstick of tests/trace_ref.py and metrics.trace_figures hold on hand-made
numbers, and the loops carry the trace= keyword.  No GPU is touched here.
"""

import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import trace_ref as TR
from conftest import PKG, ROOT
from guided_diffusion import _hip, joint, metrics, patches
from guided_diffusion.gaussian_diffusion import GaussianDiffusion

FAKE = 1 << 20          # a non-null "device pointer" no call below may ever dereference: each fails validation first
ENTRIES = ("ddpm3d_trace_moments", "ddpm3d_trace_moments_workspace_bytes")
ONE_SHORT = "one byte less than the entry's own answer"      # resolved in the test body, not at collection


# ------------------------------------------------------------------------------------------ the C entries
def test_entries_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ddpm3d.h")).read()
    declared = set(re.findall(r"\b(ddpm3d_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in ENTRIES:
        assert name in declared and name in _hip.EXPORTS and hasattr(lib, name), name
    assert re.search(r"#define DDPM3D_ABI_VERSION 13\b", hdr) and _hip.ABI_VERSION == 13
    assert _hip.load().ddpm3d_abi_version() == 13
    cols = dict((n, int(v)) for n, v in re.findall(r"\bDDPM3D_TR_([A-Z0-9_]+) = (\d+)", hdr))
    mine = {k[3:]: getattr(_hip, k) for k in dir(_hip) if k.startswith("TR_")}
    assert cols == mine and cols["REC"] == 10 and sorted(cols.values()) == list(range(11))
    assert {k: getattr(TR, k) for k in cols} == cols                        # the yardstick's columns are the header's
    assert re.search(r"#define DDPM3D_TRACE_MAX_BATCH 4096\b", hdr) and _hip.TRACE_MAX_BATCH == 4096
    assert "trace.o" in open(os.path.join(PKG, "csrc", "Makefile")).read()


def _trace(**over):
    lib = _hip.load()
    a = dict(est=FAKE, prev=FAKE, target=FAKE, weight=FAKE, B=2, voxels=4096, target_stride=4096, weight_stride=0,
             ws=FAKE, ws_bytes=1 << 30, out=FAKE, stream=None)
    a.update(over)
    if a["ws_bytes"] == ONE_SHORT:
        a["ws_bytes"] = lib.ddpm3d_trace_moments_workspace_bytes(a["B"], a["voxels"]) - 1
        assert a["ws_bytes"] > 0
    rc = lib.ddpm3d_trace_moments(*a.values())
    return rc, lib.ddpm3d_last_error().decode()


@pytest.mark.parametrize("over", [
    dict(est=None), dict(out=None), dict(ws=None),
    dict(B=0), dict(B=-3), dict(B=4097), dict(voxels=0), dict(voxels=-4096), dict(voxels=(1 << 40) + 1),
    dict(target_stride=1), dict(target_stride=4095), dict(target_stride=-4096), dict(target_stride=8192),
    dict(weight_stride=4), dict(weight_stride=4097), dict(weight_stride=-1),
    dict(target=None), dict(weight=None, weight_stride=4096), dict(target=None, weight=None, weight_stride=4096),
    dict(ws_bytes=0), dict(ws_bytes=ONE_SHORT), dict(ws=FAKE + 8), dict(ws=FAKE + 4),
])
def test_trace_moments_refuses_bad_arguments(over):
    rc, msg = _trace(**over)
    assert rc == _hip.E_INVAL and msg.startswith("trace_moments:"), (rc, msg)


def test_workspace_query():
    q = _hip.load().ddpm3d_trace_moments_workspace_bytes
    for bad in ((0, 100), (4097, 100), (-1, 100), (1, 0), (1, -5), (1, (1 << 40) + 1)):
        assert q(*bad) == 0, bad
    sizes = [1, 3, 4, 1000, 1024, 1025, 1 << 16, 96 ** 3, 2049 * 1024 + 3, 700 * 440 * 440, 1 << 40]
    for B in (1, 2, 8, 4096):
        got = [q(B, v) for v in sizes]
        assert got[0] == B * 80 and all(b >= a for a, b in zip(got, got[1:])), got
        assert got[-1] == B * 2048 * 80                        # at most 2048 records of ten doubles per estimate


# ------------------------------------------------------------------------------------------ blend shares
def _geometry(shape, res, overlap):
    D, Hh, W = shape
    if overlap is None:
        starts = patches.xy_starts(Hh, res), patches.xy_starts(W, res), patches.z_starts(D, res)
        grid = patches.patch_grid(shape, res)
    else:
        starts = tuple(patches.sliding_starts(n, res, overlap) for n in (Hh, W, D))
        grid = patches.sliding_grid(shape, res, overlap)
    assert grid == [(x, y, z) for x in starts[0] for y in starts[1] for z in starts[2]]
    return starts, grid


@pytest.mark.parametrize("shape,overlap", [((24, 40, 40), None), ((24, 40, 40), 6), ((10, 40, 33), None),
                                           ((37, 21, 50), 9)], ids=["fixed", "overlap6", "short-fixed", "overlap9"])
def test_blend_shares_sum_to_one_on_the_blend_cover(shape, overlap):
    """patch p's share of a voxel is the product of its three rows rounded once to fp32: over the patches the shares
    sum to 1 within (c + 1) 2^-24 (c roundings of at most 2^-24 each, the fp64 rows' own error far below one more)
    on the voxels blend_cover marks and are exactly 0 on the others; the cover is stitch_patches' wsum > 0"""
    res = 16
    D, Hh, W = shape
    (xs, ys, zs), grid = _geometry(shape, res, overlap)
    sx, sy, sz = (patches.blend_shares(s, n, res) for s, n in ((xs, Hh), (ys, W), (zs, D)))
    for s, starts in ((sx, xs), (sy, ys), (sz, zs)):
        assert s.shape == (len(starts), res) and s.dtype == np.float64 and s.min() >= 0 and s.max() <= 1
    total = np.zeros((Hh, W, D), dtype=np.float64)
    count = np.zeros((Hh, W, D), dtype=np.int64)
    for p, (x0, y0, z0) in enumerate(grid):
        ix, iy, iz = p // (len(ys) * len(zs)), (p // len(zs)) % len(ys), p % len(zs)
        w = ((sx[ix][:, None, None] * sy[iy][None, :, None]) * sz[iz][None, None, :]).astype(np.float32)
        hx, wy, dz = min(res, Hh - x0), min(res, W - y0), min(res, D - z0)
        assert not w[hx:].any() and not w[:, wy:].any() and not w[:, :, dz:].any()   # nothing past the volume
        total[x0:x0 + hx, y0:y0 + wy, z0:z0 + dz] += w[:hx, :wy, :dz].astype(np.float64)
        count[x0:x0 + hx, y0:y0 + wy, z0:z0 + dz] += 1
    cover = patches.blend_cover(grid, shape, res)
    _, wsum = patches.stitch_patches([np.zeros((res, res, res), np.float32)] * len(grid), grid, shape, res)
    assert np.array_equal(cover, wsum > 0) and 0 < cover.sum() < cover.size
    c = int(count.max())
    dev = np.abs(total[cover] - 1.0).max()
    print("%s overlap %s: %d patches, c = %d, largest deviation from 1 on the cover %.3g" % (shape, overlap, len(grid),
                                                                                          c, dev))
    assert dev <= (c + 1) * 2.0 ** -24
    assert np.all(total[~cover] == 0.0)


def test_blend_shares_differ_from_the_joint_table_on_the_outermost_planes():
    starts = patches.sliding_starts(40, 16, 6)
    s = patches.blend_shares(starts, 40, 16)
    assert s[0][0] == 0.0 and s[-1][-1] == 0.0                     # no Hann weight there: no share, not an equal one
    table = patches._axis_table(starts, 40, 16, "H")
    assert table[0][0] == 1.0 and np.array_equal(s[0][1:], table[0][1:16])
    with pytest.raises(ValueError):
        patches.blend_shares([0, 40], 40, 16)


# ------------------------------------------------------------------------------------------ yardstick, figures
def test_reference_moments_by_hand():
    x = np.array([[0.5, -1.0, 2.0, np.nan]], dtype=np.float32)
    p = np.array([[0.0, -1.0, 1.0, np.inf]], dtype=np.float32)
    y = np.array([1.0, -0.5, 1.0, np.nan], dtype=np.float32)
    w = np.array([0.5, 1.0, 0.25, 0.0], dtype=np.float32)
    rec, mag = TR.moments(x, p, y, w)
    want = {TR.W: 1.75, TR.N: 3, TR.SUM_E: -0.25 - 0.5 + 0.25, TR.SUM_ABS_E: 0.25 + 0.5 + 0.25,
            TR.SUM_SQ_E: 0.125 + 0.25 + 0.25, TR.SUM_SQ_Y: 0.5 + 0.25 + 0.25, TR.SUM_X: 0.25 - 1.0 + 0.5,
            TR.SUM_SQ_X: 0.125 + 1.0 + 1.0, TR.SUM_SQ_D: 0.125 + 0.0 + 0.25, TR.CLIPPED: 1.25}
    assert rec.shape == (1, TR.REC) and all(rec[0, k] == v for k, v in want.items()), rec
    assert mag[0, TR.SUM_E] == 1.0 and mag[0, TR.SUM_X] == 1.75
    bare, _ = TR.moments(x[:, :3])
    assert bare[0, TR.W] == 3 and bare[0, TR.N] == 3 and not bare[0, list(TR.NEEDS_TARGET) + [TR.SUM_SQ_D]].any()


def _record(**cols):
    r = np.zeros(TR.REC)
    for k, v in cols.items():
        r[getattr(TR, k)] = v
    return r


def test_trace_figures_on_hand_made_records():
    a = _record(W=2.0, N=2, SUM_E=-0.2, SUM_ABS_E=0.6, SUM_SQ_E=0.08, SUM_SQ_Y=2.0, SUM_X=1.0, SUM_SQ_X=1.0,
                SUM_SQ_D=0.5, CLIPPED=0.5)
    b = _record(W=2.0, N=3, SUM_E=0.6, SUM_ABS_E=0.2, SUM_SQ_E=0.08, SUM_SQ_Y=6.0, SUM_X=3.0, SUM_SQ_X=5.0,
                SUM_SQ_D=1.5, CLIPPED=0.5)
    rows = metrics.trace_figures(np.stack([np.stack([a, b]), np.stack([b, b])]), data_range=2.0)
    assert len(rows) == 2
    r = rows[0]
    assert r["weight"] == 4.0 and r["mse"] == pytest.approx(0.04) and r["psnr"] == pytest.approx(20.0)
    assert r["nrmse"] == pytest.approx(math.sqrt(0.16 / 8.0)) and r["mae"] == pytest.approx(0.2)
    assert r["bias"] == pytest.approx(0.1) and r["mean"] == 1.0 and r["std"] == pytest.approx(math.sqrt(0.5))
    assert r["clipped"] == 0.25 and r["delta_rms"] is None                  # the first step has no step before it
    assert rows[1]["delta_rms"] == pytest.approx(math.sqrt(3.0 / 4.0)) and rows[1]["mean"] == 1.5
    # a (T, REC) array is one record per step
    one = metrics.trace_figures(np.stack([a, b]), data_range=2.0)
    assert one[0]["mean"] == 0.5 and one[1]["bias"] == pytest.approx(0.3)


def test_trace_figures_none_cases_and_pooling_order():
    a = _record(W=2.0, N=2, SUM_E=-0.2, SUM_ABS_E=0.6, SUM_SQ_E=0.08, SUM_SQ_Y=2.0, SUM_X=1.0, SUM_SQ_X=1.0)
    err = ("psnr", "nrmse", "mae", "bias", "mse")
    r = metrics.trace_figures(a[None, None])[0]                              # no data range: no PSNR, the rest stays
    assert r["psnr"] is None and r["nrmse"] is not None and r["mae"] == pytest.approx(0.3)
    r = metrics.trace_figures(a[None, None], data_range=1.0, has_target=False)[0]
    assert all(r[k] is None for k in err) and r["mean"] == 0.5 and r["std"] is not None and r["clipped"] == 0.0
    r = metrics.trace_figures(_record()[None, None], data_range=1.0)[0]      # nothing counted: every ratio is None
    assert all(r[k] is None for k in err + ("mean", "std", "clipped")) and r["weight"] == 0.0
    z = a.copy()
    z[TR.SUM_SQ_Y] = 0.0
    assert metrics.trace_figures(z[None, None], data_range=1.0)[0]["nrmse"] is None
    z = a.copy()
    z[TR.SUM_SQ_E] = 0.0
    assert metrics.trace_figures(z[None, None], data_range=1.0)[0]["psnr"] == math.inf
    # negative variance from rounding is clamped
    z = _record(W=1.0, N=1, SUM_X=1.0, SUM_SQ_X=1.0 - 1e-16)
    assert metrics.trace_figures(z[None, None], has_target=False)[0]["std"] == 0.0
    # pooled by summing in index order: ((1e16 + 1) + -1e16) + 1 = 1 in that order (the first 1 is lost), 0 with the
    # last two swapped (both are lost)
    parts = [_record(W=1.0, SUM_X=v) for v in (1e16, 1.0, -1e16, 1.0)]
    assert metrics.trace_figures(np.stack(parts)[None], has_target=False)[0]["mean"] == 1.0 / 4.0
    swapped = [parts[i] for i in (0, 1, 3, 2)]
    assert metrics.trace_figures(np.stack(swapped)[None], has_target=False)[0]["mean"] == 0.0
    for bad in (np.zeros((2, 3)), np.zeros((2, 2, TR.REC + 1)), np.zeros(TR.REC)):
        with pytest.raises(ValueError):
            metrics.trace_figures(bad)
    for bad in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(ValueError):
            metrics.trace_figures(a[None, None], data_range=bad)


# ------------------------------------------------------------------------------------------ host side
def test_step_trace_refuses_host_tensors():
    x = torch.zeros(2, 1, 4, 4, 4)
    for kw in (dict(target=x), dict(weight=x), dict(target=x.numpy())):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            metrics.StepTrace(**kw)
    tr = metrics.StepTrace()
    assert tr.t == []
    with pytest.raises(ValueError, match="no step"):
        tr.records()
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        tr.add(x, None, 0, 3)


def test_every_loop_takes_trace_and_defaults_to_none():
    names = ["p_sample_loop", "ddim_sample_loop", "dpm_solver_sample_loop", "ddim_reverse_sample_loop"]
    fns = [getattr(GaussianDiffusion, n + s) for n in names for s in ("", "_progressive")]
    fns += [joint.sample_loop_progressive]
    for fn in fns:
        p = inspect.signature(fn).parameters
        assert "trace" in p and p["trace"].default is None, fn
    assert "kwargs" in inspect.signature(joint.sample_loop).parameters


def test_script_has_the_trace_flag():
    import importlib.util
    spec = importlib.util.spec_from_file_location("ddpm3d_infer_entry", os.path.join(PKG, "scripts", "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    p = mod.create_argparser()
    assert p.parse_args([]).trace is False and p.parse_args(["--trace", "True"]).trace is True
