"""
CPU tier of the image-quality metrics: the fp64 yardstick of tests/metrics_ref.py is cross-checked
so that it is not its own judge (an independent conv3d evaluation, constant volumes, x = y, scipy's taps), the test
phantoms are what the GPU tier assumes (mask share, SSIM away from 0 and 1), the four C entries are declared,
exported and bound within ABI 13, refuse bad arguments on the host before any HIP call and size their workspaces
sanely, the host formulas of PSNR / NRMSE hold, host tensors are refused, and the inference script refuses a
missing or mis-shaped --target_samples before a model is built.  No GPU is touched here.
"""

import ctypes
import importlib.util
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import metrics_ref as R
from conftest import PKG, ROOT
from guided_diffusion import _hip, metrics

FAKE = 1 << 20          # a non-null "device pointer" no call below may ever dereference: each fails validation first
ENTRIES = ("ddpm3d_error_moments", "ddpm3d_error_moments_workspace_bytes", "ddpm3d_ssim3d",
           "ddpm3d_ssim3d_workspace_bytes")
ONE_SHORT = "one byte less than the entry's own answer"      # resolved in the test body, not at collection
PAIRS = list(R.pairs())


# ------------------------------------------------------------------------------------------ the yardstick
def test_taps_are_scipys():
    t, s = R.taps(), R.scipy_taps()
    assert t.shape == s.shape == (11,) and abs(t.sum() - 1.0) < 1e-15
    assert np.abs(t - s).max() <= 2 * np.finfo(np.float64).eps
    assert np.array_equal(t, t[::-1]) and t.argmax() == 5


@pytest.mark.parametrize("name,x,y", PAIRS, ids=[p[0] for p in PAIRS])
def test_yardstick_agrees_with_an_independent_conv3d_evaluation(name, x, y):
    a, b = R.ssim_map(x, y, 1.0), R.ssim_map_conv3d(x, y, 1.0)
    assert a.shape == b.shape == tuple(n - 10 for n in x.shape) and a.dtype == np.float64
    err = np.abs(a - b).max()
    print("%s: scipy vs conv3d fp64, max per voxel %.3g" % (name, err))
    assert err <= 1e-12


@pytest.mark.parametrize("name,x,y", PAIRS, ids=[p[0] for p in PAIRS])
def test_phantoms_are_what_the_gpu_tier_assumes(name, x, y):
    """nothing can pass empty: the body mask counts 10..60 % of the voxels, the interior is non-empty and the
    yardstick's mean, masked or not, is far from both 0 and 1; the plain fp32 evaluation, which sets the GPU bound,
    is within 1e-4 of the yardstick."""
    mask = R.body_mask(y)
    share = mask.mean()
    smap = R.ssim_map(x, y, 1.0)
    plain, masked = R.masked_mean(smap, None), R.masked_mean(smap, mask)
    e32 = np.abs(R.ssim_map_fp32(x, y, 1.0) - smap).max()
    print("%s: mask share %.3f, ssim %.4f unmasked %.4f masked, e32 %.3g" % (name, share, plain, masked, e32))
    assert y.dtype == x.dtype == np.float32 and y.min() >= 0 and y.max() <= 1 and y.max() > 0.5
    assert 0.10 < share < 0.60
    assert smap.size > 0 and R.interior_mask(mask).sum() > 0
    assert 0.15 < plain < 0.95 and 0.15 < masked < 0.95
    assert 0 < e32 <= 1e-4


def test_yardstick_on_constants_and_identity():
    shape = (12, 13, 14)
    for a, b, L in ((0.3, 0.7, 1.0), (2.0, 2.5, 3.0), (0.0, 1.0, 1.0)):
        smap = R.ssim_map(np.full(shape, a), np.full(shape, b), L)
        assert smap.shape == (2, 3, 4)
        assert np.abs(smap - R.constant_ssim(a, b, L)).max() < 1e-12
    y = R.phantom((20, 24, 28), seed=7)
    assert np.abs(R.ssim_map(y, y, 1.0) - 1.0).max() < 1e-12
    assert R.ssim_map(y[:11, :11, :11], y[:11, :11, :11], 1.0).shape == (1, 1, 1)


def test_plain_fp32_loses_the_variance_on_an_offset():
    """why the kernel pivots: the same pair + 4 costs the un-pivoted fp32 evaluation two to three orders"""
    name, x, y = PAIRS[0]
    ref = R.ssim_map(x, y, 1.0)
    e0 = np.abs(R.ssim_map_fp32(x, y, 1.0) - ref).max()
    x4, y4 = (x + np.float32(4)), (y + np.float32(4))
    e4 = np.abs(R.ssim_map_fp32(x4, y4, 1.0) - R.ssim_map(x4, y4, 1.0)).max()
    print("%s: plain fp32 max per voxel %.3g, on an offset of 4 %.3g" % (name, e0, e4))
    assert e0 <= 1e-4 and e4 > 10 * e0


def test_reference_moments():
    x = np.array([1.0, 2.0, 4.0, 8.0], dtype=np.float32)
    y = np.array([1.5, 2.0, 3.0, -8.0], dtype=np.float32)
    m = R.moments(x, y, mask=np.array([1, 1, 1, 0], dtype=np.uint8), std=np.array([0.5, 0.0, 0.4, 100.0]))
    assert m["n"] == 3 and m["bias"] == pytest.approx(0.5 / 3) and m["mae"] == pytest.approx(0.5)
    assert m["mse"] == pytest.approx(1.25 / 3) and m["target_sq_mean"] == pytest.approx(15.25 / 3)
    assert (m["target_min"], m["target_max"]) == (1.5, 3.0) and (m["cover_1"], m["cover_2"]) == (2, 2)


# ------------------------------------------------------------------------------------------ host formulas
def test_psnr_and_nrmse_host_formulas():
    assert metrics.psnr(0.01, 1.0) == pytest.approx(20.0, abs=1e-12)
    assert metrics.psnr(1.0, 255.0) == pytest.approx(20 * math.log10(255.0), abs=1e-12)
    assert metrics.psnr(0.0, 1.0) == math.inf
    assert metrics.nrmse(0.04, 4.0) == pytest.approx(0.1, abs=1e-15)
    for bad in ((0.1, 0.0), (0.1, -1.0), (-0.1, 1.0), (0.1, float("nan"))):
        with pytest.raises(ValueError):
            metrics.psnr(*bad)
        with pytest.raises(ValueError):
            metrics.nrmse(*bad)


def test_host_tensors_are_refused():
    x = torch.zeros(12, 12, 12)
    for call in (lambda: metrics.error_moments(x, x), lambda: metrics.ssim3d(x, x, 1.0),
                 lambda: metrics.evaluate(x, x), lambda: metrics.evaluate(x.numpy(), x.numpy())):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            call()


# ------------------------------------------------------------------------------------------ the C entries
def test_entries_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ddpm3d.h")).read()
    declared = set(re.findall(r"\b(ddpm3d_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in ENTRIES:
        assert name in declared and name in _hip.EXPORTS and hasattr(lib, name), name
    assert re.search(r"#define DDPM3D_ABI_VERSION 13\b", hdr) and _hip.ABI_VERSION == 13
    assert _hip.load().ddpm3d_abi_version() == 13
    cols = dict((n, int(v)) for n, v in re.findall(r"\bDDPM3D_EM_([A-Z0-9_]+) = (\d+)", hdr))
    mine = {k[3:]: getattr(_hip, k) for k in dir(_hip) if k.startswith("EM_")}
    assert cols == mine and cols["REC"] == 10 and sorted(cols.values()) == list(range(11))
    assert "metrics.o" in open(os.path.join(PKG, "csrc", "Makefile")).read()


def _moments(**over):
    lib = _hip.load()
    a = dict(est=FAKE, target=FAKE, mask=None, std=None, B=2, voxels=4096, ws=FAKE, ws_bytes=1 << 30, out=FAKE,
             stream=None)
    a.update(over)
    if a["ws_bytes"] == ONE_SHORT:
        a["ws_bytes"] = lib.ddpm3d_error_moments_workspace_bytes(a["B"], a["voxels"]) - 1
        assert a["ws_bytes"] > 0
    rc = lib.ddpm3d_error_moments(*a.values())
    return rc, lib.ddpm3d_last_error().decode()


def _ssim(**over):
    lib = _hip.load()
    a = dict(est=FAKE, target=FAKE, mask=None, B=2, D=20, H=30, W=40, C1=1e-4, C2=9e-4, ws=FAKE, ws_bytes=1 << 30,
             map=None, out=FAKE, stream=None)
    a.update(over)
    if a["ws_bytes"] == ONE_SHORT:
        a["ws_bytes"] = lib.ddpm3d_ssim3d_workspace_bytes(a["B"], a["D"], a["H"], a["W"]) - 1
        assert a["ws_bytes"] > 0
    rc = lib.ddpm3d_ssim3d(*a.values())
    return rc, lib.ddpm3d_last_error().decode()


@pytest.mark.parametrize("over", [
    dict(est=None), dict(target=None), dict(out=None), dict(ws=None),
    dict(B=0), dict(B=-3), dict(B=65), dict(voxels=0), dict(voxels=-4096), dict(voxels=(1 << 40) + 1),
    dict(ws_bytes=0), dict(ws_bytes=ONE_SHORT),
    dict(ws=FAKE + 8),
])
def test_error_moments_refuses_bad_arguments(over):
    rc, msg = _moments(**over)
    assert rc == _hip.E_INVAL and msg.startswith("error_moments:"), (rc, msg)


@pytest.mark.parametrize("over", [
    dict(est=None), dict(target=None), dict(out=None), dict(ws=None),
    dict(B=0), dict(B=-1), dict(B=65),
    dict(D=0), dict(H=-30), dict(W=0), dict(D=10), dict(H=10), dict(W=10), dict(D=65536), dict(H=65536),
    dict(W=1 << 30), dict(H=65535, W=65535), dict(D=65535, H=30000, W=30000),
    dict(C1=-1e-9), dict(C2=-1.0), dict(C1=float("nan")), dict(C2=float("nan")), dict(C1=float("inf")),
    dict(C2=float("inf")), dict(C2=-float("inf")),
    dict(ws_bytes=0), dict(ws_bytes=ONE_SHORT),
    dict(ws=FAKE + 4),
])
def test_ssim3d_refuses_bad_arguments(over):
    rc, msg = _ssim(**over)
    assert rc == _hip.E_INVAL and msg.startswith("ssim3d:"), (rc, msg)


def test_workspace_sizes():
    lib = _hip.load()
    em, ss = lib.ddpm3d_error_moments_workspace_bytes, lib.ddpm3d_ssim3d_workspace_bytes
    for bad in ((0, 100), (65, 100), (-1, 100), (1, 0), (1, -5), (1, (1 << 40) + 1)):
        assert em(*bad) == 0, bad
    for bad in ((0, 20, 20, 20), (65, 20, 20, 20), (1, 10, 20, 20), (1, 20, 10, 20), (1, 20, 20, 10),
                (1, 0, 20, 20), (1, 20, -1, 20), (1, 65536, 20, 20), (1, 20, 65535, 65535)):
        assert ss(*bad) == 0, bad
    sizes = [1, 3, 4, 1000, 1 << 16, 130 * 200 * 200, 700 * 440 * 440, 17 * 128 * 1024 * 1024]
    for B in (1, 2, 8, 64):
        got = [em(B, v) for v in sizes]
        assert got[0] > 0 and all(b >= a for a, b in zip(got, got[1:])), got
        assert all(em(B, v) >= em(B - 1, v) for v in sizes if B > 1)
        assert em(B, sizes[-1]) == B * em(1, sizes[-1]) <= 64 << 20
    extents = [11, 12, 26, 27, 37, 48, 64, 130, 200, 440, 700, 1024]
    for B in (1, 3, 64):
        for axis in range(3):
            for fixed in (11, 64, 200):
                got = [ss(B, *[(e if a == axis else fixed) for a in range(3)]) for e in extents]
                assert got[0] > 0 and all(b >= a for a, b in zip(got, got[1:])), (B, axis, fixed, got)
        assert ss(B, 700, 440, 440) == B * ss(1, 700, 440, 440) <= 64 << 20
    assert ss(2, 48, 64, 64) > ss(1, 48, 64, 64)


def test_store_hazard_scan_is_green_with_the_metric_kernels():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_store_hazard.py")], capture_output=True,
                       text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    nm = subprocess.run(["nm", "-D", "--defined-only", _hip.LIB_PATH], capture_output=True, text=True)
    if nm.returncode == 0:
        assert all(e in nm.stdout for e in ENTRIES)


# ------------------------------------------------------------------------------------------ the script
def _script():
    spec = importlib.util.spec_from_file_location("ddpm3d_infer_entry", os.path.join(PKG, "scripts", "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _no_device(mod, monkeypatch):
    def no_device(*a, **kw):
        raise AssertionError("the script went past its argument checks")

    monkeypatch.setattr(mod, "sr_create_model_and_diffusion", no_device)
    monkeypatch.setattr(mod.dist_util, "setup_dist", no_device)
    monkeypatch.setattr(mod._hip, "load", no_device)


def test_script_defaults_run_no_metrics():
    args = _script().create_argparser().parse_args([])
    assert args.target_samples == "" and args.data_range == 0 and args.metrics_mask_threshold == 0
    mod = _script()
    assert mod._load_target(None, args) == (None, None)
    assert mod._write_metrics(args, "unused", None, None, None) is None


@pytest.mark.parametrize("case", ["missing", "shape", "thin", "threshold"])
def test_script_refuses_a_bad_target_before_any_device_call(case, tmp_path, monkeypatch, capsys):
    mod = _script()
    _no_device(mod, monkeypatch)
    shape = (12, 16, 10) if case == "thin" else (12, 16, 16)
    np.savez(tmp_path / "low.npz", np.zeros(shape, dtype=np.float32))
    np.savez(tmp_path / "full.npz", np.zeros((12, 16, 20) if case == "shape" else shape, dtype=np.float32))
    target = tmp_path / ("none.npz" if case == "missing" else "full.npz")
    extra = ["--metrics_mask_threshold", "1.5"] if case == "threshold" else []
    with pytest.raises(SystemExit) as e:
        mod.main(["--base_samples", str(tmp_path / "low.npz"), "--target_samples", str(target), "--save_dir",
                  str(tmp_path)] + extra)
    assert e.value.code == 2
    assert ("--metrics_mask_threshold" if case == "threshold" else "--target_samples") in capsys.readouterr().err
