"""
CPU tier of the multi-scale SSIM: the two yardsticks of tests/msssim_ref.py are checked against each
other so that neither is its own judge, the cases are what the GPU tier assumes (the plain fp32 evaluation within
its sanity cap, counted interior voxels at every scale, means away from 0), the weights helper, the three C entries
declared, exported and bound within ABI 13, their refusals on the host before any HIP call, the workspace query, the
script's refusals before a model is built, and evaluate's unchanged default.  No GPU is touched here.
"""

import ctypes
import importlib.util
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import metrics_ref as R
import msssim_ref as MS
from conftest import PKG, ROOT
from guided_diffusion import _hip, metrics

FAKE = 1 << 20          # a non-null "device pointer" no call below may ever dereference: each fails validation first
ENTRIES = ("ddpm3d_pool2", "ddpm3d_msssim3d", "ddpm3d_msssim3d_workspace_bytes")
ONE_SHORT = "one byte less than the entry's own answer"
CASE_IDS = MS.case_ids()


# ------------------------------------------------------------------------------------------ the yardsticks
def test_pooling_yardstick_on_a_worked_example():
    x = np.arange(3 * 5 * 7, dtype=np.float32).reshape(3, 5, 7)
    p = MS.pool2(x)
    assert p.shape == (1, 2, 3) and p.dtype == np.float32                  # the odd plane, row and column are dropped
    assert p[0, 1, 2] == x[0:2, 2:4, 4:6].mean()
    assert np.array_equal(MS.pool2(np.stack([x, 2 * x])), np.stack([p, 2 * p]))
    big = np.float32(2.0 ** 24)                                            # the order of the additions is the documented one
    v = np.array([[[big, 1.0], [1.0, 1.0]], [[-big, 1.0], [1.0, 1.0]]], dtype=np.float32)
    want = np.float32(np.float32(np.float32(big + np.float32(1)) + np.float32(2))
                      + np.float32(np.float32(-big + np.float32(1)) + np.float32(2))) * np.float32(0.125)
    assert MS.pool2(v)[0, 0, 0] == want and want != np.float32(v.astype(np.float64).mean())
    m = np.zeros((2, 2, 4), dtype=np.uint8)
    m[0, :, 0:2] = 1                                                       # 4 of 8
    m[0, 0, 2:4], m[1, 0, 2] = 7, 1                                        # 3 of 8
    assert MS.pool2_mask(m).tolist() == [[[1, 0]]]


@pytest.mark.parametrize("ik", CASE_IDS, ids=MS.case_name)
def test_the_two_yardsticks_agree(ik):
    """on the final value within 1e-6 (fp32 against fp64 pooling is the only difference), and per scale within 1e-12
    when both evaluate the same pooled inputs"""
    c = MS.case(*ik)
    for masked in (False, True):
        mask = c["mask"] if masked else None
        other, other_terms = MS.msssim_torch(c["x"], c["y"], 1.0, c["scales"], mask)
        print("%s masked=%s: %.9f against %.9f" % (c["name"], masked, c["value"][masked], other))
        assert abs(c["value"][masked] - other) <= 1e-6
        assert len(other_terms) == len(c["terms"][masked]) == c["scales"]
    for x, y, _ in c["levels"]:
        a, b = MS.maps(x, y, 1.0), MS.maps_conv3d(x, y, 1.0)
        assert a[0].shape == b[0].shape == tuple(n - 10 for n in x.shape) and a[0].dtype == np.float64
        assert max(np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max()) <= 1e-12


@pytest.mark.parametrize("ik", CASE_IDS, ids=MS.case_name)
def test_cases_are_what_the_gpu_tier_assumes(ik):
    c = MS.case(*ik)
    shape, M = c["shape"], c["scales"]
    assert [lv[0].shape for lv in c["levels"]] == [tuple(n >> j for n in shape) for j in range(M)]
    assert min(c["levels"][-1][0].shape) >= 11 and metrics.msssim_max_scales(shape) >= M
    counted = [int(R.interior_mask(lv[2]).sum()) for lv in c["levels"]]
    print("%s: e32 per scale %s, counted interior voxels %s, terms %s / %s masked"
          % (c["name"], ["%.3g" % e for e in c["e32"]], counted, c["terms"][False], c["terms"][True]))
    assert all(0 < e <= 1e-4 for e in c["e32"])                 # a broken yardstick cannot widen the bound
    assert all(n >= 1 for n in counted)
    for masked in (False, True):
        assert all(0.15 < t < 1 for t in c["terms"][masked]) and 0.15 < c["value"][masked] < 1


def test_one_scale_is_the_ssim_yardstick():
    for i, k in CASE_IDS[:2] + CASE_IDS[-2:]:
        c = MS.case(i, k)
        for mask in (None, c["mask"]):
            value, terms = MS.msssim(c["x"], c["y"], 1.0, 1, mask)
            assert value == terms[0] == R.ssim(c["x"], c["y"], 1.0, mask)


def test_clamp_case_is_negative_at_both_scales():
    y = np.random.default_rng(5).random((24, 24, 24), dtype=np.float32)
    value, terms = MS.msssim(np.float32(1) - y, y, 1.0, 2)
    assert terms[0] < 0 and terms[1] < 0 and value == 0.0


# ------------------------------------------------------------------------------------------ the weights
def test_weights_helper():
    assert metrics.MSSSIM_WEIGHTS == (0.0448, 0.2856, 0.3001, 0.2363, 0.1333) == MS.WEIGHTS
    assert metrics.msssim_weights(1) == (1.0,)
    for M in range(1, 6):
        w = metrics.msssim_weights(M)
        assert len(w) == M and abs(math.fsum(w) - 1.0) <= 1e-15 and list(w) == MS.weights(M)
        assert all(abs(a / w[0] - b / 0.0448) <= 1e-12 for a, b in zip(w, metrics.MSSSIM_WEIGHTS))
    assert max(abs(a - b) for a, b in zip(metrics.msssim_weights(5), metrics.MSSSIM_WEIGHTS)) <= 1e-4   # they sum to 1.0001
    for bad in (0, 6, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="scales"):
            metrics.msssim_weights(bad)
    assert [metrics.msssim_max_scales(s) for s in ((96, 96, 96), (130, 200, 200), (700, 440, 440), (22, 22, 22),
                                                   (21, 40, 40), (10, 40, 40))] == [4, 4, 5, 2, 1, 0]


# ------------------------------------------------------------------------------------------ the C entries
def test_entries_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ddpm3d.h")).read()
    declared = set(re.findall(r"\b(ddpm3d_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in ENTRIES:
        assert name in declared and name in _hip.EXPORTS and hasattr(lib, name), name
    assert re.search(r"#define DDPM3D_ABI_VERSION 13\b", hdr) and _hip.ABI_VERSION == 13
    assert _hip.load().ddpm3d_abi_version() == 13
    assert re.search(r"#define DDPM3D_MSSSIM_MAX_SCALES 5\b", hdr) and _hip.MSSSIM_MAX_SCALES == 5 == MS.MAX_SCALES
    assert "msssim.o" in open(os.path.join(PKG, "csrc", "Makefile")).read()


def _pool(**over):
    lib = _hip.load()
    a = dict(vol=FAKE, mask=None, B=2, D=20, H=30, W=40, out=FAKE, mask_out=None, stream=None)
    a.update(over)
    rc = lib.ddpm3d_pool2(*a.values())
    return rc, lib.ddpm3d_last_error().decode()


def _ms(**over):
    lib = _hip.load()
    a = dict(est=FAKE, target=FAKE, mask=None, B=2, D=44, H=50, W=60, scales=3, C1=1e-4, C2=9e-4, ws=FAKE,
             ws_bytes=1 << 30, out=FAKE, stream=None)
    a.update(over)
    if a["ws_bytes"] == ONE_SHORT:
        a["ws_bytes"] = lib.ddpm3d_msssim3d_workspace_bytes(a["B"], a["D"], a["H"], a["W"], a["scales"]) - 1
        assert a["ws_bytes"] > 0
    rc = lib.ddpm3d_msssim3d(*a.values())
    return rc, lib.ddpm3d_last_error().decode()


@pytest.mark.parametrize("over", [
    dict(vol=None), dict(out=None), dict(mask=FAKE), dict(mask_out=FAKE),
    dict(B=0), dict(B=-1), dict(B=65),
    dict(D=1), dict(H=1), dict(W=1), dict(D=0), dict(W=-4), dict(D=65536), dict(H=65536), dict(W=1 << 30),
    dict(H=65535, W=65535), dict(D=65535, H=30000, W=30000),
])
def test_pool2_refuses_bad_arguments(over):
    rc, msg = _pool(**over)
    assert rc == _hip.E_INVAL and msg.startswith("pool2:"), (rc, msg)


@pytest.mark.parametrize("over", [
    dict(est=None), dict(target=None), dict(out=None), dict(ws=None),
    dict(B=0), dict(B=-1), dict(B=65),
    dict(scales=0), dict(scales=-1), dict(scales=6),
    dict(D=43), dict(H=43), dict(W=43), dict(scales=4), dict(D=10, scales=1), dict(D=21, scales=2),
    dict(D=0), dict(H=-30), dict(D=65536), dict(H=65536), dict(W=1 << 30), dict(H=65535, W=65535),
    dict(D=65535, H=30000, W=30000),
    dict(C1=-1e-9), dict(C2=-1.0), dict(C1=float("nan")), dict(C2=float("nan")), dict(C1=float("inf")),
    dict(C2=float("inf")), dict(C2=-float("inf")),
    dict(ws_bytes=0), dict(ws_bytes=ONE_SHORT),
    dict(ws=FAKE + 8),
])
def test_msssim3d_refuses_bad_arguments(over):
    rc, msg = _ms(**over)
    assert rc == _hip.E_INVAL and msg.startswith("msssim3d:"), (rc, msg)


def test_workspace_query():
    ms = _hip.load().ddpm3d_msssim3d_workspace_bytes
    ss = _hip.load().ddpm3d_ssim3d_workspace_bytes
    for bad in ((0, 44, 44, 44, 3), (65, 44, 44, 44, 3), (1, 44, 44, 44, 0), (1, 44, 44, 44, 6), (1, 43, 44, 44, 3),
                (1, 44, 43, 44, 3), (1, 44, 44, 43, 3), (1, 10, 44, 44, 1), (1, 175, 200, 200, 5),
                (1, 65536, 44, 44, 1), (1, 44, 65535, 65535, 1), (1, -1, 44, 44, 1)):
        assert ms(*bad) == 0, bad
    extents = [176, 177, 178, 191, 192, 200, 201, 256, 257, 440, 441, 700, 1024]
    for M in range(1, 6):
        for B in (1, 3, 64):
            for axis in range(3):
                for fixed in (176, 200):
                    got = [ms(B, *[(e if a == axis else fixed) for a in range(3)], M) for e in extents]
                    assert got[0] > 0 and all(b >= a for a, b in zip(got, got[1:])), (M, B, axis, fixed, got)
            assert ms(B, 176, 200, 200, M) >= ms(max(B - 1, 1), 176, 200, 200, M)
        if M > 1:
            assert ms(1, 700, 440, 440, M) > ms(1, 700, 440, 440, M - 1)
    # room for the pooled estimates, target and mask of every scale, and for records no fewer than the SSIM's own
    D, H, W, B = 130, 200, 200, 2
    pooled = sum((B + 1) * 4 * (D >> j) * (H >> j) * (W >> j) + (D >> j) * (H >> j) * (W >> j) for j in range(1, 4))
    assert ms(B, D, H, W, 4) >= pooled + ss(B, D, H, W)
    assert ms(B, D, H, W, 4) <= pooled + 2 * ss(B, D, H, W) + 16 * 16


def test_the_march_is_shared_not_copied():
    """one body for both kernels: neither translation unit carries the filter loops itself"""
    for name in ("metrics.hip", "msssim.hip"):
        src = open(os.path.join(PKG, "csrc", name)).read()
        assert '#include "ssim3d_body.h"' in src and "ssim3d_march<" in src and "rowf[" not in src, name
    body = open(os.path.join(PKG, "csrc", "ssim3d_body.h")).read()
    assert body.count("rowf[f][row][col] = s[f]") == 1


# ------------------------------------------------------------------------------------------ Python and the script
def test_host_tensors_and_bad_arguments_are_refused_before_any_device_call():
    x = torch.zeros(24, 24, 24)
    for call in (lambda: metrics.msssim3d(x, x, 1.0, 2), lambda: metrics.pool2(x),
                 lambda: metrics.evaluate(x, x, msssim_scales=2)):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            call()
    for bad in (-1, 1.5, True, "2"):
        with pytest.raises(ValueError, match="msssim_scales"):
            metrics.evaluate(x, x, msssim_scales=bad)


def test_evaluate_keeps_its_default():
    sig = inspect.signature(metrics.evaluate)
    assert list(sig.parameters) == ["estimate", "target", "data_range", "mask", "std", "msssim_scales"]
    assert sig.parameters["msssim_scales"].default == 0
    calls = []

    def fake_moments(estimate, target, mask=None, std=None):
        return {"n": 8, "mse": 0.25, "mae": 0.5, "bias": 0.5, "target_sq_mean": 1.0, "target_mean": 1.0,
                "target_min": 0.0, "target_max": 2.0}

    saved = metrics.error_moments, metrics.ssim3d, metrics.msssim3d
    metrics.error_moments = fake_moments
    metrics.ssim3d = lambda *a, **kw: 0.5
    metrics.msssim3d = lambda e, t, L, scales, mask=None: calls.append((L, scales)) or 0.75
    try:
        plain = metrics.evaluate(None, None)
        more = metrics.evaluate(None, None, msssim_scales=3)
    finally:
        metrics.error_moments, metrics.ssim3d, metrics.msssim3d = saved
    assert list(plain) == ["psnr", "nrmse", "mae", "bias", "ssim", "data_range", "n_voxels"]
    assert list(more) == list(plain) + ["msssim"] and more["msssim"] == 0.75 and calls == [(2.0, 3)]
    assert {k: more[k] for k in plain} == plain


def _script():
    spec = importlib.util.spec_from_file_location("ddpm3d_infer_entry", os.path.join(PKG, "scripts", "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_script_default_is_no_msssim():
    mod = _script()
    args = mod.create_argparser().parse_args([])
    assert args.msssim_scales == 0 and mod._load_target(None, args) == (None, None)


@pytest.mark.parametrize("case", ["range-high", "range-low", "no-target", "small"])
def test_script_refuses_bad_msssim_scales_before_any_device_call(case, tmp_path, monkeypatch, capsys):
    mod = _script()

    def no_device(*a, **kw):
        raise AssertionError("the script went past its argument checks")

    monkeypatch.setattr(mod, "sr_create_model_and_diffusion", no_device)
    monkeypatch.setattr(mod.dist_util, "setup_dist", no_device)
    monkeypatch.setattr(mod._hip, "load", no_device)
    np.savez(tmp_path / "low.npz", np.zeros((21, 24, 24), dtype=np.float32))      # (21, 24, 24) allows one scale
    np.savez(tmp_path / "full.npz", np.zeros((21, 24, 24), dtype=np.float32))
    argv = ["--base_samples", str(tmp_path / "low.npz"), "--save_dir", str(tmp_path)]
    if case != "no-target":
        argv += ["--target_samples", str(tmp_path / "full.npz")]
    argv += ["--msssim_scales", {"range-high": "6", "range-low": "-1"}.get(case, "2")]
    with pytest.raises(SystemExit) as e:
        mod.main(argv)
    err = capsys.readouterr().err
    assert e.value.code == 2 and "--msssim_scales" in err
    if case == "no-target":
        assert "--target_samples" in err
    if case == "small":
        assert "at most 1" in err
