"""
CPU tier of the baseline denoisers: metrics.gaussian_taps against hand values and its refusals, the
fp64 yardstick of tests/baseline_ref.py against scipy and against cases worked by hand, the three C entries declared,
exported and bound within ABI 13, every host refusal of the two entries (no HIP call is made: the pointers are fake),
the Python entries' refusals before the library is touched, and the inference script's refusals of bad baseline
flags before any device call.  No GPU is touched here.
"""

import ctypes
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch
from scipy import ndimage

import baseline_ref as B
from conftest import PKG, ROOT
from guided_diffusion import _hip, metrics

FAKE = 1 << 20          # a non-null "device pointer" no call below may ever dereference: each fails validation first


# ------------------------------------------------------------------------------------------ the taps
def test_taps_against_hand_values():
    t = metrics.gaussian_taps(4.0, (2.0, 2.0, 2.0))
    assert t.radii == (3, 3, 3) and t.fwhm_mm == (4.0, 4.0, 4.0) and t.spacing == (2.0, 2.0, 2.0)
    assert all(abs(s - 0.8493) < 5e-5 for s in t.sigma_voxels)
    assert t.sigma_voxels[0] == pytest.approx(4.0 / (2.0 * math.sqrt(2.0 * math.log(2.0))) / 2.0, rel=1e-14)
    want = [np.float32(math.exp(-0.5 * j * j / t.sigma_voxels[0] ** 2)) for j in range(-3, 4)]
    assert list(t.taps[2]) == [float(v) for v in want] and t.taps[0][3] == 1.0
    assert [list(table) for table in t.tables] == [list(row) for row in t.taps]
    assert metrics.gaussian_taps(8.0, (2.0, 2.0, 2.0)).radii == (5, 5, 5)
    # anisotropic, per axis: scipy's radius rule int(truncate * sigma + 0.5)
    a = metrics.gaussian_taps((4.0, 8.0, 6.0), (3.27, 2.0, 1.5))
    sig = [f / 2.3548200450309493 / s for f, s in zip((4.0, 8.0, 6.0), (3.27, 2.0, 1.5))]
    assert a.sigma_voxels == pytest.approx(sig, rel=1e-14) and a.radii == tuple(int(3.0 * s + 0.5) for s in sig)
    assert a.radii == (2, 5, 5)
    assert metrics.gaussian_taps(4.0, (2.0, 2.0, 2.0), truncate=4.0).radii == (3, 3, 3)
    assert metrics.gaussian_taps(4.0, (2.0, 2.0, 2.0), truncate=4.2).radii == (4, 4, 4)
    assert metrics.gaussian_taps(1.0, (4.0, 4.0, 4.0)).radii == (0, 0, 0)
    assert B.taps_of(a.sigma_voxels[1], 5).tolist() == list(a.taps[1])


def test_taps_refuse_a_radius_above_the_limit_and_name_the_axis():
    with pytest.raises(ValueError, match=r"along axis 2.*DDPM3D_SMOOTH_MAX_RADIUS = 16"):
        metrics.gaussian_taps(8.0, (2.0, 2.0, 0.2))
    with pytest.raises(ValueError, match="along axis 0"):
        metrics.gaussian_taps((30.0, 4.0, 4.0), (2.0, 2.0, 2.0))
    assert metrics.gaussian_taps(25.0, (2.0, 2.0, 2.0)).radii == (16, 16, 16)
    assert metrics.gaussian_taps(26.0, (4.0, 4.0, 4.0)).radii == (8, 8, 8)
    with pytest.raises(ValueError, match="DDPM3D_SMOOTH_MAX_RADIUS"):
        metrics.gaussian_taps(26.0, (2.0, 2.0, 2.0))


@pytest.mark.parametrize("fwhm,spacing,truncate", [
    (0.0, (2, 2, 2), 3.0), (-4.0, (2, 2, 2), 3.0), (math.nan, (2, 2, 2), 3.0), (math.inf, (2, 2, 2), 3.0),
    ("4", (2, 2, 2), 3.0), (None, (2, 2, 2), 3.0), (True, (2, 2, 2), 3.0), ((4.0, 4.0), (2, 2, 2), 3.0),
    ((4.0, 0.0, 4.0), (2, 2, 2), 3.0), (4.0, (2, 2), 3.0), (4.0, (2, 0, 2), 3.0), (4.0, 2.0, 3.0),
    (4.0, (2, 2, 2), 0.0), (4.0, (2, 2, 2), math.nan),
], ids=str)
def test_taps_refuse_bad_arguments(fwhm, spacing, truncate):
    with pytest.raises(ValueError, match="gaussian_taps:"):
        metrics.gaussian_taps(fwhm, spacing, truncate)


# ------------------------------------------------------------------------------------------ the yardstick
def test_gaussian_yardstick_equals_scipy_in_the_interior():
    x = B.data((14, 25, 40), 3, offset=2.0)
    sigma, radii = (0.9, 1.7, 2.6), (3, 5, 8)                 # scipy's radii at truncate 3: int(3 sigma + 0.5)
    assert radii == tuple(int(3.0 * s + 0.5) for s in sigma)
    taps = [np.exp(-0.5 * np.arange(-r, r + 1, dtype=np.float64) ** 2 / (s * s)) for s, r in zip(sigma, radii)]
    m, bound = B.gaussian(x, taps)
    want = ndimage.gaussian_filter(x.astype(np.float64), sigma, truncate=3.0, mode="constant")
    inner = tuple(slice(r, n - r) for r, n in zip(radii, x.shape))
    assert m[inner].size > 0 and np.abs(m[inner] - want[inner]).max() <= 1e-12
    assert np.abs(m - want).max() > 1e-3                      # at the faces scipy's zeros count, here nothing does
    assert (bound > 0).all()


def test_gaussian_yardstick_on_a_case_worked_by_hand():
    x = np.array([1.0, 2.0, 4.0, 8.0], dtype=np.float32).reshape(1, 1, 4)
    taps = (np.ones(1, np.float32), np.ones(1, np.float32), np.array([0.5, 1.0, 0.5], np.float32))
    m, bound = B.gaussian(x, taps)
    assert m[0, 0].tolist() == pytest.approx([(1 + 1) / 1.5, (0.5 + 2 + 2) / 2, (1 + 4 + 4) / 2, (2 + 8) / 1.5])
    # c = (2 + 2, 1 + 2, 1 + 2) at the first voxel; M = m for a positive volume
    want = ((1 + 4 * B.U) * (1 + 3 * B.U) ** 2 - 1) * m[0, 0, 0]
    assert bound[0, 0, 0] == pytest.approx(want, rel=1e-9)
    # a swapped axis is another filter: taps along D act along D
    y = np.arange(24, dtype=np.float32).reshape(4, 3, 2)
    along_d = B.gaussian(y, (taps[2], taps[0], taps[1]))[0]
    assert along_d[0, 1, 1] == pytest.approx((y[0, 1, 1] + 0.5 * y[1, 1, 1]) / 1.5)


def test_nlm_yardstick_limits_of_h():
    x = B.data((9, 11, 13), 4, offset=1.0)
    search, patch = (1, 2, 3), (1, 1, 1)
    m, bound, wx, info = B.nlm(x, search, patch, 1e6)
    box = B.box_mean(x, search)
    assert np.abs(m - box).max() < 1e-9 and info["zero"] == 0
    size = tuple(2 * s + 1 for s in search)
    want = ndimage.uniform_filter(x.astype(np.float64), size=size, mode="constant")
    inner = tuple(slice(s, n - s) for s, n in zip(search, x.shape))
    assert np.abs(box[inner] - want[inner]).max() < 1e-12
    # at the faces only the candidates inside count
    assert box[0, 0, 0] == pytest.approx(x[:2, :3, :4].astype(np.float64).mean(), rel=1e-14)
    # an h so small that every other candidate lies beyond the cutoff: the input
    tiny = 1e-3 * B.median_distance(x, search, patch)
    m, bound, wx, info = B.nlm(x, search, patch, tiny)
    assert np.array_equal(m, x.astype(np.float64)) and info["above_half"] == 0 and info["zero"] > 0
    assert np.array_equal(wx, np.abs(x.astype(np.float64)))


def test_nlm_yardstick_on_a_case_worked_by_hand_and_sigma_shifts_d2():
    x = np.array([0.0, 1.0, 3.0], dtype=np.float32).reshape(1, 1, 3)
    for sigma in (0.0, 0.5, 0.7):
        m, bound, wx, _ = B.nlm(x, (0, 0, 1), (0, 0, 0), 1.5, sigma)
        w = lambda d2: math.exp(-max(d2 - 2.0 * sigma * sigma, 0.0) / 2.25)
        assert m[0, 0, 0] == pytest.approx((0.0 + w(1.0) * 1.0) / (1.0 + w(1.0)), rel=1e-14)
        assert m[0, 0, 1] == pytest.approx((w(1.0) * 0.0 + 1.0 + w(4.0) * 3.0) / (w(1.0) + 1.0 + w(4.0)), rel=1e-14)
        assert m[0, 0, 2] == pytest.approx((w(4.0) * 1.0 + 3.0) / (w(4.0) + 1.0), rel=1e-14)
        # c = 2 (80 (1 + 4) + 2) + N_s + 2 with N_s = 2 at the ends and 3 in the middle
        assert bound[0, 0, 0] == pytest.approx((804 + 2 + 2) * B.U * wx[0, 0, 0], rel=1e-12)
        assert bound[0, 0, 1] == pytest.approx((804 + 3 + 2) * B.U * wx[0, 0, 1], rel=1e-12)
    # 2 sigma^2 at or above every d2: all weights 1, the box mean
    m = B.nlm(x, (0, 0, 1), (0, 0, 0), 1.5, math.sqrt(2.0))[0]
    assert m[0, 0].tolist() == pytest.approx([0.5, 4.0 / 3.0, 2.0])
    # a patch reads replicate padding: d2 of voxels 0 and 1 with patch radius 1 is ((0-0)^2 + (0-1)^2 + (1-3)^2) / 3
    d2 = B.patch_distance(B._padded(x, (0, 0, 1), (0, 0, 1))[1], (0, 0, 1), (0, 0, 1))
    assert d2[0, 0].tolist() == pytest.approx([5.0 / 3.0, (1.0 + 4.0 + 0.0) / 3.0, (4.0 + 0.0 + 0.0) / 3.0])
    # the cutoff: an exponent above 80 gives exactly 0, at 80 it still counts
    m, _, _, info = B.nlm(x, (0, 0, 1), (0, 0, 0), math.sqrt(4.0 / 80.0))
    assert info["borderline"] == 2
    m, _, _, info = B.nlm(x, (0, 0, 1), (0, 0, 0), math.sqrt(4.0 / 80.5))
    assert info["zero"] == 2 and m[0, 0, 2] == 3.0


# ------------------------------------------------------------------------------------------ the C entries
NAMES = ("ddpm3d_gauss_smooth_workspace_bytes", "ddpm3d_gauss_smooth", "ddpm3d_nlm")


def test_entries_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ddpm3d.h")).read()
    declared = set(re.findall(r"\b(ddpm3d_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in NAMES:
        assert name in declared and name in _hip.EXPORTS and hasattr(lib, name), name
    assert re.search(r"#define DDPM3D_ABI_VERSION 13\b", hdr) and _hip.load().ddpm3d_abi_version() == 13
    define = lambda name: re.search(r"#define %s (\S+)" % name, hdr).group(1)
    assert int(define("DDPM3D_SMOOTH_MAX_RADIUS")) == _hip.SMOOTH_MAX_RADIUS == 16
    assert int(define("DDPM3D_NLM_MAX_SEARCH")) == _hip.NLM_MAX_SEARCH == 5
    assert int(define("DDPM3D_NLM_MAX_PATCH")) == _hip.NLM_MAX_PATCH == 2
    assert define("DDPM3D_NLM_CUTOFF") == "80.0f" and _hip.NLM_CUTOFF == B.CUTOFF == 80.0
    make = open(os.path.join(PKG, "csrc", "Makefile")).read()
    for name in ("smooth", "nlm"):
        assert re.search(r"^OBJS\s*:=.*\b%s\.o\b" % name, make, re.M)
        assert os.path.isfile(os.path.join(PKG, "csrc", name + ".hip"))
    lib = _hip.load()
    assert lib.ddpm3d_gauss_smooth_workspace_bytes(3, 5, 7) == 432 and 432 >= 3 * 5 * 7 * 4
    for bad in ((0, 5, 7), (3, -1, 7), (1 << 11, 1 << 10, 1 << 10), (46341, 46341, 1)):
        assert lib.ddpm3d_gauss_smooth_workspace_bytes(*bad) == 0


def _floats(values):
    return None if values is None else (ctypes.c_float * len(values))(*values)


def _smooth(**over):
    lib = _hip.load()
    t = metrics.gaussian_taps(4.0, (2.0, 2.0, 2.0))
    a = dict(vol=FAKE, D=20, H=30, W=40, r0=3, r1=3, r2=3, taps0=list(t.taps[0]), taps1=list(t.taps[1]),
             taps2=list(t.taps[2]), out=2 * FAKE, ws=3 * FAKE, ws_bytes=20 * 30 * 40 * 4, stream=None)
    a.update(over)
    for k in ("taps0", "taps1", "taps2"):
        a[k] = _floats(a[k])
    rc = lib.ddpm3d_gauss_smooth(*a.values())
    return rc, lib.ddpm3d_last_error().decode()


def _edited(j, value, mirror=False):
    taps = list(metrics.gaussian_taps(4.0, (2.0, 2.0, 2.0)).taps[0])
    taps[j] = value
    if mirror:
        taps[len(taps) - 1 - j] = value
    return taps


BAD_SMOOTH = {
    "vol_null": dict(vol=None), "out_null": dict(out=None), "taps0_null": dict(taps0=None),
    "taps1_null": dict(taps1=None), "taps2_null": dict(taps2=None), "in_place": dict(out=FAKE),
    "D_0": dict(D=0), "H_0": dict(H=0), "W_negative": dict(W=-40),
    "voxels_2_31": dict(D=1 << 11, H=1 << 10, W=1 << 10), "voxels_just_above": dict(D=46341, H=46341, W=1),
    "r0_negative": dict(r0=-1), "r1_17": dict(r1=17, taps1=[1.0] * 35), "r2_17": dict(r2=17, taps2=[1.0] * 35),
    "tap_zero": dict(taps0=_edited(0, 0.0, True)), "tap_negative": dict(taps1=_edited(1, -0.5, True)),
    "tap_nan": dict(taps2=_edited(3, math.nan)), "tap_inf": dict(taps0=_edited(3, math.inf)),
    "not_symmetric": dict(taps1=_edited(0, 0.5)),
    "ws_null": dict(ws=None), "ws_small": dict(ws_bytes=20 * 30 * 40 * 4 - 1), "ws_misaligned": dict(ws=3 * FAKE + 4),
    "ws_is_vol": dict(ws=FAKE), "ws_is_out": dict(ws=2 * FAKE),
}


@pytest.mark.parametrize("case", sorted(BAD_SMOOTH))
def test_gauss_smooth_refuses_bad_arguments(case):
    rc, msg = _smooth(**BAD_SMOOTH[case])
    assert rc == _hip.E_INVAL and msg.startswith("gauss_smooth:"), (rc, msg)


def _nlm(**over):
    lib = _hip.load()
    a = dict(vol=FAKE, D=20, H=30, W=40, s0=3, s1=3, s2=3, p0=1, p1=1, p2=1, h=1.0, sigma=0.0, out=2 * FAKE,
             stream=None)
    a.update(over)
    rc = lib.ddpm3d_nlm(*a.values())
    return rc, lib.ddpm3d_last_error().decode()


BAD_NLM = {
    "vol_null": dict(vol=None), "out_null": dict(out=None), "in_place": dict(out=FAKE),
    "D_0": dict(D=0), "H_negative": dict(H=-3), "W_0": dict(W=0),
    "voxels_2_31": dict(D=1 << 11, H=1 << 10, W=1 << 10), "voxels_just_above": dict(D=46341, H=46341, W=1),
    "s0_6": dict(s0=6), "s1_negative": dict(s1=-1), "s2_6": dict(s2=6),
    "p0_3": dict(p0=3), "p1_3": dict(p1=3), "p2_negative": dict(p2=-1),
    "h_0": dict(h=0.0), "h_negative": dict(h=-1.0), "h_nan": dict(h=math.nan), "h_inf": dict(h=math.inf),
    "h_tiny": dict(h=1e-30),
    "sigma_negative": dict(sigma=-0.1), "sigma_nan": dict(sigma=math.nan), "sigma_inf": dict(sigma=math.inf),
    "sigma_over_h": dict(h=1e-10, sigma=1e10),
}


@pytest.mark.parametrize("case", sorted(BAD_NLM))
def test_nlm_refuses_bad_arguments(case):
    rc, msg = _nlm(**BAD_NLM[case])
    assert rc == _hip.E_INVAL and msg.startswith("nlm:"), (rc, msg)


def test_refusals_name_what_is_wrong():
    assert "null" in _smooth(vol=None)[1] and "out must not be vol" in _smooth(out=FAKE)[1]
    assert "2^31 - 1" in _smooth(D=46341, H=46341, W=1)[1] and "r1=17" in _smooth(r1=17, taps1=[1.0] * 35)[1]
    assert "taps0[0]" in _smooth(taps0=_edited(0, 0.0, True))[1] and "symmetric" in _smooth(taps1=_edited(0, 0.5))[1]
    assert "workspace" in _smooth(ws_bytes=16)[1]
    assert "s0=6" in _nlm(s0=6)[1] and "p0=3" in _nlm(p0=3)[1] and "h=0" in _nlm(h=0.0)[1]
    assert "sigma=-0.1" in _nlm(sigma=-0.1)[1] and "too small" in _nlm(h=1e-30)[1]


# ------------------------------------------------------------------------------------------ the Python entries
def test_python_refusals_come_before_the_library(monkeypatch):
    def no_device(*a, **kw):
        raise AssertionError("a refusal reached the library")

    monkeypatch.setattr(metrics.H, "load", no_device)
    taps = metrics.gaussian_taps(4.0, (2.0, 2.0, 2.0))
    vol = torch.zeros((4, 5, 6))
    for bad in (vol, vol.numpy(), vol.double()):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            metrics.gaussian_smooth(bad, taps)
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            metrics.nlm(bad, 1.0)
    with pytest.raises(ValueError, match="gaussian_taps' return"):
        metrics.gaussian_smooth(vol, [[1.0], [1.0], [1.0]])
    for h in (0.0, -1.0, math.nan, math.inf, "1", None, True, 1e-30, 1e-60, 1e39):
        with pytest.raises(ValueError, match="nlm: h"):
            metrics.nlm(vol, h)
    for search in (6, -1, (3, 3), (3, 3, 6), 2.0, (1, 1, 1.0), None, True):
        with pytest.raises(ValueError, match="nlm: the search radius"):
            metrics.nlm(vol, 1.0, search=search)
    for patch in (3, -1, (1, 1), (1, 3, 1), 1.0, None):
        with pytest.raises(ValueError, match="nlm: the patch radius"):
            metrics.nlm(vol, 1.0, patch=patch)
    for sigma in (-0.5, math.nan, math.inf, "0", None, 1e39):
        with pytest.raises(ValueError, match="nlm: (h and )?sigma"):
            metrics.nlm(vol, 1.0, sigma=sigma)
    with pytest.raises(ValueError, match="too small"):
        metrics.nlm(vol, 1e-10, sigma=1e10)
    assert metrics.nlm_check(2, 3, 1) == (2.0, (3, 3, 3), (1, 1, 1), 0.0)
    assert metrics.nlm_check(0.1, (1, 2, 3), (0, 1, 2), 0.5) == (float(np.float32(0.1)), (1, 2, 3), (0, 1, 2), 0.5)


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


def _files(tmp_path):
    shape = (12, 16, 24)
    np.savez(tmp_path / "low.npz", np.zeros(shape, dtype=np.float32))
    np.savez(tmp_path / "full.npz", np.ones(shape, dtype=np.float32))
    return ["--base_samples", str(tmp_path / "low.npz"), "--save_dir", str(tmp_path)]


def test_script_default_is_no_baseline():
    mod = _script()
    args = mod.create_argparser().parse_args([])
    assert args.baseline_gaussian_fwhm is None and args.baseline_nlm_h is None
    assert (args.baseline_nlm_search, args.baseline_nlm_patch, args.baseline_nlm_sigma) == (3, 1, 0.0)
    assert mod._check_baselines(None, args) is None


SPACING = ["--voxel_spacing", "2", "2", "2"]
GAUSS, NLM = ["--baseline_gaussian_fwhm", "4"], ["--baseline_nlm_h", "0.5"]
CASES = {
    "gaussian_no_spacing": (GAUSS, "--voxel_spacing"),
    "gaussian_no_target": (GAUSS + SPACING, "--target_samples"),
    "nlm_no_target": (NLM, "--target_samples"),
    "fwhm_zero": (["--baseline_gaussian_fwhm", "0"] + SPACING, "positive finite"),
    "fwhm_negative": (["--baseline_gaussian_fwhm", "-4"] + SPACING, "positive finite"),
    "fwhm_nan": (["--baseline_gaussian_fwhm", "nan"] + SPACING, "positive finite"),
    "fwhm_inf": (["--baseline_gaussian_fwhm", "inf"] + SPACING, "positive finite"),
    "fwhm_not_a_number": (["--baseline_gaussian_fwhm", "four"] + SPACING, "--baseline_gaussian_fwhm"),
    "radius_above_16": (["--baseline_gaussian_fwhm", "30", "--voxel_spacing", "2", "0.5", "2"],
                        "DDPM3D_SMOOTH_MAX_RADIUS"),
    "h_zero": (["--baseline_nlm_h", "0"], "positive finite"),
    "h_negative": (["--baseline_nlm_h", "-1"], "positive finite"),
    "h_nan": (["--baseline_nlm_h", "nan"], "positive finite"),
    "h_inf": (["--baseline_nlm_h", "inf"], "positive finite"),
    "h_tiny": (["--baseline_nlm_h", "1e-30"], "too small"),
    "search_6": (NLM + ["--baseline_nlm_search", "6"], "--baseline_nlm_search must be in 0..5"),
    "search_negative": (NLM + ["--baseline_nlm_search", "-1"], "--baseline_nlm_search must be in 0..5"),
    "patch_3": (NLM + ["--baseline_nlm_patch", "3"], "--baseline_nlm_patch must be in 0..2"),
    "patch_negative": (NLM + ["--baseline_nlm_patch", "-1"], "--baseline_nlm_patch must be in 0..2"),
    "sigma_negative": (NLM + ["--baseline_nlm_sigma", "-0.1"], "sigma"),
    "sigma_nan": (NLM + ["--baseline_nlm_sigma", "nan"], "sigma"),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_script_refuses_bad_baseline_flags_before_any_device_call(case, tmp_path, monkeypatch, capsys):
    mod = _script()
    _no_device(mod, monkeypatch)
    extra, names = CASES[case]
    argv = _files(tmp_path) + extra
    if not case.endswith("no_target"):
        argv += ["--target_samples", str(tmp_path / "full.npz")]
    with pytest.raises(SystemExit) as e:
        mod.main(argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert names in err[err.rindex("error:"):]                # the message itself, not the usage lines above it


@pytest.mark.parametrize("flags", [GAUSS + SPACING, NLM, GAUSS + SPACING + NLM + ["--roi_threshold", "0.5"],
                                   NLM + ["--baseline_nlm_search", "5", "--baseline_nlm_patch", "2",
                                          "--baseline_nlm_sigma", "0.1", "--num_draws", "2"]],
                         ids=["gaussian", "nlm", "both-threshold", "nlm-largest-draws"])
def test_script_accepts_good_baseline_flags_before_it_builds_the_model(flags, tmp_path, monkeypatch):
    """the same set-up with nothing wrong reaches the first device call: the refusals above are the checks' own"""
    mod = _script()
    _no_device(mod, monkeypatch)
    with pytest.raises(AssertionError, match="went past its argument checks"):
        mod.main(_files(tmp_path) + ["--target_samples", str(tmp_path / "full.npz")] + flags)


def test_script_permutes_the_taps_with_the_volumes():
    mod = _script()
    parser = mod.create_argparser()
    args = parser.parse_args(["--voxel_spacing", "3.27", "2.0", "1.5", "--target_samples", "t.npz",
                              "--baseline_gaussian_fwhm", "6", "--baseline_nlm_h", "0.25", "--baseline_nlm_search", "2"])
    assert mod._check_spacing(parser, args) is None           # no regions: the spacing serves the Gaussian alone
    base = mod._check_baselines(parser, args)
    assert base["gaussian"].spacing == (2.0, 1.5, 3.27)       # (D, H, W) of the file -> (H, W, Z) of the volumes
    assert base["gaussian"].radii == metrics.gaussian_taps(6.0, (2.0, 1.5, 3.27)).radii == (4, 5, 2)
    assert base["nlm"] == {"h": 0.25, "search": (2, 2, 2), "patch": (1, 1, 1), "sigma": 0.0}
