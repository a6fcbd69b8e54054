"""
CPU tier of the per-region texture figures: the numpy restatement of tests/texture_ref.py against
cases with a known answer (a constant box, an alternating line, two regions sharing a face, a 2 x 2 matrix worked by
hand, the binning's edges, and the phantom of the feature's motivation: smoothing lowers contrast and entropy and
raises the inverse difference moment), texture_figures against the restatement's figures on host matrices, the host
refusals of roi_texture, roi_report and the inference script before any device call, and the C entry declared, exported
and bound within ABI 13.  No GPU is touched here.
"""

import ctypes
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch

import texture_ref as T
from conftest import PKG, ROOT
from guided_diffusion import _hip, metrics


# ------------------------------------------------------------------------------------------ the restatement
def test_the_directions_are_half_the_26_neighbourhood():
    assert len(T.DIRECTIONS) == 13 and T.DIRECTIONS[0] == (0, 0, 1) and T.DIRECTIONS[-1] == (1, 1, 1)
    both = set(T.DIRECTIONS) | {tuple(-v for v in d) for d in T.DIRECTIONS}
    assert len(both) == 26 and (0, 0, 0) not in both


def test_a_constant_box_puts_everything_in_one_cell():
    D, H, W = 5, 6, 7
    vol = np.full((D, H, W), 0.52, dtype=np.float32)
    glcm, hist, counts = T.region_texture(vol, np.ones(vol.shape, bool), 0.0, 1 / 0.05, 64)
    want = 2 * sum((D - abs(dz)) * (H - abs(dy)) * (W - abs(dx)) for dz, dy, dx in T.DIRECTIONS)
    assert want == 3742
    assert glcm[10, 10] == want and glcm.sum() == want and hist[10] == 210 and hist.sum() == 210
    assert counts.tolist() == [210, 0, 0, want // 2]
    f, _ = T.figures(glcm, hist, counts, 0.0, 20.0)
    assert f["joint_entropy"] == 0 and f["angular_second_moment"] == 1 and f["contrast"] == 0
    assert f["inverse_difference_moment"] == 1 and f["joint_average"] == 10 and f["joint_variance"] == 0
    assert f["correlation"] is None and f["hist_uniformity"] == 1 and f["clamped"] == 0
    assert f["p10"] == f["p50"] == f["p90"] == pytest.approx(0.525)


def test_an_alternating_line_has_only_off_diagonal_pairs():
    n = 9
    vol = (np.arange(n) % 2).astype(np.float32).reshape(1, 1, n)
    glcm, hist, counts = T.region_texture(vol, np.ones(vol.shape, bool), 0.0, 1.0, 2)
    assert glcm.tolist() == [[0, n - 1], [n - 1, 0]] and glcm[0, 1] + glcm[1, 0] == 2 * (n - 1)
    assert hist.tolist() == [5, 4] and counts.tolist() == [n, 0, 0, n - 1]
    line = vol.reshape(n, 1, 1)                                   # along depth: the same matrix
    assert np.array_equal(T.region_texture(line, np.ones(line.shape, bool), 0.0, 1.0, 2)[0], glcm)


def test_two_regions_sharing_a_face_contribute_no_cross_pairs():
    vol = np.random.default_rng(1).random((5, 6, 7)).astype(np.float32)
    labels = np.ones(vol.shape, dtype=np.int32)
    labels[:, :, 4:] = 2
    glcm, hist, counts = T.roi_texture(vol, labels, 0.0, 8.0, 8)
    for r, cut in enumerate((vol[:, :, :4], vol[:, :, 4:])):
        alone = T.region_texture(cut, np.ones(cut.shape, bool), 0.0, 8.0, 8)
        assert np.array_equal(glcm[0, r], alone[0]) and np.array_equal(hist[0, r], alone[1])
        assert np.array_equal(counts[0, r], alone[2])
    whole = T.region_texture(vol, np.ones(vol.shape, bool), 0.0, 8.0, 8)
    assert counts[0, :, T.PAIRS].sum() < whole[2][T.PAIRS]        # the pairs across the face are gone
    assert np.array_equal(glcm[0], glcm[0].transpose(0, 2, 1)) and (glcm[0].sum(axis=(1, 2)) == 2 * counts[0, :, 3]).all()


def test_binning_clamps_counts_its_edges_and_drops_nan():
    x = np.array([-np.inf, -0.01, -0.0, 0.0, 0.049, 0.05, 3.15, 3.2, 1e30, np.inf, np.nan], dtype=np.float32)
    g, counted, below, above = T.grey_levels(x, 0.0, 1 / 0.05, 64)
    assert counted.tolist() == [True] * 10 + [False]
    assert g[:10].tolist() == [0, 0, 0, 0, 0, 1, 63, 63, 63, 63]
    assert below.tolist() == [True, True] + [False] * 9 and above.tolist() == [False] * 7 + [True] * 3 + [False]
    vol = x.reshape(1, 1, -1)
    glcm, hist, counts = T.region_texture(vol, np.ones(vol.shape, bool), 0.0, 1 / 0.05, 64)
    assert counts.tolist() == [10, 2, 3, 9] and hist.sum() == 10           # the NaN voxel pairs with nobody
    flat = T.region_texture(vol, np.ones(vol.shape, bool), 0.0, 0.0, 64)   # a flat region's inv_w = 0: inf * 0 is NaN
    assert flat[2].tolist() == [8, 0, 0, 7] and flat[1][0] == 8


def test_the_figures_of_a_2_x_2_matrix_worked_by_hand():
    glcm = np.array([[4, 2], [2, 8]], dtype=np.int64)              # p = [[1/4, 1/8], [1/8, 1/2]]
    hist = np.array([3, 5], dtype=np.int64)
    counts = np.array([8, 1, 0, 8], dtype=np.int64)
    f, mag = T.figures(glcm, hist, counts, 1.0, 2.0)
    assert f["joint_entropy"] == pytest.approx(0.25 * 2 + 2 * 0.125 * 3 + 0.5 * 1, rel=1e-15)       # 1.75 bits
    assert f["angular_second_moment"] == pytest.approx(1 / 16 + 2 / 64 + 1 / 4, rel=1e-15)
    assert f["contrast"] == f["dissimilarity"] == 0.25
    assert f["inverse_difference"] == f["inverse_difference_moment"] == pytest.approx(0.75 + 0.25 / 2, rel=1e-15)
    assert f["joint_average"] == 0.625                              # 1/8 + 1/2
    assert f["joint_variance"] == pytest.approx(0.375 * 0.625 ** 2 + 0.625 * 0.375 ** 2, rel=1e-15)
    assert f["correlation"] == pytest.approx((0.5 - 0.625 ** 2) / (0.625 * 0.375), rel=1e-14)
    assert f["hist_entropy"] == pytest.approx(-(0.375 * math.log2(0.375) + 0.625 * math.log2(0.625)), rel=1e-15)
    assert f["hist_uniformity"] == pytest.approx(0.375 ** 2 + 0.625 ** 2, rel=1e-15)
    assert (f["p10"], f["p50"], f["p90"]) == (1.25, 1.75, 1.75)     # the cumulative counts 3, 8 against 0.8, 4, 7.2
    assert f["clamped"] == 0.125 and f["n"] == 8 and f["pairs"] == 8
    assert mag["contrast"] == 0.25 and mag["joint_entropy"] == pytest.approx(1.75)
    none, _ = T.figures(np.zeros((2, 2), np.int64), np.array([1, 0]), np.array([1, 0, 0, 0]), 0.0, 1.0)
    assert none["n"] == 1 and none["pairs"] == 0 and all(none[k] is None for k in T.FIGURES)


def test_smoothing_the_phantom_moves_the_texture_figures():
    """the table of the feature's motivation: noise raises contrast and entropy by an order of magnitude, a Gaussian
    filter of sigma 1 brings them back near the clean volume's"""
    from scipy import ndimage
    clean, noisy, labels = T.phantom()
    smooth = ndimage.gaussian_filter(noisy, 1.0).astype(np.float32)
    fig = {}
    for name, vol in (("clean", clean), ("noisy", noisy), ("smooth", smooth)):
        glcm, hist, counts = T.roi_texture(vol, labels, 0.0, 1 / 0.05, 64)
        fig[name] = T.figures(glcm[0, 0], hist[0, 0], counts[0, 0], 0.0, np.float32(1 / 0.05))[0]
        print(name, {k: round(fig[name][k], 3) for k in ("contrast", "joint_entropy", "inverse_difference_moment")})
        assert fig[name]["n"] == 12 * 20 * 20 and fig[name]["clamped"] == 0
    assert fig["smooth"]["contrast"] < 0.2 * fig["noisy"]["contrast"]
    assert fig["smooth"]["joint_entropy"] < fig["noisy"]["joint_entropy"] - 1
    assert fig["smooth"]["inverse_difference_moment"] > 2 * fig["noisy"]["inverse_difference_moment"]
    assert fig["clean"]["contrast"] < fig["smooth"]["contrast"] < fig["noisy"]["contrast"]


# ------------------------------------------------------------------------------------------ the host figures
def test_texture_figures_match_the_restatement_on_host_matrices():
    clean, noisy, labels = T.phantom()
    labels[0:3, 0:4, 0:4] = 2
    labels[23, 39, 39] = 3                                         # one voxel: no pair, every figure None
    stack = np.stack([clean, noisy])
    for levels, inv_w in ((64, 20.0), (8, 2.5), (2, 1.0)):
        lo = np.full((2, 3), 0.25, dtype=np.float32)
        iw = np.full((2, 3), inv_w, dtype=np.float32)
        glcm, hist, counts = T.roi_texture(stack, labels, lo, iw, levels)
        got = metrics.texture_figures(metrics.RoiTexture(glcm, hist, counts, lo, iw, levels, [1, 2, 3], True))
        assert len(got) == 2 and len(got[0]) == 3
        single = metrics.texture_figures(metrics.RoiTexture(glcm[1:], hist[1:], counts[1:], lo[1:], iw[1:], levels,
                                                            [1, 2, 3], False))
        assert single == got[1]
        for b in range(2):
            for r in range(3):
                want, mag = T.figures(glcm[b, r], hist[b, r], counts[b, r], lo[b, r], iw[b, r])
                assert set(got[b][r]) == set(want) == {"n", "pairs"} | set(metrics.TEXTURE_FIGURES)
                for k, w in want.items():
                    g = got[b][r][k]
                    if w is None or isinstance(w, int):
                        assert g == w, (levels, b, r, k)
                    else:
                        assert abs(g - w) <= (levels ** 2 + 2) * 2.0 ** -53 * mag[k], (levels, b, r, k, g, w)
        assert all(got[b][2][k] is None for b in range(2) for k in metrics.TEXTURE_FIGURES)
        assert levels < 64 or got[1][0]["contrast"] > 10 * got[0][0]["contrast"]


def test_relative_figures_and_spread_over_draws():
    a = {"contrast": 2.0, "correlation": None, "joint_entropy": 3.0, "n": 10}
    t = {"contrast": 4.0, "correlation": 0.5, "joint_entropy": 0.0, "n": 10}
    assert metrics._texture_rel(a, t) == {"contrast": -0.5, "correlation": None, "joint_entropy": None, "n": 0.0}
    draws = [dict(a, contrast=1.0), dict(a, contrast=2.0), dict(a, contrast=None, correlation=0.25)]
    std = metrics._texture_std(draws)
    assert std["contrast"] == pytest.approx(np.std([1.0, 2.0], ddof=1)) and std["correlation"] is None
    assert std["joint_entropy"] == 0.0
    recs = [[10.0, 5.0, 3.0, 0.1, 0.9, 0.0, 0.0, 0.0]]
    fig = metrics.roi_figures(recs, target_records=recs, texture=[a], target_texture=[t], draw_texture=[[d] for d in draws])
    assert fig[0]["texture"] == a and fig[0]["texture_rel"]["contrast"] == -0.5
    assert fig[0]["draw_texture"] == draws and fig[0]["texture_std"] == std
    assert "texture" not in metrics.roi_figures(recs)[0]
    with pytest.raises(ValueError, match="texture"):
        metrics.roi_figures(recs, texture=[a, a])
    with pytest.raises(ValueError, match="draw_texture"):
        metrics.roi_figures(recs, draw_texture=[[a]])


# ------------------------------------------------------------------------------------------ host refusals
class _Index:
    """what roi_texture reads of an index before its first device call"""
    shape, voxels, device, labels = (5, 6, 7), 210, torch.device("cpu"), [1]

    def __len__(self):
        return 1


@pytest.mark.parametrize("kw", [dict(levels=1), dict(levels=65), dict(levels=8.0), dict(levels=True),
                                dict(bin_width=0.0), dict(bin_width=-1.0), dict(bin_width=float("inf")),
                                dict(bin_width=float("nan")), dict(bin_width="1"), dict(bin_width=1e-39),
                                dict(lower=float("nan")), dict(lower=float("inf")), dict(lower=None)])
def test_roi_texture_refuses_bad_parameters_on_the_host(kw, monkeypatch):
    monkeypatch.setattr(_hip, "load", lambda: pytest.fail("a device call was made"))
    with pytest.raises(ValueError, match="roi_texture: (levels|bin_width|lower)"):
        metrics.roi_texture(torch.zeros(5, 6, 7), _Index(), **kw)


def test_roi_texture_refuses_a_host_tensor_and_roi_report_a_bad_request(monkeypatch):
    monkeypatch.setattr(_hip, "load", lambda: pytest.fail("a device call was made"))
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        metrics.roi_texture(torch.zeros(5, 6, 7), _Index(), bin_width=0.1)
    x = torch.zeros(5, 6, 7)
    for bad in (dict(levels=8), dict(bin_width=None), dict(bin_width=0.1, bins=3), 0.1, dict(bin_width=0.1, levels=1)):
        with pytest.raises(ValueError, match="roi_report: "):
            metrics.roi_report(x, x, _Index(), texture=bad)
    with pytest.raises(ValueError, match="need texture"):
        metrics.roi_report(x, x, _Index(), draw_texture=[])


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
    return ["--base_samples", str(tmp_path / "low.npz"), "--save_dir", str(tmp_path)], \
        ["--target_samples", str(tmp_path / "full.npz")]


def test_script_defaults_leave_the_texture_off():
    mod = _script()
    args = mod.create_argparser().parse_args([])
    assert args.roi_texture_bin is None and args.roi_texture_levels is None and args.roi_texture_lower is None
    assert mod._check_texture(None, args) is None
    args = mod.create_argparser().parse_args("--roi_texture_bin 0.25 --target_samples t --roi_threshold 2.5".split())
    assert mod._check_texture(None, args) == {"bin_width": 0.25, "levels": 64, "lower": 0.0}


@pytest.mark.parametrize("flags,names", [
    ("--roi_texture_bin 0", "--roi_texture_bin"), ("--roi_texture_bin=-0.25", "--roi_texture_bin must"),
    ("--roi_texture_bin inf", "--roi_texture_bin"), ("--roi_texture_bin 1e-39", "--roi_texture_bin"), ("--roi_texture_bin nan", "--roi_texture_bin"),
    ("--roi_texture_bin 0.25 --roi_texture_levels 1", "--roi_texture_levels"),
    ("--roi_texture_bin 0.25 --roi_texture_levels 65", "--roi_texture_levels"),
    ("--roi_texture_bin 0.25 --roi_texture_lower nan", "--roi_texture_lower"),
    ("--roi_texture_bin 0.25 --roi_texture_lower=-inf", "--roi_texture_lower must"),
    ("--roi_texture_levels 32", "--roi_texture_bin"), ("--roi_texture_lower 0.5", "--roi_texture_bin"),
    ("NO_TARGET --roi_texture_bin 0.25", "--target_samples"),
    ("NO_REGIONS --roi_texture_bin 0.25", "--roi_threshold")])
def test_script_refuses_bad_texture_flags_before_any_device_call(flags, names, tmp_path, monkeypatch, capsys):
    mod = _script()
    _no_device(mod, monkeypatch)
    base, target = _files(tmp_path)
    argv = base + ([] if "NO_TARGET" in flags else target)
    if "NO_TARGET" not in flags and "NO_REGIONS" not in flags:
        argv += ["--roi_threshold", "0.5"]
    argv += [f for f in flags.split() if not f.startswith("NO_")]
    with pytest.raises(SystemExit) as e:
        mod.main(argv)
    assert e.value.code == 2
    assert names in capsys.readouterr().err


def test_script_accepts_good_texture_flags_before_it_builds_the_model(tmp_path, monkeypatch):
    """the same set-up with nothing wrong reaches the first device call: the refusals above are the checks' own"""
    mod = _script()
    _no_device(mod, monkeypatch)
    base, target = _files(tmp_path)
    with pytest.raises(AssertionError, match="went past its argument checks"):
        mod.main(base + target + "--roi_threshold 0.5 --roi_texture_bin 0.05 --roi_texture_levels 32 "
                                 "--roi_texture_lower 0.1".split())


# ------------------------------------------------------------------------------------------ the C entry
def test_entry_is_declared_exported_and_bound_within_abi_13():
    hdr = open(os.path.join(ROOT, "include", "ddpm3d.h")).read()
    declared = set(re.findall(r"\b(ddpm3d_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_hip.LIB_PATH)
    name = "ddpm3d_roi_texture"
    assert name in declared and name in _hip.EXPORTS and hasattr(lib, name)
    assert re.search(r"#define DDPM3D_ABI_VERSION 13\b", hdr) and _hip.ABI_VERSION == 13
    assert int(re.search(r"#define DDPM3D_TEX_MAX_LEVELS (\S+)", hdr).group(1)) == _hip.TEX_MAX_LEVELS == 64
    enum = re.search(r"enum \{ DDPM3D_TEX_N = 0, DDPM3D_TEX_BELOW = 1, DDPM3D_TEX_ABOVE = 2, DDPM3D_TEX_PAIRS = 3, "
                     r"DDPM3D_TEX_REC = 4 \};", hdr)
    assert enum and (_hip.TEX_N, _hip.TEX_BELOW, _hip.TEX_ABOVE, _hip.TEX_PAIRS, _hip.TEX_REC) == (0, 1, 2, 3, 4)
    assert (T.N, T.BELOW, T.ABOVE, T.PAIRS) == (0, 1, 2, 3)
    res, args = _hip.EXPORTS[name]
    assert res is ctypes.c_int and len(args) == 14
    make = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert "texture.o" in make and os.path.exists(os.path.join(PKG, "csrc", "texture.hip"))
