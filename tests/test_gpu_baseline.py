"""
GPU tier of the baseline denoisers: ddpm3d_gauss_smooth and ddpm3d_nlm through
metrics.gaussian_smooth and metrics.nlm against the fp64 yardstick of tests/baseline_ref.py, every voxel within the
entry's own bound, on volumes thinner than the window, no multiple of the tile, with the largest radii and with
radii that differ per axis; impulses, limits of h, a constant volume, a hot voxel in noise, bit-repeatability; every
refusal of the two entries with real buffers, none of which may be written; and the inference script's baseline
flags on two of its paths.

Largest share of the bound used in one run on an MI355X: Gaussian 0.17 on centred data and 0.20 on an offset of
1000; non-local means 0.0013 and 0.0031 over the five cases, 0.0036 on the constant volume.
"""

import ctypes
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

import baseline_ref as B
from conftest import PKG
from guided_diffusion import _hip, metrics

pytestmark = pytest.mark.gpu

# shape, radii: a single row; thinner than the window along D and no tile multiple; the largest radius along W with
# radii that differ per axis (a swapped axis cannot pass); the largest radius along D and none along H
GAUSS_CASES = [
    ((1, 1, 9), (0, 0, 3)),
    ((5, 37, 70), (3, 2, 5)),
    ((19, 21, 67), (1, 4, 16)),
    ((40, 9, 130), (16, 0, 1)),
]
# shape, search, patch: a single row; thinner than the halo along D; the default windows on no tile multiple; radii
# that differ per axis (a swapped axis cannot pass); the largest halo
NLM_CASES = [
    ((1, 1, 9), (0, 0, 3), (0, 0, 1)),
    ((5, 9, 70), (1, 2, 3), (1, 1, 1)),
    ((13, 21, 67), (3, 3, 3), (1, 1, 1)),
    ((12, 12, 66), (2, 0, 5), (2, 1, 0)),
    ((9, 10, 65), (5, 5, 1), (2, 2, 2)),
]
name_of = lambda v: "x".join(str(a) for a in v)


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()               # a copy: the shared references are read-only


def bits(t):
    return t.contiguous().view(torch.int32)


def within_bound(got, mean, bound, what):
    """every voxel within the bound of the yardstick; prints the largest share of the bound used"""
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == mean.shape
    got = got.cpu().numpy().astype(np.float64)
    err = np.abs(got - mean)
    used = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print("%s: largest deviation %.3g = %.4g of the bound" % (what, float(err.max()), used))
    assert (err <= bound).all(), (what, float(err.max()), used)
    return used


def taps_object(radii, taps):
    return metrics.GaussianTaps(None, None, None, tuple(radii), [[float(v) for v in t] for t in taps])


# ------------------------------------------------------------------------------------------ Gaussian
@pytest.mark.parametrize("offset", [0.0, 1000.0], ids=["centred", "offset1000"])
@pytest.mark.parametrize("shape,radii", GAUSS_CASES, ids=name_of)
def test_gaussian_every_voxel_within_the_bound(shape, radii, offset):
    x, taps, m, bound = B.gauss_case(shape, radii, offset)
    got = metrics.gaussian_smooth(dev(x), taps_object(radii, taps))
    within_bound(got, m, bound, "gaussian %s radii %s offset %g" % (shape, radii, offset))


def test_gaussian_of_public_taps_equals_the_yardstick():
    """gaussian_taps' own taps, anisotropic: 6 mm FWHM on 3.27 x 2 x 1.5 mm voxels"""
    t = metrics.gaussian_taps(6.0, (3.27, 2.0, 1.5))
    assert t.radii == (2, 4, 5)
    x = B.data((9, 20, 70), 8, offset=3.0)
    m, bound = B.gaussian(x, [np.array(row, dtype=np.float32) for row in t.taps])
    within_bound(metrics.gaussian_smooth(dev(x), t), m, bound, "gaussian 6 mm FWHM")


def test_gaussian_impulses_give_the_renormalised_outer_product():
    shape, radii = (7, 12, 70), (1, 3, 4)
    taps = tuple(B.taps_of(max(r, 1) / 3.0, r) for r in radii)
    obj = taps_object(radii, taps)
    for at in [(0, 0, 0), (6, 11, 69), (3, 0, 40), (0, 6, 30), (3, 6, 30), (3, 6, 64), (6, 8, 2)]:
        x = np.zeros(shape, dtype=np.float32)
        x[at] = 1.0
        want = np.ones(shape)
        for axis in range(3):
            t, r, n = taps[axis].astype(np.float64), radii[axis], shape[axis]
            line = np.zeros(n)
            for v in range(n):
                if abs(at[axis] - v) <= r:                    # t[at - v] over the taps counted around v
                    line[v] = t[at[axis] - v + r] / t[max(0, r - v):min(2 * r + 1, n - v + r)].sum()
            want = want * line.reshape([n if a == axis else 1 for a in range(3)])
        m, bound = B.gaussian(x, taps)
        assert np.abs(m - want).max() <= 1e-15
        got = metrics.gaussian_smooth(dev(x), obj)
        assert np.array_equal(got.cpu().numpy() != 0, want != 0), at
        within_bound(got, m, bound, "impulse at %s" % (at,))


def test_gaussian_runs_repeat_bit_for_bit():
    shape, radii = (19, 21, 67), (1, 4, 16)
    x, taps, _, _ = B.gauss_case(shape, radii, 1000.0)
    obj = taps_object(radii, taps)
    first = metrics.gaussian_smooth(dev(x), obj)
    assert torch.equal(bits(first), bits(metrics.gaussian_smooth(dev(x), obj)))
    # no radius at all: a copy
    none = taps_object((0, 0, 0), [[1.0]] * 3)
    assert torch.equal(bits(metrics.gaussian_smooth(dev(x), none)), bits(dev(x)))


# ------------------------------------------------------------------------------------------ non-local means
@pytest.mark.parametrize("offset", [0.0, 1000.0], ids=["centred", "offset1000"])
@pytest.mark.parametrize("shape,search,patch", NLM_CASES, ids=name_of)
def test_nlm_every_voxel_within_the_bound(shape, search, patch, offset):
    x, h, m, bound, _, info = B.nlm_case(shape, search, patch, offset)
    assert info["above_half"] > 0 and info["zero"] > 0       # the weights span the whole range, cutoff included
    got = metrics.nlm(dev(x), h, search=search, patch=patch)
    within_bound(got, m, bound, "nlm %s search %s patch %s offset %g h %.4g (%d weights of 0, %d borderline)"
                 % (shape, search, patch, offset, h, info["zero"], info["borderline"]))


def test_nlm_with_a_noise_std():
    shape, search, patch = (13, 21, 67), (3, 3, 3), (1, 1, 1)
    x, h, m, bound, _, info = B.nlm_case(shape, search, patch, 0.0, 0.6)
    plain = B.nlm_case(shape, search, patch, 0.0)
    assert info["above_half"] > plain[5]["above_half"] and info["zero"] > 0      # 2 sigma^2 = 0.72 came off every d2
    got = metrics.nlm(dev(x), h, search=search, patch=patch, sigma=0.6)
    within_bound(got, m, bound, "nlm %s sigma 0.6" % (shape,))
    assert np.abs(got.cpu().numpy() - plain[2]).max() > 1e-3


def test_nlm_with_an_int_for_the_radii():
    x = B.data((6, 7, 20), 9, offset=1.0)
    a = metrics.nlm(dev(x), 1.5, search=2, patch=1)
    assert torch.equal(bits(a), bits(metrics.nlm(dev(x), 1.5, search=(2, 2, 2), patch=(1, 1, 1))))
    m, bound, _, _ = B.nlm(x, (2, 2, 2), (1, 1, 1), float(np.float32(1.5)))
    within_bound(a, m, bound, "nlm int radii")


def test_nlm_tiny_h_returns_the_input_bit_for_bit():
    shape, search, patch = (13, 21, 67), (3, 3, 3), (1, 1, 1)
    x = B.nlm_case(shape, search, patch, 0.0)[0].copy()
    x[0, 0, :3] = [0.0, -0.0, np.float32(1e-42)]             # signed zeros and a denormal keep their bits
    got = metrics.nlm(dev(x), 1e-6, search=search, patch=patch)
    assert torch.equal(bits(got), bits(dev(x)))


def test_nlm_large_h_is_the_box_mean():
    shape, search, patch = (5, 9, 70), (1, 2, 3), (1, 1, 1)
    x = B.data(shape, 12, offset=1000.0)
    m, bound, _, info = B.nlm(x, search, patch, 1e6)
    assert info["zero"] == 0 and np.abs(m - B.box_mean(x, search)).max() < 1e-9
    within_bound(metrics.nlm(dev(x), 1e6, search=search, patch=patch), m, bound, "nlm h = 1e6")


def test_nlm_of_a_constant_volume():
    shape, search, patch = (6, 10, 66), (2, 2, 2), (1, 1, 1)
    x = np.full(shape, np.float32(3.7), dtype=np.float32)
    m, bound, _, _ = B.nlm(x, search, patch, 0.5)
    assert np.abs(m - np.float64(np.float32(3.7))).max() < 1e-14
    within_bound(metrics.nlm(dev(x), 0.5, search=search, patch=patch), m, bound, "nlm constant")


def test_nlm_keeps_a_hot_voxel_where_the_gaussian_of_equal_noise_reduction_does_not():
    c = B.hot_case()
    assert c["kept"](c["nlm"]) > 0.9 > c["kept"](c["gaussian"])            # the definition's property first
    got = metrics.nlm(dev(c["x"]), c["h"], search=c["search"], patch=c["patch"])
    within_bound(got, c["nlm"], c["nlm_bound"], "nlm hot voxel")
    radii = tuple(len(t) // 2 for t in c["taps"])
    smooth = metrics.gaussian_smooth(dev(c["x"]), taps_object(radii, c["taps"]))
    within_bound(smooth, c["gaussian"], c["gaussian_bound"], "gaussian hot voxel")
    far = c["far"]
    std = lambda y: float(y.cpu().numpy().astype(np.float64)[far].std())
    print("hot voxel: nlm keeps %.6f, the Gaussian of sigma %.3f voxels %.4f; std out of reach %.4f / %.4f of the "
          "input's" % (c["kept"](got.cpu().numpy()), c["sigma"], c["kept"](smooth.cpu().numpy()),
                       std(got) / std(dev(c["x"])), std(smooth) / std(dev(c["x"]))))
    assert c["kept"](got.cpu().numpy()) > 0.9 > c["kept"](smooth.cpu().numpy())


def test_nlm_runs_repeat_bit_for_bit():
    shape, search, patch = (13, 21, 67), (3, 3, 3), (1, 1, 1)
    x, h, _, _, _, _ = B.nlm_case(shape, search, patch, 1000.0)
    first = metrics.nlm(dev(x), h, search=search, patch=patch)
    assert torch.equal(bits(first), bits(metrics.nlm(dev(x), h, search=search, patch=patch)))


# ------------------------------------------------------------------------------------------ refusals
SENTINEL = 7.0
SHAPE = (4, 6, 20)


def _buffers():
    vol = torch.full(SHAPE, 1.0, device="cuda")
    out = torch.full(SHAPE, SENTINEL, device="cuda")
    ws = torch.full((SHAPE[0] * SHAPE[1] * SHAPE[2],), SENTINEL, device="cuda")
    return vol, out, ws


def _untouched(vol, out, ws):
    torch.cuda.synchronize()
    assert bool((vol == 1.0).all()) and bool((out == SENTINEL).all()) and bool((ws == SENTINEL).all())


def _floats(values):
    return None if values is None else (ctypes.c_float * len(values))(*values)


TAPS = [0.5, 1.0, 0.5]
BAD_SMOOTH = {
    "vol_null": dict(vol=None), "out_null": dict(out=None), "taps1_null": dict(taps1=None), "in_place": dict(out="vol"),
    "D_0": dict(D=0), "W_negative": dict(W=-20), "voxels_2_31": dict(D=1 << 11, H=1 << 10, W=1 << 10),
    "r0_negative": dict(r0=-1), "r2_17": dict(r2=17, taps2=[1.0] * 35),
    "tap_zero": dict(taps0=[0.0, 1.0, 0.0]), "tap_negative": dict(taps1=[-0.5, 1.0, -0.5]),
    "tap_nan": dict(taps2=[0.5, math.nan, 0.5]), "tap_inf": dict(taps2=[0.5, math.inf, 0.5]),
    "not_symmetric": dict(taps0=[0.5, 1.0, 0.25]),
    "ws_null": dict(ws=None), "ws_small": dict(ws_bytes=SHAPE[0] * SHAPE[1] * SHAPE[2] * 4 - 4),
    "ws_is_out": dict(ws="out"),
}
BAD_NLM = {
    "vol_null": dict(vol=None), "out_null": dict(out=None), "in_place": dict(out="vol"),
    "H_0": dict(H=0), "voxels_2_31": dict(D=1 << 11, H=1 << 10, W=1 << 10),
    "s0_6": dict(s0=6), "s2_negative": dict(s2=-1), "p1_3": dict(p1=3), "p2_negative": dict(p2=-1),
    "h_0": dict(h=0.0), "h_negative": dict(h=-1.0), "h_nan": dict(h=math.nan), "h_inf": dict(h=math.inf),
    "h_tiny": dict(h=1e-30), "sigma_negative": dict(sigma=-0.1), "sigma_nan": dict(sigma=math.nan),
    "sigma_inf": dict(sigma=math.inf),
}


def _resolve(a, vol, out, ws):
    named = {"vol": vol, "out": out, "ws": ws}
    for k in ("vol", "out", "ws"):
        if k in a:
            a[k] = _hip.ptr(named[a[k]]) if isinstance(a[k], str) else (None if a[k] is None else _hip.ptr(a[k]))
    return a


@pytest.mark.parametrize("case", sorted(BAD_SMOOTH))
def test_gauss_smooth_refuses_and_writes_nothing(case):
    lib = _hip.load()
    vol, out, ws = _buffers()
    a = dict(vol=vol, D=SHAPE[0], H=SHAPE[1], W=SHAPE[2], r0=1, r1=1, r2=1, taps0=TAPS, taps1=TAPS, taps2=TAPS,
             out=out, ws=ws, ws_bytes=ws.numel() * 4, stream=_hip.stream())
    a.update(BAD_SMOOTH[case])
    a = _resolve(a, vol, out, ws)
    for k in ("taps0", "taps1", "taps2"):
        a[k] = _floats(a[k])
    rc = lib.ddpm3d_gauss_smooth(*a.values())
    assert rc == _hip.E_INVAL and lib.ddpm3d_last_error().decode().startswith("gauss_smooth:")
    _untouched(vol, out, ws)


@pytest.mark.parametrize("case", sorted(BAD_NLM))
def test_nlm_refuses_and_writes_nothing(case):
    lib = _hip.load()
    vol, out, ws = _buffers()
    a = dict(vol=vol, D=SHAPE[0], H=SHAPE[1], W=SHAPE[2], s0=1, s1=1, s2=1, p0=1, p1=1, p2=1, h=1.0, sigma=0.0,
             out=out, stream=_hip.stream())
    a.update(BAD_NLM[case])
    a = _resolve(a, vol, out, ws)
    rc = lib.ddpm3d_nlm(*a.values())
    assert rc == _hip.E_INVAL and lib.ddpm3d_last_error().decode().startswith("nlm:")
    _untouched(vol, out, ws)


def test_the_same_calls_with_nothing_wrong_do_write():
    lib = _hip.load()
    vol, out, ws = _buffers()
    t = _floats(TAPS)
    _hip.check(lib.ddpm3d_gauss_smooth(_hip.ptr(vol), *SHAPE, 1, 1, 1, t, t, t, _hip.ptr(out), _hip.ptr(ws),
                                       ws.numel() * 4, _hip.stream()))
    torch.cuda.synchronize()
    assert torch.allclose(out, vol, rtol=1e-6)
    out.fill_(SENTINEL)
    _hip.check(lib.ddpm3d_nlm(_hip.ptr(vol), *SHAPE, 1, 1, 1, 1, 1, 1, 1.0, 0.0, _hip.ptr(out), _hip.stream()))
    torch.cuda.synchronize()
    assert torch.equal(out, vol)


def test_python_entries_refuse_what_they_cannot_take():
    taps = metrics.gaussian_taps(4.0, (2.0, 2.0, 2.0))
    x = torch.zeros((4, 5, 6), device="cuda")
    for bad in (torch.zeros((5, 6), device="cuda"), torch.zeros((2, 4, 5, 6), device="cuda")):
        with pytest.raises(ValueError, match="gaussian_smooth: volume of shape"):
            metrics.gaussian_smooth(bad, taps)
        with pytest.raises(ValueError, match="nlm: volume of shape"):
            metrics.nlm(bad, 1.0)
    for bad in (x.permute(2, 0, 1), x.double(), x.cpu()):
        with pytest.raises(RuntimeError):
            metrics.gaussian_smooth(bad, taps)
        with pytest.raises(RuntimeError):
            metrics.nlm(bad, 1.0)
    with pytest.raises(ValueError, match="search radius"):
        metrics.nlm(x, 1.0, search=6)


# ------------------------------------------------------------------------------------------ the script
FLAGS = ("--large_size 16 --small_size 16 --num_channels 32 --num_res_blocks 1 --num_head_channels 64 "
         "--attention_resolutions 1000 --learn_sigma True --resblock_updown True --use_scale_shift_norm True "
         "--timestep_respacing 3").split()
FILE_SPACING = (3.27, 2.0, 1.5)                               # along the file's (D, H, W)
EVALUATE_KEYS = {"psnr", "nrmse", "mae", "bias", "ssim", "data_range", "n_voxels"}


def _script():
    spec = importlib.util.spec_from_file_location("ddpm3d_infer_entry", os.path.join(PKG, "scripts", "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _inputs(tmp_path):
    import metrics_ref
    target = metrics_ref.phantom((20, 40, 40), seed=4)                      # (D, H, W): 3 x 3 x 2 patches of 16^3
    low = metrics_ref.noisy(target, 0.1, seed=4)
    np.savez(tmp_path / "pet.npz", low)
    np.savez(tmp_path / "full.npz", target)
    common = FLAGS + ["--base_samples", str(tmp_path / "pet.npz"), "--target_samples", str(tmp_path / "full.npz"),
                      "--roi_threshold", repr(0.4 * float(target.max())), "--roi_connectivity", "6"]
    return target, low, common


@pytest.mark.parametrize("extra", [[], ["--patch_overlap", "4"]], ids=["one-shot", "sliding"])
def test_script_scores_the_baselines(extra, tmp_path):
    target, low, common = _inputs(tmp_path)
    mod = _script()
    path = mod.main(common + extra + ["--save_dir", str(tmp_path / "bb"), "--voxel_spacing"]
                    + [str(v) for v in FILE_SPACING]
                    + ["--baseline_gaussian_fwhm", "5", "--baseline_nlm_h", "0.2", "--baseline_nlm_search", "2",
                       "--baseline_nlm_sigma", "0.05"])
    report = json.load(open(tmp_path / "bb" / "metrics_pet.json"))
    assert list(report) == ["denoised", "input", "target", "mask_threshold", "baselines", "roi"]
    base = report["baselines"]
    assert list(base) == ["gaussian", "nlm"]
    assert set(base["gaussian"]) == {"fwhm_mm", "sigma_voxels", "radii"} | EVALUATE_KEYS
    assert set(base["nlm"]) == {"h", "sigma", "search", "patch"} | EVALUATE_KEYS
    spacing = (FILE_SPACING[1], FILE_SPACING[2], FILE_SPACING[0])           # (H, W, Z), as the volumes are scored
    taps = metrics.gaussian_taps(5.0, spacing)
    back = lambda v: [v[2], v[0], v[1]]                                      # listed along the file's (D, H, W)
    assert base["gaussian"]["fwhm_mm"] == 5.0 and base["gaussian"]["radii"] == back(taps.radii)
    assert base["gaussian"]["sigma_voxels"] == pytest.approx(back(taps.sigma_voxels), rel=1e-12)
    assert base["nlm"]["h"] == float(np.float32(0.2)) and base["nlm"]["sigma"] == float(np.float32(0.05))
    assert base["nlm"]["search"] == [2, 2, 2] and base["nlm"]["patch"] == [1, 1, 1]

    # the same figures recomputed here: the input filtered on the device, scored with the script's mask and range
    arr = np.load(path)["arr_0"]                                            # (H, W, Z)
    hwz = lambda a: dev(np.ascontiguousarray(a.transpose(1, 2, 0)))
    keep = torch.zeros(arr.shape, dtype=torch.uint8, device="cuda")         # Hann weight 0: the outermost planes
    keep[1:-1, 1:-1, 1:-1] = 1
    tgt, inp = hwz(target), hwz(low)
    want = metrics.evaluate(metrics.gaussian_smooth(inp, taps), tgt, mask=keep)
    assert {k: base["gaussian"][k] for k in EVALUATE_KEYS} == want
    want = metrics.evaluate(metrics.nlm(inp, 0.2, search=2, patch=1, sigma=0.05), tgt, mask=keep)
    assert {k: base["nlm"][k] for k in EVALUATE_KEYS} == want
    assert report["input"] == metrics.evaluate(inp, tgt, mask=keep)
    for name in ("gaussian", "nlm"):
        assert base[name]["n_voxels"] == report["input"]["n_voxels"]
        assert base[name]["data_range"] == report["input"]["data_range"]
        assert base[name]["psnr"] > report["input"]["psnr"]                 # either filter does lower the noise
        print("%s: PSNR %.3f dB against the input's %.3f" % (name, base[name]["psnr"], report["input"]["psnr"]))
    regions = report["roi"]["regions"]
    assert len(regions) >= 3 and "detection" in report["roi"]
    for r in regions.values():
        assert list(r) == ["n", "target", "input", "gaussian", "nlm", "denoised"]
        for name in ("gaussian", "nlm"):
            assert set(r[name]) == set(r["input"]) - {"found", "overlap"}   # baselines get no detection figures
            assert r[name]["peak"] is not None and r[name]["tlg"] is not None and r[name]["n"] == r["n"]
        assert r["gaussian"]["peak"] != r["input"]["peak"] != r["nlm"]["peak"]
    assert set(report["roi"]["detection"]) == {"input", "denoised"}


def test_script_without_the_flags_writes_what_it_wrote_before(tmp_path):
    _, _, common = _inputs(tmp_path)
    mod = _script()
    spaced = ["--voxel_spacing"] + [str(v) for v in FILE_SPACING]
    plain_path = mod.main(common + spaced + ["--save_dir", str(tmp_path / "plain")])
    plain = json.load(open(tmp_path / "plain" / "metrics_pet.json"))
    assert list(plain) == ["denoised", "input", "target", "mask_threshold", "roi"] and "baselines" not in plain
    for r in plain["roi"]["regions"].values():
        assert list(r) == ["n", "target", "input", "denoised"]
    log = open(tmp_path / "plain" / "log.txt").read()
    assert "gaussian" not in log and "nlm" not in log and log.count("vs target") == 2
    # with the flags: the old entries keep their values, the written volume its bytes, the log gains two lines
    path = mod.main(common + spaced + ["--save_dir", str(tmp_path / "bb"), "--baseline_gaussian_fwhm", "5",
                                       "--baseline_nlm_h", "0.2"])
    both = json.load(open(tmp_path / "bb" / "metrics_pet.json"))
    for key in ("denoised", "input", "target", "mask_threshold"):
        assert both[key] == plain[key]
    for v, r in both["roi"]["regions"].items():
        assert {k: x for k, x in r.items() if k not in ("gaussian", "nlm")} == plain["roi"]["regions"][v]
    assert {k: x for k, x in both["roi"].items() if k not in ("regions", "labels")} \
        == {k: x for k, x in plain["roi"].items() if k not in ("regions", "labels")}
    assert open(plain_path, "rb").read() == open(path, "rb").read()
    log = open(tmp_path / "bb" / "log.txt").read()
    assert log.count("vs target") == 4 and "gaussian vs target: PSNR" in log and "nlm      vs target: PSNR" in log
