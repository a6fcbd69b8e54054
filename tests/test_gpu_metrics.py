"""
GPU tier of the image-quality metrics: ddpm3d_error_moments against numpy fp64, ddpm3d_ssim3d against
the fp64 yardstick of tests/metrics_ref.py under a bound taken from a plain fp32 host evaluation of the same pair
(which must also hold on an offset of 4, where the plain evaluation fails: the pivot works), bit-repeatability,
batching, one case past 2^31 elements, and the inference script's --target_samples on all three of its paths.
"""

import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import metrics_ref as R
from conftest import PKG
from guided_diffusion import metrics

pytestmark = pytest.mark.gpu

PAIRS = list(R.pairs())
IDS = [p[0] for p in PAIRS]
REL = 1e-10             # both sides sum exact fp64 terms, only the order differs: n * 2^-53 = 4e-11 at the largest size


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------ error moments
def check_moments(got, want, std):
    assert got["n"] == want["n"] > 0
    for k in ("mse", "mae", "target_sq_mean"):
        assert abs(got[k] - want[k]) <= REL * abs(want[k]), (k, got[k], want[k])
    # terms that change sign: against the size of the terms, not of their sum
    assert abs(got["bias"] - want["bias"]) <= REL * want["mae"], (got["bias"], want["bias"])
    assert abs(got["target_mean"] - want["target_mean"]) <= REL * want["target_abs_mean"]
    assert got["target_min"] == want["target_min"] and got["target_max"] == want["target_max"]
    if std:
        assert got["cover_1"] == want["cover_1"] and got["cover_2"] == want["cover_2"]
        assert got["coverage_1"] == want["cover_1"] / want["n"] and got["coverage_2"] == want["cover_2"] / want["n"]
        assert 0 < want["cover_1"] < want["cover_2"] < want["n"]            # the std test data bite
    else:
        assert "cover_1" not in got and "coverage_1" not in got


@pytest.mark.parametrize("shape", [(48, 64, 64), (23, 37, 61), (11, 11, 11), (40, 96, 96)])
@pytest.mark.parametrize("use_mask", [False, True])
@pytest.mark.parametrize("use_std", [False, True])
def test_error_moments_match_numpy_fp64(shape, use_mask, use_std):
    y = R.phantom(shape, seed=3)
    y = y - np.float32(0.05)                                   # a target whose terms change sign
    xs = np.stack([R.noisy(y, s, seed=i) for i, s in enumerate((0.02, 0.1, 0.3))])
    mask = R.body_mask(y + np.float32(0.05)) if use_mask else None
    std = np.abs(R.noisy(np.zeros_like(y), 0.1, seed=9)) if use_std else None
    dm, ds = (None if a is None else dev(a) for a in (mask, std))
    batch = metrics.error_moments(dev(xs), dev(y), mask=dm, std=ds)
    assert all(isinstance(v, list) and len(v) == 3 for v in batch.values())
    for i in range(3):
        want = R.moments(xs[i], y, mask, std)
        check_moments({k: v[i] for k, v in batch.items()}, want, use_std)
        single = metrics.error_moments(dev(xs[i]), dev(y), mask=dm, std=ds)
        assert isinstance(single["mse"], float) and isinstance(single["n"], int)
        assert single == {k: v[i] for k, v in batch.items()}                    # K = 3 in one launch: the same bits
    assert len({batch["mse"][i] for i in range(3)}) == 3


def test_error_moments_on_a_misaligned_view_and_odd_sizes():
    """a view 4 bytes into a buffer cannot take 16-byte loads; 13 x 17 x 19 is no multiple of 4: same figures"""
    for shape in ((24, 32, 32), (13, 17, 19)):
        y = R.phantom(shape, seed=5)
        x = R.noisy(y, 0.05, seed=5)
        mask, std = R.body_mask(y), np.abs(R.noisy(np.zeros_like(y), 0.05, seed=6))
        n = y.size
        bx, by, bs = (torch.zeros(n + 1, dtype=torch.float32, device="cuda") for _ in range(3))
        bm = torch.zeros(n + 1, dtype=torch.uint8, device="cuda")
        for buf, a in ((bx, x), (by, y), (bs, std), (bm, mask)):
            buf[1:] = dev(a).reshape(-1)
        vx, vy, vs, vm = (b[1:].view(shape) for b in (bx, by, bs, bm))
        assert vx.data_ptr() % 16 == 4 and vx.is_contiguous() and vm.data_ptr() % 4 == 1
        got = metrics.error_moments(vx, vy, mask=vm, std=vs)
        check_moments(got, R.moments(x, y, mask, std), True)


def test_error_moments_do_not_cancel():
    """x = 1e4 + 1e-3 noise against y = 1e4: e is formed in fp64 before anything is squared or summed"""
    shape = (24, 40, 40)
    rng = np.random.default_rng(11)
    y = np.full(shape, 1e4, dtype=np.float32)
    x = (1e4 + 1e-3 * rng.standard_normal(shape)).astype(np.float32)
    want = R.moments(x, y)
    assert 0 < want["mse"] < 1e-5 and want["mae"] > 1e-4
    check_moments(metrics.error_moments(dev(x), dev(y)), want, False)


def test_error_moments_refuse_what_they_cannot_count():
    y = dev(R.phantom((12, 12, 12)))
    with pytest.raises(ValueError, match="counts no voxel"):
        metrics.error_moments(y, y, mask=torch.zeros_like(y, dtype=torch.uint8))
    with pytest.raises(ValueError):
        metrics.error_moments(y[:11], y)
    with pytest.raises(ValueError):
        metrics.error_moments(y, y, mask=torch.zeros_like(y))                   # a float mask


# ------------------------------------------------------------------------------------------ SSIM
def bound_of(x, y, ref):
    """e32: the largest per-voxel deviation from the yardstick of a plain fp32 host evaluation of the same pair"""
    e32 = float(np.abs(R.ssim_map_fp32(x, y, 1.0) - ref).max())
    assert 0 < e32 <= 1e-4, e32                     # a broken yardstick cannot widen the bound
    return e32


@pytest.mark.parametrize("name,x,y", PAIRS, ids=IDS)
def test_ssim_matches_the_yardstick_with_and_without_an_offset(name, x, y):
    """map within 4 e32 per voxel, mean within e32, e32 taken from the un-shifted pair; the same bound for (x + 4, y + 4)
    at the same L, where the plain fp32 evaluation itself is off by 1e-3 .. 1e-2; masked mean under the same bound"""
    ref = R.ssim_map(x, y, 1.0)
    e32 = bound_of(x, y, ref)
    mask = R.body_mask(y)
    assert 0.10 < mask.mean() < 0.60 and R.interior_mask(mask).sum() > 0
    for offset in (0.0, 4.0):
        xo, yo = x + np.float32(offset), y + np.float32(offset)
        want = R.ssim_map(xo, yo, 1.0) if offset else ref
        plain, masked = R.masked_mean(want, None), R.masked_mean(want, mask)
        assert 0.15 < plain < 0.95 and 0.15 < masked < 0.95
        mean, smap = metrics.ssim3d(dev(xo), dev(yo), 1.0, full=True)
        assert smap.shape == want.shape and smap.dtype == torch.float32 and isinstance(mean, float)
        err = float(np.abs(smap.cpu().numpy().astype(np.float64) - want).max())
        got_masked = metrics.ssim3d(dev(xo), dev(yo), 1.0, mask=dev(mask))
        host32 = float(np.abs(R.ssim_map_fp32(xo, yo, 1.0) - want).max())
        print("%s + %g: e32 %.3g | GPU map max %.3g, mean %.3g, masked mean %.3g | plain fp32 on this input %.3g"
              % (name, offset, e32, err, abs(mean - plain), abs(got_masked - masked), host32))
        assert err <= 4 * e32
        assert abs(mean - plain) <= e32
        assert abs(got_masked - masked) <= e32
        if offset:
            assert host32 > 10 * e32              # the case is hard: the bound is not met without a pivot


@pytest.mark.parametrize("name,x,y", PAIRS[-2:], ids=IDS[-2:])
def test_ssim_of_one_interior_voxel_matches_the_yardstick(name, x, y):
    """11 x 11 x 11 with real data: one tile, one chunk, 11 input planes, a map of one voxel.  The volume is a crop of
    a phantom pair, so its one window is a window of that pair and the yardstick's value is that voxel of the pair's
    map.  The bound is the pair's own per-voxel bound, 4 e32 with e32 the maximum over the pair's whole map: the error
    of a plain fp32 evaluation of a single voxel is one draw of rounding errors and can be anywhere down to 0, so it
    bounds nothing by itself.  With and without the offset."""
    ref = R.ssim_map(x, y, 1.0)
    e32 = bound_of(x, y, ref)
    for origin in ((6, 13, 25), (2, 4, 40), (12, 20, 8)):
        crop = tuple(slice(o, o + 11) for o in origin)
        cx, cy = np.ascontiguousarray(x[crop]), np.ascontiguousarray(y[crop])
        want = float(ref[origin])
        assert abs(float(R.ssim_map(cx, cy, 1.0)[0, 0, 0]) - want) <= 1e-12 and 0.01 < want < 0.999
        for offset in (0.0, 4.0):
            xo, yo = cx + np.float32(offset), cy + np.float32(offset)
            want_o = float(R.ssim_map(xo, yo, 1.0)[0, 0, 0])
            mean, smap = metrics.ssim3d(dev(xo), dev(yo), 1.0, full=True)
            assert smap.shape == (1, 1, 1) and mean == float(smap.reshape(-1)[0])
            err = abs(mean - want_o)
            print("%s crop at %s + %g: yardstick %.6f, pair's e32 %.3g, GPU off by %.3g"
                  % (name, origin, offset, want_o, e32, err))
            assert err <= 4 * e32


@pytest.mark.parametrize("name,x,y", PAIRS[:1] + PAIRS[-1:], ids=IDS[:1] + IDS[-1:])
def test_ssim_is_bit_repeatable_and_batches(name, x, y):
    xs = np.stack([x, R.noisy(y, 0.05, seed=77), y])
    mask = dev(R.body_mask(y))
    dx, dy = dev(xs), dev(y)
    means, maps = metrics.ssim3d(dx, dy, 1.0, full=True)
    assert len(means) == 3 and maps.shape == (3,) + tuple(n - 10 for n in y.shape)
    again, maps2 = metrics.ssim3d(dx, dy, 1.0, full=True)
    assert means == again and torch.equal(maps, maps2)                          # twice: the same bits
    assert metrics.ssim3d(dx, dy, 1.0) == means                                 # full=False: the same mean
    masked = metrics.ssim3d(dx, dy, 1.0, mask=mask)
    assert masked == metrics.ssim3d(dx, dy, 1.0, mask=mask, full=True)[0] and masked != means
    for i in range(3):                                                          # three single calls: the same bits
        m, mp = metrics.ssim3d(dx[i], dy, 1.0, full=True)
        assert m == means[i] and torch.equal(mp, maps[i])
        assert metrics.ssim3d(dx[i], dy, 1.0, mask=mask) == masked[i]
    assert abs(means[2] - 1.0) <= 1e-6 and means[0] != means[1] and max(means[:2]) < 0.95


@pytest.mark.parametrize("shape", [(11, 11, 11), (12, 27, 43), (30, 16, 32)])
def test_ssim_of_constants_and_of_identity(shape):
    for a, b, L in ((0.3, 0.7, 1.0), (2.0, 2.5, 3.0), (0.0, 1.0, 1.0), (5.0, 5.0, 1.0)):
        x = torch.full(shape, a, dtype=torch.float32, device="cuda")
        y = torch.full(shape, b, dtype=torch.float32, device="cuda")
        mean, smap = metrics.ssim3d(x, y, L, full=True)
        want = R.constant_ssim(np.float32(a).astype(np.float64), np.float32(b).astype(np.float64), L)
        assert smap.shape == tuple(n - 10 for n in shape)
        assert abs(mean - want) <= 1e-6 and float((smap.double() - want).abs().max()) <= 1e-6
    y = dev(R.phantom(shape, seed=2))
    mean, smap = metrics.ssim3d(y, y, 1.0, full=True)
    assert abs(mean - 1.0) <= 1e-6 and float((smap - 1.0).abs().max()) <= 1e-6


def test_ssim_refuses_what_it_cannot_window():
    y = dev(R.phantom((12, 12, 12)))
    with pytest.raises(ValueError, match="at least 11"):
        metrics.ssim3d(y[:, :, :10].contiguous(), y[:, :, :10].contiguous(), 1.0)
    for bad in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="data_range"):
            metrics.ssim3d(y, y, bad)
    mask = torch.zeros_like(y, dtype=torch.uint8)
    mask[0, 0, 0] = 1                                                           # counted, but not in the interior
    with pytest.raises(ValueError, match="no interior voxel"):
        metrics.ssim3d(y, y, 1.0, mask=mask)


def test_evaluate_puts_the_figures_together():
    name, x, y = PAIRS[1]
    mask = R.body_mask(y)
    std = np.full_like(y, 0.1)
    got = metrics.evaluate(dev(x), dev(y), mask=dev(mask), std=dev(std))
    m = R.moments(x, y, mask, std)
    L = m["target_max"] - m["target_min"]
    assert set(got) == {"psnr", "nrmse", "mae", "bias", "ssim", "data_range", "n_voxels", "coverage_1", "coverage_2"}
    assert all(isinstance(v, float) for k, v in got.items() if k != "n_voxels") and got["n_voxels"] == m["n"]
    assert got["data_range"] == L
    assert abs(got["psnr"] - 10 * np.log10(L * L / m["mse"])) <= 1e-9
    assert abs(got["nrmse"] - np.sqrt(m["mse"] / m["target_sq_mean"])) <= 1e-12
    assert abs(got["ssim"] - R.ssim(x, y, L, mask)) <= bound_of(x, y, R.ssim_map(x, y, 1.0))
    assert 0.5 < got["coverage_1"] < 0.8 < got["coverage_2"] <= 1.0             # noise of 0.1 against a std of 0.1
    both = metrics.evaluate(dev(np.stack([x, y])), dev(y), data_range=2.0)
    assert set(both) == {"psnr", "nrmse", "mae", "bias", "ssim", "data_range", "n_voxels"}
    assert both["data_range"] == 2.0 and both["n_voxels"] == y.size
    assert both["psnr"][1] == float("inf") and both["nrmse"][1] == 0.0 and abs(both["ssim"][1] - 1.0) <= 1e-6
    assert both["psnr"][0] == pytest.approx(10 * np.log10(4.0 / R.moments(x, y)["mse"]), abs=1e-9)


def test_metrics_past_2_to_the_31_elements():
    """17 constant estimates of 128 x 1024 x 1024 (2.28e9 elements, 9.1 GB) against a constant target: offsets are
    64-bit.  Analytic answers only; nothing of this size is evaluated on the host."""
    shape, K, b = (128, 1024, 1024), 17, 0.5
    free, _ = torch.cuda.mem_get_info()
    assert free > 12 << 30, "this case needs 10 GB of device memory"
    a = [0.25 + d / 64.0 for d in range(K)]                                     # exact in fp32
    x = torch.empty((K,) + shape, dtype=torch.float32, device="cuda")
    for d in range(K):
        x[d].fill_(a[d])
    y = torch.full(shape, b, dtype=torch.float32, device="cuda")
    assert x.numel() > 2 ** 31
    m = metrics.error_moments(x, y)
    ssim = metrics.ssim3d(x, y, 1.0)
    for d in range(K):
        e = a[d] - b
        assert m["n"][d] == y.numel() and m["target_min"][d] == m["target_max"][d] == b
        assert abs(m["mse"][d] - e * e) <= REL * e * e and abs(m["bias"][d] - e) <= REL * abs(e)
        assert abs(m["mae"][d] - abs(e)) <= REL * abs(e) and abs(m["target_sq_mean"][d] - b * b) <= REL
        assert abs(ssim[d] - R.constant_ssim(a[d], b, 1.0)) <= 1e-6
    del x, y
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------ the script
FLAGS = ("--large_size 16 --small_size 16 --num_channels 32 --num_res_blocks 1 --num_head_channels 64 "
         "--attention_resolutions 1000 --learn_sigma True --resblock_updown True --use_scale_shift_norm True "
         "--timestep_respacing 3").split()


def _script():
    spec = importlib.util.spec_from_file_location("ddpm3d_infer_entry", os.path.join(PKG, "scripts", "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("extra,threshold", [([], 0.0), ([], 0.1), (["--num_draws", "2"], 0.1),
                                             (["--joint_patches", "True"], 0.0)],
                         ids=["independent", "independent-masked", "draws", "joint"])
def test_script_scores_its_output_against_a_target(extra, threshold, tmp_path):
    target = R.phantom((20, 40, 40), seed=4)                               # (D, H, W): 3 x 3 x 2 patches of 16^3
    low = R.noisy(target, 0.1, seed=4)
    np.savez(tmp_path / "pet.npz", low)
    np.savez(tmp_path / "full.npz", target)
    mod = _script()
    common = FLAGS + ["--base_samples", str(tmp_path / "pet.npz")] + extra
    plain = mod.main(common + ["--save_dir", str(tmp_path / "plain")])
    assert not os.path.exists(tmp_path / "plain" / "metrics_pet.json")
    path = mod.main(common + ["--save_dir", str(tmp_path / "scored"), "--target_samples", str(tmp_path / "full.npz"),
                              "--metrics_mask_threshold", str(threshold)])
    assert open(plain, "rb").read() == open(path, "rb").read()             # the .npz: byte for byte as without
    rep = json.load(open(tmp_path / "scored" / "metrics_pet.json"))
    assert set(rep) == {"denoised", "input", "target", "mask_threshold"}
    assert rep["target"] == str(tmp_path / "full.npz") and rep["mask_threshold"] == threshold

    out = np.load(path)
    arr, tgt, inp = out["arr_0"], target.transpose(1, 2, 0), low.transpose(1, 2, 0)        # (H, W, Z)
    joint = "--joint_patches" in extra
    counted = np.ones(arr.shape, dtype=bool)
    if threshold:
        counted &= tgt > np.float32(threshold) * tgt.max()
    if not joint:                                                          # Hann weight 0: the outermost planes
        counted[[0, -1]] = False
        counted[:, [0, -1]] = False
        counted[:, :, [0, -1]] = False
        assert np.all(arr[0] == 0) and np.all(arr[:, :, -1] == 0)
    mask = None if counted.all() else counted.astype(np.uint8)
    dmask = None if mask is None else dev(mask)
    std = out["std"] if "std" in out.files else None
    assert (std is not None) == ("--num_draws" in extra)
    want = metrics.evaluate(dev(arr), dev(tgt), mask=dmask, std=None if std is None else dev(std))
    assert set(rep["denoised"]) == set(want) and set(rep["input"]) == set(want) - {"coverage_1", "coverage_2"}
    for k, v in want.items():
        assert abs(rep["denoised"][k] - v) <= 1e-12, (k, rep["denoised"][k], v)
    if std is not None:
        assert 0 <= rep["denoised"]["coverage_1"] <= rep["denoised"]["coverage_2"] <= 1
    # the input block against the host yardsticks
    m = R.moments(inp, tgt, mask)
    L = m["target_max"] - m["target_min"]
    got = rep["input"]
    assert got["n_voxels"] == m["n"] and got["data_range"] == L
    # mse and mean(target^2) are within REL relative: d psnr = 10 / ln 10 * REL, d nrmse = nrmse * REL (half of each
    # of the two relative errors), plus a few ulp of log10 / sqrt themselves
    psnr, nrmse = 10 * np.log10(L * L / m["mse"]), np.sqrt(m["mse"] / m["target_sq_mean"])
    assert abs(got["psnr"] - psnr) <= 10 / np.log(10) * REL + 1e-13
    assert abs(got["nrmse"] - nrmse) <= nrmse * REL + 1e-15
    assert abs(got["mae"] - m["mae"]) <= REL * m["mae"] and abs(got["bias"] - m["bias"]) <= REL * m["mae"]
    e32 = bound_of(inp, tgt, R.ssim_map(inp, tgt, 1.0))
    assert abs(got["ssim"] - R.ssim(inp, tgt, L, mask)) <= e32
    assert 0.05 < got["ssim"] < 0.95 and got["psnr"] > 10
