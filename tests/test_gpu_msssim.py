"""
GPU tier of the multi-scale SSIM: ddpm3d_pool2 bit for bit against the numpy fp32 yardstick of
tests/msssim_ref.py on both of its load paths, ddpm3d_msssim3d against the fp64 yardstick under a bound taken from a
plain fp32 host evaluation of the same pyramid (which must also hold on an offset of 4: the pivot survives the
pooling), its ties to ddpm3d_ssim3d, bit-repeatability and batching, the clamp, constants, the refusals through
Python, and the inference script's --msssim_scales.
"""

import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

import metrics_ref as R
import msssim_ref as MS
from conftest import PKG
from guided_diffusion import _hip, metrics

pytestmark = pytest.mark.gpu

CASE_IDS = MS.case_ids()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def misaligned(a):
    """a contiguous device view of `a` whose pointer is 4 bytes (floats) or 1 byte (masks) past a 16-byte boundary"""
    t = dev(a)
    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device="cuda")
    buf[1:] = t.reshape(-1)
    view = buf[1:].view(t.shape)
    assert view.data_ptr() % 8 == t.element_size() and view.is_contiguous()
    return view


# ------------------------------------------------------------------------------------------------ pooling
@pytest.mark.parametrize("i", range(len(MS.CASES)), ids=["%dx%dx%d" % c[0] for c in MS.CASES])
def test_pool2_is_bit_equal_to_the_yardstick(i):
    """a 3-stack, each member alone, a view misaligned by 4 bytes (the scalar path), the pooled mask, and the second
    level; (45, 50, 91) and (23, 37, 61) have an odd W (the scalar path), the others an even one (the wide path)"""
    c = MS.case(i, 0)
    stack = np.stack([c["x"], c["y"], MS.case(i, 1)["x"]])
    want, want_mask = MS.pool2(stack), MS.pool2_mask(c["mask"])
    assert 0 < want_mask.mean() < 1 and want.shape == (3,) + tuple(n // 2 for n in c["shape"])
    got, got_mask = metrics.pool2(dev(stack), mask=dev(c["mask"]))
    assert got.dtype == torch.float32 and got_mask.dtype == torch.uint8
    assert torch.equal(got.cpu(), torch.from_numpy(want)) and torch.equal(got_mask.cpu(), torch.from_numpy(want_mask))
    for b in range(3):
        single = metrics.pool2(dev(stack[b]))
        assert single.shape == want.shape[1:] and torch.equal(single, got[b])
    off, off_mask = metrics.pool2(misaligned(stack), mask=misaligned(c["mask"]))
    assert torch.equal(off, got) and torch.equal(off_mask, got_mask)
    if c["scales"] > 2:                                                    # the next level, from the pooled tensors
        again, again_mask = metrics.pool2(got, mask=got_mask)
        assert torch.equal(again.cpu(), torch.from_numpy(MS.pool2(want)))
        assert torch.equal(again_mask.cpu(), torch.from_numpy(MS.pool2_mask(want_mask)))


def test_pool2_paths_and_edges():
    """even W on the wide path against the same data on the scalar path; extents of 2 and 3; many tiles along w and h"""
    rng = np.random.default_rng(3)
    for shape in ((2, 2, 2), (3, 3, 3), (2, 11, 262), (5, 9, 131), (4, 2, 130)):
        x = rng.standard_normal(shape).astype(np.float32) * np.float32(1e3)
        mask = (rng.random(shape) < 0.5).astype(np.uint8) * np.uint8(200)
        want, want_mask = MS.pool2(x), MS.pool2_mask(mask)
        for vol, m in ((dev(x), dev(mask)), (misaligned(x), misaligned(mask))):
            got, got_mask = metrics.pool2(vol, mask=m)
            assert torch.equal(got.cpu(), torch.from_numpy(want)), shape
            assert torch.equal(got_mask.cpu(), torch.from_numpy(want_mask)), shape
    with pytest.raises(ValueError, match="at least 2"):
        metrics.pool2(torch.zeros(1, 4, 4, device="cuda"))
    with pytest.raises(ValueError, match="mask"):
        metrics.pool2(torch.zeros(4, 4, 4, device="cuda"), mask=torch.zeros(4, 4, 2, dtype=torch.uint8, device="cuda"))


# ----------------------------------------------------------------------------------------------- accuracy
@pytest.mark.parametrize("ik", CASE_IDS, ids=MS.case_name)
def test_msssim_matches_the_yardstick_with_and_without_an_offset(ik):
    """every per-scale mean within e = max_j e32_j of the yardstick's, masked and not; the final value within the
    first-order propagation of e through the product, ms_ref * sum_j w_j e / v_j; the same for (x + 4, y + 4) at the
    same L, with e taken from the un-shifted pair"""
    c = MS.case(*ik)
    M, w = c["scales"], MS.weights(c["scales"])
    e = max(c["e32"])
    assert 0 < e <= 1e-4, c["e32"]                  # a broken yardstick cannot widen the bound
    for offset in (0.0, 4.0):
        xo, yo = c["x"] + np.float32(offset), c["y"] + np.float32(offset)
        for masked in (False, True):
            mask = c["mask"] if masked else None
            if offset:
                want, terms = MS.msssim(xo, yo, 1.0, M, mask)
            else:
                want, terms = c["value"][masked], c["terms"][masked]
            assert all(0.15 < t < 1 for t in terms)
            got, parts = metrics.msssim3d(dev(xo), dev(yo), 1.0, M, mask=None if mask is None else dev(mask),
                                          parts=True)
            assert isinstance(got, float) and len(parts["cs"]) == M - 1 and isinstance(parts["ssim"], float)
            got_terms = parts["cs"] + [parts["ssim"]]
            bound = MS.first_order_bound(want, terms, w, e)
            print("%s + %g masked=%s: e %.3g | per scale off by %s | value %.9f against %.9f: off by %.3g, bound %.3g"
                  % (c["name"], offset, masked, e, ["%.3g" % abs(a - b) for a, b in zip(got_terms, terms)], got, want,
                     abs(got - want), bound))
            assert all(abs(a - b) <= e for a, b in zip(got_terms, terms))
            assert abs(got - want) <= bound
            assert got == math.prod(t ** wj for t, wj in zip(got_terms, w))


# ------------------------------------------------------------------------------------- ties to existing code
@pytest.mark.parametrize("ik", CASE_IDS[:1] + CASE_IDS[-3:], ids=MS.case_name)
def test_one_scale_is_ssim3d_and_scale_0_carries_its_bits(ik):
    c = MS.case(*ik)
    x, y, mask = dev(c["x"]), dev(c["y"]), dev(c["mask"])
    for m in (None, mask):
        assert metrics.msssim3d(x, y, 1.0, 1, mask=m) == metrics.ssim3d(x, y, 1.0, mask=m)
        value, parts = metrics.msssim3d(x, y, 1.0, 1, mask=m, parts=True)
        assert parts == {"cs": [], "ssim": value}
    lib = _hip.load()
    D, H, W = c["shape"]
    M, K = c["scales"], 2
    xs = dev(np.stack([c["x"], c["y"]]))
    for m in (None, mask):
        ws = torch.empty(max(lib.ddpm3d_msssim3d_workspace_bytes(K, D, H, W, M),
                             lib.ddpm3d_ssim3d_workspace_bytes(K, D, H, W)) // 8, dtype=torch.float64, device="cuda")
        ms = torch.empty((K, M, 3), dtype=torch.float64, device="cuda")
        ss = torch.empty((K, 2), dtype=torch.float64, device="cuda")
        _hip.check(lib.ddpm3d_msssim3d(_hip.ptr(xs), _hip.ptr(y), _hip.ptr(m), K, D, H, W, M, 1e-4, 9e-4,
                                       _hip.ptr(ws), ws.numel() * 8, _hip.ptr(ms), _hip.stream()))
        _hip.check(lib.ddpm3d_ssim3d(_hip.ptr(xs), _hip.ptr(y), _hip.ptr(m), K, D, H, W, 1e-4, 9e-4, _hip.ptr(ws),
                                     ws.numel() * 8, None, _hip.ptr(ss), _hip.stream()))
        assert torch.equal(ms[:, 0, [0, 2]], ss) and float(ss[0, 1]) > 0
        interior = lambda lv: math.prod(n - 10 for n in lv[0].shape) if m is None else R.interior_mask(lv[2]).sum()
        assert ms[0, :, 2].cpu().tolist() == [float(interior(lv)) for lv in c["levels"]]        # the pooled mask counts


# ------------------------------------------------------------------------------------------- repeatability
@pytest.mark.parametrize("ik", [CASE_IDS[0], CASE_IDS[3], CASE_IDS[-1]], ids=MS.case_name)
def test_msssim_is_bit_repeatable_and_batches(ik):
    c = MS.case(*ik)
    M = c["scales"]
    xs = np.stack([c["x"], R.noisy(c["y"], 0.05, seed=77), c["y"]])
    dx, dy, mask = dev(xs), dev(c["y"]), dev(c["mask"])
    for m in (None, mask):
        values, parts = metrics.msssim3d(dx, dy, 1.0, M, mask=m, parts=True)
        assert len(values) == len(parts) == 3
        assert (values, parts) == metrics.msssim3d(dx, dy, 1.0, M, mask=m, parts=True)       # twice: the same bits
        assert metrics.msssim3d(dx, dy, 1.0, M, mask=m) == values
        for i in range(3):                                                                   # three single calls
            assert metrics.msssim3d(dx[i], dy, 1.0, M, mask=m, parts=True) == (values[i], parts[i])
        assert all(abs(t - 1.0) <= 1e-6 for t in parts[2]["cs"] + [parts[2]["ssim"]])          # the identity
        assert abs(values[2] - 1.0) <= 1e-6 and values[0] != values[1] and max(values[:2]) < 0.999
    assert metrics.msssim3d(dx, dy, 1.0, M) != metrics.msssim3d(dx, dy, 1.0, M, mask=mask)


# --------------------------------------------------------------------------------------- clamp, constants
def test_negative_scales_clamp_to_zero():
    y = np.random.default_rng(5).random((24, 24, 24), dtype=np.float32)
    x = np.float32(1) - y
    want, terms = MS.msssim(x, y, 1.0, 2)
    assert terms[0] < 0 and terms[1] < 0 and want == 0.0
    got, parts = metrics.msssim3d(dev(x), dev(y), 1.0, 2, parts=True)
    assert parts["cs"][0] < 0 and parts["ssim"] < 0
    assert got == 0.0 and math.isfinite(got) and math.copysign(1.0, got) == 1.0


@pytest.mark.parametrize("shape,M", [((22, 22, 22), 2), ((24, 54, 86), 2), ((60, 44, 64), 3)])
def test_msssim_of_constants(shape, M):
    """the volumes of test_ssim_of_constants_and_of_identity at sizes that allow M scales: every CS is 1 and the result
    is constant_ssim ** w_last"""
    w = metrics.msssim_weights(M)
    for a, b, L in ((0.3, 0.7, 1.0), (2.0, 2.5, 3.0), (0.0, 1.0, 1.0), (5.0, 5.0, 1.0)):
        x = torch.full(shape, a, dtype=torch.float32, device="cuda")
        y = torch.full(shape, b, dtype=torch.float32, device="cuda")
        got, parts = metrics.msssim3d(x, y, L, M, parts=True)
        want = R.constant_ssim(np.float32(a).astype(np.float64), np.float32(b).astype(np.float64), L)
        assert all(abs(v - 1.0) <= 1e-6 for v in parts["cs"]) and abs(parts["ssim"] - want) <= 1e-6
        assert abs(got - want ** w[-1]) <= 1e-6


# ------------------------------------------------------------------------------------------------ refusals
def test_msssim_refuses_what_it_cannot_scale():
    y = dev(R.phantom((24, 40, 40)))
    for bad in (0, 6, -1, 2.0, True):
        with pytest.raises(ValueError, match="scales"):
            metrics.msssim3d(y, y, 1.0, bad)
    small = dev(R.phantom((21, 40, 40)))
    with pytest.raises(ValueError, match="at most 1"):
        metrics.msssim3d(small, small, 1.0, 2)
    assert metrics.msssim3d(small, small, 1.0, 1) == metrics.ssim3d(small, small, 1.0)
    for bad in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="data_range"):
            metrics.msssim3d(y, y, bad, 2)
    for bad in ([1.0], [0.5, 0.25, 0.25], [0.5, -0.5], [0.5, float("nan")], [0.5, float("inf")], 0.5):
        with pytest.raises(ValueError, match="weights"):
            metrics.msssim3d(y, y, 1.0, 2, weights=bad)
    x = dev(R.noisy(R.phantom((24, 40, 40)), 0.1))
    value, parts = metrics.msssim3d(x, y, 1.0, 2, weights=[0.0, 2.0], parts=True)
    assert value == parts["ssim"] ** 2.0
    # one counted voxel in the interior of scale 0: 1 of 8 at scale 1, where it is not counted
    mask = torch.zeros((24, 40, 40), dtype=torch.uint8, device="cuda")
    mask[12, 20, 20] = 1
    assert isinstance(metrics.msssim3d(x, y, 1.0, 1, mask=mask), float)
    with pytest.raises(ValueError, match="no interior voxel at scale 1"):
        metrics.msssim3d(x, y, 1.0, 2, mask=mask)
    with pytest.raises(ValueError, match="no interior voxel at scale 0"):
        metrics.msssim3d(x, y, 1.0, 2, mask=torch.zeros_like(mask))


def test_evaluate_adds_msssim_on_request():
    c = MS.case(0, 1)
    x, y, mask = dev(c["x"]), dev(c["y"]), dev(c["mask"])
    plain = metrics.evaluate(x, y, mask=mask)
    more = metrics.evaluate(x, y, mask=mask, msssim_scales=3)
    assert set(plain) == {"psnr", "nrmse", "mae", "bias", "ssim", "data_range", "n_voxels"}
    assert set(more) == set(plain) | {"msssim"} and {k: more[k] for k in plain} == plain
    assert more["msssim"] == metrics.msssim3d(x, y, plain["data_range"], 3, mask=mask)
    both = metrics.evaluate(dev(np.stack([c["x"], c["y"]])), y, data_range=1.0, msssim_scales=2)
    assert len(both["msssim"]) == 2 and abs(both["msssim"][1] - 1.0) <= 1e-6 and both["msssim"][0] < 0.999


# ------------------------------------------------------------------------------------------ the script
FLAGS = ("--large_size 16 --small_size 16 --num_channels 32 --num_res_blocks 1 --num_head_channels 64 "
         "--attention_resolutions 1000 --learn_sigma True --resblock_updown True --use_scale_shift_norm True "
         "--timestep_respacing 3").split()


def _script():
    spec = importlib.util.spec_from_file_location("ddpm3d_infer_entry", os.path.join(PKG, "scripts", "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_script_adds_msssim_to_its_rows(tmp_path):
    target = R.phantom((24, 40, 40), seed=4)                               # (D, H, W): every extent at least 22
    low = R.noisy(target, 0.1, seed=4)
    np.savez(tmp_path / "pet.npz", low)
    np.savez(tmp_path / "full.npz", target)
    mod = _script()
    common = FLAGS + ["--base_samples", str(tmp_path / "pet.npz"), "--target_samples", str(tmp_path / "full.npz"),
                      "--metrics_mask_threshold", "0.1", "--baseline_nlm_h", "0.1"]
    plain = mod.main(common + ["--save_dir", str(tmp_path / "plain")])
    path = mod.main(common + ["--save_dir", str(tmp_path / "scored"), "--msssim_scales", "2"])
    assert open(plain, "rb").read() == open(path, "rb").read()             # the .npz: byte for byte as without
    old = json.load(open(tmp_path / "plain" / "metrics_pet.json"))
    rep = json.load(open(tmp_path / "scored" / "metrics_pet.json"))
    row = {"psnr", "nrmse", "mae", "bias", "ssim", "data_range", "n_voxels"}
    assert set(old) == {"denoised", "input", "target", "mask_threshold", "baselines"}          # the old key sets
    assert set(old["denoised"]) == set(old["input"]) == row and set(old["baselines"]) == {"nlm"}
    assert set(rep) == set(old) | {"msssim_scales", "msssim_weights"}
    assert rep["msssim_scales"] == 2 and rep["msssim_weights"] == list(metrics.msssim_weights(2))
    assert set(rep["denoised"]) == set(rep["input"]) == row | {"msssim"}
    assert set(rep["baselines"]["nlm"]) == set(old["baselines"]["nlm"]) | {"msssim"}
    for name in ("denoised", "input"):
        assert {k: v for k, v in rep[name].items() if k != "msssim"} == old[name]
    log = open(tmp_path / "scored" / "log.txt").read()
    assert log.count("MS-SSIM") == 3 and "MS-SSIM" not in open(tmp_path / "plain" / "log.txt").read()

    arr = np.load(path)["arr_0"]                                           # (H, W, Z)
    tgt, inp = target.transpose(1, 2, 0), low.transpose(1, 2, 0)
    counted = tgt > np.float32(0.1) * tgt.max()
    counted[[0, -1]] = False                                               # Hann weight 0: the outermost planes
    counted[:, [0, -1]] = False
    counted[:, :, [0, -1]] = False
    mask = dev(counted.astype(np.uint8))
    L = rep["input"]["data_range"]
    for name, vol in (("denoised", arr), ("input", inp)):
        want = metrics.msssim3d(dev(vol), dev(tgt), L, 2, mask=mask)
        assert abs(rep[name]["msssim"] - want) <= 1e-12 and 0 <= want < 1, (name, rep[name]["msssim"], want)
    assert rep["input"]["msssim"] > 0.5
    # the input row against the host yardstick
    ref, terms = MS.msssim(inp, tgt, L, 2, counted.astype(np.uint8))
    e = max(MS.e32_per_scale(MS.pyramid(inp, tgt, None, 2), L))
    assert abs(rep["input"]["msssim"] - ref) <= MS.first_order_bound(ref, terms, MS.weights(2), e)
