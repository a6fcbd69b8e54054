"""
GPU tier of the per-region statistics: ddpm3d_roi_moments against the exact sums of tests/roi_ref.py
under the derived summation bound (regions of 1, 1, 4095, 4096 and 4097 voxels on a 24 x 20 x 28 volume, contiguous
and scattered, B = 1 and 3, with and without a target, with and without an offset of 1000), an empty region through
the C entry, bit-repeatability and batching, the index against np.nonzero, roi_report against roi_figures of the
yardstick's sums, one device-to-host copy per call, and the inference script's --roi_labels on three of its paths.
"""

import ctypes
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import roi_ref as R
from conftest import PKG
from guided_diffusion import _hip, metrics

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module", params=[False, True], ids=["runs", "scattered"])
def case(request):
    """labels, the host lists and the device index of one label volume: built once, never changed"""
    labels = R.labels_volume(request.param)
    found, lists = R.region_lists(labels)
    return labels, found, lists, metrics.roi_index(dev(labels))


# ------------------------------------------------------------------------------------------ the index
def test_index_holds_the_voxels_np_nonzero_finds(case):
    labels, found, lists, index = case
    assert index.labels == found == sorted(R.SIZES) and index.counts == [R.SIZES[v] for v in found]
    assert index.shape == R.SHAPE and index.voxels == labels.size and len(index) == 5
    flat = index.index.cpu().numpy()
    assert flat.dtype == np.int64 and index.offsets == [0] + list(np.cumsum(index.counts))
    for r, at in enumerate(lists):
        assert np.array_equal(flat[index.offsets[r]:index.offsets[r + 1]], at)
    assert flat[0] == 0 and flat[1] == labels.size - 1                     # labels 1 and 2: the first and last voxel


def test_index_applies_keep_and_takes_any_integer_dtype(case):
    labels = case[0]
    keep = (np.random.default_rng(3).random(R.SHAPE) < 0.6).astype(np.uint8)
    keep.reshape(-1)[0] = 0                                                # label 1 loses its only voxel: no region
    keep.reshape(-1)[-1] = 1                                               # label 2 keeps its only voxel
    found, lists = R.region_lists(labels, keep)
    assert found == [2, 7, 300, 4000]
    for dtype in (torch.int32, torch.int64, torch.int16):
        index = metrics.roi_index(dev(labels).to(dtype), keep=dev(keep))
        assert index.labels == found and index.counts == [len(a) for a in lists]
        flat = index.index.cpu().numpy()
        for r, at in enumerate(lists):
            assert np.array_equal(flat[index.offsets[r]:index.offsets[r + 1]], at)


def test_index_refuses_what_it_cannot_take():
    lab = torch.zeros(R.SHAPE, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="no labelled voxel"):
        metrics.roi_index(lab)
    with pytest.raises(ValueError, match="integer"):
        metrics.roi_index(lab.float())
    with pytest.raises(ValueError, match="negative"):
        metrics.roi_index(lab - 1)
    many = torch.arange(lab.numel(), dtype=torch.int32, device="cuda").reshape(R.SHAPE)
    with pytest.raises(ValueError, match="regions"):
        metrics.roi_index(many)
    many[many > _hip.ROI_MAX_REGIONS] = 0
    assert len(metrics.roi_index(many)) == _hip.ROI_MAX_REGIONS
    with pytest.raises(ValueError, match="keep"):
        metrics.roi_index(many, keep=torch.ones(R.SHAPE, device="cuda"))
    one = lab.clone()
    one[1, 2, 3] = 9
    with pytest.raises(ValueError, match="no labelled voxel"):
        metrics.roi_index(one, keep=(one == 0).to(torch.uint8))


# ------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("offset", [0.0, 1000.0])
@pytest.mark.parametrize("with_target", [False, True], ids=["alone", "target"])
def test_moments_match_the_exact_sums(case, with_target, offset):
    labels, found, lists, index = case
    xs, y = R.volumes(offset)
    ty = y if with_target else None
    dy = dev(y) if with_target else None
    batch = metrics.roi_moments(dev(xs), index, target=dy)
    assert len(batch) == 3 and all(len(b) == 5 and len(b[0]) == _hip.ROI_REC for b in batch)
    for i in range(3):
        want, bounds = R.moments(xs[i], lists, ty), R.bound(xs[i], lists, ty)
        worst = max(abs(g[k] - w[k]) / b[k] for g, w, b in zip(batch[i], want, bounds) for k in R.SUMS if b[k] > 0)
        print("estimate %d: largest deviation %.3g of its bound" % (i, worst))
        R.check(batch[i], want, bounds)
        if not with_target:
            assert all(rec[R.SUM_E:] == [0.0, 0.0, 0.0] for rec in batch[i])
        single = metrics.roi_moments(dev(xs[i]), index, target=dy)                 # B = 1
        assert single == batch[i]                                                  # row b of the stack, bitwise
    assert batch[0] != batch[1]
    assert metrics.roi_moments(dev(xs), index, target=dy) == batch                 # twice: the same bits


def test_an_empty_region_through_the_c_entry(case):
    """offsets by hand: regions of 5, 0, 4097 and 0 entries of the index's own list"""
    labels, found, lists, index = case
    xs, y = R.volumes()
    offsets = [0, 5, 5, 4102, 4102]
    chunks = [0, 1, 1, 3, 3]
    host = (ctypes.c_int64 * 5)(*offsets)
    tab = torch.tensor([offsets, chunks], dtype=torch.int64).cuda()
    desc = _hip.RoiIndex(4, 4102, host, _hip.ptr(tab[0]), _hip.ptr(tab[1]), _hip.ptr(index.index))
    lib = _hip.load()
    need = lib.ddpm3d_roi_moments_workspace_bytes(2, desc)
    assert need == 2 * 3 * _hip.ROI_REC * 8
    ws = torch.empty(need // 8, dtype=torch.float64, device="cuda")
    out = torch.full((2, 4, _hip.ROI_REC), 7.0, dtype=torch.float64, device="cuda")
    x, t = dev(xs[:2]), dev(y)
    _hip.check(lib.ddpm3d_roi_moments(_hip.ptr(x), _hip.ptr(t), 2, index.voxels, desc, _hip.ptr(ws), need,
                                      _hip.ptr(out), _hip.stream()))
    got = out.cpu().tolist()
    flat = index.index.cpu().numpy()
    mine = [flat[0:5], flat[5:5], flat[5:4102], flat[4102:4102]]
    inf = float("inf")
    for b in range(2):
        R.check(got[b], R.moments(xs[b], mine, y), R.bound(xs[b], mine, y))
        assert got[b][1] == got[b][3] == [0.0, 0.0, 0.0, inf, -inf, 0.0, 0.0, 0.0]
        assert got[b][2][R.N] == 4097


def test_arguments_that_do_not_fit_the_index_are_refused(case):
    index = case[3]
    x = torch.zeros(R.SHAPE, device="cuda")
    with pytest.raises(ValueError):
        metrics.roi_moments(x[:, :, :27].contiguous(), index)
    with pytest.raises(ValueError):
        metrics.roi_moments(x, index, target=x[:23].contiguous())
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        metrics.roi_moments(x.cpu(), index)
    with pytest.raises(ValueError):
        metrics.roi_moments(torch.zeros((65,) + R.SHAPE, device="cuda"), index)


def test_one_device_to_host_copy_per_call(case):
    """under torch's sync debug mode every blocking call warns: roi_moments makes one, the copy of the records"""
    index = case[3]
    xs, y = R.volumes()
    x, t = dev(xs), dev(y)
    metrics.roi_moments(x, index, target=t)                                        # the library is loaded
    torch.cuda.synchronize()
    import warnings
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            metrics.roi_moments(x, index, target=t)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    blocking = [w for w in seen if "synchroniz" in str(w.message).lower()]
    assert len(blocking) == 1, [str(w.message) for w in seen]


# ------------------------------------------------------------------------------------------ the report
def _close(got, want, path=""):
    """two nested figure dicts: the same keys, None where None, numbers to 1e-12 relative"""
    if isinstance(want, dict):
        assert isinstance(got, dict) and set(got) == set(want), (path, sorted(got), sorted(want))
        for k in want:
            _close(got[k], want[k], "%s/%s" % (path, k))
    elif isinstance(want, list):
        assert len(got) == len(want), path
        for i, (g, w) in enumerate(zip(got, want)):
            _close(g, w, "%s[%d]" % (path, i))
    elif want is None or isinstance(want, int):
        assert got == want, (path, got, want)
    else:
        assert abs(got - want) <= 1e-12 * abs(want), (path, got, want)


def test_report_is_the_figures_of_the_exact_sums(case):
    """every figure to 1e-12 relative.  The sums themselves agree far inside that; the figures that are differences
    of them (bias, contrast, the spread of the draw means) stay conditioned because the data are PET-like: positive,
    regions of different uptake, estimates with a bias of their own (roi_ref.report_volumes)."""
    labels, found, lists, index = case
    xs, y = R.report_volumes(labels)
    mean = xs.mean(axis=0, dtype=np.float64).astype(np.float32)
    got = metrics.roi_report(dev(mean), dev(y), index, background=300, draws=dev(xs))
    trec = R.moments(y, lists)
    want_e = metrics.roi_figures(R.moments(mean, lists, y), target_records=trec, labels=found, background=300,
                                 draw_records=[R.moments(x, lists) for x in xs])
    want_t = metrics.roi_figures(trec, labels=found)
    assert list(got) == found
    for label in found:
        assert set(got[label]) == {"n", "target", "estimate"} and got[label]["n"] == R.SIZES[label]
        _close(got[label]["target"], want_t[label], "%d/target" % label)
        _close(got[label]["estimate"], want_e[label], "%d/estimate" % label)
    lesion = got[7]["estimate"]
    assert len(lesion["draw_means"]) == 3 and lesion["mean_std"] > 0 and lesion["cnr"] > 1 and lesion["crc"] > 0
    assert abs(lesion["mean_std"] - np.std(lesion["draw_means"], ddof=1)) <= 1e-12 * lesion["mean_std"]
    assert "contrast" not in got[300]["estimate"] and "mean_z" in got[300]["estimate"]
    by_records = metrics.roi_report(dev(mean), dev(y), index, background=300,
                                    draws=[metrics.roi_moments(dev(x), index) for x in xs])
    assert by_records == got                                               # draws as records: the same report


# ------------------------------------------------------------------------------------------ the script
FLAGS = ("--large_size 16 --small_size 16 --num_channels 32 --num_res_blocks 1 --num_head_channels 64 "
         "--attention_resolutions 1000 --learn_sigma True --resblock_updown True --use_scale_shift_norm True "
         "--timestep_respacing 3").split()
BASE_KEYS = {"n", "mean", "std", "min", "max", "cov"}
VS_TARGET = BASE_KEYS | {"mean_bias", "mean_bias_rel", "max_bias_rel", "rmse", "mae"}
DRAW_KEYS = {"draw_means", "mean_std", "mean_z"}


def _script():
    spec = importlib.util.spec_from_file_location("ddpm3d_infer_entry", os.path.join(PKG, "scripts", "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _script_labels(shape):
    lab = np.zeros(shape, dtype=np.int32)                                   # (D, H, W)
    lab[8:12, 18:23, 17:22] = 3                                              # a lesion inside
    lab[0:3, 0:6, 0:5] = 11                                                  # a corner: touches three outer planes
    lab[5:15, 5:15, 25:35] = 40                                              # an organ, the reference region
    lab[19, 10:14, 10:14] = 41                                               # wholly on the last plane along depth
    return lab


@pytest.mark.parametrize("extra,draws", [([], 0), (["--joint_patches", "True", "--num_draws", "3"], 3),
                                         (["--patch_overlap", "4", "--num_draws", "2"], 2)],
                         ids=["one-shot", "joint-draws", "sliding-draws"])
def test_script_writes_region_statistics(extra, draws, tmp_path):
    import metrics_ref
    target = metrics_ref.phantom((20, 40, 40), seed=4)                      # (D, H, W): 3 x 3 x 2 patches of 16^3
    low = metrics_ref.noisy(target, 0.1, seed=4)
    labels = _script_labels(target.shape)
    np.savez(tmp_path / "pet.npz", low)
    np.savez(tmp_path / "full.npz", target)
    np.save(tmp_path / "lab.npy", labels)
    mod = _script()
    common = FLAGS + ["--base_samples", str(tmp_path / "pet.npz"), "--target_samples", str(tmp_path / "full.npz")]
    common += extra
    path = mod.main(common + ["--save_dir", str(tmp_path / "roi"), "--roi_labels", str(tmp_path / "lab.npy"),
                              "--roi_background", "40"])
    rep = json.load(open(tmp_path / "roi" / "metrics_pet.json"))
    assert set(rep) == {"denoised", "input", "target", "mask_threshold", "roi"}
    if not draws:                                                          # without the flag: today's file
        plain = mod.main(common + ["--save_dir", str(tmp_path / "plain")])
        assert open(plain, "rb").read() == open(path, "rb").read()
        old = json.load(open(tmp_path / "plain" / "metrics_pet.json"))
        assert set(old) == {"denoised", "input", "target", "mask_threshold"}
        assert old == {k: v for k, v in rep.items() if k != "roi"}
    roi = rep["roi"]
    assert set(roi) == {"labels", "background", "regions"}
    assert roi["labels"] == str(tmp_path / "lab.npy") and roi["background"] == 40

    out = np.load(path)
    arr, tgt, inp = out["arr_0"], target.transpose(1, 2, 0), low.transpose(1, 2, 0)        # (H, W, Z)
    lab = np.ascontiguousarray(labels.transpose(1, 2, 0))
    joint = "--joint_patches" in extra
    keep = np.ones(arr.shape, dtype=np.uint8)
    if not joint:                                                          # Hann weight 0: the outermost planes
        keep[[0, -1]] = 0
        keep[:, [0, -1]] = 0
        keep[:, :, [0, -1]] = 0
    sizes = {int(v): int(((lab == v) & (keep != 0)).sum()) for v in (3, 11, 40, 41)}
    if joint:
        assert sizes == {3: 100, 11: 90, 40: 1000, 41: 16}
    else:
        assert sizes == {3: 100, 11: 2 * 5 * 4, 40: 1000, 41: 0}           # the corner shrinks, label 41 is gone
    present = [v for v in (3, 11, 40, 41) if sizes[v]]
    assert list(roi["regions"]) == [str(v) for v in present]
    index = metrics.roi_index(dev(lab), keep=None if joint else dev(keep))
    want_den = metrics.roi_report(dev(arr), dev(tgt), index, background=40)
    want_inp = metrics.roi_report(dev(inp), dev(tgt), index, background=40)
    for v in present:
        r = roi["regions"][str(v)]
        assert set(r) == {"n", "target", "input", "denoised"} and r["n"] == sizes[v]
        contrast = set() if v == 40 else {"contrast", "crc", "cnr"}
        assert set(r["target"]) == BASE_KEYS and set(r["input"]) == VS_TARGET | contrast
        assert set(r["denoised"]) == VS_TARGET | contrast | (DRAW_KEYS if draws else set())
        den = {k: x for k, x in r["denoised"].items() if k not in DRAW_KEYS}
        assert r["target"] == want_den[v]["target"] and r["input"] == want_inp[v]["estimate"]
        assert den == want_den[v]["estimate"]                              # the same kernel on the same bits
        if draws:
            d = r["denoised"]
            assert len(d["draw_means"]) == draws and len(set(d["draw_means"])) == draws
            want = float(np.std(d["draw_means"], ddof=1))
            assert abs(d["mean_std"] - want) <= 1e-12 * want
            assert abs(d["mean_z"] - (np.mean(d["draw_means"]) - r["target"]["mean"]) / d["mean_std"]) <= 1e-9
            # arr_0 is the fp32-rounded mean of the draws, voxel by voxel: half an ulp of the largest voxel at most
            assert abs(np.mean(d["draw_means"]) - d["mean"]) <= 2.0 ** -23 * max(abs(d["min"]), abs(d["max"]))
