"""
scripts/test.py --model_spacing / --regrid_mode on the tiny synthetic model of test_gpu_script.py:
a 16 x 20 x 20 phantom of 3 x 4 x 4 mm voxels is sampled on the 24 x 40 x 40 grid of 2 mm voxels those tests run.  Equal
spacings give the run without the flags; on the one-shot path, --patch_overlap and --joint_patches the flagged run
equals, bit for bit, regrid.apply forward, the script without flags on that volume and regrid.apply back; with
--num_draws the std is the moments of the back-regridded draws; the metrics file gains "regrid", keeps its "input"
row and counts keep_after's voxels.
"""

import importlib.util
import json
import os
import zipfile

import numpy as np
import pytest
import torch

from conftest import PKG
from guided_diffusion import patches, regrid, uncertainty
from test_gpu_script import FLAGS

pytestmark = pytest.mark.gpu

NATIVE, MODEL_GRID = (16, 20, 20), (24, 40, 40)
COARSE = ["--voxel_spacing", "3", "4", "4"]
FINE = ["--model_spacing", "2", "2", "2"]
PATHS = {"one_shot": [], "sliding": ["--patch_overlap", "6"], "joint": ["--joint_patches", "True"]}


def _script():
    spec = importlib.util.spec_from_file_location("ddpm3d_infer_entry", os.path.join(PKG, "scripts", "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run(src, save, *extra, mod=None):
    path = (mod or _script()).main(FLAGS + ["--base_samples", str(src), "--save_dir", str(save)] + list(extra))
    return path


def _plan(mode="linear"):
    return regrid.plan(NATIVE, MODEL_GRID, mode)


def _back(arr_hwz, plan):
    """a written (H, W, Z) array on the model's grid -> the file's grid, by hand"""
    t = torch.from_numpy(np.ascontiguousarray(arr_hwz)).cuda().permute(2, 0, 1).contiguous()
    return regrid.apply(t, plan.inverse()).permute(1, 2, 0).contiguous().cpu().numpy()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """the phantom, a full-dose target beside it, and the phantom regridded forward by hand (linear and cubic)"""
    d = tmp_path_factory.mktemp("regrid_script")
    rng = np.random.default_rng(5)
    target = rng.random(NATIVE, dtype=np.float32)
    vol = (target + 0.1 * rng.standard_normal(NATIVE).astype(np.float32)).astype(np.float32)
    np.savez(d / "pet.npz", vol)
    np.savez(d / "full.npz", target)
    out = {"dir": d, "vol": vol, "src": d / "pet.npz", "target": d / "full.npz"}
    for mode in ("linear", "cubic"):
        fwd = regrid.apply(torch.from_numpy(vol).cuda(), _plan(mode)).cpu().numpy()
        assert fwd.shape == MODEL_GRID
        np.savez(d / ("pet_%s.npz" % mode), fwd)
        out[mode] = d / ("pet_%s.npz" % mode)
    return out


def _members(path):
    with zipfile.ZipFile(path) as z:
        return {n: z.read(n) for n in z.namelist()}


def test_equal_spacings_give_the_run_without_the_flags(files, tmp_path):
    target = ["--target_samples", str(files["target"])]
    plain = _run(files["src"], tmp_path / "plain", *target)
    same = _run(files["src"], tmp_path / "same", *target, *COARSE, "--model_spacing", "3", "4", "4")
    assert _members(plain) == _members(same) and set(_members(plain)) == {"arr_0.npy"}      # every byte of every array
    a = json.load(open(tmp_path / "plain" / "metrics_pet.json"))
    b = json.load(open(tmp_path / "same" / "metrics_pet.json"))
    assert b.pop("regrid") == {"voxel_spacing": [3.0, 4.0, 4.0], "model_spacing": [3.0, 4.0, 4.0], "mode": "linear",
                               "native_shape": [16, 20, 20], "model_shape": [16, 20, 20],
                               "effective_spacing": [3.0, 4.0, 4.0]}
    assert a == b and "regrid" not in a
    # and with --num_draws, whose mean and std then come from the stitcher as before
    plain = _run(files["src"], tmp_path / "plain2", "--num_draws", "2")
    same = _run(files["src"], tmp_path / "same2", "--num_draws", "2", *COARSE, "--model_spacing", "3", "4", "4")
    assert _members(plain) == _members(same) and set(_members(plain)) == {"arr_0.npy", "std.npy"}


@pytest.mark.parametrize("path,mode", [("one_shot", "linear"), ("one_shot", "cubic"), ("sliding", "linear"),
                                       ("joint", "cubic")])
def test_flagged_run_equals_forward_script_back(files, tmp_path, path, mode):
    flagged = np.load(_run(files["src"], tmp_path / "flagged", *COARSE, *FINE, "--regrid_mode", mode, *PATHS[path]))
    by_hand = np.load(_run(files[mode], tmp_path / "by_hand", *PATHS[path]))
    assert by_hand["arr_0"].shape == (40, 40, 24) and flagged.files == ["arr_0"]
    want = _back(by_hand["arr_0"], _plan(mode))
    got = flagged["arr_0"]
    assert got.shape == (20, 20, 16) and got.dtype == np.float32 and np.abs(got).max() > 0
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    log = open(tmp_path / "flagged" / "log.txt").read()
    assert "regridding (16, 20, 20)" in log and "(24, 40, 40)" in log and mode in log


def test_tif_input_is_written_at_the_native_shape(files, tmp_path):
    from guided_diffusion import tiff_io
    src = tmp_path / "pet.tif"
    tiff_io.imwrite(str(src), files["vol"])
    out = _run(src, tmp_path / "o", *COARSE, *FINE)
    arr = np.load(out)["arr_0"]
    tif = tiff_io.imread(out.replace(".npz", ".tif"))
    assert arr.shape == (20, 20, 16) and tif.shape == NATIVE and np.array_equal(tif, arr.transpose(2, 0, 1))


@pytest.mark.parametrize("path", ["one_shot", "sliding", "joint"])
def test_draws_come_back_as_one_stack_and_the_std_is_their_moments(files, tmp_path, path, monkeypatch):
    mod = _script()
    seen = []
    real = mod.regrid.apply

    def spy(volume, plan):
        out = real(volume, plan)
        if volume.dim() == 4:
            seen.append((volume.clone(), plan, out.clone()))
        return out

    monkeypatch.setattr(mod.regrid, "apply", spy)
    out = np.load(_run(files["src"], tmp_path / "flagged", *COARSE, *FINE, "--num_draws", "2", *PATHS[path], mod=mod))
    monkeypatch.undo()
    assert len(seen) == 1                                               # the K draws went back as one stack
    stack, plan, back = seen[0]
    assert tuple(stack.shape) == (2,) + MODEL_GRID and plan.shape_out == NATIVE and plan.shape_in == MODEL_GRID
    assert torch.equal(back.view(torch.int32), regrid.apply(stack, _plan().inverse()).view(torch.int32))
    # mean and std are ddpm3d_draw_moments of the draws on the file's grid
    layout = (lambda t: t.permute(0, 2, 3, 1).contiguous()) if path != "joint" else (lambda t: t)
    mean, std = uncertainty.draw_moments(layout(back))
    hwz = (lambda t: t) if path != "joint" else (lambda t: t.permute(1, 2, 0))
    assert out["arr_0"].shape == out["std"].shape == (20, 20, 16)
    assert np.array_equal(out["arr_0"], hwz(mean).cpu().numpy()) and np.array_equal(out["std"], hwz(std).cpu().numpy())
    assert out["std"].max() > 0
    # they are the draws of the run without the flags on the volume regridded by hand: its mean is theirs
    plain = np.load(_run(files["linear"], tmp_path / "by_hand", "--num_draws", "2", *PATHS[path]))
    model_mean = stack.mean(dim=0).permute(1, 2, 0).cpu().numpy()
    assert np.abs(model_mean - plain["arr_0"]).max() <= 1e-5 * np.abs(plain["arr_0"]).max()
    # and the std of regridded draws is not the regridded std
    assert not np.array_equal(out["std"], _back(plain["std"], _plan()))


def test_metrics_stay_on_the_native_grid(files, tmp_path):
    target = ["--target_samples", str(files["target"])]
    _run(files["src"], tmp_path / "plain", *target)
    out = _run(files["src"], tmp_path / "flagged", *target, *COARSE, *FINE)
    a = json.load(open(tmp_path / "plain" / "metrics_pet.json"))
    b = json.load(open(tmp_path / "flagged" / "metrics_pet.json"))
    assert b["regrid"] == {"voxel_spacing": [3.0, 4.0, 4.0], "model_spacing": [2.0, 2.0, 2.0], "mode": "linear",
                           "native_shape": [16, 20, 20], "model_shape": [24, 40, 40],
                           "effective_spacing": pytest.approx([2.0, 2.0, 2.0], rel=1e-15)}
    # the blend's weight-0 voxels on the model's grid, carried back: what both rows count
    res = 16
    cover = patches.blend_cover(patches.patch_grid(MODEL_GRID, res), MODEL_GRID, res)          # (H, W, Z) bool
    live = torch.from_numpy(cover.astype(np.uint8)).cuda().permute(2, 0, 1).contiguous()
    keep = regrid.keep_after(live, _plan().inverse())
    n = int(keep.sum())
    assert 0 < n < 16 * 20 * 20 and b["denoised"]["n_voxels"] == b["input"]["n_voxels"] == n
    assert np.load(out)["arr_0"].shape == (20, 20, 16)
    # here those are the voxels off the volume's faces, which is what the blend of a run without the flags leaves out
    # too (every extent holds a whole patch): the input row is that run's, figure for figure
    assert n == 14 * 18 * 18 == a["input"]["n_voxels"] and a["input"] == b["input"]
    assert a["denoised"] != b["denoised"]
    assert a["target"] == b["target"] and a["mask_threshold"] == b["mask_threshold"]


def test_regions_and_baselines_ride_along(files, tmp_path):
    """--roi_threshold_frac segments the native target under keep_after's mask; the Gaussian baseline filters the native
    input; --voxel_spacing serves them and the regridding at once"""
    out = _run(files["src"], tmp_path / "o", "--target_samples", str(files["target"]), *COARSE, *FINE,
               "--roi_threshold_frac", "0.9", "--baseline_gaussian_fwhm", "6", "--num_draws", "2")
    m = json.load(open(tmp_path / "o" / "metrics_pet.json"))
    assert m["regrid"]["model_shape"] == [24, 40, 40] and "gaussian" in m["baselines"] and m["roi"]["regions"]
    labels = np.load(tmp_path / "o" / "roi_labels_pet.npz")["arr_0"]
    assert labels.shape == NATIVE and labels.max() > 0
    z = np.load(out)
    assert z["arr_0"].shape == z["std"].shape == (20, 20, 16)
    region = next(iter(m["roi"]["regions"].values()))
    assert "peak" in region["target"] and "mean_std" in region["denoised"]
