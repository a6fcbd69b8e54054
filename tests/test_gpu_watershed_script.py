"""
The inference script's --roi_split_prominence on a target of two touching blobs: one tiny run without
the flag, one with a prominence below the dimmer blob's dynamic, one above it, and one with --roi_split_fwhm.
"""

import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import watershed_ref as R
from conftest import PKG
from guided_diffusion import metrics

pytestmark = pytest.mark.gpu

FLAGS = ("--large_size 16 --small_size 16 --num_channels 32 --num_res_blocks 1 --num_head_channels 64 "
         "--attention_resolutions 1000 --learn_sigma True --resblock_updown True --use_scale_shift_norm True "
         "--timestep_respacing 2").split()
THRESHOLD = 0.3


def _script():
    spec = importlib.util.spec_from_file_location("ddpm3d_infer_entry", os.path.join(PKG, "scripts", "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_script_splits_touching_lesions(tmp_path, capsys):
    target, _ = R.two_blobs(shape=(20, 40, 40))                             # (D, H, W): 3 x 3 x 2 patches of 16^3
    low = (target + 0.05 * np.random.default_rng(3).standard_normal(target.shape)).astype(np.float32)
    np.savez(tmp_path / "pet.npz", low)
    np.savez(tmp_path / "full.npz", target)
    mod = _script()
    common = FLAGS + ["--base_samples", str(tmp_path / "pet.npz"), "--target_samples", str(tmp_path / "full.npz"),
                      "--roi_threshold", str(THRESHOLD)]

    def run(name, extra):
        mod.main(common + ["--save_dir", str(tmp_path / name)] + extra)
        roi = json.load(open(tmp_path / name / "metrics_pet.json"))["roi"]
        return roi, np.load(tmp_path / name / "roi_labels_pet.npz")["arr_0"]

    plain, plain_labels = run("plain", [])
    assert "split" not in plain and len(plain["regions"]) == 1 and "component" not in plain["regions"]["1"]
    capsys.readouterr()
    split, split_labels = run("split", ["--roi_split_prominence", "0.05"])
    assert "components -> 2 basins -> 2 regions" in capsys.readouterr().out
    assert split["split"] == {"prominence": 0.05, "fwhm_mm": 0.0, "connectivity": 26, "n_components": 1,
                              "n_basins": 2, "n_regions": 2}
    assert sorted(split["regions"]) == ["1", "2"]
    assert [split["regions"][k]["component"] for k in ("1", "2")] == [1, 1]
    assert len(split["detection"]["denoised"]["found"]) == 2
    assert {k: v for k, v in split.items() if k not in ("split", "regions", "detection", "labels")} == \
        {k: v for k, v in plain.items() if k not in ("regions", "detection", "labels")}

    # the labels file is metrics.split_components of the same inputs: the target on the script's (H, W, Z) grid, the
    # voxels the one-shot blend leaves at 0 (the outermost planes) dropped before the split
    tgt = torch.from_numpy(target).cuda().permute(1, 2, 0).contiguous()
    keep = torch.zeros(tgt.shape, dtype=torch.uint8, device="cuda")
    keep[1:-1, 1:-1, 1:-1] = 1
    lab, n = metrics.segment(tgt, float(np.float32(THRESHOLD)), keep=keep)
    want, n_want, _ = metrics.split_components(lab, tgt, 0.05)
    assert n == 1 and n_want == 2
    assert np.array_equal(split_labels, want.permute(2, 0, 1).cpu().numpy())
    assert np.array_equal(plain_labels, lab.permute(2, 0, 1).cpu().numpy())
    assert np.array_equal(split_labels > 0, plain_labels > 0)

    # above the dimmer blob's dynamic the basins merge: the unsplit run's regions
    high, high_labels = run("high", ["--roi_split_prominence", "0.5"])
    assert high["split"]["n_basins"] == 2 and high["split"]["n_regions"] == 1
    assert np.array_equal(high_labels, plain_labels)
    assert {k: v for k, v in high["regions"]["1"].items() if k != "component"} == plain["regions"]["1"]
    assert high["regions"]["1"]["component"] == 1 and high["detection"] == plain["detection"]

    # with --roi_split_fwhm the height is the target's Gaussian smoothing at that FWHM
    smooth, smooth_labels = run("smooth", ["--roi_split_prominence", "0.05", "--roi_split_fwhm", "4",
                                           "--voxel_spacing", "2", "2", "2"])
    assert smooth["split"]["fwhm_mm"] == 4.0 and smooth["split"]["n_regions"] == 2
    height = metrics.gaussian_smooth(tgt, metrics.gaussian_taps(4.0, (2.0, 2.0, 2.0)))
    want, n_want, _ = metrics.split_components(lab, height, 0.05)
    assert n_want == 2 and np.array_equal(smooth_labels, want.permute(2, 0, 1).cpu().numpy())
    assert "height smoothed at 4 mm FWHM" in capsys.readouterr().out
