"""
Fixtures of tests/test_gpu_script_paths.py: what scripts/test.py writes on each of its paths (fixed grid, sliding
grid, joint; one draw and K draws; regridding, quantiles, keyed noise, the three samplers, .tif input) for small
seeded volumes.  Run by hand on a GPU, from a commit whose output is to be held:

    python tests/golden/make_script_paths.py [--out DIR]          # default: tests/golden

writes script_paths.npz (every array of every written .npz as "<case>/<file>/<key>", every written .tif decoded as
"<case>/<file>") and script_paths.json ({"files": {case: sorted names in --save_dir}, "json": {case: {file: parsed
metrics_*.json / trace_*.json}}}; path-valued fields reduced to their basename).  The test module imports CASES,
write_inputs and collect from here, so the fixture and the test cannot drift apart.

Flags the script's own argument checks refuse are left out of a case: the sliding cases of (10, 44, 20) carry no
--target_samples (the 3-D SSIM needs every extent >= 11); slide_1t and slide_2t, on (12, 20, 18), score the sliding
grid against a target instead.
"""

import argparse
import importlib.util
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
PKG = os.path.join(ROOT, "3d-denoising-diffusion-model_amd")

# tests/test_gpu_script.py::FLAGS without the respacing, which three cases change
NET = ("--large_size 16 --small_size 16 --num_channels 32 --num_res_blocks 1 --num_head_channels 64 "
       "--attention_resolutions 1000 --learn_sigma True --resblock_updown True --use_scale_shift_norm True").split()
VOLUME_SEED, TARGET_SEED = 40, 41
PATH_FIELDS = ("target", "labels")

# name: (shape (D, H, W), flags beyond the common ones, with --target_samples, --timestep_respacing, input suffix)
CASES = {
    "fixed_1": ((18, 24, 20), "--batch_size 4 --metrics_mask_threshold 0.1 --roi_threshold_frac 0.6 "
                              "--voxel_spacing 2 2 2 --msssim_scales 1 --trace True", True, "3", ".npz"),
    "fixed_3q": ((18, 24, 20), "--num_draws 3 --batch_size 4 --draw_quantiles 0.1 0.5 0.9 --trace True",
                 True, "3", ".npz"),
    "fixed_thin": ((10, 24, 20), "", False, "3", ".npz"),
    "slide_1": ((10, 44, 20), "--patch_overlap 4 --batch_size 3 --trace True", False, "3", ".npz"),
    "slide_3q": ((10, 44, 20), "--patch_overlap 4 --num_draws 3 --draw_quantiles 0.25 0.75", False, "3", ".npz"),
    "slide_1t": ((12, 20, 18), "--patch_overlap 4 --batch_size 3 --trace True", True, "3", ".npz"),
    "slide_2t": ((12, 20, 18), "--patch_overlap 4 --num_draws 2 --batch_size 3 --draw_quantiles 0.25 0.75",
                 True, "3", ".npz"),
    "regrid_fixed_2": ((18, 24, 20), "--num_draws 2 --voxel_spacing 2 2 2 --model_spacing 2 2.5 2 "
                                     "--draw_quantiles 0.5", True, "3", ".npz"),
    "regrid_slide_1": ((10, 44, 20), "--patch_overlap 4 --voxel_spacing 2 2 2 --model_spacing 2 2.5 2",
                       False, "3", ".npz"),
    "joint_1": ((18, 24, 20), "--joint_patches True --trace True", True, "3", ".npz"),
    "joint_2q": ((18, 24, 20), "--joint_patches True --num_draws 2 --draw_quantiles 0.5", True, "3", ".npz"),
    "keyed_fixed_2": ((18, 24, 20), "--device_noise True --noise_seed 11 --num_draws 2", False, "3", ".npz"),
    "ddim_fixed": ((16, 24, 20), "--use_ddim True --eta 0.5", False, "ddim3", ".npz"),
    "dpm_slide": ((10, 44, 20), "--use_dpm_solver True --patch_overlap 4", False, "logsnr3", ".npz"),
    "tif_2": ((18, 24, 20), "--num_draws 2", False, "3", ".tif"),
}


def load_script():
    spec = importlib.util.spec_from_file_location("ddpm3d_infer_entry", os.path.join(PKG, "scripts", "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def write_inputs(case, directory):
    """Writes the case's seeded input (and target) into `directory` -> the script's argv but for --save_dir"""
    shape, flags, with_target, respacing, suffix = CASES[case]
    os.makedirs(directory, exist_ok=True)
    vol = np.random.default_rng(VOLUME_SEED).random(shape, dtype=np.float32)
    src = os.path.join(directory, "pet" + suffix)
    if suffix == ".tif":
        if PKG not in sys.path:
            sys.path.insert(0, PKG)
        from guided_diffusion import tiff_io
        tiff_io.imwrite(src, (vol * 4000).astype(np.uint16))
    else:
        np.savez(src, vol)
    argv = NET + ["--timestep_respacing", respacing, "--base_samples", src] + flags.split()
    if with_target:
        tgt = os.path.join(directory, "full_dose.npz")
        np.savez(tgt, np.random.default_rng(TARGET_SEED).random(shape, dtype=np.float32))
        argv += ["--target_samples", tgt]
    return argv


def _basenames(node):
    if isinstance(node, dict):
        return {k: os.path.basename(v) if k in PATH_FIELDS and isinstance(v, str) else _basenames(v)
                for k, v in node.items()}
    if isinstance(node, list):
        return [_basenames(v) for v in node]
    return node


def collect(save_dir):
    """What a run left in its --save_dir -> (sorted file names, {"<file>/<key>" | "<tif file>": array},
    {"<json file>": parsed, path fields as basenames}).  log.txt is listed, not read."""
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    from guided_diffusion import tiff_io
    files = sorted(os.listdir(save_dir))
    arrays, parsed = {}, {}
    for name in files:
        path = os.path.join(save_dir, name)
        if name.endswith(".npz"):
            with np.load(path) as z:
                for key in z.files:
                    arrays["%s/%s" % (name, key)] = z[key]
        elif name.endswith(".tif"):
            arrays[name] = tiff_io.imread(path)
        elif name.endswith(".json"):
            with open(path) as f:
                parsed[name] = _basenames(json.load(f))
    return files, arrays, parsed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    out = ap.parse_args().out
    os.makedirs(out, exist_ok=True)
    arrays, report = {}, {"files": {}, "json": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for case in CASES:
            argv = write_inputs(case, os.path.join(tmp, case, "in"))
            save = os.path.join(tmp, case, "out")
            load_script().main(argv + ["--save_dir", save])
            files, arrs, parsed = collect(save)
            report["files"][case], report["json"][case] = files, parsed
            arrays.update({"%s/%s" % (case, k): v for k, v in arrs.items()})
            print("%-16s %s" % (case, " ".join(files)), flush=True)
    np.savez_compressed(os.path.join(out, "script_paths.npz"), **arrays)
    with open(os.path.join(out, "script_paths.json"), "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d arrays of %d cases to %s" % (len(arrays), len(CASES), out))


if __name__ == "__main__":
    main()
