"""
Inference entry point with the reference's command line (scripts/test.py:264-278
+ test_DDPM_3d_mpi.sh flags): denoise one whole-body PET volume by tiling it
into sub-volumes, sampling every sub-volume on the GPU(s) and blending the
results with a 3-D Hann window.

    python scripts/test.py --model_path ckpt.pt --base_samples vol.npz --save_dir out \
        --large_size 96 --small_size 96 --num_channels 128 --num_head_channels 64 \
        --attention_resolutions 1000 --learn_sigma True --resblock_updown True \
        --use_scale_shift_norm True --timestep_respacing 250
    python -m torch.distributed.run --nproc-per-node 8 scripts/test.py ...   # one rank per GPU (RCCL)

Differences from the reference script, all on the host side: `.npz`/`.npy`
inputs are accepted besides `.tif` (README.md:67 asks users to edit the loader;
scripts/test.py:187 rejects them); volumes need not be 200x200, but the default
tiling is the reference's fixed grid of 3 x 3 x (1 | 2) patches, which covers a
volume only up to 3 x 3 x 2 patch sizes (H, W, D): beyond that it leaves gaps
(written as 0, with one warning in the log), and `--patch_overlap N` (N in
2..patch size - 1) tiles a volume of any size without gaps instead, with as many
evenly spread patches per axis as it takes for neighbours to overlap by at
least N voxels (patches.sliding_starts; 44 extends the reference's grid for
200 x 200 volumes).  With it the volume is uploaded once and every batch's
conditioning patches are cut on the device, for all of the one-shot path,
`--num_draws` and `--joint_patches`.  On either grid the independent paths
(one draw or `--num_draws`) run one round loop, and finished patches are blended
on rank 0's device as they arrive, with the arithmetic of
patches.stitch_patches; `--use_ddim`
is honoured (the reference parses it but always runs DDPM, scripts/test.py:63);
`--use_dpm_solver True` (with `--solver_order`, `--solver_stochastic`) samples
with DPM-Solver++ instead and takes precedence over `--use_ddim`; pair it with
`--timestep_respacing logsnrN`;
ranks get an evenly padded work list (the reference hangs in all_gather on an
uneven one); `--model_path ""` uses seeded synthetic weights (no checkpoint
ships with the reference); `--num_draws K` (K >= 2) samples every patch K times
with independent noise and writes the per-voxel mean as `arr_0` and the sample
std (ddof = 1) of the K stitched volumes as `std` (plus denoised_<name>_std.tif
for .tif input): the uncertainty maps of README.md:44, which the reference
script (one draw, seed 10) cannot produce; `--joint_patches True` samples the
patches jointly (guided_diffusion/joint.py): one state and one noise draw per
voxel of the whole volume, blended after every reverse step, so that overlaps
are not an average of independent draws (which lowers `std` there in the
pattern of the patch grid).  DDPM and DDIM only.  `--device_noise True` (any
path, any sampler; `--noise_seed N`, default 10) takes all sampler noise from a
counter-based key evaluated inside the step kernels (no
generators, no noise tensors; stream = patch index + (draw << 32)); it is not
torch's stream, so the result is another draw than the default path's, which
stays byte for byte what it was.  Unlike the one-shot blend,
whose Hann weights are 0 on the outermost planes of the volume (those voxels
are written as 0), the joint path writes real values there;
`--target_samples full_dose.npz` (a volume of the input's shape) scores the
written volume and the low-dose input itself against that target on the GPU
(guided_diffusion/metrics.py: PSNR, NRMSE, MAE, bias, 3-D SSIM and, with
`--num_draws`, the coverage of the std map) and writes metrics_<name>.json
beside the .npz, which keeps its keys and contents; `--data_range` fixes L
(default: the target's range), `--metrics_mask_threshold F` counts only
voxels with target > F * max(target); `--roi_labels labels.npz` (an integer
volume of the input's shape, 0 = unlabelled; needs `--target_samples`) adds
per-region statistics of the target, the input and the written volume
(guided_diffusion/metrics.py roi_report: mean, max, CoV, bias, and with
`--roi_background LABEL` contrast recovery and contrast-to-noise against that
region; with `--num_draws` the spread of every region mean over the draws)
under the key "roi" of metrics_<name>.json; `--roi_threshold F` (absolute, in
the target's units, e.g. SUV 2.5) or `--roi_threshold_frac F` (a fraction of
the target's maximum) makes the labels instead of reading them: the target's
voxels above the threshold, grouped into connected components on the GPU
(`--roi_connectivity 6|18|26`, components of fewer than `--roi_min_voxels`
voxels dropped; guided_diffusion/metrics.py segment).  The target is segmented
before the first sampling step and the labels are written as
roi_labels_<name>.npz, which `--roi_labels` reads back; the "roi" entry is built
from them as from a file and also carries "detection": which of the target's
lesions are still there in the input and in the denoised volume (and in every
draw), and how many hot spots either has that the target has not;
`--roi_split_prominence P` (positive, in the target's units; needs a
`--roi_threshold`) splits touching lesions: every component is cut along the
watershed of the target, or of its Gaussian smoothing at `--roi_split_fwhm MM`
(needs `--voxel_spacing`), and basins whose peak stands less than P above the
saddle to a higher one are merged (guided_diffusion/metrics.py
split_components); the labels file holds the split labels, "roi" gains "split"
and every region "component", the unsplit component it came from;
`--voxel_spacing S0 S1 S2` (mm per voxel along the input file's axes (D, H, W);
needs `--target_samples` and `--roi_labels` or a `--roi_threshold`) adds to
every region's target, input and denoised figures its volume in ml (the MTV of
a lesion), its TLG = volume x mean and its SUVpeak: the largest mean of a 1 cm^3
sphere centred on a voxel of the region (guided_diffusion/metrics.py
sphere_mean, roi_peak), with their relative bias against the target and, with
`--num_draws`, the spread of the peak over the draws;
`--baseline_gaussian_fwhm MM` (needs `--target_samples` and `--voxel_spacing`,
which then needs no regions) and `--baseline_nlm_h H` (needs
`--target_samples`; `--baseline_nlm_search N`, default 3, `--baseline_nlm_patch
N`, default 1, `--baseline_nlm_sigma S`, default 0) filter the low-dose input
once on the GPU with the clinic's Gaussian post-filter of that FWHM and with
non-local means (guided_diffusion/metrics.py gaussian_smooth, nlm) and score
the two like the input and the written volume: the entry "baselines" of
metrics_<name>.json and, with regions, "gaussian" and "nlm" beside "input" in
every region.  The filtered volumes are not written;
`--roi_texture_bin W` (the fixed bin width in the target's units, e.g. 0.25 for
SUV; needs `--target_samples` and regions; `--roi_texture_levels N`, 2..64,
default 64, and `--roi_texture_lower L`, default 0) adds "texture" to every
region's target, input, baseline and denoised figures: contrast, joint entropy,
inverse difference moment and the other second-order figures of the region's
grey-level co-occurrence matrix as IBSI defines them (13 directions at distance
1, merged; guided_diffusion/metrics.py roi_texture, texture_figures), with
"texture_rel" against the target's and, with `--num_draws`, their spread over
the draws: whether the texture inside a lesion survives, which a smoothing
filter's first-order figures do not show;
`--msssim_scales N` (1..5; needs `--target_samples` and every extent to be at
least 11 after N - 1 halvings) adds "msssim", the multi-scale SSIM over N
scales (guided_diffusion/metrics.py msssim3d), to the "denoised", "input" and
baseline rows of metrics_<name>.json, and "msssim_scales" and
"msssim_weights" beside them;
`--spectrum True` (needs `--target_samples` and `--voxel_spacing`, which then
needs no regions) adds "spectrum" to the same rows: per radial frequency shell
the power of estimate, target and error, the Fourier shell correlation, the
power ratio to the target, and the resolutions in mm at FSC = 0.5 and 1/7 and
at amplitude ratio 1/2 (guided_diffusion/metrics.py shell_spectrum, one launch
for all rows and the `--num_draws` draws); `--spectrum_window hann|none`; the
one-shot blends are transformed over [1, n - 1) of each axis, where their
written zeros are no edge; the file gains a top-level "spectrum" block;
`--mip_angles N` (1..64; needs `--voxel_spacing`, which then needs neither a
target nor regions) writes mip_<name>.npz beside the .npz: the rotating
maximum-intensity projection about the input file's axis 0 at the angles
k 360 / N (guided_diffusion/metrics.py project, DESIGN.md 3.22, one launch for
all rows), each (N, D, U) float32: "denoised" and "input", with
`--target_samples` "target" and "error" (the MIP of |denoised - target|), with
`--num_draws` "std", with baselines "gaussian" and "nlm", and "angles_deg" and
"pitch_mm"; .tif input also gets mip_<name>.tif, the denoised stack; the
one-shot paths project [1, n - 1) of each axis, `--joint_patches` the whole
volume;
`--roi_boundary True` (needs `--roi_threshold` or `--roi_threshold_frac`, and
`--voxel_spacing`) adds "boundary" beside "detection": where the input's and
the denoised volume's own segmentations put the lesion boundaries against the
target's (guided_diffusion/metrics.py boundary, DESIGN.md 3.23: Dice, Jaccard,
Hausdorff distance, its 95th percentile and the average symmetric surface
distance in mm, from two exact distance transforms on the GPU), "boundary" in
every region's "input" and "denoised" figures (mean, 95th percentile and
maximum of the distance from that lesion's surface to the estimate's) and, with
`--num_draws`, "draws": Dice and HD95 of every draw;
`--roi_edge_profile_mm W` (needs `--target_samples`, `--voxel_spacing` and
regions; W at least the smallest spacing) adds "edge_profile" to "roi": the
mean of target, input, baselines and written volume in 3 shells of W mm inside
and 5 outside the regions' boundary (`--roi_background`'s region is not
foreground), the activity profile that shows spill-out
(guided_diffusion/metrics.py edge_profile);
`--trace True` (any path, any sampler, no other flag needed) records how every
reverse step's pred_xstart moves (guided_diffusion/metrics.py StepTrace: one
small reduction per step on the GPU, nothing waits inside the loop) and writes
trace_<name>.json beside the .npz: per step the mean, std, share of clipped
voxels and RMS change against the step before and, with `--target_samples`,
PSNR, NRMSE, MAE and bias against the target over the voxels the metrics file
counts.  On the independent paths the patches are scored before blending, each
voxel of a patch weighted with the patch's share of the Hann blend
("pooling": "patch"); `--joint_patches` scores the blended canvas ("canvas");
`--model_spacing M0 M1 M2` (mm per voxel of the grid the model was trained at,
along the input file's (D, H, W); needs `--voxel_spacing`, which then needs
neither a target nor regions) regrids the volume on the GPU to
regrid.grid_shape(shape, voxel_spacing, model_spacing) before sampling
(guided_diffusion/regrid.py, DESIGN.md 3.17: separable, anti-aliased when
shrinking; `--regrid_mode linear|cubic`, default linear; cubic can undershoot
below 0 and the output is not clamped), runs the chosen path on that volume
(any of the four, any sampler) and regrids the stitched result back before it
is written: `arr_0`, `std` and the .tif have the file's shape.  With
`--num_draws` the K stitched draws go back as one stack and mean and std are
taken on the file's grid.  The target, the labels, the baselines and the
"input" row of the metrics file stay on the file's grid; the voxels the
one-shot blend leaves at 0 become regrid.keep_after's mask; metrics_<name>.json
gains "regrid".  Equal spacings give the run without the flags.  Not with
`--trace True`;
`--draw_quantiles Q [Q ...]` (at most 8 levels in [0, 1], strictly ascending;
needs `--num_draws K >= 2`; any of the four paths, any sampler, with or without
`--device_noise`) adds the per-voxel quantiles of the K stitched draws at those
levels (numpy.quantile's "linear" method; guided_diffusion/uncertainty.py
draw_quantiles) to the .npz as `quantiles`, (levels, H, W, Z)
float32 in the layout of `arr_0`, with `quantile_levels`; no .tif is written
for them.  With `--model_spacing`, and on the joint path, they are taken of the
draws on the file's grid, like the std.  With `--target_samples` the "denoised"
row of metrics_<name>.json gains "quantiles": the rank histogram of the target
among the K draws over the voxels the row counts ("rank_histogram", K + 1 bins:
flat if the target is exchangeable with the draws, U-shaped if their spread is
too small, a dome if it is too large, a slope if they are biased; voxels where
a draw equals the target are counted in "rank_ties" instead), with two levels
or more "interval" (the outermost pair's coverage of the target and mean width;
"nominal" is simply upper - lower, which K draws can only meet approximately:
for small K the rank histogram is the exact calibration statement) and, with
0.5 among the levels, "median": the row's figures for the median volume;
`--consistency_fwhm MM` (0: pointwise; a positive one needs `--voxel_spacing`,
which then needs neither a target nor regions; any of the four paths, any
sampler, with or without `--device_noise`) pulls every reverse step's x_start
prediction towards the input volume's local means in the band of a Gaussian of
that FWHM, before the clip and the posterior mean (guided_diffusion/guidance.py
LowPassPull): `--consistency_weight W` in [0, 1] (default 1; 0
samples as without the flags and only reports), on the steps whose original
timestep is >= `--consistency_stop_t T` (default 0).  With `--model_spacing`
the taps are built at the sampled grid's effective spacing.  metrics_<name>.json
gains "consistency": the parameters and "lowpass_rms", the RMS of the low-passed
difference between the input and the written volume; without `--target_samples`
the file holds that block alone.
"""

import argparse
import collections
import json
import math
import os
import sys

sys.path.append(os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

import numpy as np
import torch as th

from guided_diffusion import _hip, dist_util, guidance, joint, logger, metrics, patches, regrid, synth, uncertainty
from guided_diffusion.gaussian_diffusion import NoiseKey
from guided_diffusion.script_util import (
    add_dict_to_argparser,
    args_to_dict,
    sr_create_model_and_diffusion,
    sr_model_and_diffusion_defaults,
)


def create_argparser():
    defaults = dict(save_dir="", clip_denoised=True, batch_size=1, use_ddim=False, eta=0.0,
                    timestep_respacing="", base_samples="", model_path="",
                    # DPM-Solver++ multistep sampling (not in the reference); takes precedence over use_ddim
                    use_dpm_solver=False, solver_order=2, solver_stochastic=False,
                    # launch-side extras (not in the reference): collective backend ("" = RCCL on
                    # GPUs) and all ranks on cuda:0, to rehearse the multi-rank flow on a one-GPU box
                    dist_backend="", share_gpu=False,
                    # one captured hipGraph per UNet forward / the library's own launch plan (both bit-identical
                    # to the default launch-by-launch replay of the Python plan)
                    step_graph=False, native_plan=False,
                    # posterior draws per patch (not in the reference): K >= 2 adds the per-voxel std map
                    num_draws=1,
                    # one state for the whole volume, blended after every step (not in the reference)
                    joint_patches=False,
                    # minimum overlap of neighbouring patches of the gap-free sliding grid (not in the reference);
                    # -1 = the reference's fixed 3 x 3 x (1 | 2) grid
                    patch_overlap=-1,
                    # sampler noise from a counter-based key, evaluated inside the step kernels (not in the reference;
                    # DESIGN.md 3.16): no generators, no noise tensors, one stream per (patch, draw).  noise_seed is
                    # read only with device_noise; the default path's seed stays the literal 10
                    device_noise=False, noise_seed=10,
                    # full-dose volume to score the result against (not in the reference); "" = no metrics
                    target_samples="", data_range=0.0, metrics_mask_threshold=0.0,
                    # scales of the multi-scale SSIM added to every metric row (not in the reference); 0 = none
                    msssim_scales=0,
                    # a per-step convergence trace of pred_xstart, written as trace_<name>.json (not in the reference)
                    trace=False,
                    # integer label volume for per-region statistics and the reference region of contrast and CNR
                    # (not in the reference); "" = no region statistics, -1 = no reference region
                    roi_labels="", roi_background=-1,
                    # lesion labels made from the target instead (not in the reference): connected components of the
                    # voxels above --roi_threshold / --roi_threshold_frac, specks below roi_min_voxels dropped
                    roi_connectivity=26, roi_min_voxels=1,
                    # radial power spectra and Fourier shell correlation of every metric row (not in the reference;
                    # needs --target_samples and --voxel_spacing), and their window: hann or none
                    spectrum=False, spectrum_window="hann",
                    # surface distances (Dice, HD, HD95, ASSD) of the input's and the denoised volume's segmentation
                    # against the target's (not in the reference; needs a --roi_threshold and --voxel_spacing)
                    roi_boundary=False)
    defaults.update(sr_model_and_diffusion_defaults())
    parser = argparse.ArgumentParser()
    add_dict_to_argparser(parser, defaults)
    parser.add_argument("--roi_threshold", type=float, default=None)          # absolute, in the target's units
    parser.add_argument("--roi_threshold_frac", type=float, default=None)     # in (0, 1), of the target's maximum
    # mm per voxel along the input file's (D, H, W): adds SUVpeak, volume in ml and TLG to every region
    parser.add_argument("--voxel_spacing", type=float, nargs="+", default=None, metavar="MM")
    # baseline denoisers of the input, scored beside it: a Gaussian post-filter of this FWHM in mm, and non-local
    # means with this h (in the volume's units), these window radii in voxels and this noise std
    parser.add_argument("--baseline_gaussian_fwhm", type=float, default=None, metavar="MM")
    parser.add_argument("--baseline_nlm_h", type=float, default=None, metavar="H")
    parser.add_argument("--baseline_nlm_search", type=int, default=3, metavar="N")
    parser.add_argument("--baseline_nlm_patch", type=int, default=1, metavar="N")
    parser.add_argument("--baseline_nlm_sigma", type=float, default=0.0, metavar="S")
    # mm per voxel of the grid the model was trained at, along the input file's (D, H, W): the volume is regridded to it
    # before sampling and the result back to the file's grid (needs --voxel_spacing); linear or cubic taps
    parser.add_argument("--model_spacing", type=float, nargs="+", default=None, metavar="MM")
    parser.add_argument("--regrid_mode", type=str, default="linear")
    # per-voxel quantiles of the --num_draws draws at these levels in [0, 1] (at most 8, ascending): the .npz gains
    # "quantiles" and "quantile_levels", the metrics file the rank histogram of the target among the draws
    # low-pass data-consistency guidance (guidance.LowPassPull on every sampling loop): the FWHM of the band in mm (0:
    # pointwise; a positive one needs --voxel_spacing), the weight in [0, 1] and the original timestep it stops below
    parser.add_argument("--consistency_fwhm", type=float, default=None, metavar="MM")
    parser.add_argument("--consistency_weight", type=float, default=None, metavar="W")
    parser.add_argument("--consistency_stop_t", type=int, default=None, metavar="T")
    parser.add_argument("--draw_quantiles", type=float, nargs="+", default=None, metavar="Q")
    # per-region texture (grey-level co-occurrence figures, IBSI): the fixed bin width in the target's units (e.g. 0.25
    # for SUV; giving it turns the feature on), the number of grey levels (default 64) and the first bin's lower edge
    parser.add_argument("--roi_texture_bin", type=float, default=None, metavar="W")
    parser.add_argument("--roi_texture_levels", type=int, default=None, metavar="N")
    parser.add_argument("--roi_texture_lower", type=float, default=None, metavar="L")
    # rotating maximum-intensity projections about the input file's axis 0, at the angles k * 360 / N, written as
    # mip_<name>.npz (needs --voxel_spacing, which then needs neither a target nor regions)
    parser.add_argument("--mip_angles", type=int, default=None, metavar="N")
    # the mean of every scored volume in shells of this width in mm across the regions' boundary (needs
    # --target_samples, --voxel_spacing and regions)
    parser.add_argument("--roi_edge_profile_mm", type=float, default=None, metavar="W")
    # split the target's components along the watershed of the target (or, with a FWHM above 0, of its Gaussian
    # smoothing): basins whose peak stands less than P above the saddle to a higher one are merged
    parser.add_argument("--roi_split_prominence", type=float, default=None, metavar="P")
    parser.add_argument("--roi_split_fwhm", type=float, default=0.0, metavar="MM")
    return parser


def main(argv=None):
    parser = create_argparser()
    args = parser.parse_args(argv)
    if not 1 <= args.num_draws <= _hip.MAX_DRAWS:
        parser.error("--num_draws must be in 1..%d (got %d)" % (_hip.MAX_DRAWS, args.num_draws))
    if args.joint_patches and args.use_dpm_solver:
        parser.error("--joint_patches True samples with DDPM or DDIM; it cannot be combined with "
                     "--use_dpm_solver True")
    if args.patch_overlap != -1 and not 2 <= args.patch_overlap <= args.large_size - 1:
        parser.error("--patch_overlap must be in 2..%d for patches of %d (got %d); -1 keeps the fixed 3 x 3 x (1 | 2) "
                     "grid" % (args.large_size - 1, args.large_size, args.patch_overlap))
    if not args.device_noise and args.noise_seed != 10:
        parser.error("--noise_seed needs --device_noise True (the default path draws from torch generators seeded "
                     "with the literal 10, and its outputs stay as they are)")
    if not 0 <= args.noise_seed < 2 ** 64:
        parser.error("--noise_seed must be in 0 .. 2^64 - 1 (got %d)" % args.noise_seed)
    _check_quantiles(parser, args)
    _check_segmentation(parser, args)
    _check_regrid(parser, args)
    _check_consistency(parser, args)
    _check_spectrum(parser, args)
    _check_mip(parser, args)
    _check_boundary(parser, args)
    args.peak = _check_spacing(parser, args)
    args.split = _check_split(parser, args)
    args.texture = _check_texture(parser, args)
    args.baselines = _check_baselines(parser, args)
    vol, target = _load_target(parser, args)
    _plan_boundary(parser, args, vol)
    vol = _plan_mip(parser, args, vol)
    vol = _plan_regrid(parser, args, vol)
    _plan_consistency(parser, args)
    roi = _load_roi(parser, args, vol)
    dist_util.setup_dist(backend=args.dist_backend or None, share_gpu=args.share_gpu)
    logger.configure(dir=args.save_dir)
    dev = dist_util.dev()

    if args.consistency is not None:
        logger.log(args.consistency["log"])
    logger.log("creating model...")
    model, diffusion = sr_create_model_and_diffusion(
        **args_to_dict(args, sr_model_and_diffusion_defaults().keys()))
    if args.model_path:
        model.load_state_dict(dist_util.load_state_dict(args.model_path, map_location="cpu"))
    else:
        logger.log("no --model_path: using seeded synthetic weights")
        model.load_state_dict({k: th.from_numpy(synth.synth_param(k, tuple(v.shape)))
                               for k, v in model.state_dict().items()})
    model.to(dev)
    if args.use_fp16:
        model.convert_to_fp16()
    model.step_graph, model.native_plan = args.step_graph, args.native_plan
    model.eval()
    if args.device_noise:
        logger.log("sampler noise: Philox4x32-10 keyed by (seed %d, patch and draw, step, voxel), evaluated in the "
                   "step kernels (not torch's stream)" % args.noise_seed)

    logger.log("loading data...")
    if vol is None:
        vol = patches.load_volume(args.base_samples)             # (D, H, W)
    native = vol
    if args.regrid is not None:
        vol = _regrid_forward(args, vol)                         # from here on vol is on the model's grid
    if _segmenting(args):
        roi = _segment_target(parser, args, vol, target)
    if args.joint_patches:
        out = _main_joint(args, model, diffusion, vol, target)
    else:
        tiling = _sliding_tiling(args, vol) if args.patch_overlap >= 0 else _fixed_tiling(args, vol)
        out = _run_patches(args, model, diffusion, vol, tiling, target)
    out_path = None
    if dist_util.rank() == 0:
        out_path = _write_outputs(args, native, target, roi, **out)
    dist_util.barrier()
    logger.log("Full image denoising complete")
    return out_path


def _load_target(parser, args):
    """--target_samples: (base volume, target), both (D, H, W), read and checked before the model is built or any
    device call is made; (None, None) without the flag."""
    if not 0 <= args.msssim_scales <= _hip.MSSSIM_MAX_SCALES:
        parser.error("--msssim_scales must be in 0..%d (got %d)" % (_hip.MSSSIM_MAX_SCALES, args.msssim_scales))
    if not args.target_samples:
        if args.msssim_scales:
            parser.error("--msssim_scales needs --target_samples: the multi-scale SSIM is taken against the "
                         "full-dose target")
        return None, None
    if args.metrics_mask_threshold < 0 or args.metrics_mask_threshold >= 1 or args.data_range < 0:
        parser.error("--metrics_mask_threshold must be in [0, 1) and --data_range must not be negative")
    for flag, path in (("--target_samples", args.target_samples), ("--base_samples", args.base_samples)):
        if not os.path.isfile(path):
            parser.error("%s: no such file: %r" % (flag, path))
    vol = patches.load_volume(args.base_samples)
    target = patches.load_volume(args.target_samples)
    if target.shape != vol.shape:
        parser.error("--target_samples: the target has shape %s, the base volume %s"
                     % (tuple(target.shape), tuple(vol.shape)))
    if min(vol.shape) < 2 * metrics.SSIM_RADIUS + 1:
        parser.error("--target_samples: the 3-D SSIM needs every extent to be at least %d (volume %s)"
                     % (2 * metrics.SSIM_RADIUS + 1, tuple(vol.shape)))
    if args.msssim_scales > metrics.msssim_max_scales(vol.shape):
        parser.error("--msssim_scales: a volume of %s is too small for %d scales (every extent must be at least %d "
                     "after %d halvings); it allows at most %d"
                     % (tuple(vol.shape), args.msssim_scales, 2 * metrics.SSIM_RADIUS + 1, args.msssim_scales - 1,
                        metrics.msssim_max_scales(vol.shape)))
    if args.spectrum:
        lo, hi = _spectrum_box(args, vol.shape)
        if not all(2 <= b - a <= _hip.SPEC_MAX_EXTENT for a, b in zip(lo, hi)):
            parser.error("--spectrum: the transformed box of a %s volume has extents %s; each must be in 2..%d"
                         % (tuple(vol.shape), tuple(b - a for a, b in zip(lo, hi)), _hip.SPEC_MAX_EXTENT))
    return vol, target


def _check_spectrum(parser, args):
    """--spectrum / --spectrum_window, checked before any file is read (and before --voxel_spacing, which this flag
    frees from needing regions)"""
    if not args.spectrum:
        return
    if args.spectrum_window not in metrics.SPECTRUM_WINDOWS:
        parser.error("--spectrum_window must be one of %s (got %r)"
                     % (", ".join(metrics.SPECTRUM_WINDOWS), args.spectrum_window))
    if not args.target_samples:
        parser.error("--spectrum needs --target_samples: the shell correlation is taken against the full-dose target")
    if args.voxel_spacing is None:
        parser.error("--spectrum needs --voxel_spacing: its frequencies are in cycles/mm")
    rows = 2 + (args.baseline_gaussian_fwhm is not None) + (args.baseline_nlm_h is not None)
    if rows + (args.num_draws if args.num_draws > 1 else 0) > _hip.MAX_DRAWS:
        parser.error("--spectrum transforms the %d rows and the --num_draws draws in one launch of at most %d "
                     "volumes (got %d draws)" % (rows, _hip.MAX_DRAWS, args.num_draws))


def _spectrum_box(args, shape):
    """(lo, hi) per axis of `shape`: the one-shot blends write zeros on the outermost planes (Hann weight 0), which
    would be an edge, so every row is transformed over [1, n - 1); the joint path over the whole volume"""
    if args.joint_patches:
        return [0] * 3, list(shape)
    return [1] * 3, [n - 1 for n in shape]


def _spectrum_block(args, tgt, rows, draws, n_draws):
    """--spectrum: one metrics.shell_spectrum over the stack of `rows` ({name: (H, W, Z) device volume}, "denoised"
    among them) and the n_draws stitched draws (any iterable: each is cut into the stack as it comes, none is held)
    against tgt, all cut to the box -> ({name: figures}, the file's top-level block); the "denoised" figures carry
    the draws' summaries.  Memory on this device: the stack of len(rows) + n_draws boxed volumes, and the driver's
    workspace of 2 (len(rows) + n_draws) + 4 half-spectrum planes of the same size."""
    s0, s1, s2 = args.voxel_spacing
    lo, hi = _spectrum_box(args, tgt.shape)
    cut = lambda t: t[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
    box = tuple(b - a for a, b in zip(lo, hi))
    plan = metrics.spectrum_plan(box, (s1, s2, s0), window=args.spectrum_window)
    stack = th.empty((len(rows) + n_draws,) + box, dtype=th.float32, device=tgt.device)
    filled = 0
    for source in (rows.values(), draws):
        for v in source:
            stack[filled] = cut(v)
            filled += 1
    assert filled == stack.shape[0], (filled, tuple(stack.shape))
    figs = metrics.spectrum_figures(metrics.shell_spectrum(stack, plan, cut(tgt).contiguous()), plan)
    out = dict(zip(rows, figs))
    if n_draws:
        out["denoised"] = {**out["denoised"],
                           "draws": [{"fsc_resolution_mm": f["fsc_resolution_mm"], "ratio_half_mm": f["ratio_half_mm"]}
                                     for f in figs[len(rows):]]}
    for name, f in out.items():
        res = f["fsc_resolution_mm"]
        mm = lambda v: "not reached" if v is None else "%.3f mm" % v
        logger.log("  %-8s spectrum: FSC 0.5 at %s, FSC 1/7 at %s, amplitude ratio 1/2 at %s"
                   % (name, mm(res["0.5"]), mm(res["0.143"]), mm(f["ratio_half_mm"])))
    return out, {"window": plan.window, "shell_width": plan.shell_width, "shells": plan.shells,
                 "n_reported": plan.n_reported, "box": [[a, b] for a, b in zip(lo, hi)]}


def _check_mip(parser, args):
    """--mip_angles, checked before any file is read (and before --voxel_spacing, which this flag frees from needing a
    target or regions)"""
    if args.mip_angles is None:
        return
    if not 1 <= args.mip_angles <= _hip.PROJECT_MAX_ANGLES:
        parser.error("--mip_angles must be in 1..%d (got %d)" % (_hip.PROJECT_MAX_ANGLES, args.mip_angles))
    if args.voxel_spacing is None:
        parser.error("--mip_angles needs --voxel_spacing: the detector's pitch and the ray step are in mm")


def _mip_box(args, shape):
    """(lo, hi) per axis of the file's (D, H, W): the box _spectrum_box cuts, for the same reason"""
    return _spectrum_box(args, shape)


def _plan_mip(parser, args, vol):
    """--mip_angles: the projected box and its default detector from the volume's shape, on the host and before the
    model is built; the volume is read now if --target_samples has not done so.  -> the (D, H, W) volume (None without
    the flag and without a target, as before)."""
    if args.mip_angles is None:
        return vol
    if vol is None:
        if not os.path.isfile(args.base_samples):
            parser.error("--base_samples: no such file: %r" % args.base_samples)
        vol = patches.load_volume(args.base_samples)
    lo, hi = _mip_box(args, vol.shape)
    box = tuple(b - a for a, b in zip(lo, hi))
    if min(box) < 1:
        parser.error("--mip_angles: the projected box of a %s volume has extents %s; each must be at least 1"
                     % (tuple(vol.shape), box))
    bins = metrics.projection_default_bins(box, args.voxel_spacing)
    if bins > _hip.PROJECT_MAX_BINS:
        parser.error("--mip_angles: the diagonal of the projected %d x %d slices at %g x %g mm takes %d bins; at most "
                     "%d" % (box[1], box[2], args.voxel_spacing[1], args.voxel_spacing[2], bins,
                             _hip.PROJECT_MAX_BINS))
    return vol


def _write_mip(args, out_path, native, target, result, std):
    """--mip_angles N: mip_<name>.npz beside the .npz, the maximum-intensity projections about the file's axis 0 at
    the angles k 360 / N of every row, each (N, D, U) float32 with rows along the file's axis 0: "denoised" and
    "input"; with --target_samples "target" and "error" (the MIP of |denoised - target|); with --num_draws "std"; with
    baselines "gaussian" and "nlm"; "angles_deg" and "pitch_mm".  One metrics.project over the stack of rows, cut to
    _mip_box.  native and target are (D, H, W) host arrays, result and std (H, W, Z) host arrays.  For .tif input also
    mip_<name>.tif, the denoised stack.  -> the .npz's path"""
    dev = dist_util.dev()

    def dhw(a, permute=False):
        t = th.as_tensor(a).to(device=dev, dtype=th.float32)
        return t.permute(2, 0, 1) if permute else t                          # (H, W, Z) -> (D, H, W)

    rows = {"denoised": dhw(result, True), "input": dhw(native)}
    if target is not None:
        rows["target"] = dhw(target)
        rows["error"] = (rows["denoised"] - rows["target"]).abs()
    if std is not None:
        rows["std"] = dhw(std, True)
    for name, (x, _) in _baseline_volumes(args, rows["input"].permute(1, 2, 0).contiguous()).items():
        rows[name] = x.permute(2, 0, 1)
    lo, hi = _mip_box(args, native.shape)
    box = tuple(b - a for a, b in zip(lo, hi))
    angles = [k * 360.0 / args.mip_angles for k in range(args.mip_angles)]
    plan = metrics.projection_plan(box, args.voxel_spacing, angles)
    stack = th.empty((len(rows),) + box, dtype=th.float32, device=dev)
    for k, v in enumerate(rows.values()):
        stack[k] = v[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
    images = metrics.project(stack, plan, mode="max").cpu().numpy()
    name = _base_name(args.base_samples)
    path = os.path.join(os.path.dirname(out_path), "mip_%s.npz" % name)
    np.savez(path, **{row: images[k] for k, row in enumerate(rows)}, angles_deg=np.asarray(angles, dtype=np.float64),
             pitch_mm=np.float64(plan.pitch))
    logger.log(f"saved {args.mip_angles} maximum-intensity projections of {', '.join(rows)} to {path}")
    if args.base_samples.lower().endswith((".tif", ".tiff")):
        from guided_diffusion import tiff_io
        tiff_io.imwrite(path.replace(".npz", ".tif"), images[0])
        logger.log(f"Saved TIFF: {path.replace('.npz', '.tif')}")
    return path


def _check_boundary(parser, args):
    """--roi_boundary / --roi_edge_profile_mm, checked before any file is read"""
    if args.roi_boundary:
        if not _segmenting(args):
            parser.error("--roi_boundary needs --roi_threshold or --roi_threshold_frac: it compares segmentations made "
                         "at one threshold")
        if args.voxel_spacing is None:
            parser.error("--roi_boundary needs --voxel_spacing: its distances are in mm")
    width = args.roi_edge_profile_mm
    if width is None:
        return
    if not (np.isfinite(width) and width > 0):
        parser.error("--roi_edge_profile_mm must be a positive finite width in mm (got %r)" % width)
    if not args.target_samples:
        parser.error("--roi_edge_profile_mm needs --target_samples: the profile is taken beside the target's")
    if args.voxel_spacing is None:
        parser.error("--roi_edge_profile_mm needs --voxel_spacing: the shells are in mm")
    if not (args.roi_labels or _segmenting(args)):
        parser.error("--roi_edge_profile_mm needs regions: give --roi_labels, --roi_threshold or --roi_threshold_frac")
    spacing = args.voxel_spacing
    if len(spacing) == 3 and all(np.isfinite(v) and v > 0 for v in spacing) and width < min(spacing):
        parser.error("--roi_edge_profile_mm %g is below the smallest voxel spacing %g mm: a shell thinner than a voxel "
                     "holds no voxel" % (width, min(spacing)))


def _plan_boundary(parser, args, vol):
    """--roi_boundary / --roi_edge_profile_mm: the distance transform's extent limit against the file's shape, the
    grid the figures are taken on, before the model is built"""
    if not (args.roi_boundary or args.roi_edge_profile_mm is not None):
        return
    if max(vol.shape) > _hip.EDT_MAX_EXTENT:
        parser.error("%s: the distance transform takes extents up to %d (volume %s)"
                     % ("--roi_boundary" if args.roi_boundary else "--roi_edge_profile_mm", _hip.EDT_MAX_EXTENT,
                        tuple(vol.shape)))


def _load_roi(parser, args, vol):
    """--roi_labels: the (D, H, W) int32 label volume, read and checked before the model is built or any device call
    is made; None without the flag."""
    if not args.roi_labels:
        return None
    if not args.target_samples:
        parser.error("--roi_labels needs --target_samples: regions are scored against the full-dose target")
    if not os.path.isfile(args.roi_labels):
        parser.error("--roi_labels: no such file: %r" % args.roi_labels)
    try:
        labels = patches.load_labels(args.roi_labels)
    except ValueError as e:
        parser.error("--roi_labels: %s" % e)
    if labels.shape != vol.shape:
        parser.error("--roi_labels: the labels have shape %s, the base volume %s"
                     % (tuple(labels.shape), tuple(vol.shape)))
    found = np.unique(labels)
    found = found[found > 0]
    if found.size == 0:
        parser.error("--roi_labels: no voxel carries a positive label")
    if found.size > _hip.ROI_MAX_REGIONS:
        parser.error("--roi_labels: %d labels (at most %d)" % (found.size, _hip.ROI_MAX_REGIONS))
    if args.roi_background != -1 and (args.roi_background <= 0 or args.roi_background not in found):
        parser.error("--roi_background: %d is not a positive label of --roi_labels" % args.roi_background)
    return labels


def _check_quantiles(parser, args):
    """--draw_quantiles, checked before any file is read"""
    levels = args.draw_quantiles
    if levels is None:
        return
    if args.num_draws < 2:
        parser.error("--draw_quantiles needs --num_draws K with K >= 2: the quantiles are taken over the K draws")
    if len(levels) > _hip.MAX_QUANTILES:
        parser.error("--draw_quantiles takes at most %d levels (got %d)" % (_hip.MAX_QUANTILES, len(levels)))
    if not all(0.0 <= q <= 1.0 for q in levels):
        parser.error("--draw_quantiles: every level must lie in [0, 1] (got %s)" % (levels,))
    if any(b <= a for a, b in zip(levels, levels[1:])):
        parser.error("--draw_quantiles: the levels must be strictly ascending (got %s)" % (levels,))


def _quantile_maps(args, stitcher=None, draws=None, to_hwz=None):
    """--draw_quantiles on rank 0: the per-voxel quantiles of the K stitched draws, from the stitcher's accumulators
    (no K-volume temporary) or from the (K, ...) stack the draw moments are taken of; to_hwz permutes the stack's volume
    axes to the written (H, W, Z) layout.  -> None without the flag, else {"quant": (nq, H, W, Z) device tensor,
    "ranks": (H, W, Z) target -> (below, equal), the second launch _write_metrics makes once it has the target}."""
    levels = args.draw_quantiles
    if levels is None:
        return None
    if draws is None:
        return {"quant": stitcher.quantiles(levels), "ranks": lambda tgt: stitcher.quantiles((), target=tgt)[1:]}
    if to_hwz is None:
        return {"quant": uncertainty.draw_quantiles(draws, levels),
                "ranks": lambda tgt: uncertainty.draw_quantiles(draws, (), target=tgt)[1:]}
    back = tuple(int(v) for v in np.argsort(to_hwz))

    def ranks(tgt):
        _, below, equal = uncertainty.draw_quantiles(draws, (), target=tgt.permute(*back).contiguous())
        return below.permute(*to_hwz).contiguous(), equal.permute(*to_hwz).contiguous()

    quant = uncertainty.draw_quantiles(draws, levels)
    return {"quant": quant.permute(0, *(1 + v for v in to_hwz)).contiguous(), "ranks": ranks}


def _quantile_arrays(args, qmaps):
    """The .npz entries of --draw_quantiles ({} without the flag): "quantiles" (nq, H, W, Z) float32, the layout of
    arr_0, and "quantile_levels" float64"""
    if qmaps is None:
        return {}
    return {"quantiles": qmaps["quant"].cpu().numpy(),
            "quantile_levels": np.asarray(args.draw_quantiles, dtype=np.float64)}


def _quantile_block(args, qmaps, tgt, mask, evaluate):
    """"quantiles" of the metrics file's "denoised" row, over the voxels that row counts (mask): the rank histogram
    of the target among the K draws, the outermost interval's coverage and width, and the median scored like the
    mean (evaluate: volume -> the row's figures)."""
    levels, K = list(args.draw_quantiles), args.num_draws
    quant = qmaps["quant"]
    below, equal = qmaps["ranks"](tgt)
    hist = uncertainty.rank_histogram(below, equal, K, mask=mask)
    block = {"levels": levels, "rank_histogram": hist["counts"], "rank_ties": hist["ties"], "rank_n": hist["n"]}
    ends = (hist["counts"][0] + hist["counts"][K]) / max(hist["n"], 1)
    logger.log("  rank histogram of the target among %d draws: %.4f of %d voxels in the two end bins (%.4f if the "
               "target were one more draw), %d ties" % (K, ends, hist["n"], 2.0 / (K + 1), hist["ties"]))
    if len(levels) >= 2:
        f = metrics.interval_figures(quant[0], quant[-1], tgt, mask=mask)
        block["interval"] = {"lower": levels[0], "upper": levels[-1], "nominal": levels[-1] - levels[0],
                             "coverage": f["coverage"], "mean_width": f["mean_width"]}
        logger.log("  interval [q%g, q%g]: covers %.4f of the target (nominal %.4f), mean width %.5g"
                   % (levels[0], levels[-1], f["coverage"], levels[-1] - levels[0], f["mean_width"]))
    if 0.5 in levels:
        block["median"] = evaluate(quant[levels.index(0.5)])
    return block


def _segmenting(args):
    return args.roi_threshold is not None or args.roi_threshold_frac is not None


def _check_segmentation(parser, args):
    """--roi_threshold / --roi_threshold_frac and their options, checked before any file is read"""
    if args.roi_connectivity not in (6, 18, 26):
        parser.error("--roi_connectivity must be 6, 18 or 26 (got %d)" % args.roi_connectivity)
    if args.roi_min_voxels < 1:
        parser.error("--roi_min_voxels must be at least 1 (got %d)" % args.roi_min_voxels)
    if not _segmenting(args):
        return
    if args.roi_threshold is not None and args.roi_threshold_frac is not None:
        parser.error("--roi_threshold and --roi_threshold_frac cannot be combined: give one threshold")
    flag = "--roi_threshold" if args.roi_threshold is not None else "--roi_threshold_frac"
    if args.roi_labels or args.roi_background != -1:
        parser.error("%s makes the labels itself: it cannot be combined with --roi_labels or --roi_background" % flag)
    if not args.target_samples:
        parser.error("%s needs --target_samples: the full-dose target is what gets segmented" % flag)
    if args.roi_threshold is not None and not np.isfinite(args.roi_threshold):
        parser.error("--roi_threshold must be a finite number (got %r)" % args.roi_threshold)
    if args.roi_threshold_frac is not None and not 0.0 < args.roi_threshold_frac < 1.0:
        parser.error("--roi_threshold_frac must lie in (0, 1) (got %r)" % args.roi_threshold_frac)


def _check_split(parser, args):
    """--roi_split_prominence / --roi_split_fwhm, checked before any file is read (and after --voxel_spacing): None
    without the first, else {"prominence", "fwhm", "taps": the smoothing's taps on the volumes' (H, W, Z) grid or
    None}"""
    p, fwhm = args.roi_split_prominence, args.roi_split_fwhm
    if p is None:
        if fwhm != 0.0:
            parser.error("--roi_split_fwhm needs --roi_split_prominence: it smooths the height the split climbs")
        return None
    if not (np.isfinite(p) and p > 0):
        parser.error("--roi_split_prominence must be a positive finite number, in the target's units (got %r)" % p)
    if args.roi_labels:
        parser.error("--roi_split_prominence splits the components the script makes itself: it cannot be combined "
                     "with --roi_labels")
    if not _segmenting(args):
        parser.error("--roi_split_prominence needs --roi_threshold or --roi_threshold_frac: it splits their components")
    if not (np.isfinite(fwhm) and fwhm >= 0):
        parser.error("--roi_split_fwhm must be 0 or a positive finite number of mm (got %r)" % fwhm)
    taps = None
    if fwhm > 0:
        if args.voxel_spacing is None:
            parser.error("--roi_split_fwhm needs --voxel_spacing: the FWHM is in mm")
        s0, s1, s2 = args.voxel_spacing
        try:
            taps = metrics.gaussian_taps(fwhm, (s1, s2, s0))                # (D, H, W) -> (H, W, Z)
        except ValueError as e:
            parser.error("--roi_split_fwhm: %s" % e)
    return {"prominence": float(p), "fwhm": float(fwhm), "taps": taps}


def _check_texture(parser, args):
    """--roi_texture_bin / _levels / _lower, checked before any file is read: None without the first, else
    roi_report's texture= dict"""
    if args.roi_texture_bin is None:
        for flag, value in (("--roi_texture_levels", args.roi_texture_levels),
                            ("--roi_texture_lower", args.roi_texture_lower)):
            if value is not None:
                parser.error("%s needs --roi_texture_bin: the bin width is what turns the texture figures on" % flag)
        return None
    levels = 64 if args.roi_texture_levels is None else args.roi_texture_levels
    lower = 0.0 if args.roi_texture_lower is None else args.roi_texture_lower
    if not (np.isfinite(args.roi_texture_bin) and args.roi_texture_bin > 0):
        parser.error("--roi_texture_bin must be a positive finite number (got %r)" % args.roi_texture_bin)
    if not 2 <= levels <= _hip.TEX_MAX_LEVELS:
        parser.error("--roi_texture_levels must be in 2..%d (got %d)" % (_hip.TEX_MAX_LEVELS, levels))
    if not np.isfinite(lower):
        parser.error("--roi_texture_lower must be a finite number (got %r)" % lower)
    if not args.target_samples:
        parser.error("--roi_texture_bin needs --target_samples: its figures are taken per region against the target")
    if not (args.roi_labels or _segmenting(args)):
        parser.error("--roi_texture_bin needs regions: give --roi_labels, --roi_threshold or --roi_threshold_frac")
    try:                                       # what roi_texture itself would refuse later (a width whose inverse overflows)
        metrics._check_texture("--roi_texture_bin", int(levels), float(args.roi_texture_bin), float(lower))
    except ValueError as e:
        parser.error(str(e))
    return {"bin_width": float(args.roi_texture_bin), "levels": int(levels), "lower": float(lower)}


def _check_spacing(parser, args):
    """--voxel_spacing, checked before any file is read: None without the flag, else {"spacing": the three values
    permuted along with the volumes, (D, H, W) -> (H, W, Z), "footprint": PERCIST's 1 cm^3 sphere on that grid}"""
    if args.voxel_spacing is None:
        return None
    if len(args.voxel_spacing) != 3:
        parser.error("--voxel_spacing takes three numbers, mm per voxel along (D, H, W) (got %d)"
                     % len(args.voxel_spacing))
    if not all(np.isfinite(v) and v > 0 for v in args.voxel_spacing):
        parser.error("--voxel_spacing must be three positive finite numbers (got %s)" % (args.voxel_spacing,))
    if not args.target_samples:
        if args.model_spacing is not None or args.consistency_fwhm is not None or args.mip_angles is not None:
            return None                        # the spacing serves the regridding, the guidance or the MIP alone
        parser.error("--voxel_spacing needs --target_samples: its figures are taken per region against the target")
    if not (args.roi_labels or _segmenting(args)):
        if (args.baseline_gaussian_fwhm is not None or args.model_spacing is not None
                or args.consistency_fwhm is not None or args.spectrum or args.mip_angles is not None):
            # the spacing serves the Gaussian baseline, the regridding, the guidance, the spectrum or the MIP
            return None
        parser.error("--voxel_spacing needs regions: give --roi_labels, --roi_threshold or --roi_threshold_frac")
    s0, s1, s2 = args.voxel_spacing
    try:
        footprint = metrics.sphere_footprint((s1, s2, s0))
    except ValueError as e:
        parser.error("--voxel_spacing: %s" % e)
    return {"spacing": (s1, s2, s0), "footprint": footprint}


def _check_regrid(parser, args):
    """--model_spacing / --regrid_mode, checked before any file is read (and before --voxel_spacing, whose own checks
    follow); args.regrid is None until _plan_regrid has the volume's shape"""
    args.regrid = None
    if args.regrid_mode not in regrid.MODES:
        parser.error("--regrid_mode must be linear or cubic (got %r)" % args.regrid_mode)
    if args.model_spacing is None:
        return
    if len(args.model_spacing) != 3:
        parser.error("--model_spacing takes three numbers, mm per voxel along (D, H, W) (got %d)"
                     % len(args.model_spacing))
    if not all(np.isfinite(v) and v > 0 for v in args.model_spacing):
        parser.error("--model_spacing must be three positive finite numbers (got %s)" % (args.model_spacing,))
    if args.voxel_spacing is None:
        parser.error("--model_spacing needs --voxel_spacing: the file's own spacing, mm per voxel along (D, H, W)")
    if args.trace:
        parser.error("--trace True cannot be combined with --model_spacing: the trace scores the sampled grid, the "
                     "target lives on the file's")


def _plan_regrid(parser, args, vol):
    """--model_spacing: the regridding plan from the volume's shape, on the host and before the model is built; the
    volume is read now if --target_samples has not done so.  -> the (D, H, W) volume (None without the flag and
    without a target, as before).  args.regrid = {"plan", "native": the volume on the file's grid}."""
    if args.model_spacing is None:
        return vol
    if vol is None:
        if not os.path.isfile(args.base_samples):
            parser.error("--base_samples: no such file: %r" % args.base_samples)
        vol = patches.load_volume(args.base_samples)
    try:
        shape = regrid.grid_shape(vol.shape, args.voxel_spacing, args.model_spacing)
        plan = regrid.plan(vol.shape, shape, args.regrid_mode)
    except ValueError as e:
        parser.error("--model_spacing: %s" % e)
    args.regrid = {"plan": plan, "native": vol}
    return vol


def _regridding(args):
    """True when some axis changes its extent: with equal spacings nothing is regridded and the run is the run without
    the flags"""
    rg = getattr(args, "regrid", None)
    return rg is not None and not rg["plan"].identity


def _regrid_forward(args, vol):
    """The (D, H, W) host volume on the model's grid (regridded on the device), with the log's line"""
    plan = args.regrid["plan"]
    logger.log(f"regridding {plan.shape_in} at {tuple(args.voxel_spacing)} mm to {plan.shape_out} at "
               f"{tuple(args.model_spacing)} mm ({plan.mode}); outputs return to {plan.shape_in}")
    if plan.identity:
        return vol
    x = th.from_numpy(np.ascontiguousarray(vol, dtype=np.float32)).to(dist_util.dev())
    return regrid.apply(x, plan).cpu().numpy()


def _regrid_back(args, x):
    """A stitched (H, W, Z) volume or (K, H, W, Z) stack on the model's grid -> the same on the file's grid, host
    array or device tensor as given: regridded as (D, H, W) with the inverse plan.  Unchanged without --model_spacing."""
    if not _regridding(args):
        return x
    t = th.as_tensor(x).to(device=dist_util.dev(), dtype=th.float32)
    to_dhw, to_hwz = ((2, 0, 1), (1, 2, 0)) if t.dim() == 3 else ((0, 3, 1, 2), (0, 2, 3, 1))
    y = regrid.apply(t.permute(*to_dhw).contiguous(), args.regrid["plan"].inverse()).permute(*to_hwz).contiguous()
    return y if isinstance(x, th.Tensor) else y.cpu().numpy()


def _regrid_keep(args, weight):
    """The one-shot blend's (H, W, Z) weight sum on the model's grid -> the uint8 mask of the file's voxels that no
    weight-0 voxel enters (regrid.keep_after), which stands in for the weight from there on.  Unchanged without
    --model_spacing."""
    if not _regridding(args):
        return weight
    live = (th.as_tensor(weight).to(dist_util.dev()) > 0).to(th.uint8).permute(2, 0, 1).contiguous()
    keep = regrid.keep_after(live, args.regrid["plan"].inverse()).permute(1, 2, 0).contiguous()
    return keep if isinstance(weight, th.Tensor) else keep.cpu().numpy()


def _check_consistency(parser, args):
    """--consistency_fwhm / _weight / _stop_t, checked before any file is read; args.consistency is None without the
    flag and until _plan_consistency has the sampled grid's spacing"""
    args.consistency = None
    fwhm, w, stop = args.consistency_fwhm, args.consistency_weight, args.consistency_stop_t
    if fwhm is None:
        if w is not None or stop is not None:
            parser.error("--consistency_weight and --consistency_stop_t need --consistency_fwhm")
        return
    if not (np.isfinite(fwhm) and fwhm >= 0):
        parser.error("--consistency_fwhm must be a finite number of mm, 0 (pointwise) or more (got %r)" % fwhm)
    if w is not None and not 0 <= w <= 1:                      # NaN fails both comparisons
        parser.error("--consistency_weight must be in [0, 1] (got %r)" % w)
    if stop is not None and stop < 0:
        parser.error("--consistency_stop_t must not be negative (got %d)" % stop)
    if fwhm > 0 and args.voxel_spacing is None:
        parser.error("--consistency_fwhm needs --voxel_spacing: the FWHM is in mm")
    if fwhm > 0 and len(args.voxel_spacing) == 3 and all(np.isfinite(v) and v > 0 for v in args.voxel_spacing):
        try:
            guidance.pull_taps(fwhm, args.voxel_spacing)
        except ValueError as e:
            parser.error("--consistency_fwhm: %s" % e)


def _plan_consistency(parser, args):
    """--consistency_fwhm: the pull, built on the host before the model is (after _plan_regrid: with --model_spacing
    its taps are taken at the sampled grid's effective spacing).  args.consistency = {"pull": what the loops take as
    guide= (None at weight 0: nothing is launched), "taps": the Gaussian on the file's (H, W, Z) grid for the report,
    the report's own parameters, per-axis figures along the sampled grid's (D, H, W), and the log's one line}"""
    if args.consistency_fwhm is None:
        return
    fwhm = args.consistency_fwhm
    w = 1.0 if args.consistency_weight is None else args.consistency_weight
    stop = 0 if args.consistency_stop_t is None else args.consistency_stop_t
    spacing = args.voxel_spacing
    if spacing is not None and args.regrid is not None:
        spacing = [s * r for s, r in zip(args.voxel_spacing, args.regrid["plan"].scale)]
    try:
        pull = guidance.LowPassPull(fwhm, spacing, weight=w, stop_t=stop)
        s0, s1, s2 = args.voxel_spacing if fwhm > 0 else (1.0, 1.0, 1.0)
        file_taps = guidance.pull_taps(fwhm, (s1, s2, s0))                   # (D, H, W) -> (H, W, Z)
    except ValueError as e:
        parser.error("--consistency_fwhm: %s" % e)
    args.consistency = {"pull": pull if pull.weight > 0 else None, "taps": file_taps,
                        "log": "consistency guidance: FWHM %g mm (radii %s voxels), weight %g, original timesteps >= %d"
                               % (fwhm, list(pull.radii), pull.weight, stop)
                               + ("" if pull.weight > 0 else "; weight 0 samples as without it and only reports"),
                        "params": {"fwhm_mm": fwhm, "sigma_voxels": list(pull.taps.sigma_voxels),
                                   "radii": list(pull.radii), "weight": pull.weight, "stop_t": stop}}


def _guide(args):
    """guide= of the sampling loops: {} without --consistency_fwhm and at weight 0"""
    cons = getattr(args, "consistency", None)
    return {} if cons is None or cons["pull"] is None else {"guide": cons["pull"]}


def _consistency_block(args, inp, den, mask):
    """metrics_<name>.json's "consistency": the pull's parameters and lowpass_rms, the RMS of G(input - written volume)
    over the counted voxels on the file's grid (inp, den: (H, W, Z) device tensors)"""
    cons = args.consistency
    low = metrics.gaussian_smooth((inp - den).contiguous(), cons["taps"])
    rms = math.sqrt(metrics.error_moments(low, th.zeros_like(low), mask=mask)["mse"])
    return dict(cons["params"], lowpass_rms=rms)


def _check_baselines(parser, args):
    """--baseline_gaussian_fwhm / --baseline_nlm_h and their options, checked before any file is read (and after
    --voxel_spacing): None without either flag, else {"gaussian": the taps on the volumes' (H, W, Z) grid, "nlm":
    {"h", "search", "patch", "sigma"}} with the entries of the flags given"""
    out = {}
    if args.baseline_gaussian_fwhm is not None:
        fwhm = args.baseline_gaussian_fwhm
        if not (np.isfinite(fwhm) and fwhm > 0):
            parser.error("--baseline_gaussian_fwhm must be a positive finite number of mm (got %r)" % fwhm)
        if not args.target_samples:
            parser.error("--baseline_gaussian_fwhm needs --target_samples: baselines are scored against the target")
        if args.voxel_spacing is None:
            parser.error("--baseline_gaussian_fwhm needs --voxel_spacing: the FWHM is in mm")
        s0, s1, s2 = args.voxel_spacing
        try:
            out["gaussian"] = metrics.gaussian_taps(fwhm, (s1, s2, s0))     # (D, H, W) -> (H, W, Z)
        except ValueError as e:
            parser.error("--baseline_gaussian_fwhm: %s" % e)
    if args.baseline_nlm_h is not None:
        h = args.baseline_nlm_h
        if not (np.isfinite(h) and h > 0):
            parser.error("--baseline_nlm_h must be a positive finite number (got %r)" % h)
        if not args.target_samples:
            parser.error("--baseline_nlm_h needs --target_samples: baselines are scored against the target")
        if not 0 <= args.baseline_nlm_search <= _hip.NLM_MAX_SEARCH:
            parser.error("--baseline_nlm_search must be in 0..%d (got %d)" % (_hip.NLM_MAX_SEARCH, args.baseline_nlm_search))
        if not 0 <= args.baseline_nlm_patch <= _hip.NLM_MAX_PATCH:
            parser.error("--baseline_nlm_patch must be in 0..%d (got %d)" % (_hip.NLM_MAX_PATCH, args.baseline_nlm_patch))
        try:
            h, search, patch, sigma = metrics.nlm_check(h, args.baseline_nlm_search, args.baseline_nlm_patch,
                                                        args.baseline_nlm_sigma)
        except ValueError as e:
            parser.error("--baseline_nlm_h / --baseline_nlm_sigma: %s" % e)
        out["nlm"] = {"h": h, "search": search, "patch": patch, "sigma": sigma}
    return out or None


def _baseline_volumes(args, inp):
    """The input filtered once per baseline flag, on the device: {name: ((H, W, Z) tensor, its parameters as the
    metrics file states them)}, "gaussian" before "nlm".  The Gaussian's per-axis figures are listed along the input
    file's (D, H, W), like --voxel_spacing."""
    base = getattr(args, "baselines", None) or {}
    out = {}
    if "gaussian" in base:
        g = base["gaussian"]
        file_order = lambda v: [v[2], v[0], v[1]]                            # (H, W, Z) -> (D, H, W)
        out["gaussian"] = (metrics.gaussian_smooth(inp, g),
                           {"fwhm_mm": args.baseline_gaussian_fwhm, "sigma_voxels": file_order(g.sigma_voxels),
                            "radii": file_order(g.radii)})
    if "nlm" in base:
        n = base["nlm"]
        out["nlm"] = (metrics.nlm(inp, n["h"], search=n["search"], patch=n["patch"], sigma=n["sigma"]),
                      {"h": n["h"], "sigma": n["sigma"], "search": list(n["search"]), "patch": list(n["patch"])})
    return out


def _segment_target(parser, args, vol, target):
    """--roi_threshold / --roi_threshold_frac: the target's lesion labels, made once on the device before the first
    sampling step so that a threshold that cannot be used stops the run now.  -> {"labels": int32 (H, W, Z) on the
    device, "n", "keep": uint8 (H, W, Z) or None, "threshold": the absolute threshold as applied (fp32),
    "connectivity", "min_voxels"}.  keep holds the voxels the one-shot blend will give a weight above 0, known from
    the grid alone (the joint path writes every voxel)."""
    dev = dist_util.dev()
    res = args.large_size
    keep = None
    if not args.joint_patches:
        grid = (patches.sliding_grid(vol.shape, res, args.patch_overlap) if args.patch_overlap >= 0
                else patches.patch_grid(vol.shape, res))
        keep = th.from_numpy(patches.blend_cover(grid, vol.shape, res).astype(np.uint8)).to(dev).contiguous()
        keep = _regrid_keep(args, keep)
    if args.roi_threshold is not None:
        threshold = float(np.float32(args.roi_threshold))
    else:
        threshold = float(np.float32(args.roi_threshold_frac * float(target.max())))
    tgt = th.from_numpy(target).to(dev).permute(1, 2, 0).contiguous()                 # (D, H, W) -> (H, W, Z)
    labels, n = metrics.segment(tgt, threshold, connectivity=args.roi_connectivity, min_voxels=args.roi_min_voxels,
                                keep=keep)
    if n == 0:
        parser.error("the target has no region of at least %d voxels above the threshold %g (its maximum is %g): "
                     "lower the threshold or --roi_min_voxels" % (args.roi_min_voxels, threshold, float(target.max())))
    split = getattr(args, "split", None)
    if split is not None:
        # the voxels the one-shot blend leaves at 0 are background in `labels` already
        height = tgt if split["taps"] is None else metrics.gaussian_smooth(tgt, split["taps"])
        try:
            labels, n_split, info = metrics.split_components(labels, height, split["prominence"],
                                                             connectivity=args.roi_connectivity)
        except ValueError as e:
            parser.error("--roi_split_prominence: %s (see --roi_split_fwhm)" % e)
        if n_split > _hip.ROI_MAX_REGIONS:
            parser.error("the target has %d regions above the threshold %g after the split at prominence %g (at most "
                         "%d): raise --roi_split_prominence or --roi_split_fwhm, raise --roi_min_voxels to drop the "
                         "specks, or raise the threshold"
                         % (n_split, threshold, split["prominence"], _hip.ROI_MAX_REGIONS))
    if n > _hip.ROI_MAX_REGIONS:
        parser.error("the target has %d regions above the threshold %g (at most %d): raise --roi_min_voxels to drop "
                     "the specks, or raise the threshold" % (n, threshold, _hip.ROI_MAX_REGIONS))
    logger.log(f"target segmented at {threshold:g} (connectivity {args.roi_connectivity}, at least "
               f"{args.roi_min_voxels} voxels): {n} regions")
    seg = {"labels": labels, "n": n, "keep": keep, "threshold": threshold, "connectivity": args.roi_connectivity,
           "min_voxels": args.roi_min_voxels}
    if split is not None:
        logger.log(f"target split at prominence {split['prominence']:g} (height smoothed at {split['fwhm']:g} mm FWHM): "
                   f"{n} components -> {info['n_basins']} basins -> {n_split} regions")
        seg.update(n=n_split, component=info["parent"],
                   split={"prominence": split["prominence"], "fwhm_mm": split["fwhm"],
                          "connectivity": args.roi_connectivity, "n_components": n, "n_basins": info["n_basins"],
                          "n_regions": n_split})
    return seg


def _detection_block(seg, regions, inp, den, draw_found, edges=None, draw_edges=None):
    """"detection" of the "roi" entry: the target's lesions against the input's and the denoised volume's own
    segmentation at the same threshold; every region gains "found" and "overlap" under "input" and "denoised".  With
    --roi_boundary (edges = (the spacing, metrics.boundary_target of the labels)) the same two segmentations also give
    "boundary", and every region "boundary" under "input" and "denoised".  -> the entries to add to "roi"."""
    out, bound = {}, {}
    for name, x in (("input", inp), ("denoised", den)):
        est, _ = metrics.segment(x, seg["threshold"], connectivity=seg["connectivity"], min_voxels=seg["min_voxels"],
                                 keep=seg["keep"])
        out[name] = d = metrics.detection(seg["labels"], est)
        for r in range(seg["n"]):
            regions[str(r + 1)][name]["found"] = d["found"][r]
            regions[str(r + 1)][name]["overlap"] = d["overlap"][r]
        if edges is not None:
            b = metrics.boundary(seg["labels"], est, edges[0], index=edges[1])
            for label, figures in b.pop("regions").items():
                regions[str(label)][name]["boundary"] = figures
            bound[name] = b
    if draw_found is not None:
        out["denoised"]["draws"] = draw_found
    if edges is not None and draw_edges is not None:
        bound["denoised"]["draws"] = draw_edges
    logger.log("  lesions: %d in the target; input finds %d, misses %d, %d false positives; denoised finds %d, "
               "misses %d, %d false positives"
               % (seg["n"], out["input"]["n_found"], out["input"]["n_missed"], out["input"]["false_positives"],
                  out["denoised"]["n_found"], out["denoised"]["n_missed"], out["denoised"]["false_positives"]))
    if edges is None:
        return {"detection": out}
    show = lambda v: "n/a" if v is None else "%.4g" % v
    logger.log("  boundaries: " + "; ".join(
        "%s Dice %s, HD95 %s mm, ASSD %s mm" % (name, show(b["dice"]), show(b["hd95_mm"]), show(b["assd_mm"]))
        for name, b in bound.items()))
    return {"detection": out, "boundary": bound}


def _roi_block(args, roi, tgt, inp, den, keep, draws, out_path=None, baselines=None):
    """The "roi" entry of the metrics file: per-region figures of target, input and written volume, all (H, W, Z) on
    the device, and of the `baselines` ({name: volume}), which get no detection figures; keep drops the voxels the blend left at 0; draws yields the K stitched draws one volume at a time,
    of which only the small records are kept.  roi is the (D, H, W) label volume of --roi_labels or _segment_target's
    dict, whose labels are written beside out_path first."""
    seg = roi if isinstance(roi, dict) else None
    if seg is not None:
        labels, keep = seg["labels"], seg["keep"]
        labels_path = os.path.join(os.path.dirname(out_path), "roi_labels_%s.npz" % _base_name(args.base_samples))
        np.savez(labels_path, labels.permute(2, 0, 1).cpu().numpy())                 # (H, W, Z) -> (D, H, W), int32
        logger.log(f"saved lesion labels to {labels_path}")
    else:
        labels = th.from_numpy(roi).to(tgt.device).permute(1, 2, 0).contiguous()     # (D, H, W) -> (H, W, Z)
    index = metrics.roi_index(labels, keep=keep)
    background = args.roi_background if args.roi_background > 0 else None
    if background is not None and background not in index.labels:
        logger.log("  WARNING: --roi_background %d has no voxel of non-zero blend weight: no contrast figures"
                   % background)
        background = None
    peak = getattr(args, "peak", None)
    more = {}
    if peak is not None:                       # the footprint and the target's peaks once, for both reports
        more = {"spacing": peak["spacing"], "keep": keep, "footprint": peak["footprint"],
                "target_peaks": metrics.roi_peak(tgt, index, peak["footprint"], keep=keep)}
    texture = getattr(args, "texture", None)
    if texture is not None:                    # the target's own figures once, for every report
        more.update(texture=texture,
                    target_texture=metrics.texture_figures(metrics.roi_texture(tgt, index, **texture)))
    edges = None
    if seg is not None and args.roi_boundary:  # the target's surface and its distance map once, for every estimate
        edges = (peak["spacing"], metrics.boundary_target(labels, peak["spacing"]))
    records = draw_found = draw_edges = None
    if draws is not None:
        records, draw_found, draw_edges = [], [], []
        if peak is not None:
            more["draw_peaks"] = []
        if texture is not None:
            more["draw_texture"] = []
        for d in draws:
            records.append(metrics.roi_moments(d, index))
            if texture is not None:
                more["draw_texture"].append(metrics.texture_figures(metrics.roi_texture(d, index, **texture)))
            if peak is not None:
                more["draw_peaks"].append(metrics.roi_peak(d, index, peak["footprint"], keep=keep))
            if seg is not None:
                est, _ = metrics.segment(d, seg["threshold"], connectivity=seg["connectivity"],
                                         min_voxels=seg["min_voxels"], keep=keep)
                found = metrics.detection(labels, est)
                draw_found.append({"n_found": found["n_found"], "false_positives": found["false_positives"]})
                if edges is not None:
                    b = metrics.boundary(labels, est, edges[0], index=edges[1])
                    draw_edges.append({"dice": b["dice"], "hd95_mm": b["hd95_mm"]})
    den_rep = metrics.roi_report(den, tgt, index, background=background, draws=records, **more)
    inp_rep = metrics.roi_report(inp, tgt, index, background=background,
                                 **{k: v for k, v in more.items() if k not in ("draw_peaks", "draw_texture")})
    base_rep = {name: metrics.roi_report(x, tgt, index, background=background,
                                         **{k: v for k, v in more.items() if k not in ("draw_peaks", "draw_texture")})
                for name, x in (baselines or {}).items()}
    regions = {str(label): {"n": den_rep[label]["n"], "target": den_rep[label]["target"],
                            "input": inp_rep[label]["estimate"],
                            **{name: rep[label]["estimate"] for name, rep in base_rep.items()},
                            "denoised": den_rep[label]["estimate"]}
               for label in index.labels}
    show = lambda v: "n/a" if v is None else "%.5g" % v
    for label in index.labels[:20]:
        r = regions[str(label)]
        logger.log("  region %d (%d voxels): mean %s target, %s input, %s denoised; max %s / %s / %s%s%s%s"
                   % (label, r["n"], show(r["target"]["mean"]), show(r["input"]["mean"]), show(r["denoised"]["mean"]),
                      show(r["target"]["max"]), show(r["input"]["max"]), show(r["denoised"]["max"]),
                      "; mean over draws +- %s" % show(r["denoised"]["mean_std"]) if records else "",
                      "; peak %s / %s / %s" % (show(r["target"]["peak"]), show(r["input"]["peak"]),
                                               show(r["denoised"]["peak"])) if peak is not None else "",
                      "".join("; %s %s / %s / %s" % ((k,) + tuple(show(r[w]["texture"][k])
                                                                  for w in ("target", "input", "denoised")))
                              for k in ("contrast", "joint_entropy")) if texture is not None else ""))
    if len(index.labels) > 20:
        logger.log("  (%d more regions in the metrics file)" % (len(index.labels) - 20))
    spaced = {}
    if peak is not None:
        spaced = {"voxel_spacing": list(args.voxel_spacing), "peak_volume_mm3": peak["footprint"].volume_mm3,
                  "peak_taps": peak["footprint"].taps}
    if texture is not None:
        spaced["texture"] = dict(texture, directions=metrics.TEXTURE_DIRECTIONS)
        if any((r["target"]["texture"]["clamped"] or 0.0) > 0.05 for r in regions.values()):
            logger.log("  WARNING: more than 5 %% of a region of the target falls outside the grey levels: choose "
                       "--roi_texture_bin (and --roi_texture_levels / --roi_texture_lower) so that %d bins span the "
                       "target's values" % texture["levels"])
    if args.roi_edge_profile_mm is not None:
        # --roi_background's region is not foreground; the written volume is the mean of the draws with --num_draws
        lesions = labels if args.roi_background <= 0 else th.where(labels == args.roi_background,
                                                                   th.zeros_like(labels), labels)
        spaced["edge_profile"] = prof = metrics.edge_profile(
            {"target": tgt, "input": inp, **(baselines or {}), "denoised": den}, lesions, peak["spacing"],
            args.roi_edge_profile_mm, keep=keep)
        logger.log("  edge profile, %g mm shells (distance: target / input / denoised): %s"
                   % (prof["width_mm"], ", ".join("%+g: %s / %s / %s" % (
                       (r["distance_mm"],) + tuple(show(r["mean"][k]) for k in ("target", "input", "denoised")))
                       for r in prof["rows"])))
    if seg is None:
        return {"labels": args.roi_labels, "background": background, "regions": regions, **spaced}
    split = {}
    if "split" in seg:
        split = {"split": seg["split"]}
        for label in index.labels:
            regions[str(label)]["component"] = seg["component"][label - 1]
    return {"labels": labels_path, "background": None, "threshold": seg["threshold"],
            "connectivity": seg["connectivity"], "min_voxels": seg["min_voxels"], **split, "regions": regions,
            **_detection_block(seg, regions, inp, den, draw_found, edges, draw_edges), **spaced}


def _write_metrics(args, out_path, target, vol, result, std=None, weight=None, roi=None, draws=None, quantiles=None):
    """Rank 0, after the .npz is written: scores the written volume `result` (and `std`, with --num_draws) and the
    low-dose input `vol` against `target` on the device and writes metrics_<name>.json beside the .npz.  target and
    vol are (D, H, W) host arrays; result, std and weight (the one-shot blend's Hann weight sum, whose zeros are not
    counted) are (H, W, Z) host arrays or device tensors.  With --roi_labels (roi, (D, H, W) int32) the file gains the
    "roi" entry; draws then yields the K draws of --num_draws as (H, W, Z) device tensors.  Nothing happens without
    --target_samples.  quantiles: _quantile_maps' dict with --draw_quantiles, which adds "quantiles" to the "denoised"
    row."""
    cons = getattr(args, "consistency", None)
    if target is None and cons is None:
        return None
    dev = dist_util.dev()

    def hwz(a, permute=False):
        t = th.as_tensor(a).to(device=dev, dtype=th.float32)
        return (t.permute(1, 2, 0) if permute else t).contiguous()

    path = os.path.join(os.path.dirname(out_path), "metrics_%s.json" % _base_name(args.base_samples))
    if target is None:                          # --consistency_fwhm alone: its block is the whole file
        live = None if weight is None else (th.as_tensor(weight).to(dev) > 0).to(th.uint8).contiguous()
        with open(path, "w") as f:
            json.dump({"consistency": _consistency_block(args, hwz(vol, True), hwz(result), live)}, f, indent=2)
        logger.log(f"saved metrics to {path}")
        return path
    tgt, inp, den = hwz(target, True), hwz(vol, True), hwz(result)
    counted = None
    if args.metrics_mask_threshold > 0:
        counted = tgt > args.metrics_mask_threshold * tgt.max()
    if weight is not None:
        live = th.as_tensor(weight).to(dev) > 0
        counted = live if counted is None else counted & live
    mask = None if counted is None else counted.to(th.uint8).contiguous()
    data_range = args.data_range if args.data_range > 0 else None
    more = {"msssim_scales": args.msssim_scales} if args.msssim_scales else {}

    def log_msssim(name, r):
        if more:
            logger.log("  %-8s vs target: MS-SSIM %.5f over %d scales" % (name, r["msssim"], args.msssim_scales))

    report = {
        "denoised": metrics.evaluate(den, tgt, data_range=data_range, mask=mask,
                                     std=None if std is None else hwz(std), **more),
        "input": metrics.evaluate(inp, tgt, data_range=data_range, mask=mask, **more),
        "target": args.target_samples,
        "mask_threshold": args.metrics_mask_threshold,
    }
    if more:
        report["msssim_scales"] = args.msssim_scales
        report["msssim_weights"] = list(metrics.msssim_weights(args.msssim_scales))
    for name in ("input", "denoised"):
        r = report[name]
        logger.log("  %-8s vs target: PSNR %.3f dB  NRMSE %.5f  SSIM %.5f  MAE %.5g  bias %.5g  (L = %.6g, %d voxels)"
                   % (name, r["psnr"], r["nrmse"], r["ssim"], r["mae"], r["bias"], r["data_range"], r["n_voxels"]))
        log_msssim(name, r)
    if std is not None:
        r = report["denoised"]
        logger.log("  std map coverage: %.4f of the errors within 1 std, %.4f within 2"
                   % (r["coverage_1"], r["coverage_2"]))
    if quantiles is not None:
        report["denoised"]["quantiles"] = _quantile_block(
            args, quantiles, tgt, mask,
            lambda x: metrics.evaluate(x.contiguous(), tgt, data_range=data_range, mask=mask,
                                       std=None if std is None else hwz(std), **more))
    filtered = _baseline_volumes(args, inp)
    if filtered:
        report["baselines"] = {}
    for name, (x, params) in filtered.items():
        report["baselines"][name] = r = {**params,
                                         **metrics.evaluate(x, tgt, data_range=data_range, mask=mask, **more)}
        logger.log("  %-8s vs target: PSNR %.3f dB  NRMSE %.5f  SSIM %.5f  MAE %.5g  bias %.5g  (L = %.6g, %d voxels)"
                   % (name, r["psnr"], r["nrmse"], r["ssim"], r["mae"], r["bias"], r["data_range"], r["n_voxels"]))
        log_msssim(name, r)
    if args.spectrum:
        # the K stitched draws come one volume at a time; they are held only where the region block needs them again
        n_draws = args.num_draws if draws is not None and args.num_draws > 1 else 0
        draws = [] if draws is None else (list(draws) if roi is not None else draws)
        figs, report["spectrum"] = _spectrum_block(
            args, tgt, {"input": inp, "denoised": den, **{name: x for name, (x, _) in filtered.items()}}, draws,
            n_draws)
        report["input"]["spectrum"], report["denoised"]["spectrum"] = figs["input"], figs["denoised"]
        for name in filtered:
            report["baselines"][name]["spectrum"] = figs[name]
        draws = iter(draws) if roi is not None and draws else None
    if roi is not None:
        keep = None if weight is None else live.to(th.uint8).contiguous()
        report["roi"] = _roi_block(args, roi, tgt, inp, den, keep, draws, out_path=out_path,
                                   baselines={name: x for name, (x, _) in filtered.items()})
    if getattr(args, "regrid", None) is not None:
        plan = args.regrid["plan"]
        report["regrid"] = {"voxel_spacing": list(args.voxel_spacing), "model_spacing": list(args.model_spacing),
                            "mode": plan.mode, "native_shape": list(plan.shape_in),
                            "model_shape": list(plan.shape_out),
                            "effective_spacing": [s * r for s, r in zip(args.voxel_spacing, plan.scale)]}
    if cons is not None:
        report["consistency"] = _consistency_block(args, inp, den, mask)
    with open(path, "w") as f:
        json.dump(report, f, indent=2)
    logger.log(f"saved metrics to {path}")
    return path


def _counted(args, target):
    """--metrics_mask_threshold as _write_metrics applies it: (D, H, W) bool on the device, or None"""
    if target is None or not args.metrics_mask_threshold > 0:
        return None
    tgt = th.from_numpy(target).to(device=dist_util.dev(), dtype=th.float32)
    return tgt > args.metrics_mask_threshold * tgt.max()


class _PatchTrace:
    """--trace True on the independent paths: every batch gets a metrics.StepTrace whose target is the batch's
    target patches and whose weight is each patch's share of the one-shot Hann blend (patches.blend_shares; the
    product of three rows, rounded once to fp32), times the mask of --metrics_mask_threshold: every voxel the
    metrics file counts carries a total weight of 1 over the patches.  Target, mask and shares are cut once per
    batch.  The records travel with each round (dist_util.gather_round); rank 0 keeps them per (patch, draw) and
    pools them in that order, so the file depends on neither the batch size nor the world size."""

    def __init__(self, args, diffusion, vol, target, grid, bs, starts):
        self.args, self.grid, self.bs = args, grid, bs
        self.K, self.res, self.T = args.num_draws, args.large_size, diffusion.num_timesteps
        tmap = getattr(diffusion, "timestep_map", None) or list(range(self.T))
        self.t = [int(tmap[i]) for i in range(self.T - 1, -1, -1)]
        D, Hh, W = vol.shape
        xs, ys, zs = (list(v) for v in starts)           # the grid is their product, p = (ix * ny + iy) * nz + iz
        assert grid == [(x, y, z) for x in xs for y in ys for z in zs]
        self.ny, self.nz = len(ys), len(zs)
        self.sx, self.sy, self.sz = (patches.blend_shares(v, extent, self.res)
                                     for v, extent in ((xs, Hh), (ys, W), (zs, D)))
        self.target = target
        counted = _counted(args, target)
        self.counted = None if counted is None else counted.cpu().numpy()
        self.recs = {}

    def _cut(self, volume, g, dtype):
        xs, ys, zs = g
        r = self.res
        out = np.zeros((r, r, r), dtype=dtype)
        p = volume[zs:zs + r, xs:xs + r, ys:ys + r]
        out[:p.shape[0], :p.shape[1], :p.shape[2]] = p
        return out

    def begin(self, idx):
        """The StepTrace of the batch of patches idx (patch-major, draw-minor, like the batch)."""
        dev = dist_util.dev()
        weight, target = [], []
        for i in idx:
            ix, iy, iz = i // (self.ny * self.nz), (i // self.nz) % self.ny, i % self.nz
            w = ((self.sx[ix][None, :, None] * self.sy[iy][None, None, :])
                 * self.sz[iz][:, None, None]).astype(np.float32)                # (Z, H, W), like the samples
            if self.counted is not None:
                w = w * self._cut(self.counted, self.grid[i], np.float32)
            weight.append(w)
            if self.target is not None:
                target.append(self._cut(self.target, self.grid[i], np.float32))

        def up(blocks):
            t = th.from_numpy(np.stack(blocks)[:, None]).to(dev)
            return (t.repeat_interleave(self.K, dim=0) if self.K > 1 else t).contiguous()

        return metrics.StepTrace(target=up(target) if target else None, weight=up(weight))

    def gather(self, trace, b):
        """After round b's samples (every rank calls it; trace is None on a padding round)."""
        rows = self.bs * self.K
        block = th.zeros((self.T, rows, _hip.TR_REC), dtype=th.float64, device=dist_util.dev())
        if b is not None:
            rec = trace.device_records()
            block[:, :rec.shape[1]] = rec
        for bb, blk in dist_util.gather_round(block, b):
            if dist_util.rank() != 0:
                continue
            host = blk.cpu().numpy()
            for j, i in enumerate(range(bb * self.bs, min((bb + 1) * self.bs, len(self.grid)))):
                for d in range(self.K):
                    self.recs[(i, d)] = host[:, j * self.K + d]

    def write(self, out_path, metrics_path):
        keys = sorted(self.recs)
        assert keys == [(i, d) for i in range(len(self.grid)) for d in range(self.K)], "a patch was not traced"
        records = np.stack([self.recs[k] for k in keys], axis=1)               # (T, P * K, REC)
        return _write_trace(self.args, out_path, metrics_path, "patch", records, self.t, self.target is not None)


def _canvas_trace(args, vol, target, geom):
    """--trace True with --joint_patches: a StepTrace over the blended canvases; the weight is 1 inside the volume
    and on the mask of --metrics_mask_threshold, 0 on the rest of the canvas."""
    dev = dist_util.dev()
    D, Hh, W = vol.shape
    weight = th.zeros(tuple(geom.canvas), dtype=th.float32, device=dev)
    counted = _counted(args, target)
    weight[:D, :Hh, :W] = 1.0 if counted is None else counted.to(th.float32)
    tgt = None
    if target is not None:
        tgt = th.zeros(tuple(geom.canvas), dtype=th.float32, device=dev)
        tgt[:D, :Hh, :W] = th.from_numpy(target).to(dev)
    return metrics.StepTrace(target=tgt, weight=weight)


def _write_trace(args, out_path, metrics_path, pooling, records, t, has_target):
    """Rank 0, after the metrics file: trace_<name>.json beside the .npz from the (T, M, REC) records, pooled in
    index order; data_range is the number the metrics file reports."""
    data_range = None
    if metrics_path is not None:
        with open(metrics_path) as f:
            data_range = json.load(f)["denoised"]["data_range"]
    rows = metrics.trace_figures(records, data_range=data_range, has_target=has_target)
    keys = ("psnr", "nrmse", "mae", "bias", "mean", "std", "delta_rms", "clipped")
    sampler = "dpm_solver" if args.use_dpm_solver else "ddim" if args.use_ddim else "ddpm"
    report = {"sampler": sampler, "steps": len(rows), "pooling": pooling,
              "target": args.target_samples or None, "data_range": data_range,
              "mask_threshold": args.metrics_mask_threshold, "draws": args.num_draws,
              "n_voxels": int(round(rows[-1]["weight"] / args.num_draws)),
              "rows": [{"step": k, "t": t[k], **{key: r[key] for key in keys}} for k, r in enumerate(rows)]}
    show = lambda v, f="%.5g": "n/a" if v is None else f % v
    logger.log("per-step trace of pred_xstart (%s, %d steps, pooled per %s):" % (sampler, len(rows), pooling))
    for k in sorted({int(round(v)) for v in np.linspace(0, len(rows) - 1, min(len(rows), 10))}):
        r = report["rows"][k]
        logger.log("  step %4d  t %4d  PSNR %s dB  NRMSE %s  mean %s  std %s  delta_rms %s  clipped %s"
                   % (k, r["t"], show(r["psnr"], "%.3f"), show(r["nrmse"]), show(r["mean"]), show(r["std"]),
                      show(r["delta_rms"]), show(r["clipped"])))
    path = os.path.join(os.path.dirname(out_path), "trace_%s.json" % _base_name(args.base_samples))
    with open(path, "w") as f:
        json.dump(report, f, indent=2)
    logger.log(f"saved trace to {path}")
    return path


def _sampler(args, diffusion):
    if args.use_dpm_solver:
        return diffusion.dpm_solver_sample_loop, dict(order=args.solver_order, stochastic=args.solver_stochastic)
    if args.use_ddim:
        return diffusion.ddim_sample_loop, dict(eta=args.eta)
    return diffusion.p_sample_loop, {}


def _batch_noise(args, dev, idx, K, shape):
    """(x_T, the loop's noise arguments) of one batch: patches idx x K draws, patch-major.  All randomness is keyed by
    the GLOBAL patch index and the draw, so the result depends on neither the world size nor the batch size: one torch
    generator per (patch, draw), or, with --device_noise True, one stream of a NoiseKey each (x_T is then the key's
    draw 0, made by the loop)."""
    if args.device_noise:
        key = NoiseKey(args.noise_seed, [dist_util.noise_stream(i, d) for i in idx for d in range(K)], device=dev)
        return None, {"noise_key": key}
    gens = [dist_util.volume_generator(i, seed=10, device=dev, draw=d) for i in idx for d in range(K)]

    def draw(_k=None, _img=None):
        return th.cat([th.randn(1, *shape[1:], device=dev, generator=g) for g in gens])

    return draw(), {"step_noise": draw}


def _base_name(path):
    base = os.path.basename(path)
    for ext in (".tiff", ".tif", ".npz", ".npy"):
        if base.lower().endswith(ext):
            base = base[:-len(ext)]
    return base


class _Tiling(collections.namedtuple("_Tiling", "grid starts cond")):
    """How the independent paths see a grid: grid, the patch origins in patch order; starts = (x_starts, y_starts,
    z_starts), whose product the grid is; cond(idx) -> the (len(idx), 1, res, res, res) float32 device tensor of the
    conditioning patches idx (consecutive indices)."""


def _fixed_tiling(args, vol):
    """The reference's fixed 3 x 3 x (1 | 2) grid: patches cut (and zero-padded) on the host, uploaded per batch"""
    res = args.large_size
    low_res, grid = patches.split_volume(vol, res)               # (P, 1, Z, H, W)
    logger.log(f"volume {vol.shape}: {len(grid)} patches of {res}^3")
    gaps = patches.grid_gaps(vol.shape, res)
    if any(gaps.values()):
        logger.log("WARNING: the fixed 3 x 3 x (1 | 2) grid does not cover this volume (coordinates without a patch: "
                   + ", ".join("%d of %d along %s" % (gaps[a], n, a) for a, n in zip("DHW", vol.shape) if gaps[a])
                   + "); those voxels are written as 0.  --patch_overlap N tiles a volume of any size without gaps.")
    D, Hh, W = vol.shape
    dev = dist_util.dev()
    return _Tiling(grid, (patches.xy_starts(Hh, res), patches.xy_starts(W, res), patches.z_starts(D, res)),
                   lambda idx: th.from_numpy(low_res[idx]).to(dev))


def _sliding_tiling(args, vol):
    """--patch_overlap N: the gap-free sliding grid.  The volume is uploaded once as a zero-extended canvas and every
    batch's conditioning patches are cut from it on the device (ddpm3d_tiles_gather)."""
    res = args.large_size
    geom = patches.joint_geometry(vol.shape, res, min_overlap=args.patch_overlap)
    logger.log(f"volume {vol.shape}: {len(geom.grid)} patches of {res}^3 ({len(geom.x_starts)} x "
               f"{len(geom.y_starts)} x {len(geom.z_starts)} along H, W, D; neighbours overlap by at least "
               f"{args.patch_overlap})")
    canvas = joint._canvas_of(vol, geom, dist_util.dev())
    return _Tiling(geom.grid, (geom.x_starts, geom.y_starts, geom.z_starts),
                   lambda idx: joint.gather(canvas, geom, idx[0], len(idx)))


def _run_patches(args, model, diffusion, vol, tiling, target=None):
    """The independent paths, either grid, K = --num_draws >= 1.  Work units are batches of --batch_size patches;
    batch b goes to rank b mod W (scripts/test.py:243 with batch_size 1) and every rank runs the same number of
    rounds.  Every forward batch is bs patches x K draws, patch-major; the noise of draw d of patch i is keyed by
    (i, d) (_batch_noise), so the result depends on neither K, the batch size nor the world size.  Gathered rounds
    are blended on rank 0's device in ascending patch order as they arrive (uncertainty.VolumeStitcher:
    patches.stitch_patches' arithmetic), so no rank holds all patches.  -> _write_outputs' volumes on rank 0, None
    on the others."""
    dev = dist_util.dev()
    rank = dist_util.rank()
    K, res, bs = args.num_draws, args.large_size, max(1, args.batch_size)
    grid = tiling.grid
    sample_loop, extra = _sampler(args, diffusion)
    stitcher = uncertainty.VolumeStitcher(vol.shape, res, K, dev) if rank == 0 else None
    tracer = _PatchTrace(args, diffusion, vol, target, grid, bs, tiling.starts) if args.trace else None
    for b in dist_util.partition((len(grid) + bs - 1) // bs):
        block = th.zeros(bs * K, 1, res, res, res, device=dev)               # padded so collectives stay aligned
        if b is not None:
            idx = list(range(b * bs, min((b + 1) * bs, len(grid))))
            cond = tiling.cond(idx)
            if K > 1:
                cond = cond.repeat_interleave(K, dim=0)
            shape = tuple(cond.shape)
            noise, noise_args = _batch_noise(args, dev, idx, K, shape)
            logger.log(f"rank {rank}: patches {idx[0]}..{idx[-1]} x {K} draws shape={shape}")
            if tracer is not None:
                extra["trace"] = tracer.begin(idx)
            block[:len(idx) * K] = sample_loop(model, shape, noise, clip_denoised=args.clip_denoised,
                                               model_kwargs={"low_res": cond}, **noise_args, **extra, **_guide(args))
        for bb, blk in dist_util.gather_round(block, b):
            if stitcher is None:
                continue
            blk = blk.to(dev)
            for j, i in enumerate(range(bb * bs, min((bb + 1) * bs, len(grid)))):
                stitcher.add(i, blk[j * K:(j + 1) * K], grid[i])
        if tracer is not None:
            tracer.gather(extra.get("trace"), b)
    if rank != 0:
        return None
    logger.log("Reconstructing full image with Hann window blending...")
    return dict(_stitched_volumes(args, stitcher), trace=None if tracer is None else tracer.write)


def _stitched_volumes(args, stitcher):
    """Rank 0: the stitcher's accumulators -> the volumes _write_outputs takes, all (H, W, Z) on the file's grid:
    result, weight (the Hann weight sum, or with --model_spacing regrid.keep_after's mask), and with K >= 2 draws
    std, draws (the K stitched draws, one volume at a time) and qmaps (_quantile_maps)."""
    K = args.num_draws
    if K == 1:
        result, weight = stitcher.finish_single()
        return {"result": _regrid_back(args, result), "weight": _regrid_keep(args, weight)}
    mean, std, weight = stitcher.finish()
    draws = None
    if _regridding(args):                      # the K draws go back as one stack; moments on the file's grid
        draws = _regrid_back(args, th.stack([stitcher.draw(k) for k in range(K)]))
        mean, std = uncertainty.draw_moments(draws)
        weight = _regrid_keep(args, weight)
    qmaps = _quantile_maps(args, stitcher, draws)
    covered = std[weight > 0]
    logger.log(f"  Mean per-voxel std over {K} draws (voxels of non-zero weight): "
               f"{float(covered.double().mean()) if covered.numel() else 0.0:.6f}")
    return {"result": mean, "std": std, "weight": weight, "qmaps": qmaps,
            "draws": (stitcher.draw(k) for k in range(K)) if draws is None else iter(draws)}


def _write_outputs(args, native, target, roi, result, std=None, weight=None, draws=None, qmaps=None, trace=None):
    """Rank 0, every path: denoised_<name>.npz (arr_0 [+ std, quantiles, quantile_levels], (H, W, Z) like the
    reference), for .tif input denoised_<name>.tif [+ _std.tif] as (Z, H, W) float32 without scaling, then the
    metrics file and the trace file (trace(out_path, metrics_path) writes it).  native is the (D, H, W) input on the
    file's grid; result and std come as (H, W, Z) host arrays or device tensors and go on as host arrays.
    -> the .npz's path"""
    host = lambda x: x.cpu().numpy() if isinstance(x, th.Tensor) else x
    result, std = host(result), host(std)
    logger.log(f"  Original std: {float(native.std()):.4f}  Denoised std: {float(result.std()):.4f}")
    out_path = os.path.join(logger.get_dir(), f"denoised_{_base_name(args.base_samples)}.npz")
    logger.log(f"saving to {out_path}")
    np.savez(out_path, result, **({} if std is None else {"std": std}), **_quantile_arrays(args, qmaps))
    if args.base_samples.lower().endswith((".tif", ".tiff")):
        from guided_diffusion import tiff_io
        for path, x in ((out_path.replace(".npz", ".tif"), result), (out_path.replace(".npz", "_std.tif"), std)):
            if x is not None:
                tiff_io.imwrite(path, x.transpose(2, 0, 1).astype(np.float32))       # (H,W,Z) -> (Z,H,W)
                logger.log(f"Saved TIFF: {path}")
    if args.mip_angles is not None:
        _write_mip(args, out_path, native, target, result, std)
    mpath = _write_metrics(args, out_path, target, native, result, std=std, weight=weight, roi=roi, draws=draws,
                           quantiles=qmaps)
    if trace is not None:
        trace(out_path, mpath)
    return out_path


def _main_joint(args, model, diffusion, vol, target=None):
    """--joint_patches True: every rank holds the whole canvas and runs its share of each step's forwards
    (joint.sample_loop_progressive); rank 0 crops the canvas to the volume.  With --num_draws K >= 2 the K canvases
    are reduced to the per-voxel mean and sample std.  -> _write_outputs' volumes on rank 0, None on the others."""
    K, res = args.num_draws, args.large_size
    geom = patches.joint_geometry(vol.shape, res, min_overlap=args.patch_overlap if args.patch_overlap >= 0 else None)
    logger.log(f"volume {vol.shape}: {geom.n_patches} patches of {res}^3, sampled jointly on a {geom.canvas} canvas")
    more, out = {}, {}
    if args.trace:
        more["trace"] = trace = _canvas_trace(args, vol, target, geom)
        out["trace"] = lambda out_path, mpath: _write_trace(args, out_path, mpath, "canvas", trace.records(),
                                                            trace.t, target is not None)
    if args.device_noise:
        more["noise_key"] = joint.draw_key(args.noise_seed, K, dist_util.dev())
    sample = joint.sample_loop(diffusion, model, vol, geom, kind="ddim" if args.use_ddim else "ddpm", num_draws=K,
                               batch_size=max(1, args.batch_size), clip_denoised=args.clip_denoised, eta=args.eta,
                               device=dist_util.dev(), **more, **_guide(args))
    if dist_util.rank() != 0:
        return None
    draws = sample[:, :vol.shape[0], :vol.shape[1], :vol.shape[2]].contiguous()     # (K, D, H, W)
    if _regridding(args):
        draws = regrid.apply(draws, args.regrid["plan"].inverse())                  # the K draws back as one stack
    if K == 1:
        return dict(out, result=draws[0].permute(1, 2, 0))                          # (D, H, W) -> (H, W, Z)
    mean, std = uncertainty.draw_moments(draws)
    logger.log(f"  Mean per-voxel std over {K} draws: {float(std.double().mean()):.6f}")
    return dict(out, result=mean.permute(1, 2, 0), std=std.permute(1, 2, 0),
                draws=(draws[k].permute(1, 2, 0).contiguous() for k in range(K)),
                qmaps=_quantile_maps(args, draws=draws, to_hwz=(1, 2, 0)))


if __name__ == "__main__":
    main()
