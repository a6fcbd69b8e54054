"""
ctypes binding of include/ddpm3d.h (csrc/libddpm3d.so, gfx950).

There is deliberately no fallback: if the shared library is missing or a call
fails, a RuntimeError is raised.  torch is used here only for device memory
and the current HIP stream.
"""

import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# DDPM3D_LIB: developer override to A/B an experimental build of the same ABI
LIB_PATH = os.environ.get("DDPM3D_LIB") or os.path.normpath(os.path.join(_HERE, "..", "csrc", "libddpm3d.so"))

IN_SAME, IN_POOL, IN_UP, IN_PLANAR2, IN_STRIDE2 = 0, 1, 2, 3, 4
RES_NONE, RES_SAME, RES_POOL, RES_UP = 0, 1, 2, 3
ACT_NONE, ACT_SILU = 0, 1
OUT_NDHWC, OUT_NCDHW = 0, 1
F_LEARN_SIGMA, F_PREDICT_XSTART, F_CLIP = 1, 2, 4
NCOEF = 8
NQCOEF = 4      # [T][NQCOEF] forward-process table of the variational bound: sqrt_acp, sqrt_1m_acp, log_1m_acp,
                # posterior_log_variance_clipped
NSCOEF = 8      # [T][NSCOEF] DPM-Solver++ table: weights of x, m0, m1, m2, z (ddpm3d_dpm_solver_step)
S_CX, S_W0, S_W1, S_W2, S_CZ = 0, 1, 2, 3, 4
PREC_F32, PREC_F16X3, PREC_F16, PREC_F16X3_WZ, PREC_F16_WZ, PREC_BF16, PREC_BF16_WZ = 0, 1, 2, 3, 4, 5, 6
PRECISIONS = {"f32": PREC_F32, "f16x3": PREC_F16X3, "f16": PREC_F16, "bf16": PREC_BF16}
# the Winograd-along-depth form of a mode (same arithmetic, 2/3 of the MFMAs), where one exists
WINOGRAD_OF = {PREC_F16X3: PREC_F16X3_WZ, PREC_F16: PREC_F16_WZ, PREC_BF16: PREC_BF16_WZ}
# ddpm3d_conv_desc.io_dtype bits: which activation tensors hold bf16
IO_SRC0_BF16, IO_SRC1_BF16, IO_OUT_BF16, IO_RES_BF16 = 1, 2, 4, 8
IO_HALF_IS_F16 = 16    # the flagged tensors hold IEEE f16 (the --use_fp16 storage), not bf16
ABI_VERSION = 13
MAX_DRAWS = 64  # DDPM3D_MAX_DRAWS: draws per uncertainty map (ddpm3d_draw_stitch / ddpm3d_draw_moments)
MAX_QUANTILES = 8   # DDPM3D_MAX_QUANTILES: quantile levels per ddpm3d_draw_quantiles call
# ddpm3d_conv_desc.kernel_hint bits (launch orders of identical arithmetic; tests and A/B measurements)
HINT_WSTAT_OFF, HINT_WSTAT_ON = 0x100, 0x200
HINT_SPLITK_SHIFT = 16      # bits 16..21: forced split factor (measurement only, tools/splitk_sweep.py)
HINT_WZ_ORDER_SHIFT = 12     # bits 12..14: tap issue order of the f16x3 Winograd-D kernel (A/B measurements)
# w_packed is ddpm3d_pack_up_phase_weight's image: an IN_UP f16x3 Winograd-D conv runs as four 2x2 phase convs on
# the low-resolution source (the one hint that selects a weight image and so changes rounding)
HINT_UP_PHASE = 0x400
WZ_UP_PHASE_IMAGE = 0x100    # flag in ddpm3d_conv_weights.precision_wz: w_packed_wz is that image
SKIP_TWO_CALLS = 0x100       # flag in ddpm3d_conv_weights.precision of a skip conv: never plan ddpm3d_conv3d_skip

_fp = C.c_void_p


class ConvDesc(C.Structure):
    """struct ddpm3d_conv_desc (field order is the ABI)."""
    _fields_ = [
        ("N", C.c_int32), ("D", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
        ("Cin", C.c_int32), ("Cout", C.c_int32), ("ksize", C.c_int32), ("in_mode", C.c_int32),
        ("src0", _fp), ("src1", _fp), ("C0", C.c_int32), ("C1", C.c_int32),
        ("aff_a", _fp), ("aff_b", _fp), ("act", C.c_int32), ("precision", C.c_int32),
        ("w_packed", _fp), ("bias", _fp), ("bias_stride_n", C.c_int32), ("res_mode", C.c_int32),
        ("res", _fp), ("out", _fp), ("out_layout", C.c_int32), ("stats_rows", C.c_int32),
        ("stats", _fp), ("workspace", _fp), ("workspace_bytes", C.c_size_t),
        ("kernel_hint", C.c_int32), ("in_bound_count", C.c_int32), ("in_bound", _fp),
        ("in_bound_stride", C.c_int32), ("io_dtype", C.c_int32),
    ]


class ConvSkip(C.Structure):
    """struct ddpm3d_conv_skip: the ResBlock's 1x1 skip conv of ddpm3d_conv3d_skip"""
    _fields_ = [("src0", _fp), ("src1", _fp), ("C0", C.c_int32), ("C1", C.c_int32), ("w_packed", _fp), ("bias", _fp),
                ("in_bound", _fp), ("in_bound_count", C.c_int32), ("in_bound_stride", C.c_int32),
                ("io_dtype", C.c_int32)]


class ConvWeights(C.Structure):
    """struct ddpm3d_conv_weights"""
    _fields_ = [("w_packed", _fp), ("w_packed_wz", _fp), ("bias", _fp), ("Cout", C.c_int32), ("Cin", C.c_int32),
                ("ksize", C.c_int32), ("precision", C.c_int32), ("precision_wz", C.c_int32)]


class Layer(C.Structure):
    """struct ddpm3d_layer"""
    _fields_ = [("kind", C.c_int32), ("updown", C.c_int32), ("heads", C.c_int32), ("film_off", C.c_int32),
                ("norm1_gamma", _fp), ("norm1_beta", _fp), ("norm2_gamma", _fp), ("norm2_beta", _fp),
                ("conv1", ConvWeights), ("conv2", ConvWeights), ("skip", ConvWeights)]


class UnetDesc(C.Structure):
    """struct ddpm3d_unet_desc"""
    _fields_ = [("n_layers", C.c_int32), ("layers", C.POINTER(Layer)),
                ("n_input_blocks", C.c_int32), ("input_block_layers", C.POINTER(C.c_int32)),
                ("n_middle_layers", C.c_int32),
                ("n_output_blocks", C.c_int32), ("output_block_layers", C.POINTER(C.c_int32)),
                ("first", ConvWeights), ("out_gamma", _fp), ("out_beta", _fp), ("out", ConvWeights),
                ("film", C.c_int32), ("planar", C.c_int32), ("in_channels", C.c_int32), ("cin_pad", C.c_int32),
                ("arithmetic", C.c_int32)]


STEP_CONV, STEP_FINALIZE, STEP_ABSMAX, STEP_PAD, STEP_POOL_ACT, STEP_ATTENTION = range(6)
# ddpm3d_plan_step.flags: the arguments that belong to the forward call, not to the plan
STEP_X, STEP_LOW_RES, STEP_OUT, STEP_FILM, STEP_FILM_BIAS = 1, 2, 4, 8, 16


class PlanStep(C.Structure):
    """struct ddpm3d_plan_step: one call of a plan's launch list (ddpm3d_unet_plan_steps)"""
    _fields_ = [("kind", C.c_int32), ("flags", C.c_int32), ("film_off", C.c_int32), ("reserved", C.c_int32),
                ("conv", _fp), ("skip", _fp), ("in_", _fp * 4), ("out", _fp * 3), ("n", C.c_int64 * 8),
                ("count", C.c_double), ("eps", C.c_float)]


# DDPM3D_EM_*: columns of a ddpm3d_error_moments record
(EM_N, EM_SUM_E, EM_SUM_ABS_E, EM_SUM_SQ_E, EM_SUM_Y, EM_SUM_SQ_Y, EM_MIN_Y, EM_MAX_Y, EM_COVER_1, EM_COVER_2,
 EM_REC) = range(11)

# DDPM3D_TR_*: columns of a ddpm3d_trace_moments record
(TR_W, TR_N, TR_SUM_E, TR_SUM_ABS_E, TR_SUM_SQ_E, TR_SUM_SQ_Y, TR_SUM_X, TR_SUM_SQ_X, TR_SUM_SQ_D, TR_CLIPPED,
 TR_REC) = range(11)
TRACE_MAX_BATCH = 4096  # DDPM3D_TRACE_MAX_BATCH: estimates per ddpm3d_trace_moments call

MSSSIM_MAX_SCALES = 5   # DDPM3D_MSSSIM_MAX_SCALES: scales of ddpm3d_msssim3d

# DDPM3D_ROI_*: columns of a ddpm3d_roi_moments record, and the limits of a region index
(ROI_N, ROI_SUM_X, ROI_SUM_SQ_X, ROI_MIN_X, ROI_MAX_X, ROI_SUM_E, ROI_SUM_ABS_E, ROI_SUM_SQ_E, ROI_REC) = range(9)
ROI_MAX_REGIONS, ROI_CHUNK = 4096, 4096
# DDPM3D_TEX_*: the most grey levels of ddpm3d_roi_texture and the columns of its side counters
TEX_MAX_LEVELS = 64
(TEX_N, TEX_BELOW, TEX_ABOVE, TEX_PAIRS, TEX_REC) = range(5)
CCL_TILE = (8, 8, 64)   # DDPM3D_CCL_TILE_D / _H / _W: the brick one workgroup of ddpm3d_label_components labels in LDS
# DDPM3D_EDT_COLUMNS / _MAX_EXTENT: the columns a workgroup of ddpm3d_distance_sq stages in LDS, the longest line
EDT_COLUMNS, EDT_MAX_EXTENT = 16, 1024
PEAK_MAX_RADIUS = 8     # DDPM3D_PEAK_MAX_RADIUS: the largest per-axis radius, in voxels, of ddpm3d_sphere_mean's footprint
SMOOTH_MAX_RADIUS = 16  # DDPM3D_SMOOTH_MAX_RADIUS: the largest per-axis radius, in voxels, of ddpm3d_gauss_smooth's taps
NLM_MAX_SEARCH, NLM_MAX_PATCH = 5, 2    # DDPM3D_NLM_MAX_SEARCH / _PATCH: ddpm3d_nlm's largest window radii per axis
NLM_CUTOFF = 80.0       # DDPM3D_NLM_CUTOFF: beyond this exponent a candidate's weight is exactly 0

JOINT_MAX_STARTS = 8    # DDPM3D_JOINT_MAX_STARTS


class JointStarts(C.Structure):
    """struct ddpm3d_joint_starts"""
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("xs", C.c_int32 * JOINT_MAX_STARTS),
                ("ys", C.c_int32 * JOINT_MAX_STARTS), ("zs", C.c_int32 * JOINT_MAX_STARTS)]


class Tiling(C.Structure):
    """struct ddpm3d_tiling: host starts per axis (H, W, D) and the device copies of the starts, the per-coordinate
    {first covering patch, count} lookup and the three fp64 weight tables"""
    _fields_ = [("n", C.c_int32 * 3), ("starts", C.POINTER(C.c_int32) * 3), ("d_starts", C.c_void_p),
                ("d_cover", C.c_void_p), ("d_tables", C.c_void_p)]


class RoiIndex(C.Structure):
    """struct ddpm3d_roi_index: R regions over `entries` sorted flat voxel indices in CSR form; host offsets and the
    device copies of the offsets, the per-region first-chunk prefix and the index itself"""
    _fields_ = [("regions", C.c_int32), ("entries", C.c_int64), ("offsets", C.POINTER(C.c_int64)),
                ("d_offsets", C.c_void_p), ("d_chunks", C.c_void_p), ("d_index", C.c_void_p)]


SPEC_MAX_EXTENT = 2048  # DDPM3D_SPEC_MAX_EXTENT: the largest extent per axis of ddpm3d_dft3
# DDPM3D_SP_*: columns of a ddpm3d_shell_sums record (column 5 is padding)
(SP_N, SP_SUM_XX, SP_SUM_YY, SP_SUM_XY, SP_SUM_EE) = range(5)
SP_REC = 6


class DftAxis(C.Structure):
    """struct ddpm3d_dft_axis: transform length, table rows and the device cos / sin tables [rows][n]"""
    _fields_ = [("n", C.c_int32), ("rows", C.c_int32), ("cos_t", C.c_void_p), ("sin_t", C.c_void_p)]


class NoiseKeyDesc(C.Structure):
    """struct ddpm3d_noise_key: seed, device stream ids [N], draw, device origins [N][3] or NULL, and the patch and
    canvas extents (D, H, W order) the origins refer to"""
    _fields_ = [("seed", C.c_uint64), ("stream", C.c_void_p), ("draw", C.c_int64), ("origin", C.c_void_p),
                ("patch", C.c_int32 * 3), ("canvas", C.c_int32 * 3)]


REGRID_MAX_TAPS = 18    # DDPM3D_REGRID_MAX_TAPS: the most taps per output coordinate of a ddpm3d_regrid axis


class RegridAxis(C.Structure):
    """struct ddpm3d_regrid_axis: extents, tap capacity (0 = identity) and the device tables first [out_len], count
    [out_len] and weights [taps][out_len]"""
    _fields_ = [("in_len", C.c_int), ("out_len", C.c_int), ("taps", C.c_int), ("first", C.c_void_p),
                ("count", C.c_void_p), ("weights", C.c_void_p)]


PROJECT_MAX_ANGLES, PROJECT_MAX_BINS = 64, 4096     # DDPM3D_PROJECT_MAX_ANGLES / _BINS (bins and samples per ray)
PROJECT_MAX, PROJECT_SUM = 0, 1                     # DDPM3D_PROJECT_MAX / _SUM: the modes of ddpm3d_project


class ProjectTable(C.Structure):
    """struct ddpm3d_project_table: angles, bins, samples, the step in mm and per angle {h0, hu, hj, w0, wu, wj}"""
    _fields_ = [("angles", C.c_int32), ("bins", C.c_int32), ("samples", C.c_int32), ("step", C.c_float),
                ("coef", (C.c_float * 6) * PROJECT_MAX_ANGLES)]


LAYER_RES, LAYER_ATTN, LAYER_DOWNCONV, LAYER_UPCONV = 1, 2, 3, 4
UPDOWN = {None: 0, "down": 1, "up": 2}

EXPORTS = {
    # name: (restype, argtypes)
    "ddpm3d_abi_version": (C.c_int, []),
    "ddpm3d_last_error": (C.c_char_p, []),
    "ddpm3d_packed_weight_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "ddpm3d_pack_conv_weight": (C.c_int, [_fp, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp]),
    "ddpm3d_packed_up_phase_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "ddpm3d_pack_up_phase_weight": (C.c_int, [_fp, C.c_int, C.c_int, _fp, _fp]),
    "ddpm3d_conv_stats_rows": (C.c_int, [C.c_int] * 8),
    "ddpm3d_conv_workspace_bytes": (C.c_size_t, [C.c_int] * 8),
    "ddpm3d_conv3d": (C.c_int, [C.POINTER(ConvDesc), _fp]),
    "ddpm3d_conv_kernel_family": (C.c_int, [C.POINTER(ConvDesc), C.c_char_p, C.c_int]),
    "ddpm3d_conv_plan": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(C.c_int), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    "ddpm3d_conv3d_skip": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(ConvSkip), _fp]),
    "ddpm3d_conv_skip_fused": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(ConvSkip)]),
    "ddpm3d_conv_kernel_instance": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(ConvSkip), C.c_char_p, C.c_int]),
    "ddpm3d_unet_plan_bytes": (C.c_size_t, [C.POINTER(UnetDesc), C.c_int, C.c_int, C.c_int, C.c_int]),
    "ddpm3d_unet_plan_create": (C.c_int, [C.POINTER(UnetDesc), C.c_int, C.c_int, C.c_int, C.c_int, _fp, C.c_size_t,
                                          C.POINTER(_fp)]),
    "ddpm3d_unet_forward": (C.c_int, [_fp, _fp, _fp, _fp, C.c_int, _fp, _fp]),
    "ddpm3d_unet_plan_destroy": (None, [_fp]),
    "ddpm3d_unet_plan_steps": (C.c_int, [_fp, C.POINTER(PlanStep), C.c_int]),
    "ddpm3d_unet_last_error": (C.c_char_p, []),
    "ddpm3d_gn_finalize": (C.c_int, [_fp, C.c_int, C.c_int, _fp, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_double, C.c_float, _fp, _fp, _fp, C.c_int, C.c_int, _fp, _fp, _fp, _fp]),
    "ddpm3d_absmax": (C.c_int, [_fp, _fp, C.c_int, C.c_size_t, _fp, _fp]),
    "ddpm3d_gn_stats_rows": (C.c_int, [C.c_int]),
    "ddpm3d_gn_stats": (C.c_int, [_fp, C.c_int, C.c_int, C.c_int, _fp, _fp]),
    "ddpm3d_timestep_embedding": (C.c_int, [_fp, C.c_int, C.c_int, _fp, _fp, _fp]),
    "ddpm3d_linear": (C.c_int, [_fp, C.c_int, C.c_int, _fp, _fp, C.c_int, C.c_int, _fp, C.c_int, _fp]),
    "ddpm3d_attention": (C.c_int, [_fp, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp]),
    "ddpm3d_attention_p": (C.c_int, [_fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _fp, C.c_int, C.c_int,
                                     _fp, _fp]),
    "ddpm3d_ncdhw_to_ndhwc": (C.c_int, [_fp, C.c_int, C.c_int, C.c_int, _fp, _fp]),
    "ddpm3d_ndhwc_to_ncdhw": (C.c_int, [_fp, C.c_int, C.c_int, C.c_int, _fp, _fp]),
    "ddpm3d_ncdhw_to_ndhwc_pad": (C.c_int, [_fp, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp]),
    "ddpm3d_subsample_hw2": (C.c_int, [_fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp]),
    "ddpm3d_p_sample_step": (C.c_int, [_fp, _fp, _fp, _fp, _fp, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp]),
    "ddpm3d_ddim_step": (C.c_int, [_fp, _fp, _fp, _fp, _fp, C.c_int, C.c_int, C.c_int, C.c_float,
                                   _fp, _fp, _fp]),
    "ddpm3d_add_embedding": (C.c_int, [_fp, _fp, _fp, C.c_int, C.c_int, C.c_int, _fp]),
    "ddpm3d_pool_act": (C.c_int, [_fp, _fp, _fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _fp,
                                  C.c_int, _fp]),
    "ddpm3d_q_sample": (C.c_int, [_fp, _fp, _fp, _fp, C.c_int, C.c_int, C.c_int, _fp, _fp]),
    "ddpm3d_vb_terms_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "ddpm3d_vb_terms": (C.c_int, [_fp, _fp, _fp, _fp, _fp, _fp, _fp, C.c_int, C.c_int, C.c_int, C.c_int, _fp,
                                  C.c_size_t, _fp, _fp, _fp, C.c_int, _fp, _fp]),
    "ddpm3d_prior_bpd": (C.c_int, [_fp, _fp, C.c_int, C.c_int, C.c_int, _fp, C.c_size_t, _fp, _fp]),
    "ddpm3d_p_mean_variance": (C.c_int, [_fp, _fp, _fp, _fp, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp,
                                         _fp, _fp]),
    "ddpm3d_ddim_reverse_step": (C.c_int, [_fp, _fp, _fp, _fp, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp]),
    "ddpm3d_dpm_solver_step": (C.c_int, [_fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, C.c_int, C.c_int, C.c_int,
                                         C.c_int, C.c_int, _fp, _fp, _fp]),
    "ddpm3d_draw_stitch": (C.c_int, [_fp, C.c_int, C.c_int, _fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                     _fp, _fp, _fp]),
    "ddpm3d_draw_moments": (C.c_int, [_fp, _fp, C.c_int, C.c_int64, _fp, _fp, _fp]),
    "ddpm3d_draw_quantiles": (C.c_int, [_fp, _fp, C.c_int, C.c_int64, C.c_int, C.POINTER(C.c_int),
                                        C.POINTER(C.c_float), _fp, _fp, _fp, _fp, _fp]),
    "ddpm3d_joint_gather": (C.c_int, [_fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(JointStarts),
                                      C.c_int, C.c_int, _fp, _fp]),
    "ddpm3d_joint_blend": (C.c_int, [_fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(JointStarts), _fp,
                                     _fp, _fp]),
    "ddpm3d_tiles_gather": (C.c_int, [_fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Tiling), C.c_int,
                                      C.c_int, _fp, _fp]),
    "ddpm3d_tiles_blend": (C.c_int, [_fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Tiling), _fp, _fp]),
    "ddpm3d_error_moments_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int64]),
    "ddpm3d_error_moments": (C.c_int, [_fp, _fp, _fp, _fp, C.c_int, C.c_int64, _fp, C.c_size_t, _fp, _fp]),
    "ddpm3d_ssim3d_workspace_bytes": (C.c_size_t, [C.c_int] * 4),
    "ddpm3d_ssim3d": (C.c_int, [_fp, _fp, _fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, _fp,
                                C.c_size_t, _fp, _fp, _fp]),
    "ddpm3d_trace_moments_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int64]),
    "ddpm3d_trace_moments": (C.c_int, [_fp, _fp, _fp, _fp, C.c_int, C.c_int64, C.c_int64, C.c_int64, _fp, C.c_size_t,
                                       _fp, _fp]),
    "ddpm3d_pool2": (C.c_int, [_fp, _fp, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp]),
    "ddpm3d_msssim3d_workspace_bytes": (C.c_size_t, [C.c_int] * 5),
    "ddpm3d_msssim3d": (C.c_int, [_fp, _fp, _fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                                  _fp, C.c_size_t, _fp, _fp]),
    "ddpm3d_roi_moments_workspace_bytes": (C.c_size_t, [C.c_int, C.POINTER(RoiIndex)]),
    "ddpm3d_roi_moments": (C.c_int, [_fp, _fp, C.c_int, C.c_int64, C.POINTER(RoiIndex), _fp, C.c_size_t, _fp, _fp]),
    "ddpm3d_roi_texture": (C.c_int, [_fp] + [C.c_int] * 4 + [C.POINTER(RoiIndex), _fp, _fp, _fp, C.c_int, _fp, _fp, _fp,
                                     _fp]),
    "ddpm3d_dft3_workspace_bytes": (C.c_size_t, [C.c_int] * 4),
    "ddpm3d_dft3": (C.c_int, [_fp, _fp] + [C.c_int] * 4 + [C.POINTER(DftAxis), _fp, C.c_size_t, _fp, _fp, _fp]),
    "ddpm3d_dft3_pass": (C.c_int, [C.c_int, _fp, _fp] + [C.c_int] * 4 + [C.POINTER(DftAxis), _fp, C.c_size_t, _fp, _fp,
                                   _fp]),
    "ddpm3d_shell_sums_workspace_bytes": (C.c_size_t, [C.c_int, C.POINTER(RoiIndex)]),
    "ddpm3d_shell_sums": (C.c_int, [_fp] * 4 + [C.c_int] * 4 + [C.POINTER(RoiIndex), _fp, C.c_size_t, _fp, _fp]),
    "ddpm3d_shell_spectrum_workspace_bytes": (C.c_size_t, [C.c_int] * 4 + [C.POINTER(RoiIndex), C.c_int]),
    "ddpm3d_shell_spectrum": (C.c_int, [_fp] * 4 + [C.c_int] * 4 + [C.POINTER(DftAxis), C.POINTER(RoiIndex), _fp,
                                        C.c_size_t, _fp, _fp]),
    "ddpm3d_label_components_workspace_bytes": (C.c_size_t, [C.c_int] * 3),
    "ddpm3d_label_components": (C.c_int, [_fp, _fp, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp,
                                          C.c_size_t, _fp, _fp]),
    "ddpm3d_sphere_mean": (C.c_int, [_fp, _fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.POINTER(C.c_int32), _fp, _fp]),
    "ddpm3d_gauss_smooth_workspace_bytes": (C.c_size_t, [C.c_int] * 3),
    "ddpm3d_gauss_smooth": (C.c_int, [_fp] + [C.c_int] * 6 + [C.POINTER(C.c_float)] * 3 + [_fp, _fp, C.c_size_t, _fp]),
    "ddpm3d_nlm": (C.c_int, [_fp] + [C.c_int] * 9 + [C.c_float, C.c_float, _fp, _fp]),
    "ddpm3d_regrid_workspace_bytes": (C.c_size_t, [C.c_int] * 7),
    "ddpm3d_regrid": (C.c_int, [_fp] + [C.c_int] * 4 + [C.POINTER(RegridAxis), _fp, _fp, C.c_size_t, _fp]),
    "ddpm3d_project_table_fill": (C.c_int, [C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_double,
                                            C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(ProjectTable)]),
    "ddpm3d_project": (C.c_int, [_fp] + [C.c_int] * 4 + [C.POINTER(ProjectTable), C.c_int, _fp, _fp]),
    "ddpm3d_distance_sq": (C.c_int, [_fp] + [C.c_int] * 5 + [C.c_double] * 3 + [_fp, _fp]),
    "ddpm3d_basins_workspace_bytes": (C.c_size_t, [C.c_int] * 3),
    "ddpm3d_basins": (C.c_int, [_fp, _fp] + [C.c_int] * 4 + [_fp, _fp, C.c_size_t, _fp, _fp]),
    "ddpm3d_basin_saddles_workspace_bytes": (C.c_size_t, [C.c_int] * 3),
    "ddpm3d_basin_saddles": (C.c_int, [_fp] * 3 + [C.c_int] * 5 + [_fp, _fp, _fp, C.c_size_t, _fp, _fp]),
    "ddpm3d_noise_fill": (C.c_int, [C.POINTER(NoiseKeyDesc), C.c_int, C.c_int, _fp, _fp]),
    "ddpm3d_noise_bits": (C.c_int, [C.POINTER(NoiseKeyDesc), C.c_int, C.c_int, _fp, _fp]),
    "ddpm3d_p_sample_step_keyed": (C.c_int, [_fp, _fp, C.POINTER(NoiseKeyDesc), _fp, _fp, C.c_int, C.c_int, C.c_int,
                                             _fp, _fp, _fp]),
    "ddpm3d_ddim_step_keyed": (C.c_int, [_fp, _fp, C.POINTER(NoiseKeyDesc), _fp, _fp, C.c_int, C.c_int, C.c_int,
                                         C.c_float, _fp, _fp, _fp]),
    "ddpm3d_dpm_solver_step_keyed": (C.c_int, [_fp, _fp, _fp, _fp, C.POINTER(NoiseKeyDesc), _fp, _fp, _fp, C.c_int,
                                               C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp]),
    "ddpm3d_q_sample_keyed": (C.c_int, [_fp, C.POINTER(NoiseKeyDesc), _fp, _fp, C.c_int, C.c_int, C.c_int, _fp, _fp]),
    "ddpm3d_xstart_pull_workspace_bytes": (C.c_size_t, [C.c_int] * 4),
    "ddpm3d_xstart_pull": (C.c_int, [_fp] * 5 + [C.c_int] * 6 + [C.c_float] + [C.c_int] * 3
                           + [C.POINTER(C.c_float)] * 3 + [_fp, _fp, C.c_size_t, _fp]),
    "ddpm3d_p_sample_step_x0": (C.c_int, [_fp, _fp, _fp, _fp, C.POINTER(NoiseKeyDesc), _fp, _fp, C.c_int, C.c_int,
                                          C.c_int, _fp, _fp, _fp]),
    "ddpm3d_ddim_step_x0": (C.c_int, [_fp, _fp, _fp, _fp, C.POINTER(NoiseKeyDesc), _fp, _fp, C.c_int, C.c_int, C.c_int,
                                      C.c_float, _fp, _fp, _fp]),
    "ddpm3d_dpm_solver_step_x0": (C.c_int, [_fp, _fp, _fp, _fp, _fp, _fp, C.POINTER(NoiseKeyDesc), _fp, _fp, _fp,
                                            C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp]),
    "ddpm3d_mfma_probe_flops_per_iter": (C.c_double, [C.c_int]),
    "ddpm3d_mfma_probe": (C.c_int, [C.c_int, C.c_int, C.c_int, _fp, _fp, _fp]),
}

_lib = None


def load():
    """The loaded library (cached).  Raises if it is absent or of another ABI."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "ddpm3d HIP library not found at %s -- build it with "
            "`make -C 3d-denoising-diffusion-model_amd/csrc` (or __graft_entry__.build()); "
            "there is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in EXPORTS.items():
        fn = getattr(lib, name)  # AttributeError if a declared symbol is missing
        fn.restype = res
        fn.argtypes = args
    if lib.ddpm3d_abi_version() != ABI_VERSION:
        raise RuntimeError("libddpm3d ABI %d, binding expects %d" % (lib.ddpm3d_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


E_INVAL, E_LAUNCH, E_NOSUP, E_2BIG = -1, -2, -3, -4
PROBE_F16_32X32X16, PROBE_F16_16X16X32, PROBE_F32_32X32X2, PROBE_BF16_32X32X16, PROBE_BF16_16X16X32 = 0, 1, 2, 3, 4


class Ddpm3dError(RuntimeError):
    """A failed C-ABI call; `.code` is the DDPM3D_E* value it returned."""

    def __init__(self, code, msg):
        super().__init__("ddpm3d error %d: %s" % (code, msg))
        self.code = code


def check(rc):
    if rc != 0:
        raise Ddpm3dError(rc, load().ddpm3d_last_error().decode())


def conv_plan(desc):
    """(stats rows, workspace bytes, split factor over Cin) of ddpm3d_conv3d on this descriptor"""
    rows, ws, split = C.c_int(0), C.c_size_t(0), C.c_int(0)
    check(load().ddpm3d_conv_plan(C.byref(desc), C.byref(rows), C.byref(ws), C.byref(split)))
    return rows.value, ws.value, split.value


def conv_instance(desc, skip=None):
    """the kernel instance ddpm3d_conv3d (skip None) or ddpm3d_conv3d_skip runs, e.g. "conv3d_wz_kernel<0,4,8,4>" """
    name = C.create_string_buffer(96)
    check(load().ddpm3d_conv_kernel_instance(C.byref(desc), None if skip is None else C.byref(skip), name, 96))
    return name.value.decode()


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return 0 if t is None else t.data_ptr()


def require_device(t, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise RuntimeError("%s must live on the GPU: this package runs on HIP kernels only "
                           "(got %s)" % (what, getattr(t, "device", type(t))))
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise RuntimeError("%s must be contiguous float32" % what)
