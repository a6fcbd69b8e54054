"""
The fp32-grade conv kernels (precision 0: exact fp32 MFMA; 1: f16x3 in the direct, 1x1 and last-layer kernels;
3: f16x3 on the Winograd-D form) against an emulation of their own arithmetic (conv32_emul.py), element by
element.

The emulation rounds where the kernels round (the GroupNorm affine as fmaf, the SiLU, pool means, the
activation and weight scales, the hi / lo split, the Winograd-D input and weight transforms), with exact
products -- hi*hi + hi*lo + lo*hi in the split modes, lo*lo left out as the kernels leave it out -- and fp64
sums.  What it cannot reproduce is (a) the order of the fp32 accumulation and (b) the last ulps of the SiLU.
The bars bound exactly those two, per output element v, with the model of test_gpu_conv16.py:

  (a) fp32 accumulation.  An accumulator takes m rounded additions: p per term (p = 3 MFMA products per term in
      the f16x3 modes, 1 in the exact mode) over K = taps x CinPad terms (27 or 1 taps per input channel in the
      direct kernels, 9 per transformed accumulator in the Winograd-D form, which sums three accumulators in its
      output transform), plus the split-K slab sums (S), the epilogue's bias and residual additions and the
      reduce: m = p K + S + 8.  Rounding i adds e_i = d_i P_i, |d_i| <= u = 2^-24, P_i the partial sum it rounds.
      With the d_i independent and zero-mean, sum e_i has variance <= u^2/3 sum P_i^2, and for a fixed order
      sum P_i^2 <= m (sum t_j^2 + acc^2) (a random walk plus the drift to the final value): `sqterms`, summed over
      the accumulators an output combines.  Bar: 8 sigma, E_acc = 8 u sqrt(m sqterms / 3).  The Winograd-D
      output transform adds two roundings of |M0| + |M1| + |M2| (`trabs`), the epilogue's bias and residual
      additions one each of |out|: + 2u (trabs + |out|).
  (b) the SiLU.  The kernels' SiLU (expf and an IEEE divide in the exact mode; v_exp_f32 / v_rcp_f32 in the
      f16x3 modes) differs from the emulation's correctly rounded steps by at most delta = 2^-24 (8 + 2|y|) |v|
      per operand (conv32_emul._silu).  In the exact mode that moves the output by at most sum delta |w|.  In the
      split modes the kernel then splits its own value: lo lands on a different f16 grid point (one ulp of lo),
      and where hi can round the other way the weight's lo meets the other hi.  The emulator sums
      (delta + ulp(lo)) |w_hi| + (hi flip) |w_lo| over the operands: `silu`, a rigorous bound.  Without an
      activation it is zero and only (a) remains.

Per element:              |got - emul| <= E_acc + silu                              (`elem_bound`)
the classical form:       |got - emul| <= 7 u sqrt(m) sum|terms| + silu              (Hoeffding: P < 1e-10)
Per (sample, output channel): max|got - emul| / max|emul| <= max(E_acc + silu) / max|emul|.
Statistics: against the fp64 sums of the emulation's output, within the sum of the element bounds.  Every case
runs twice: bitwise equal.

test_f16x3_error_against_fp64_within_twice_f32 pins DESIGN.md §3.1d's claim across the f16x3 cases: per
(sample, cout), the f16x3 kernel's error against the fp64 convolution is at most twice the exact mode's on the
same inputs plus 4u max|ref|.  test_conv32_emul_cpu.py proves on the CPU that each case's bar sees the plausible
bugs by at least 10x, and test_plan_tuples_are_covered ties the table to the routes the f16x3 and f32 plans take.
"""

import dataclasses
import math
from dataclasses import dataclass

import numpy as np
import pytest
import torch

import conv32_emul as E
import test_gpu_conv16 as G16

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
IN, RES = G16.IN, G16.RES
ALT_MAX = 2.0 - 2.0 ** -12      # mantissa of the bound just below 2: gain 1 instead of 2 would overflow V2 = d2 - d1


@dataclass
class Case:
    name: str
    prec: int                 # 0 (f32), 1 (f16x3), 3 (f16x3 Winograd-D)
    family: str               # ddpm3d_conv_kernel_family's answer the case claims
    wz: str = "8,8"           # Winograd-D: the tile (TX, TY) of the instance the case is meant for (t4 families: 4,4)
    inst: str = ""            # ddpm3d_conv_kernel_instance's answer, where it is not test_gpu_conv16.claimed_instance's
    N: int = 1
    D: int = 5
    H: int = 8
    W: int = 10
    C: tuple = (32,)          # channels per source (two = virtual concat)
    Cout: int = 128
    k: int = 3
    in_mode: str = "same"
    res_mode: str = "none"
    act: bool = True          # GroupNorm affine + SiLU (affine without SiLU when act is False and aff is True)
    aff: bool = True
    ncdhw: bool = False
    stats: bool = True
    split: int = 0            # 0: the rule's split; > 1: forced through kernel_hint
    expect_split: bool = False
    mags: tuple = (1.0,)      # per-sample magnitude of the input
    small_cout: bool = False  # one output channel with weights 1e-5 of the others
    loose: float = 1.0        # in_bound = loose x the true maximum
    alt_max: bool = False     # |x| = ALT_MAX everywhere, the sign alternating along depth
    seed: int = 0

    def key(self):
        return (self.family, self.prec, IN[self.in_mode], RES[self.res_mode], int(self.act), 0, self.expect_split)


def _modes(name, precs, family_fmt, **kw):
    """the same case in each of the given precisions"""
    return [Case("%s_p%d" % (name, p), p, family_fmt % p, **kw) for p in precs]


D8, D4 = "conv3d_p%d_k3_wn4_t8", "conv3d_p%d_k3_wn4_t4"
K18, K14 = "conv3d_p%d_k1_wn4_t8", "conv3d_p%d_k1_wn4_t4"
R8 = dict(D=5, H=8, W=10, wz="8,8")     # 8x8 tiles (Winograd-D: 8x8x2), odd D, ragged W
R84 = dict(D=8, H=8, W=12, wz="8,4")    # Winograd-D 8x4x4 tiles (H % 8 == 0, D % 4 == 0), ragged W
R4 = dict(D=9, H=4, W=6, wz="4,4")      # 4x4 tiles (Winograd-D: 4x4x8), D not a multiple of 8, ragged W
FS = dict(split=2, expect_split=True)
NOIN = dict(aff=False, act=False)
DIRECT = (0, 1)

CASES = []
# ---- the Winograd-D form (precision 3): three tile geometries, with and without a forced split
for geo, fam in ((R8, D8), (R84, D8), (R4, D4)):
    g = "t%dx%dx%d" % ((8, 8, 2) if geo is R8 else (8, 4, 4) if geo is R84 else (4, 4, 8))
    for sp, sk in ((dict(), ""), (FS, "_split")):
        CASES += _modes("wz_%s_conv1%s" % (g, sk), (3,), fam, Cout=256 if geo is R8 else 128, **geo, **sp)
        CASES += _modes("wz_%s_resid%s" % (g, sk), (3,), fam, res_mode="same", **geo, **sp)
        CASES += _modes("wz_%s_resid_pool%s" % (g, sk), (3,), fam, res_mode="pool", **geo, **sp)
        CASES += _modes("wz_%s_resid_up%s" % (g, sk), (3,), fam, res_mode="up", **geo, **sp)
        CASES += _modes("wz_%s_aff_noact%s" % (g, sk), (3,), fam, act=False, **geo, **sp)
        CASES += _modes("wz_%s_raw%s" % (g, sk), (3,), fam, **NOIN, **geo, **sp)
        CASES += _modes("wz_%s_concat%s" % (g, sk), (3,), fam, C=(16, 32) if sp else (16, 16), **geo, **sp)
        CASES += _modes("wz_%s_up%s" % (g, sk), (3,), fam, in_mode="up", **geo, **sp)
CASES += [
    *_modes("wz_d1", (3,), D8, D=1, H=8, W=8, res_mode="same"),
    *_modes("wz_d1_t4", (3,), D4, D=1, H=4, W=4),
    # (48 and 64 input channels: the rule splits them in two)
    *_modes("wz_d3_two_cout_blocks", (3,), D8, D=3, H=9, W=11, C=(32, 16), Cout=256, expect_split=True),
    *_modes("wz_up_concat_resid_up", (3,), D8, in_mode="up", C=(32, 32), res_mode="up", expect_split=True, **R84),
]
# ---- the direct kernels (precisions 0 and 1): t8 / t4 tiles at each WN the rule picks (Cout > 64: 4, > 32: 2,
# else 1), partial cout tiles, every input and residual mode, concat, affine with / without SiLU, raw input
CASES += [
    *_modes("direct_t8_wn4_partial_cout", DIRECT, D8, Cout=96, **R8),
    *_modes("direct_t8_wn2", DIRECT, "conv3d_p%d_k3_wn2_t8", Cout=64, act=False, **R8),
    *_modes("direct_t8_wn1", DIRECT, "conv3d_p%d_k3_wn1_t8", Cout=32, **NOIN, **R8),
    *_modes("direct_t4_wn4_partial_cout", DIRECT, D4, Cout=160, res_mode="same", **R4),
    *_modes("direct_t4_wn2", DIRECT, "conv3d_p%d_k3_wn2_t4", Cout=48, **R4),
    *_modes("direct_t4_wn1", DIRECT, "conv3d_p%d_k3_wn1_t4", Cout=16, act=False, **R4),
    *_modes("direct_t8_resid_pool", DIRECT, D8, Cout=96, res_mode="pool", **R8),
    *_modes("direct_t8_resid_up", DIRECT, D8, Cout=96, res_mode="up", **R8),
    *_modes("direct_t8_concat", DIRECT, D8, C=(16, 16), Cout=96, **R8),
    *_modes("direct_t8_up", DIRECT, D8, in_mode="up", Cout=96, **R8),
    *_modes("direct_t4_up_resid_up", DIRECT, D4, in_mode="up", Cout=96, res_mode="up", D=5, H=4, W=8),
    *_modes("direct_pool_t8", DIRECT, D8, in_mode="pool", **R8),
    *_modes("direct_pool_t8_resid_pool", DIRECT, D8, in_mode="pool", res_mode="pool", Cout=96, **R8),
    *_modes("direct_pool_t4_noact", DIRECT, D4, in_mode="pool", act=False, **R4),
    *_modes("direct_stride2_t4", DIRECT, D4, in_mode="stride2", D=4, H=6, W=6),
    *_modes("direct_stride2_t8", DIRECT, D8, in_mode="stride2", D=3, H=8, W=9, **NOIN),
    *_modes("direct_planar_t8", DIRECT, D8, in_mode="planar", C=(1, 1), **NOIN, **R8),
    *_modes("direct_planar_t4", DIRECT, D4, in_mode="planar", C=(1, 1), **NOIN, **R4),
    *_modes("direct_t4_split", DIRECT, D4, C=(64,), **R4, **FS),
    *_modes("direct_t8_split_resid", DIRECT, D8, C=(64,), res_mode="same", **R8, **FS),
    *_modes("direct_t8_split_resid_pool", DIRECT, D8, C=(64,), in_mode="pool", res_mode="pool", **R8, **FS),
    # the exact mode's own Winograd-free layers of the f32 plans: Cout % 128 == 0, same / up input, and the
    # split ones, in every input and residual mode the f32 plans split
    *_modes("direct_t8_cout128_resid", (0,), D8, res_mode="same", **R84),
    *_modes("direct_t4_cout128_up", (0,), D4, in_mode="up", res_mode="up", D=5, H=4, W=8),
    *_modes("direct_t8_split", (0,), D8, C=(64,), **R8, **FS),
    *_modes("direct_t8_split_resid_up", (0,), D8, C=(64,), res_mode="up", **R8, **FS),
    *_modes("direct_t8_split_pool", (0,), D8, C=(64,), in_mode="pool", **R8, **FS),
    *_modes("direct_t8_split_up", (0,), D8, C=(64,), in_mode="up", **R8, **FS),
    *_modes("direct_t8_split_resid_pool_only", (0,), D8, C=(64,), res_mode="pool", **R8, **FS),
    *_modes("direct_t4_split_resid", (0,), D4, C=(64,), res_mode="same", **R4, **FS),
    *_modes("direct_t4_split_resid_pool", (0,), D4, C=(64,), res_mode="pool", **R4, **FS),
    *_modes("direct_t4_split_resid_up", (0,), D4, C=(64,), res_mode="up", **R4, **FS),
    *_modes("direct_t4_split_pool", (0,), D4, C=(64,), in_mode="pool", **R4, **FS),
    *_modes("direct_t4_split_up", (0,), D4, C=(64,), in_mode="up", **R4, **FS),
]
# ---- the 2-D network's layers (depth-1 volumes; 32 and 64 channels: WN 1 and 2), in both modes
R2 = dict(D=1, H=8, W=12)
CASES += [
    *_modes("d1_wn1_conv", DIRECT, "conv3d_p%d_k3_wn1_t8", Cout=32, **R2),
    *_modes("d1_wn1_resid", DIRECT, "conv3d_p%d_k3_wn1_t8", Cout=32, res_mode="same", **R2),
    *_modes("d1_wn1_upsample", DIRECT, "conv3d_p%d_k3_wn1_t8", Cout=32, in_mode="up", **NOIN, **R2),
    *_modes("d1_wn1_downsample", DIRECT, "conv3d_p%d_k3_wn1_t8", Cout=32, in_mode="stride2", **NOIN, **R2),
    *_modes("d1_wn2_resid", DIRECT, "conv3d_p%d_k3_wn2_t8", C=(64,), Cout=64, res_mode="same", **R2),
    *_modes("d1_wn2_upsample", DIRECT, "conv3d_p%d_k3_wn2_t8", C=(64,), Cout=64, in_mode="up", **NOIN, **R2),
    *_modes("d1_wn2_downsample", DIRECT, "conv3d_p%d_k3_wn2_t8", Cout=64, in_mode="stride2", **NOIN, **R2),
    *_modes("d1_k1_wn1_skip", DIRECT, "conv3d_p%d_k1_wn1_t8", C=(64,), Cout=32, k=1, **NOIN, **R2),
    *_modes("d1_k1_wn2_skip", DIRECT, "conv3d_p%d_k1_wn2_t8", Cout=64, k=1, **NOIN, **R2),
    *_modes("d1_k1_wn2_proj_out", DIRECT, "conv3d_p%d_k1_wn2_t8", C=(64,), Cout=64, k=1, res_mode="same", **NOIN,
            **R2),
]
# ---- the published level shapes, the rule's split (384 -> 384 @ 16x8x8, 512 -> 512 @ 16x4x4), and a forced one
CASES += [
    *_modes("level_8x8", (0, 3), D8, D=16, H=8, W=8, wz="8,4", C=(384,), Cout=384, res_mode="same", expect_split=True),
    *_modes("level_4x4", (0, 3), D4, D=16, H=4, W=4, C=(512,), Cout=512, expect_split=True),
    *_modes("level_4x4_forced", (0, 3), D4, D=16, H=4, W=4, C=(256,), Cout=128, split=4, expect_split=True),
]
# ---- 1x1: the skip connections (raw input, no statistics; concat), the attention's qkv (affine, no SiLU) and
# proj_out (residual) convs.  f16x3 takes the skip convs to conv1x1.hip, the exact mode to the general kernel.
PW = dict(k=1, **NOIN, stats=False)
CASES += [
    *_modes("pw_t8", (1,), "conv1x1_p%d_t8", **PW, **R8),
    *_modes("pw_t8_concat", (1,), "conv1x1_p%d_t8", C=(32, 64), **PW, **R8),
    *_modes("pw_t8_concat_split", (1,), "conv1x1_p%d_t8", C=(64, 64), **PW, **R8, **FS),
    *_modes("pw_t4", (1,), "conv1x1_p%d_t4", C=(64,), **PW, **R4),
    *_modes("pw_t4_concat", (1,), "conv1x1_p%d_t4", C=(32, 64), **PW, **R4),
    *_modes("pw_t4_split", (1,), "conv1x1_p%d_t4", C=(128,), **PW, **R4, **FS),
    *_modes("skip_t8", (0,), K18, **PW, **R8),
    *_modes("skip_t8_concat", (0,), K18, C=(32, 64), **PW, **R8),
    *_modes("skip_t8_split", (0,), K18, C=(64,), **PW, **R8, **FS),
    *_modes("skip_t4_concat_split", (0,), K14, C=(64, 64), **PW, **R4, **FS),
    *_modes("k1_qkv_t8", DIRECT, K18, k=1, act=False, Cout=384, **R8),
    *_modes("k1_qkv_t4", DIRECT, K14, k=1, act=False, Cout=384, **R4),
    *_modes("k1_qkv_t4_split", DIRECT, K14, k=1, C=(128,), act=False, Cout=384, **R4, **FS),
    *_modes("k1_proj_out_t8", DIRECT, K18, k=1, **NOIN, res_mode="same", **R8),
    *_modes("k1_proj_out_t4", DIRECT, K14, k=1, **NOIN, res_mode="same", **R4),
    *_modes("k1_proj_out_t4_split", DIRECT, K14, k=1, C=(128,), **NOIN, res_mode="same", **R4, **FS),
]
# ---- the last layer: GroupNorm + SiLU, 2 output channels, NCDHW (f16x3: conv3d_skinny.hip; f32: the general one)
LAST = dict(Cout=2, ncdhw=True, stats=False)
CASES += [
    *_modes("skinny_ncdhw", (1,), "conv3d_p%d_k3_skinny", D=6, H=12, W=9, **LAST),
    *_modes("skinny_ncdhw_c64", (1,), "conv3d_p%d_k3_skinny", C=(64,), D=4, H=8, W=8, **LAST),
    *_modes("last_ncdhw", (0,), "conv3d_p%d_k3_wn1_t8", D=6, H=12, W=9, **LAST),
]
# ---- range: two samples 10^6 apart (the per-sample activation scale; the small one first, so that its scale on
# the large one would overflow f16), one output channel with weights 1e-5 of the others (the per-cout weight
# scale), in_bound 16x and 2^10x above the true maximum (gn_finalize's bounds are upper bounds), and |x| at the
# bound's largest mantissa with the sign alternating along depth (the Winograd-D transform's gain of 2)
CASES += [
    *_modes("wz_two_samples_1e6", (3,), D8, N=2, mags=(1e-6, 1.0), **R8),
    *_modes("direct_two_samples_1e6", DIRECT, D8, N=2, mags=(1e-6, 1.0), Cout=96, **NOIN, **R8),
    *_modes("pw_two_samples_1e6", (1,), "conv1x1_p%d_t8", N=2, mags=(1e-6, 1.0), **PW, **R8),
    *_modes("wz_small_cout", (3,), D8, small_cout=True, **R84),
    *_modes("direct_small_cout", DIRECT, "conv3d_p%d_k3_wn2_t8", small_cout=True, Cout=64, **R8),
    *_modes("wz_bound_x16", (3,), D8, loose=16.0, **R8),
    *_modes("wz_bound_x1024", (3,), D4, loose=1024.0, **R4),
    *_modes("direct_bound_x16", (1,), D4, loose=16.0, Cout=96, **R4),
    *_modes("direct_bound_x1024", (1,), D8, loose=1024.0, Cout=96, **R8),
    *_modes("skinny_bound_x1024", (1,), "conv3d_p%d_k3_skinny", loose=1024.0, D=4, H=8, W=8, **LAST),
    *_modes("wz_alternating_max", (3,), D8, alt_max=True, **NOIN, **R84),
    *_modes("wz_alternating_max_t4", (3,), D4, alt_max=True, **NOIN, **R4),
]
X3_CASES = [c for c in CASES if c.prec in E.SPLIT_MODES]


def inputs(c):
    """CPU tensors of a case: sources (NCDHW fp32), weights, bias, affine, residual, in_bound"""
    g = np.random.default_rng(2000 + c.seed + len(c.name))
    rn = lambda *s: torch.from_numpy(g.standard_normal(s).astype(np.float32))
    D, H, W = c.D, c.H, c.W
    Hs, Ws = {"pool": (2 * H, 2 * W), "stride2": (2 * H, 2 * W), "up": (H // 2, W // 2)}.get(c.in_mode, (H, W))
    mag = torch.tensor(c.mags, dtype=torch.float32).reshape(c.N, 1, 1, 1, 1)
    srcs = []
    for ci in c.C:
        x = rn(c.N, ci, D, Hs, Ws)
        if c.alt_max:
            zsign = torch.tensor([(-1.0) ** z for z in range(D)]).reshape(1, 1, D, 1, 1)
            x = torch.sign(x) * zsign * ALT_MAX
        if not c.aff:
            x = x * mag
        srcs.append(x.float().contiguous())
    cin = sum(c.C)
    w = rn(c.Cout, cin, c.k, c.k, c.k) * (0.05 if c.k == 3 else 0.1)
    if c.small_cout:
        w[c.Cout // 3] *= 1e-5
    b = rn(c.Cout) * 0.01
    aff = None
    if c.aff:
        m2 = mag.reshape(c.N, 1)
        aff = ((1.0 + 0.1 * rn(c.N, cin)) * m2, (0.1 * rn(c.N, cin)) * m2)
    res = None
    if c.res_mode != "none":
        Hr, Wr = {"pool": (2 * H, 2 * W), "up": (H // 2, W // 2)}.get(c.res_mode, (H, W))
        res = rn(c.N, c.Cout, D, Hr, Wr)
    # in_bound: per sample max |act(A x + B)| of the tensor the kernel reads (planar: max |x|, max |low_res|)
    if c.in_mode == "planar":
        bound = torch.stack([s.abs().reshape(c.N, -1).amax(1) for s in srcs], 1)
    else:
        xin = torch.cat(srcs, 1)
        if aff is not None:
            xin = xin * aff[0][:, :, None, None, None] + aff[1][:, :, None, None, None]
            if c.act:
                xin = torch.nn.functional.silu(xin)
        bound = xin.abs().reshape(c.N, -1).amax(1, keepdim=True)
    return dict(srcs=srcs, w=w, b=b, aff=aff, res=res, bound=(bound * c.loose).float().contiguous())


def emulate(c, t, **mut):
    return E.conv32(t["srcs"], t["w"], t["b"], c.prec, in_mode=c.in_mode, aff=t["aff"], act=c.act,
                    bound=t["bound"], res=t["res"], res_mode=c.res_mode, mut=E.Mut(**mut))


def n_acc(c):
    """m: rounded additions along one accumulator (module docstring, term (a))"""
    cinpad = 16 if c.in_mode == "planar" else -(-sum(c.C) // 16) * 16
    taps = 9 if c.prec in E.WZ_MODES else c.k ** 3
    p = 3 if c.prec in E.SPLIT_MODES else 1
    return p * taps * cinpad + max(c.split, 1) + 8 + (16 if c.expect_split else 0)


def elem_bound(c, em):
    m = n_acc(c)
    e_acc = 8.0 * U * torch.sqrt(m * em["sqterms"] / 3.0) + 2 * U * (em["trabs"] + em["out"].abs())
    return e_acc + em["silu"]


def hoeffding_bound(c, em):
    return 7.0 * U * math.sqrt(n_acc(c)) * em["absterms"] + em["silu"]


def channel_bars(c, em):
    """[N, Cout]: max_v elem_bound / max_v |emul| per (sample, output channel)"""
    den = em["out"].abs().amax(dim=(2, 3, 4)).clamp_min(1e-300)
    return elem_bound(c, em).amax(dim=(2, 3, 4)) / den


def channel_errors(got, ref):
    den = ref.abs().amax(dim=(2, 3, 4)).clamp_min(1e-300)
    return (got - ref).abs().amax(dim=(2, 3, 4)) / den


@pytest.fixture(scope="module")
def hc():
    import hipcall
    return hipcall


def run_gpu(hc, c, t):
    import guided_diffusion._hip as H
    nd = (lambda x: x.cuda()) if c.in_mode == "planar" else (lambda x: hc.to_ndhwc(x).cuda())
    kw = dict(in_mode=IN[c.in_mode] if c.in_mode != "planar" else 0, act=int(c.act), precision=c.prec,
              bound=t["bound"].cuda(), want_stats=c.stats, planar=c.in_mode == "planar",
              out_layout=H.OUT_NCDHW if c.ncdhw else H.OUT_NDHWC, hint=c.split << H.HINT_SPLITK_SHIFT)
    if t["aff"] is not None:
        kw["aff"] = (t["aff"][0].cuda(), t["aff"][1].cuda())
    if t["res"] is not None:
        kw.update(res=hc.to_ndhwc(t["res"]).cuda(), res_mode=RES[c.res_mode])
    out, stats, _ = hc.conv3d([nd(s) for s in t["srcs"]], t["w"].cuda(), t["b"].cuda(), (c.D, c.H, c.W), **kw)
    got = out.cpu().double() if c.ncdhw else hc.to_ncdhw(out.cpu()).double()
    return out.cpu(), got, (stats.cpu() if stats is not None else None), dict(hc.LAST_PLAN)


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_conv32_kernel_vs_emulation(hc, c):
    t = inputs(c)
    out, got, stats, plan = run_gpu(hc, c, t)
    # the route the case claims, and nothing else
    assert plan["family"] == c.family, (plan["family"], c.family)
    assert plan["instance"] == G16.claimed_instance(c), (plan["instance"], G16.claimed_instance(c))
    assert (plan["split"] > 1) == c.expect_split, plan
    if c.split:
        assert plan["split"] == c.split
    # repeatability: a second launch is bitwise the first
    out2, _, stats2, _ = run_gpu(hc, c, t)
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32))
    if stats is not None:
        assert torch.equal(stats.view(torch.int64), stats2.view(torch.int64))
    em = emulate(c, t)
    assert torch.isfinite(got).all()
    B = elem_bound(c, em)
    slack = U * em["out"].abs()                 # the fp32 store of an fp64 value
    err = (got - em["out"]).abs()
    bad = err > B + slack
    assert not bad.any(), G16._where(bad, got=got, emul=em["out"], bound=B, silu=em["silu"])
    assert (err <= hoeffding_bound(c, em) + slack).all()
    ratio = float((err / (B + slack)).max())
    e_nc, bar_nc = channel_errors(got, em["out"]), channel_bars(c, em)
    assert (e_nc <= bar_nc * 1.0000001 + 2 * U).all(), (float(e_nc.max()), float(bar_nc.max()))
    print("%s: max err %.3g, bar %.3g .. %.3g, err / element bound %.3g" % (
        c.name, float(e_nc.max()), float(bar_nc.min()), float(bar_nc.max()), ratio))
    if stats is not None:
        # GroupNorm partial sums of the fp32 result, fp64
        s = stats.double().sum(dim=2)
        y = em["out"]
        tol1 = B.sum(dim=(2, 3, 4)) + 1e-300
        tol2 = (2 * y.abs() * B + B * B).sum(dim=(2, 3, 4)) + 1e-300
        assert ((s[..., 0] - y.sum(dim=(2, 3, 4))).abs() <= tol1 * 1.0001 + 1e-12 * y.abs().sum(dim=(2, 3, 4))).all()
        assert ((s[..., 1] - (y * y).sum(dim=(2, 3, 4))).abs()
                <= tol2 * 1.0001 + 1e-12 * (y * y).sum(dim=(2, 3, 4))).all()


def _as_f32(c):
    """the same inputs in the exact mode (its own routes: the general kernel for every shape)"""
    return dataclasses.replace(c, prec=0)


@pytest.mark.parametrize("c", X3_CASES, ids=[c.name for c in X3_CASES])
def test_f16x3_error_against_fp64_within_twice_f32(hc, c):
    """f16x3's error against the fp64 convolution is below fp32's own.  Per (sample, cout):
    max|f16x3 - ref| <= 2 max|f32 - ref| + 4u max|ref|, ref = the fp64 conv of the same fp32 inputs (exact SiLU)."""
    t = inputs(c)
    _, got, _, _ = run_gpu(hc, c, t)
    _, got0, _, _ = run_gpu(hc, _as_f32(c), t)
    ref = emulate(c, t, exact=True)["out"]
    e_x3 = (got - ref).abs().amax(dim=(2, 3, 4))
    e_32 = (got0 - ref).abs().amax(dim=(2, 3, 4))
    top = ref.abs().amax(dim=(2, 3, 4))
    ratio = e_x3 / (e_32 + 1e-300)
    print("%s: f16x3 / f32 error per (sample, cout): median %.3g, max %.3g; worst f16x3 err / max|ref| %.3g" % (
        c.name, float(ratio.median()), float(ratio.max()), float((e_x3 / top.clamp_min(1e-300)).max())))
    bad = e_x3 > 2 * e_32 + 4 * U * top
    assert not bad.any(), [(tuple(i), float(e_x3[tuple(i)]), float(e_32[tuple(i)]), float(top[tuple(i)]))
                           for i in bad.nonzero()[:6].tolist()]


PUBLISHED = G16.PUBLISHED


def _plan_tuples(precision, nets):
    import guided_diffusion._hip as H
    found = {}
    for make, shapes in nets:
        model = make()
        model.conv_precision = precision
        model.to("cuda").eval()          # (parameters are the initialiser's: the plan depends on shapes only)
        eng = model.engine()
        for shape in shapes:
            pl = eng.plan(*shape)
            for i, (tag, _) in pl.conv_meta.items():
                fn, args = pl.steps[i]
                if not tag.startswith("conv"):
                    continue
                d = args[0]._obj
                _, _, split = H.conv_plan(d)
                key = (tag, d.precision, d.in_mode, d.res_mode, d.act, d.io_dtype, split > 1)
                found.setdefault(key, []).append(shape)
            eng.plans.clear()
            del pl
            torch.cuda.empty_cache()
        del model, eng
        torch.cuda.empty_cache()
    return found


def _published(**over):
    def make():
        from guided_diffusion import script_util as su
        fl = su.sr_model_and_diffusion_defaults()
        fl.update(PUBLISHED)
        fl.update(over)
        return su.sr_create_model_and_diffusion(**fl)[0]
    return make


def _model2d():
    from guided_diffusion import script_util as su
    fl = su.model_and_diffusion_defaults()
    fl.update(image_size=64, num_channels=32, num_res_blocks=1, channel_mult="1,2,2", num_head_channels=32,
              attention_resolutions="16", learn_sigma=True, use_scale_shift_norm=True)
    return su.create_model_and_diffusion(**fl)[0]


# the published network at BASELINE config 2's volume (1x64^3), the reference launcher's patch (1x96^3) and
# 1x8x32x32; config 5's network (attention at 16) at 1x128^3; the 2-D network at 2x32x48 (depth-1 volumes)
NETS = [(_published(), ((1, 64, 64, 64), (1, 96, 96, 96), (1, 8, 32, 32))),
        (_published(large_size=128, small_size=128, attention_resolutions="16"), ((1, 128, 128, 128),)),
        (_model2d, ((2, 1, 32, 48),))]


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_plan_tuples_are_covered(precision):
    """Build (do not run) the plans of NETS.  Every conv descriptor's (family, precision, in_mode, res_mode, act,
    io flags, split > 1) must match a case of the table above: a routing change that sends an fp32-grade layer
    down an untested path fails here until a case is added."""
    found = _plan_tuples(precision, NETS)
    have = {c.key() for c in CASES}
    print("%s plan tuples (family, precision, in_mode, res_mode, act, io, split>1):" % precision)
    for k in sorted(found, key=str):
        print("  %s %s %s" % ("ok  " if k in have else "MISS", k, sorted(set(found[k]))))
    missing = [k for k in found if k not in have]
    assert not missing, missing
