"""
The 16-bit conv kernels (precisions 2 / 4: f16 direct / Winograd-D; 5 / 6: bf16 direct / Winograd-D) against
an emulation of their own arithmetic (conv16_emul.py), element by element.

The emulation rounds where the kernels round (activation and weight scales, 16-bit operands, the Winograd-D
transforms, 16-bit stores), with exact products and fp64 sums.  What it cannot reproduce is (a) the order of
the fp32 accumulation and (b) the fast SiLU.  The bars bound exactly those two, per output element v:

  (a) fp32 accumulation.  An accumulator takes m rounded additions: at most one per product (K = taps x CinPad
      products: 27 or 1 per input channel in the direct kernels, 9 per transformed accumulator in the
      Winograd-D form, which sums three accumulators in its output transform), plus the split-K slab sums
      (S), the epilogue's bias and residual additions and the reduce: m = K + S + 8.  Rounding i adds
      e_i = d_i * P_i, |d_i| <= u = 2^-24, with P_i the partial sum it rounds.  Taking the d_i as independent
      and zero-mean, sum e_i has variance <= u^2/3 * sum P_i^2.  For a sum of K terms t_j in the kernel's
      fixed order, sum_i P_i^2 <= m * (sum t_j^2 + acc^2) (partials grow like a random walk plus the drift to
      the final value acc); the emulator returns that as `sqterms` (summed over the accumulators an output
      combines).  Bar: 8 sigma,  E_acc = 8 * u * sqrt(m * sqterms / 3).  The Winograd-D output transform adds
      two roundings of |M0| + |M1| + |M2|, the epilogue's bias / residual additions one each of |out|:
      + 2u * (trabs + |out|).
  (b) fast SiLU (v_exp_f32 / v_rcp_f32, a few ulp; conv16_emul._silu bounds it by delta = 2^-24 *
      (8 + 2|y|) relative).  It changes an operand only where its fp32 value lies within delta of a 16-bit
      rounding boundary -- probability about 2^-12 (f16) or 2^-15 (bf16) per operand -- and then by one 16-bit
      ulp.  The emulator sums one ulp times |weight| over exactly those operands: `flip`, a rigorous bound.
      Without an activation (act = NONE) the operands are exact and flip = 0: only (a) remains.

Per element:                |got - emul| <= E_acc + flip                           (`elem_bound`)
and, the classical form:    |got - emul| <= k * sum|terms| + flip,   k = 7 u sqrt(m)   (Hoeffding: each rounding
                            is at most u * sum|terms|; P(exceeding) < 1e-10 per element)
Per (sample, output channel): max|got - emul| / max|emul| < max(E_acc + flip) / max|emul|, the bar
reported per case (observed errors: DESIGN.md §3.1d).
16-bit stores: within one 16-bit ulp of the emulation's stored value.  Statistics: against the fp64 sums of the
emulation's unrounded output, within the sum of the element bounds.  Every case runs twice: bitwise equal.

test_conv16_emul_cpu.py proves on the CPU that every case's bar sees each of the plausible bugs (operands not
rounded, truncated instead of rounded, rounded before the Winograd transform, a sigmoid off by 1e-4, a lost
weight scale) by at least 10x.  test_plan_tuples_are_covered ties the table to the routes the f16 and bf16
plans of the published network really take.
"""

import math
from dataclasses import dataclass

import numpy as np
import pytest
import torch

import conv16_emul as E

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
IN = {"same": 0, "pool": 1, "up": 2, "planar": 3, "stride2": 4}
RES = {"none": 0, "same": 1, "pool": 2, "up": 3}
IO_SRC0, IO_SRC1, IO_OUT, IO_RES, IO_F16 = 1, 2, 4, 8, 16
TORCH16 = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}


@dataclass
class Case:
    name: str
    prec: int                 # 2, 4 (f16) / 5, 6 (bf16)
    family: str               # ddpm3d_conv_kernel_family's answer the case claims
    wz: str = "8,8"           # Winograd-D: the tile (TX, TY) of the instance the case is meant for (t4 families: 4,4)
    N: int = 1
    D: int = 5
    H: int = 8
    W: int = 10
    C: tuple = (32,)          # channels per source (two = virtual concat)
    Cout: int = 128
    k: int = 3
    in_mode: str = "same"
    res_mode: str = "none"
    act: bool = True          # GroupNorm affine + SiLU (aff without act when act is False and aff is True)
    aff: bool = True
    src: tuple = ("h",)       # storage per source: "h" = the mode's 16-bit type, "f32"
    res: str = "h"
    out16: bool = True
    ncdhw: bool = False
    stats: bool = True
    split: int = 0            # 0: the rule's split; > 1: forced through kernel_hint
    expect_split: bool = False
    mags: tuple = (1.0,)      # per-sample magnitude of the input
    xscale: float = 1.0
    small_cout: bool = False  # one output channel with weights 1e-5 of the others
    seed: int = 0

    @property
    def f16(self):
        return self.prec in E.F16_MODES

    def dt(self, s):
        return TORCH16["f16" if self.f16 else "bf16"] if s == "h" else torch.float32

    def io(self):
        io = 0
        if self.in_mode != "planar":
            io |= IO_SRC0 if self.src[0] == "h" else 0
            io |= IO_SRC1 if len(self.src) > 1 and self.src[1] == "h" else 0
        io |= IO_OUT if self.out16 else 0
        io |= IO_RES if self.res_mode != "none" and self.res == "h" else 0
        return io | (IO_F16 if io and self.f16 else 0)

    def key(self):
        return (self.family, self.prec, IN[self.in_mode], RES[self.res_mode], int(self.act), self.io(),
                self.expect_split)


def _both(name, f16_prec, family_fmt, **kw):
    """the same case in the f16 and the bf16 arithmetic"""
    bp = {2: 5, 4: 6}[f16_prec]
    return [Case(name + "_f16", f16_prec, family_fmt % f16_prec, **kw),
            Case(name + "_bf16", bp, family_fmt % bp, **kw)]


WZ8, WZ4 = "conv3d_p%d_k3_wn4_t8", "conv3d_p%d_k3_wn4_t4"
PW8, PW4 = "conv1x1_p%d_t8", "conv1x1_p%d_t4"
K18, K14 = "conv3d_p%d_k1_wn4_t8", "conv3d_p%d_k1_wn4_t4"
SK = "conv3d_p%d_k3_skinny"
R8 = dict(D=5, H=8, W=10, wz="8,8")     # 8x8x2 tiles, odd D, ragged W
R84 = dict(D=8, H=8, W=12, wz="8,4")    # 8x4x4 tiles (H % 8 == 0, D % 4 == 0), ragged W
R4 = dict(D=9, H=4, W=6, wz="4,4")      # 4x4x8 tiles, D not a multiple of 8, ragged W
FS = dict(split=2, expect_split=True)


def claimed_instance(c):
    """ddpm3d_conv_kernel_instance's answer the case claims, spelled from what it says of itself: the kernel and tile
    width of its family, its arithmetic, input mode and source storage, and for the Winograd-D form the tile `wz`
    (also test_gpu_conv32.py's cases, whose sources are fp32)"""
    fam, src = c.family, getattr(c, "src", ("f32",))
    txl = {"8": 3, "4": 2}[fam.rsplit("_t", 1)[-1]] if "_t" in fam else 3
    if fam.endswith("skinny"):      # <arithmetic, Cin / 16, source type: 0 fp32, 1 bf16, 2 f16>
        return "conv3d_skinny_kernel<%d,%d,%d>" % ({1: 0, 2: 1, 5: 2}[c.prec], sum(c.C) // 16,
                                                  0 if src[0] == "f32" else 2 if c.prec in E.F16_MODES else 1)
    if fam.startswith("conv1x1"):   # <PREC, 16-bit sources, TXL, TYL, wide stores>
        return "conv3d_pw_kernel<%d,%d,%d,%d,1>" % (c.prec, src[0] == "h", txl, txl)
    if c.prec in (3, 4, 6):         # <arithmetic, issue order, TX, TY>
        return "conv3d_wz_kernel<%d,%d,%s>" % ({3: 0, 4: 1, 6: 2}[c.prec], 4 if c.prec == 3 else 0,
                                              "4,4" if txl == 2 else c.wz)
    wn = int(fam.split("_wn")[1][0])
    pipe = {"same": 1, "up": 1, "stride2": 2}.get(c.in_mode, 0)
    return "conv3d_kernel<%d,%d,%d,%d,%d,%d,%d>" % (c.prec, pipe, c.k, wn, wn, txl, txl)


CASES = []
for geo, fam in ((R8, WZ8), (R84, WZ8), (R4, WZ4)):
    g = "t%dx%dx%d" % ((8, 8, 2) if geo is R8 else (8, 4, 4) if geo is R84 else (4, 4, 8))
    for sp, sk in ((dict(), ""), (FS, "_split")):
        CASES += _both("wz_%s_conv1%s" % (g, sk), 4, fam, Cout=256 if geo is R8 else 128, **geo, **sp)
        CASES += _both("wz_%s_resid%s" % (g, sk), 4, fam, res_mode="same", **geo, **sp)
        CASES += _both("wz_%s_resid_pool%s" % (g, sk), 4, fam, res_mode="pool", **geo, **sp)
        CASES += _both("wz_%s_pooled_noact%s" % (g, sk), 4, fam, act=False, aff=False, src=("f32",), **geo, **sp)
        CASES += _both("wz_%s_concat%s" % (g, sk), 4, fam, C=(16, 32), src=("h", "h"), **geo, **sp)
        CASES += _both("wz_%s_up%s" % (g, sk), 4, fam, in_mode="up", **geo, **sp)
        CASES += _both("wz_%s_resid_up%s" % (g, sk), 4, fam, res_mode="up", **geo, **sp)
CASES += [
    # concat of a 16-bit and an fp32 source, fp32 output; a second (ragged) cout block
    *_both("wz_concat_h_f32", 4, WZ8, C=(32, 16), src=("h", "f32"), out16=False, Cout=256, D=3, H=9, W=11),
    # N = 2, per-sample magnitudes seven decades apart (the activation scale per sample; f16 subnormals)
    *_both("wz_two_samples_1e-6", 4, WZ8, N=2, mags=(1.0, 1e-6), **R8),
    *_both("direct_two_samples_1e-6", 2, "conv3d_p%d_k3_wn4_t8", N=2, mags=(1e3, 1e-3), aff=False, act=False,
           src=("f32",), out16=False, Cout=96, **R8),
    # one output channel with weights 1e-5 of the others: the per-cout weight scale keeps it out of f16 subnormals
    *_both("wz_small_cout", 4, WZ8, small_cout=True, **R84),
    *_both("direct_small_cout", 2, "conv3d_p%d_k3_wn2_t8", small_cout=True, Cout=64, **R8),
    # bf16 inputs x300 (far outside f16's comfortable range: the bf16 modes carry no scale)
    Case("wz_x300_bf16", 6, WZ8 % 6, xscale=300.0, aff=False, act=False, **R8),
    Case("direct_x300_bf16", 5, "conv3d_p5_k3_wn4_t4", xscale=300.0, aff=False, act=False, D=6, H=4, W=4),
    # the network's 8x8 and 4x4 level shapes (rule's split), and 4x4 with a forced split
    *_both("wz_level_8x8", 4, WZ8, D=16, H=8, W=8, wz="8,4", C=(384,), Cout=384, res_mode="same", expect_split=True),
    *_both("wz_level_4x4", 4, WZ4, D=16, H=4, W=4, C=(512,), Cout=512, expect_split=True),
    *_both("wz_level_4x4_forced", 4, WZ4, D=16, H=4, W=4, C=(256,), Cout=128, split=4, expect_split=True),
    # the direct kernel: the planar first conv on 8x8 and 4x4 tiles, 8x8 / 4x4 tiles with a partial cout tile,
    # the pool and stride-2 input modes, split over Cin
    *_both("direct_planar_t8", 2, "conv3d_p%d_k3_wn4_t8", in_mode="planar", C=(1, 1), src=("f32", "f32"),
           aff=False, act=False, **R8),
    *_both("direct_planar_t4", 2, "conv3d_p%d_k3_wn4_t4", in_mode="planar", C=(1, 1), src=("f32", "f32"),
           aff=False, act=False, **R4),
    *_both("direct_t8_partial_cout", 2, "conv3d_p%d_k3_wn4_t8", Cout=96, **R8),
    *_both("direct_t4_partial_cout", 2, "conv3d_p%d_k3_wn4_t4", Cout=160, res_mode="same", **R4),
    *_both("direct_pool", 2, "conv3d_p%d_k3_wn4_t8", in_mode="pool", **R8),
    *_both("direct_stride2", 2, "conv3d_p%d_k3_wn4_t4", in_mode="stride2", D=4, H=6, W=6),
    *_both("direct_t4_split", 2, "conv3d_p%d_k3_wn4_t4", C=(64,), **R4, **FS),
    # 1x1: the skip connections (raw input, no statistics; concat; one 32-channel block of K) and the
    # attention projections (qkv: GroupNorm affine, fp32 output; proj_out: fp32 input + 16-bit residual)
    *_both("pw_t8", 2, PW8, k=1, aff=False, act=False, stats=False, **R8),
    *_both("pw_t8_one_block", 2, PW8, k=1, C=(32,), aff=False, act=False, stats=False, Cout=256, **R84),
    *_both("pw_t8_concat", 2, PW8, k=1, C=(32, 64), src=("h", "h"), aff=False, act=False, stats=False, **R8),
    *_both("pw_t8_concat_split", 2, PW8, k=1, C=(64, 64), src=("h", "h"), aff=False, act=False, stats=False,
           split=2, expect_split=True, **R8),
    *_both("pw_t4", 2, PW4, k=1, C=(64,), aff=False, act=False, stats=False, **R4),
    *_both("pw_t4_concat", 2, PW4, k=1, C=(32, 64), src=("h", "h"), aff=False, act=False, stats=False, **R4),
    *_both("pw_t4_concat_split", 2, PW4, k=1, C=(64, 64), src=("h", "h"), aff=False, act=False, stats=False,
           split=2, expect_split=True, **R4),
    *_both("pw_t4_split", 2, PW4, k=1, C=(128,), aff=False, act=False, stats=False, split=2, expect_split=True,
           **R4),
    *_both("k1_qkv_t8", 2, K18, k=1, act=False, out16=False, Cout=384, **R8),
    *_both("k1_qkv_t4", 2, K14, k=1, act=False, out16=False, Cout=384, **R4),
    *_both("k1_qkv_t4_split", 2, K14, k=1, C=(128,), act=False, out16=False, Cout=384, split=2,
           expect_split=True, **R4),
    *_both("k1_proj_out_t8", 2, K18, k=1, aff=False, act=False, src=("f32",), res_mode="same", **R8),
    *_both("k1_proj_out_t4", 2, K14, k=1, aff=False, act=False, src=("f32",), res_mode="same", **R4),
    *_both("k1_proj_out_t4_split", 2, K14, k=1, C=(128,), aff=False, act=False, src=("f32",), res_mode="same",
           split=2, expect_split=True, **R4),
    # the last-layer kernel: NCDHW fp32 (the network's) and NDHWC 16-bit outputs
    *_both("skinny_ncdhw", 2, SK, Cout=2, ncdhw=True, out16=False, stats=False, D=6, H=12, W=9),
    *_both("skinny_ndhwc", 2, SK, Cout=2, C=(64,), stats=False, D=4, H=8, W=8),
]


def inputs(c):
    """CPU tensors of a case: sources (NCDHW, storage dtype), weights, bias, affine, residual, in_bound"""
    g = np.random.default_rng(1000 + c.seed + len(c.name))
    rn = lambda *s: torch.from_numpy(g.standard_normal(s).astype(np.float32))
    D, H, W = c.D, c.H, c.W
    Hs, Ws = {"pool": (2 * H, 2 * W), "stride2": (2 * H, 2 * W), "up": (H // 2, W // 2)}.get(c.in_mode, (H, W))
    mag = torch.tensor(c.mags, dtype=torch.float32).reshape(c.N, 1, 1, 1, 1)
    srcs = []
    for ci, s in zip(c.C, c.src):
        x = rn(c.N, ci, D, Hs, Ws) * c.xscale
        if not c.aff:
            x = x * mag
        srcs.append(x.to(c.dt(s)))
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
        res = rn(c.N, c.Cout, D, Hr, Wr).to(c.dt(c.res))
    # in_bound: per sample max |act(A x + B)| of the tensor the kernel reads (planar: max |x|, max |low_res|)
    if c.in_mode == "planar":
        bound = torch.stack([s.abs().reshape(c.N, -1).amax(1) for s in srcs], 1)
    else:
        xin = torch.cat([s.float() for s in srcs], 1)
        if aff is not None:
            xin = xin * aff[0][:, :, None, None, None] + aff[1][:, :, None, None, None]
            if c.act:
                xin = torch.nn.functional.silu(xin)
        bound = xin.abs().reshape(c.N, -1).amax(1, keepdim=True)
    return dict(srcs=srcs, w=w, b=b, aff=aff, res=res, bound=bound.float().contiguous())


def emulate(c, t, **mut):
    return E.conv16(t["srcs"], t["w"], t["b"], c.prec, in_mode=c.in_mode, aff=t["aff"], act=c.act,
                    bound=t["bound"], res=t["res"], res_mode=c.res_mode, out16=c.out16, **mut)


def n_acc(c):
    """m: rounded additions along one accumulator (module docstring, term (a))"""
    cinpad = 16 if c.in_mode == "planar" else sum(c.C)
    taps = 9 if c.prec in E.WZ_MODES else c.k ** 3
    return taps * cinpad + max(c.split, 1) + 8 + (16 if c.expect_split else 0)


def elem_bound(c, em):
    m = n_acc(c)
    e_acc = 8.0 * U * torch.sqrt(m * em["sqterms"] / 3.0) + 2 * U * (em["trabs"] + em["out"].abs())
    return e_acc + em["flip"]


def hoeffding_bound(c, em):
    return 7.0 * U * math.sqrt(n_acc(c)) * em["absterms"] + em["flip"]


def channel_bars(c, em):
    """[N, Cout]: max_v elem_bound / max_v |emul| per (sample, output channel)"""
    B = elem_bound(c, em)
    den = em["out"].abs().amax(dim=(2, 3, 4)).clamp_min(1e-300)
    return B.amax(dim=(2, 3, 4)) / den


def channel_errors(got, ref):
    den = ref.abs().amax(dim=(2, 3, 4)).clamp_min(1e-300)
    return (got - ref).abs().amax(dim=(2, 3, 4)) / den


def ulp16(x, f16):
    """spacing of the 16-bit grid at |x| (its larger side)"""
    a = x.abs()
    if f16:
        h = a.float().numpy().astype(np.float16)
        return torch.from_numpy((np.nextafter(h, np.float16(np.inf)).astype(np.float64) - h.astype(np.float64)))
    e = torch.floor(torch.log2(a.clamp_min(2.0 ** -126)))
    return 2.0 ** (e - 7)


def _where(bad, **vals):
    """the first few failing elements (n, c, z, y, x) with the values involved"""
    idx = bad.nonzero()[:6].tolist()
    rows = ["%s %s" % (tuple(i), " ".join("%s=%.9g" % (k, float(v[tuple(i)])) for k, v in vals.items()))
            for i in idx]
    return "%d of %d elements:\n  %s" % (int(bad.sum()), bad.numel(), "\n  ".join(rows))


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
    if c.out16:
        kw["out_f16" if c.f16 else "out_bf16"] = True
    if t["aff"] is not None:
        kw["aff"] = (t["aff"][0].cuda(), t["aff"][1].cuda())
    if t["res"] is not None:
        kw.update(res=hc.to_ndhwc(t["res"]).cuda(), res_mode=RES[c.res_mode])
    out, stats, _ = hc.conv3d([nd(s) for s in t["srcs"]], t["w"].cuda(), t["b"].cuda(), (c.D, c.H, c.W), **kw)
    return out.cpu(), (stats.cpu() if stats is not None else None), dict(hc.LAST_PLAN)


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_conv16_kernel_vs_emulation(hc, c):
    t = inputs(c)
    out, stats, plan = run_gpu(hc, c, t)
    # the route the case claims, and nothing else
    assert plan["family"] == c.family, (plan["family"], c.family)
    assert plan["instance"] == claimed_instance(c), (plan["instance"], claimed_instance(c))
    assert (plan["split"] > 1) == c.expect_split, plan
    if c.split:
        assert plan["split"] == c.split
    # repeatability: a second launch is bitwise the first
    out2, stats2, _ = run_gpu(hc, c, t)
    assert torch.equal(out.view(torch.int16) if out.element_size() == 2 else out.view(torch.int32),
                       out2.view(torch.int16) if out2.element_size() == 2 else out2.view(torch.int32))
    if stats is not None:
        assert torch.equal(stats.view(torch.int64), stats2.view(torch.int64))
    got = out.double() if c.ncdhw else hc.to_ncdhw(out).double()
    em = emulate(c, t)
    ref = em["stored"]
    assert torch.isfinite(got).all()
    B = elem_bound(c, em)
    if c.out16:
        # 16-bit stores: the kernel rounded an fp32 value within B of the emulation's, so the stored value is
        # within B + half a 16-bit ulp of it everywhere, and within one 16-bit ulp of the emulation's own
        # stored value wherever B is below half an ulp (near zero the ulp can be finer than the accumulation)
        # (half an ulp at the coarser of the two values: the kernel's may sit in the next binade)
        slack = 0.5 * torch.maximum(ulp16(em["out"], c.f16), ulp16(got, c.f16)) * 1.0000001
        fine = B <= 0.5 * ulp16(ref, c.f16)
        bad = fine & ((got - ref).abs() > ulp16(ref, c.f16) * 1.0000001)
        assert not bad.any(), _where(bad, got=got, stored=ref, emul=em["out"], bound=B, flip=em["flip"])
    else:
        slack = U * em["out"].abs()                 # the fp32 store of an fp64 value
    err = (got - em["out"]).abs()
    bad = err > B + slack
    assert not bad.any(), _where(bad, got=got, emul=em["out"], bound=B, flip=em["flip"])
    assert (err <= hoeffding_bound(c, em) + slack).all()
    ratio = float((err / (B + slack)).max())
    if not c.out16:
        e_nc, bar_nc = channel_errors(got, em["out"]), channel_bars(c, em)
        assert (e_nc <= bar_nc * 1.0000001 + 2 * U).all(), (float(e_nc.max()), float(bar_nc.max()))
        print("%s: max err %.3g, bar %.3g .. %.3g, err / element bound %.3g" % (
            c.name, float(e_nc.max()), float(bar_nc.min()), float(bar_nc.max()), ratio))
    else:
        print("%s: err / element bound %.3g (16-bit store)" % (c.name, ratio))
    if stats is not None:
        # GroupNorm partial sums of the fp32 result (before any 16-bit rounding), fp64
        s = stats.double().sum(dim=2)
        y = em["out"]
        tol1 = B.sum(dim=(2, 3, 4)) + 1e-300
        tol2 = (2 * y.abs() * B + B * B).sum(dim=(2, 3, 4)) + 1e-300
        assert ((s[..., 0] - y.sum(dim=(2, 3, 4))).abs() <= tol1 * 1.0001 + 1e-12 * y.abs().sum(dim=(2, 3, 4))).all()
        assert ((s[..., 1] - (y * y).sum(dim=(2, 3, 4))).abs()
                <= tol2 * 1.0001 + 1e-12 * (y * y).sum(dim=(2, 3, 4))).all()


PUBLISHED = dict(large_size=96, small_size=96, num_channels=128, num_res_blocks=2, num_head_channels=64,
                 attention_resolutions="1000", learn_sigma=True, resblock_updown=True, use_scale_shift_norm=True)


@pytest.mark.parametrize("precision", ["f16", "bf16"])
def test_plan_tuples_are_covered(precision):
    """Build (do not run) the Python plans of the published architecture at BASELINE config 4's volume
    (1x1x64^3), at the reference launcher's own --use_fp16 patch (1x1x96^3) and at
    test_native_plan_equals_python_plan's 1x1x8x32x32, and of config 5's network (attention at 16) at
    1x1x128^3.  Every conv descriptor's
    (family, precision, in_mode, res_mode, act, io flags, split > 1) must match a case of the table above: a
    routing change that sends a 16-bit layer down an untested path fails here until a case is added."""
    import guided_diffusion._hip as H
    from guided_diffusion import script_util as su
    found = {}
    for over, shapes in ((dict(), ((1, 64, 64, 64), (1, 96, 96, 96), (1, 8, 32, 32))),
                         (dict(large_size=128, small_size=128, attention_resolutions="16"), ((1, 128, 128, 128),))):
        fl = su.sr_model_and_diffusion_defaults()
        fl.update(PUBLISHED)
        fl.update(over)
        model, _ = su.sr_create_model_and_diffusion(**fl)
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
    have = {c.key() for c in CASES}
    print("%s plan tuples (family, precision, in_mode, res_mode, act, io, split>1):" % precision)
    for k in sorted(found, key=str):
        print("  %s %s %s" % ("ok  " if k in have else "MISS", k, sorted(set(found[k]))))
    missing = [k for k in found if k not in have]
    assert not missing, missing
