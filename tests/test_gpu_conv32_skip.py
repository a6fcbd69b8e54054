"""
ddpm3d_conv3d_skip -- the tail of a ResBlock whose skip connection is a 1x1 conv, the 1x1 products accumulated inside
conv2's f16x3 Winograd-D launch (conv3d_wz.h SKIP) -- against the emulation of ITS arithmetic (conv32_skip_emul.py),
element by element, with the model of test_gpu_conv32.py:

  |got - emul| <= E_acc + silu,   E_acc = 8 u sqrt(m sqterms / 3) + 2u (trabs + |out|),
  m = 3 (9 CinPad_h + CinPad_x) + S + 8 (+ 16 when split)

-- one accumulator now takes conv2's nine taps per channel of h and one product per channel of x.  And, since the form
regroups the same products ("results stay what they were"): the result also lies within the SUM of the bounds
test_gpu_conv32.py puts on the two shipped launches (the 1x1 conv at precision 1, then conv2 at precision 3 with that
tensor as its residual) around their composed emulation.  Every case runs twice (bitwise equal), is known to have
taken the fused form by ddpm3d_conv_skip_fused, writes statistics within that file's tolerances of the emulation's
fp64 sums, and uses the statistics rows, workspace and split that ddpm3d_conv_plan reports for the conv2 descriptor.

test_skip_error_against_fp64_within_twice_f32: that file's formula, max|f16x3 - ref| <= 2 max|f32 - ref| + 4u max|ref|
per (sample, cout), the exact mode run as its own two launches.

Where the library does not take the fused form (a 16-bit descriptor, precision 1) the entry must equal the caller's
own two ddpm3d_conv3d calls bit for bit.
"""

import ctypes as C
import functools
from dataclasses import dataclass

import pytest
import torch

import conv32_skip_emul as S
import test_gpu_conv32 as G

pytestmark = pytest.mark.gpu

U = G.U


@dataclass
class Case:
    name: str
    wz: str = "8,8"           # the tile (TX, TY) of the Winograd-D instance the case is meant for
    N: int = 1
    D: int = 5
    H: int = 8
    W: int = 10
    Cx: tuple = (32,)
    Cout: int = 128           # conv2 is Cout -> Cout
    split: int = 0            # 0: the rule's split; >= 1: forced through conv2's kernel_hint (1: one unsplit launch)
    expect_split: object = None   # None: whatever the rule says
    mags: tuple = ((1.0, 1.0),)
    alt_max_x: bool = False

    def inputs(self):
        return S.skip_inputs(N=self.N, D=self.D, H=self.H, W=self.W, Ch=self.Cout, Cx=self.Cx, Cout=self.Cout,
                             mags=self.mags, alt_max_x=self.alt_max_x, seed=len(self.name))


CASES = []
for geo, g in ((G.R8, "t8x8x2"), (G.R84, "t8x4x4"), (G.R4, "t4x4x8")):
    for cx, ck in (((32,), ""), ((32, 32), "_concat")):
        # (128 channels of h at these sizes: the rule would split; the unsplit launch is the 64^3 levels' path)
        for sp, sk in ((dict(split=1, expect_split=False), ""), (G.FS, "_split")):
            CASES.append(Case("skip_%s%s%s" % (g, ck, sk), Cx=cx, **geo, **sp))
CASES += [
    # three x blocks over four splits: the last split gets none
    Case("skip_x96_split4", Cx=(96,), split=4, expect_split=True, **G.R8),
    Case("skip_two_cout_blocks", Cout=256, **G.R84),
    Case("skip_d1", D=1, H=8, W=8),
    # rho far from 1 both ways: sample 0 has h at 1e-6 of x, sample 1 x at 1e-6 of h
    Case("skip_two_samples_1e6", N=2, mags=((1e-6, 1.0), (1.0, 1e-6)), **G.R8),
    Case("skip_x_alternating_max", alt_max_x=True, **G.R84),
    # the published network's (512 + 512) -> 512 ResBlock at 64x4x4, the rule's 16-way split
    Case("skip_published_1024_512_64x4x4", D=64, H=4, W=4, wz="4,4", Cx=(512, 512), Cout=512, expect_split=True),
]


@functools.lru_cache(maxsize=2)
def _inputs(name):
    return next(c for c in CASES if c.name == name).inputs()


@functools.lru_cache(maxsize=2)
def _emul(name):
    return S.emulate(_inputs(name))


def n_acc(c, split):
    pad = lambda v: -(-v // 16) * 16
    return 3 * (9 * pad(c.Cout) + pad(sum(c.Cx))) + max(split, 1) + 8 + (16 if split > 1 else 0)


def elem_bound(c, em, split):
    e_acc = 8.0 * U * torch.sqrt(n_acc(c, split) * em["sqterms"] / 3.0) + 2 * U * (em["trabs"] + em["out"].abs())
    return e_acc + em["silu"]


@pytest.fixture(scope="module")
def hc():
    import hipcall
    return hipcall


def run(hc, c, t, prec2=3, half=None, two_calls=False):
    """The ResBlock tail on the GPU: ddpm3d_conv3d_skip, or (two_calls) the caller's own 1x1 conv into out and conv2
    with out as its residual.  prec2: conv2's precision (3: f16x3 Winograd-D, 1: f16x3 direct, 0: exact); half: a
    16-bit torch dtype for h, x and out.  Returns out (NDHWC, cpu), stats (cpu), info."""
    import guided_diffusion._hip as H
    lib = H.load()
    prec1 = {3: 1, 1: 1, 0: 0}[prec2]
    dev = "cuda"
    cast = (lambda x: x.to(half)) if half is not None else (lambda x: x)
    h = cast(hc.to_ndhwc(t["h"][0]).to(dev))
    xs = [cast(hc.to_ndhwc(x).to(dev)) for x in t["xs"]]
    keep = [h, xs]
    N, Cout, cx = c.N, c.Cout, sum(c.Cx)
    io16 = 0
    if half is not None:
        io16 = H.IO_HALF_IS_F16 if half == torch.float16 else 0
    d = H.ConvDesc()
    d.N, d.D, d.H, d.W, d.Cin, d.Cout, d.ksize, d.in_mode = N, c.D, c.H, c.W, Cout, Cout, 3, H.IN_SAME
    d.src0, d.C0 = H.ptr(h), Cout
    A, B = t["aff"][0].to(dev), t["aff"][1].to(dev)
    d.aff_a, d.aff_b, d.act = H.ptr(A), H.ptr(B), H.ACT_SILU
    d.precision = prec2
    w2p, w1p = hc.pack(t["w2"].to(dev), prec2), hc.pack(t["w1"].to(dev), prec1)
    b2, b1 = t["b2"].to(dev), t["b1"].to(dev)
    d.w_packed, d.bias = H.ptr(w2p), H.ptr(b2)
    d.out_layout = H.OUT_NDHWC
    d.kernel_hint = c.split << H.HINT_SPLITK_SHIFT
    bh, bx = t["bound_h"].to(dev), t["bound_x"].to(dev)
    d.in_bound, d.in_bound_count, d.in_bound_stride = H.ptr(bh), 1, 1
    if half is not None:
        d.io_dtype = H.IO_SRC0_BF16 | H.IO_OUT_BF16 | io16
    out = torch.full((N, c.D, c.H, c.W, Cout), float("nan"), dtype=half or torch.float32, device=dev)
    d.out = H.ptr(out)
    sk = H.ConvSkip()
    sk.src0, sk.C0 = H.ptr(xs[0]), c.Cx[0]
    if len(xs) > 1:
        sk.src1, sk.C1 = H.ptr(xs[1]), c.Cx[1]
    sk.w_packed, sk.bias = H.ptr(w1p), H.ptr(b1)
    sk.in_bound, sk.in_bound_count, sk.in_bound_stride = H.ptr(bx), 1, 1
    if half is not None:
        sk.io_dtype = H.IO_SRC0_BF16 | (H.IO_SRC1_BF16 if len(xs) > 1 else 0)
    fused = bool(lib.ddpm3d_conv_skip_fused(C.byref(d), C.byref(sk)))
    instance = H.conv_instance(d, sk)
    # statistics rows, workspace and split: what ddpm3d_conv_plan reports for the conv2 descriptor
    rows, need, split = H.conv_plan(d)
    if not c.split:
        assert rows == lib.ddpm3d_conv_stats_rows(N, c.D, c.H, c.W, Cout, Cout, 3, prec2)
        assert need == lib.ddpm3d_conv_workspace_bytes(N, c.D, c.H, c.W, Cout, Cout, 3, prec2)
    assert need == (split * N * c.D * c.H * c.W * Cout * 4 if split > 1 else 0)
    if not fused:
        # the two-call form's first call may be split too
        need = max(need, lib.ddpm3d_conv_workspace_bytes(N, c.D, c.H, c.W, cx, Cout, 1, prec1))
    ws = torch.full((max(need, 16) // 4,), float("nan"), dtype=torch.float32, device=dev)
    if need:
        d.workspace, d.workspace_bytes = H.ptr(ws), need
    stats = torch.full((N, Cout, rows, 2), float("nan"), dtype=torch.float64, device=dev)
    d.stats, d.stats_rows = H.ptr(stats), rows
    # the caller's own first call (and how the library would run it: the composed bound's accumulator length)
    d1 = H.ConvDesc()
    d1.N, d1.D, d1.H, d1.W, d1.Cin, d1.Cout, d1.ksize, d1.in_mode = N, c.D, c.H, c.W, cx, Cout, 1, H.IN_SAME
    d1.src0, d1.C0, d1.src1, d1.C1 = sk.src0, sk.C0, sk.src1, sk.C1
    d1.precision, d1.w_packed, d1.bias = prec1, sk.w_packed, sk.bias
    d1.out, d1.out_layout = d.out, H.OUT_NDHWC
    d1.in_bound, d1.in_bound_count, d1.in_bound_stride = sk.in_bound, 1, 1
    d1.workspace, d1.workspace_bytes = d.workspace, d.workspace_bytes
    d1.io_dtype = sk.io_dtype | (d.io_dtype & (H.IO_OUT_BF16 | H.IO_HALF_IS_F16))
    split1 = H.conv_plan(d1)[2]
    if not two_calls:
        H.check(lib.ddpm3d_conv3d_skip(C.byref(d), C.byref(sk), H.stream()))
    else:
        H.check(lib.ddpm3d_conv3d(C.byref(d1), H.stream()))
        d.res, d.res_mode = d.out, H.RES_SAME
        if half is not None:
            d.io_dtype |= H.IO_RES_BF16
        H.check(lib.ddpm3d_conv3d(C.byref(d), H.stream()))
    torch.cuda.synchronize()
    del keep
    return out.cpu(), stats.cpu(), dict(fused=fused, rows=rows, split=split, split1=split1, instance=instance)


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_skip_kernel_vs_emulation(hc, c):
    t = _inputs(c.name)
    out, stats, info = run(hc, c, t)
    assert info["fused"], info
    assert info["instance"] == "conv3d_wz_kernel<4,4,%s>" % c.wz, (info, c.wz)      # <mode 4: skip, issue order, TX, TY>
    if c.expect_split is not None:
        assert (info["split"] > 1) == c.expect_split, info
    if c.split:
        assert info["split"] == c.split
    out2, stats2, _ = run(hc, c, t)
    assert torch.equal(_bits(out), _bits(out2))
    assert torch.equal(stats.view(torch.int64), stats2.view(torch.int64))
    got = hc.to_ncdhw(out).double()
    assert torch.isfinite(got).all() and torch.isfinite(stats).all()
    # ---- against the emulation of the fused arithmetic
    em = _emul(c.name)
    B = elem_bound(c, em, info["split"])
    slack = U * em["out"].abs()
    err = (got - em["out"]).abs()
    print("%s: max |got - fused emulation| / bound %.3g" % (c.name, float((err / (B + slack)).max())))
    bad = err > B + slack
    assert not bad.any(), G.G16._where(bad, got=got, emul=em["out"], bound=B, silu=em["silu"])
    # GroupNorm partial sums of the fp32 result, fp64
    s = stats.double().sum(dim=2)
    y = em["out"]
    tol1 = B.sum(dim=(2, 3, 4)) + 1e-300
    tol2 = (2 * y.abs() * B + B * B).sum(dim=(2, 3, 4)) + 1e-300
    assert ((s[..., 0] - y.sum(dim=(2, 3, 4))).abs() <= tol1 * 1.0001 + 1e-12 * y.abs().sum(dim=(2, 3, 4))).all()
    assert ((s[..., 1] - (y * y).sum(dim=(2, 3, 4))).abs()
            <= tol2 * 1.0001 + 1e-12 * (y * y).sum(dim=(2, 3, 4))).all()
    # ---- results stay what they were: within the sum of the two shipped launches' own bars (test_gpu_conv32.py's
    # elem_bound of each) around their composed emulation
    c1, c2 = S.composed(em, t["b2"], t["b1"])
    k1 = G.Case("pw", 1, "", C=c.Cx, Cout=c.Cout, k=1, split=info["split1"] if info["split1"] > 1 else 0,
                expect_split=info["split1"] > 1, **G.NOIN)
    k2 = G.Case("wz", 3, "", C=(c.Cout,), Cout=c.Cout, split=info["split"], expect_split=info["split"] > 1)
    B12 = G.elem_bound(k1, c1) + G.elem_bound(k2, c2)
    err12 = (got - c2["out"]).abs()
    print("%s: max |got - composed emulation| / the two launches' bound %.3g" % (
        c.name, float((err12 / (B12 + U * c2["out"].abs())).max())))
    bad = err12 > B12 + U * c2["out"].abs()
    assert not bad.any(), G.G16._where(bad, got=got, emul=c2["out"], bound=B12, silu=c2["silu"])


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_skip_error_against_fp64_within_twice_f32(hc, c):
    """test_gpu_conv32.test_f16x3_error_against_fp64_within_twice_f32's formula on the fused form; the exact mode runs
    the tail as its own two launches"""
    t = _inputs(c.name)
    out, _, _ = run(hc, c, t)
    out0, _, info0 = run(hc, c, t, prec2=0)
    assert not info0["fused"]
    got, got0 = hc.to_ncdhw(out).double(), hc.to_ncdhw(out0).double()
    ref = S.emulate(t, exact=True)["out"]
    e_x3 = (got - ref).abs().amax(dim=(2, 3, 4))
    e_32 = (got0 - ref).abs().amax(dim=(2, 3, 4))
    top = ref.abs().amax(dim=(2, 3, 4))
    ratio = e_x3 / (e_32 + 1e-300)
    print("%s: fused f16x3 / f32 error per (sample, cout): median %.3g, max %.3g; worst err / max|ref| %.3g" % (
        c.name, float(ratio.median()), float(ratio.max()), float((e_x3 / top.clamp_min(1e-300)).max())))
    bad = e_x3 > 2 * e_32 + 4 * U * top
    assert not bad.any(), [(tuple(i), float(e_x3[tuple(i)]), float(e_32[tuple(i)]), float(top[tuple(i)]))
                           for i in bad.nonzero()[:6].tolist()]


# (conv2's instance of the two calls: the plain f16x3 Winograd-D form, or precision 1's direct kernel)
FALLBACK = [
    ("bf16_io", Case("skip_fallback_bf16_io", Cx=(32, 32), **G.R84), dict(half=torch.bfloat16), "conv3d_wz_kernel<0,4,8,4>"),
    ("bf16_io_split", Case("skip_fallback_bf16_io_split", Cx=(64,), **G.R8, **G.FS), dict(half=torch.bfloat16),
     "conv3d_wz_kernel<0,4,8,8>"),
    ("precision_1", Case("skip_fallback_p1", Cx=(32, 32), **G.R8), dict(prec2=1), "conv3d_kernel<1,1,3,4,4,3,3>"),
    ("precision_1_split", Case("skip_fallback_p1_split", Cx=(64,), **G.R4, **G.FS), dict(prec2=1),
     "conv3d_kernel<1,1,3,4,4,2,2>"),
]


@pytest.mark.parametrize("c,kw,inst", [f[1:] for f in FALLBACK], ids=[f[0] for f in FALLBACK])
def test_skip_fallback_is_the_two_shipped_calls(hc, c, kw, inst):
    t = c.inputs()
    out, stats, info = run(hc, c, t, **kw)
    assert not info["fused"] and info["instance"] == inst, (info, inst)
    out2, stats2, info2 = run(hc, c, t, two_calls=True, **kw)
    assert info2["rows"] == info["rows"] and info2["split"] == info["split"]
    assert torch.isfinite(out.float()).all()
    assert torch.equal(_bits(out), _bits(out2))
    assert torch.equal(stats.view(torch.int64), stats2.view(torch.int64))
