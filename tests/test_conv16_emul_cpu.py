"""
The 16-bit conv emulator (conv16_emul.py) on the CPU tier: its algebra against torch's fp64 conv, its rounding
on data where nothing rounds, its agreement with the construction test_gpu_ops.py already uses for the bf16
direct form, and -- per case of test_gpu_conv16.py -- that each plausible kernel bug moves the emulated output
by at least 10x the bound that case holds the kernel to.
"""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv16_emul as E
import test_gpu_conv16 as G


def _reference(srcs, w, b, in_mode="same", aff=None, act=False, res=None, res_mode="none"):
    x = torch.cat([s.double() for s in srcs], 1)
    if aff is not None:
        x = x * aff[0].double()[:, :, None, None, None] + aff[1].double()[:, :, None, None, None]
    if act:
        x = F.silu(x)
    up = lambda t: t.repeat_interleave(2, -2).repeat_interleave(2, -1)
    if in_mode == "up":
        x = up(x)
    if in_mode == "pool":
        x = F.avg_pool3d(x, (1, 2, 2))
    st = (1, 2, 2) if in_mode == "stride2" else 1
    y = F.conv3d(x, w.double(), b.double(), stride=st, padding=w.shape[2] // 2)
    if res_mode != "none":
        r = res.double()
        y = y + {"same": r, "up": up(r) if res_mode == "up" else r,
                 "pool": F.avg_pool3d(r, (1, 2, 2)) if res_mode == "pool" else r}[res_mode]
    return y


@pytest.mark.parametrize("c", G.CASES, ids=[c.name for c in G.CASES])
def test_algebra_without_rounding(c):
    """every rounding off: the emulator (the Winograd-D form as transformed planes, four (1,3,3) convs and the
    output transform) equals the plain fp64 conv -- odd D, D = 1 below, ragged H / W, concat, pool / up /
    stride-2 / planar input, every residual mode"""
    t = G.inputs(c)
    em = E.conv16(t["srcs"], t["w"], t["b"], c.prec, in_mode=c.in_mode, aff=t["aff"], act=c.act,
                  bound=t["bound"], res=t["res"], res_mode=c.res_mode, exact=True)
    ref = _reference(t["srcs"], t["w"], t["b"], c.in_mode, t["aff"], c.act, t["res"], c.res_mode)
    assert (em["out"] - ref).abs().max() <= 1e-12 * ref.abs().max()


@pytest.mark.parametrize("prec", [4, 6])
@pytest.mark.parametrize("D,H,W", [(1, 9, 12), (2, 5, 7), (7, 4, 4)])
def test_winograd_algebra_small_depths(prec, D, H, W):
    g = np.random.default_rng(D)
    x = torch.from_numpy(g.standard_normal((2, 16, D, H, W)).astype(np.float32))
    w = torch.from_numpy(g.standard_normal((128, 16, 3, 3, 3)).astype(np.float32))
    b = torch.zeros(128)
    em = E.conv16([x], w, b, prec, exact=True)
    ref = F.conv3d(x.double(), w.double(), b.double(), padding=1)
    assert (em["out"] - ref).abs().max() <= 1e-12 * ref.abs().max()


@pytest.mark.parametrize("prec,in_mode", [(p, m) for p in (2, 4, 5, 6) for m in ("same", "up", "pool", "stride2")
                                          if p in (2, 5) or m in ("same", "up")])   # (Winograd-D: SAME / UP)
def test_exact_on_small_integers(prec, in_mode):
    """the data the GPU tests use for the exact mapping (even weights for the Winograd-D form): every operand,
    transformed operand, product and sum is exact, so the emulation IS the conv, in every mode"""
    g = np.random.default_rng(5)
    D, H, W = 5, 8, 10
    Hs, Ws = {"up": (4, 5), "pool": (16, 20), "stride2": (16, 20)}.get(in_mode, (H, W))
    if in_mode == "pool":
        xi = 4 * g.integers(-3, 4, (1, 16, D, Hs, Ws))     # pool means of multiples of 4 stay integers
    else:
        xi = g.integers(-3, 4, (1, 16, D, Hs, Ws))
    x = torch.from_numpy(xi.astype(np.float32))
    w = torch.from_numpy((2 * g.integers(-2, 3, (128, 16, 3, 3, 3))).astype(np.float32))
    b = torch.from_numpy(g.integers(-5, 6, (128,)).astype(np.float32))
    bound = x.abs().reshape(1, -1).amax(1, keepdim=True)
    em = E.conv16([x], w, b, prec, in_mode=in_mode, bound=bound)
    ref = _reference([x], w, b, in_mode)
    assert torch.equal(em["out"], ref) and torch.equal(em["stored"], ref)
    assert (em["flip"] == 0).all()


@pytest.mark.parametrize("k", [1, 3])
def test_bf16_direct_equals_rounded_operand_construction(k):
    """precision 5 is test_conv3d_bf16_mode_vs_bf16_rounded_operands' construction: the fp32-activated input
    and the weights each rounded once to bf16, exact products"""
    g = np.random.default_rng(61)
    rn = lambda *s: torch.from_numpy(g.standard_normal(s).astype(np.float32))
    x, w, b = rn(2, 32, 3, 8, 8) * 3.0, rn(64, 32, k, k, k) * 0.05, rn(64)
    A, B = 1.0 + 0.1 * rn(2, 32), 0.1 * rn(2, 32)
    xa = F.silu(x * A[:, :, None, None, None] + B[:, :, None, None, None])
    ref = F.conv3d(xa.bfloat16().double(), w.bfloat16().double(), b.double(), padding=k // 2)
    em = E.conv16([x], w, b, 5, aff=(A, B), act=True)
    # (torch's SiLU and the emulator's are both within an ulp or two of the exact value: a handful of operands
    # land on the other side of a bf16 rounding boundary, which the emulator's flip term bounds)
    assert ((em["out"] - ref).abs() <= em["flip"] + 1e-12 * ref.abs().max()).all()


def _mutations(c):
    m = {"operands not rounded": dict(round_ops=False), "truncation instead of RNE": dict(round_mode="trunc")}
    if c.prec in E.WZ_MODES:
        m["rounded before the Winograd transform"] = dict(round_before_transform=True)
    if c.act:
        m["sigmoid x (1 + 1e-4)"] = dict(sig_scale=1.0 + 1e-4)
    if c.f16 and c.small_cout:
        m["weight scale 1"] = dict(use_wscale=False)
    return m


def test_every_case_sees_the_scale_mutation():
    assert any(c.f16 and c.small_cout and c.prec == p for c in G.CASES for p in (2, 4))


@pytest.mark.parametrize("c", G.CASES, ids=[c.name for c in G.CASES])
def test_bugs_move_the_output_beyond_the_bar(c):
    """Discrimination: each mutation of the arithmetic moves the emulated output by at least 10x the element
    bound the GPU test holds this case to (G.elem_bound) at some element.  Not applicable: the sigmoid to a
    case without activation, the Winograd transform order to the direct kernels, the weight scale to the bf16
    modes (which have none) and to cases without a small-weight channel (where it is exact)."""
    t = G.inputs(c)
    em = G.emulate(c, t)
    B = G.elem_bound(c, em)
    for name, kw in _mutations(c).items():
        mu = G.emulate(c, t, **kw)
        ratio = float(((mu["out"] - em["out"]).abs() / B).max())
        assert ratio >= 10.0, (name, ratio)
