"""
The fp32-grade conv emulator (conv32_emul.py) on the CPU tier: its algebra against torch's fp64 conv, its
rounding on data where nothing rounds, and -- per case of test_gpu_conv32.py -- that each plausible kernel bug
moves the emulated output by at least 10x the bound that case holds the kernel to.
"""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv32_emul as E
import test_gpu_conv32 as G
from test_conv16_emul_cpu import _reference


@pytest.mark.parametrize("c", G.CASES, ids=[c.name for c in G.CASES])
def test_algebra_without_rounding(c):
    """every rounding off: the emulator (three partial products per term in the split modes; the Winograd-D form
    as transformed planes, four (1,3,3) convs and the output transform) equals the plain fp64 conv -- odd D,
    D = 1, ragged H / W, concat, pool / up / stride-2 / planar input, every residual mode"""
    t = G.inputs(c)
    em = E.conv32(t["srcs"], t["w"], t["b"], c.prec, in_mode=c.in_mode, aff=t["aff"], act=c.act,
                  bound=t["bound"], res=t["res"], res_mode=c.res_mode, mut=E.Mut(exact=True))
    ref = _reference(t["srcs"], t["w"], t["b"], c.in_mode, t["aff"], c.act, t["res"], c.res_mode)
    assert (em["out"] - ref).abs().max() <= 1e-12 * ref.abs().max()


@pytest.mark.parametrize("prec,in_mode", [(p, m) for p in (0, 1, 3) for m in ("same", "up", "pool", "stride2")
                                          if p != 3 or m in ("same", "up")])   # (Winograd-D: SAME / UP)
def test_exact_on_small_integers(prec, in_mode):
    """small integers (even weights for the Winograd-D form's halves): every operand, scaled operand, transform,
    product and sum is exact and every lo is zero, so the emulation IS the conv, in every mode"""
    g = np.random.default_rng(7)
    D, H, W = 5, 8, 10
    Hs, Ws = {"up": (4, 5), "pool": (16, 20), "stride2": (16, 20)}.get(in_mode, (H, W))
    xi = g.integers(-3, 4, (2, 16, D, Hs, Ws)) * (4 if in_mode == "pool" else 1)   # pool means stay integers
    x = torch.from_numpy(xi.astype(np.float32))
    w = torch.from_numpy((2 * g.integers(-2, 3, (128, 16, 3, 3, 3))).astype(np.float32))
    b = torch.from_numpy(g.integers(-5, 6, (128,)).astype(np.float32))
    res = torch.from_numpy(g.integers(-5, 6, (2, 128, D, H, W)).astype(np.float32))
    bound = x.abs().reshape(2, -1).amax(1, keepdim=True)
    em = E.conv32([x], w, b, prec, in_mode=in_mode, bound=bound, res=res, res_mode="same")
    ref = _reference([x], w, b, in_mode, res=res, res_mode="same")
    assert torch.equal(em["out"], ref) and torch.equal(em["stored"], ref)
    assert (em["silu"] == 0).all()


def test_f16x3_operand_error_is_fp32_grade():
    """the split's representation error: |hi + lo - x| <= 2^-22 |x| for a scaled operand of a normal lo, and the
    exact mode's SiLU agrees with torch's fp64 SiLU to a few fp32 ulps"""
    g = np.random.default_rng(3)
    x = torch.from_numpy(g.uniform(-2.0 ** 15, 2.0 ** 15, 100000).astype(np.float32)).double()
    hi, lo = E.split(x, E.Mut(), False)
    assert ((hi + lo - x).abs() <= 2.0 ** -22 * x.abs()).all()
    y = torch.from_numpy(g.standard_normal(100000).astype(np.float32) * 4).double()
    for prec in (0, 1):
        v, delta = E._silu(y, prec, E.Mut())
        assert ((v - F.silu(y)).abs() <= delta).all()


def _mutations(c):
    """the plausible bugs that can apply to case c (test_bugs_move_the_output_beyond_the_bar's docstring)"""
    if c.prec not in E.SPLIT_MODES:
        return {}
    m = {"weights' lo dropped": dict(drop_w_lo=True)}
    taps = 9 if c.prec in E.WZ_MODES else c.k ** 3
    small_k = taps * sum(c.C) <= 4096
    if small_k:
        m["activations' lo dropped"] = dict(drop_act_lo=True)
    if c.N > 1 and len(set(c.mags)) > 1:
        m["sample 0's activation scale for every sample"] = dict(sample0_scale=True)
    if c.prec in E.WZ_MODES:
        if c.D > 1 and not c.alt_max and small_k:
            m["Winograd input transform after the split"] = dict(split_before_transform=True)
        if c.alt_max:
            m["activation-scale gain 1 on the Winograd form"] = dict(wz_gain=1.0)
    if c.small_cout:
        m["weight scale skipped before the split"] = dict(use_wscale=False)
    return m


def test_every_bug_has_a_case():
    seen = {name for c in G.CASES for name in _mutations(c)}
    assert len(seen) == 6, seen


@pytest.mark.parametrize("c", G.CASES, ids=[c.name for c in G.CASES])
def test_bugs_move_the_output_beyond_the_bar(c):
    """Discrimination: each mutation of the arithmetic moves the emulated output by at least 10x the element bound
    the GPU test holds this case to (G.elem_bound) at some element (a non-finite output counts as moved).

    Where a bug applies: the split's bugs to the f16x3 cases only (the exact mode has no split and no scale);
    sample 0's scale to the two-sample cases (with equal magnitudes the scales agree); the transform order to the
    Winograd-D form with D > 1 and varied data (at D = 1 one plane of every sum is zero, and on the alternating
    cases' one magnitude the halves add exactly); the weight scale to the cases with a small-weight channel
    (elsewhere a power-of-two scale of normal f16 halves changes nothing); the Winograd gain to the cases whose bound has the largest mantissa and
    whose planes alternate in sign (elsewhere a doubled scale only shifts every exponent: |d2 - d1| reaches
    f16's range only when both planes sit at the bound); the two activation-side bugs (lost lo, transform order) to accumulators of at
    most K = 4096 terms: the bar grows like K (m sqterms ~ K^2) and their random-sign operand errors like sqrt(K),
    so at the 512-channel level (K = 4608) they move the output 9.4-9.5x its bar; the same kernel family is held
    to >= 10x by the table's smaller cases.

    Not in the list: lo truncated instead of rounded.  It changes an operand by at most one ulp of lo, 2^-21 of
    the operand, with a random sign -- less than one fp32 rounding of the partial sums that carry that product,
    so no bound that admits fp32 accumulation can see it (test_truncated_lo_is_below_every_bar)."""
    t = G.inputs(c)
    em = G.emulate(c, t)
    B = G.elem_bound(c, em)
    for name, kw in _mutations(c).items():
        mu = G.emulate(c, t, **kw)
        r = (mu["out"] - em["out"]).abs() / B
        ratio = float(torch.where(torch.isfinite(mu["out"]), r, torch.full_like(r, float("inf"))).max())
        print("%s / %s: %.3g" % (c.name, name, ratio))
        assert ratio >= 10.0, (name, ratio)


def test_truncated_lo_is_below_every_bar():
    """why truncation is not in the discrimination list: it moves no case's output by even its bar"""
    worst = 0.0
    for c in G.X3_CASES[:12]:
        t = G.inputs(c)
        em = G.emulate(c, t)
        mu = G.emulate(c, t, trunc_lo=True)
        worst = max(worst, float(((mu["out"] - em["out"]).abs() / G.elem_bound(c, em)).max()))
    print("lo truncated: at most %.3g of the element bound" % worst)
    assert worst < 1.0
