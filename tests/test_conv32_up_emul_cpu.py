"""
The phase-form emulator (conv32_up_emul.py) on the CPU tier: its algebra against torch's fp64 conv of the
up-sampled input, its agreement with the 36-tap form's emulation (the same products, regrouped), and -- per small
case of test_gpu_conv32_up.py -- that each plausible bug of the phase form moves the emulated output by at least
10x the bound that case holds the kernel to.
"""

import numpy as np
import pytest
import torch

import conv32_emul as E
import conv32_up_emul as UE
import test_gpu_conv32 as G
import test_gpu_conv32_up as GU
from test_conv16_emul_cpu import _reference

SMALL = [c for c in GU.CASES + GU.FALLBACK if c.D * c.H * c.W * sum(c.C) * c.Cout <= 2 ** 26]
BUGS = {
    "wrong phase <-> tap grouping": dict(wrong_grouping=True),
    "phase sums made after the split": dict(sum_after_split=True),
    "epilogue scale of the 36-tap image on the 64-tap one": dict(scale36=True),
    "a swapped parity": dict(swap_parity=True),
}


@pytest.mark.parametrize("c", SMALL, ids=[c.name for c in SMALL])
def test_algebra_without_rounding(c):
    """every rounding off: four 2x2 phase convs on the source grid ARE the 3x3x3 conv of the up-sampled input --
    zero padding, odd D, D = 1, ragged W, concat, every residual mode"""
    t = G.inputs(c)
    em = GU.emulate_phase(c, t, exact=True)
    ref = _reference(t["srcs"], t["w"], t["b"], "up", t["aff"], c.act, t["res"], c.res_mode)
    assert (em["out"] - ref).abs().max() <= 1e-12 * ref.abs().max()


def test_exact_on_small_integers():
    """small integers (even weights for the Winograd-D halves): nothing rounds, every lo is zero, so the phase
    emulation IS the conv, and equal to the 36-tap form's emulation bit for bit"""
    g = np.random.default_rng(11)
    D, H, W = 5, 8, 12
    x = torch.from_numpy(g.integers(-3, 4, (2, 16, D, H // 2, W // 2)).astype(np.float32))
    w = torch.from_numpy((2 * g.integers(-2, 3, (128, 16, 3, 3, 3))).astype(np.float32))
    b = torch.from_numpy(g.integers(-5, 6, (128,)).astype(np.float32))
    res = torch.from_numpy(g.integers(-5, 6, (2, 128, D, H // 2, W // 2)).astype(np.float32))
    bound = x.abs().reshape(2, -1).amax(1, keepdim=True)
    em = UE.conv32_up([x], w, b, bound=bound, res=res, res_mode="up")
    em36 = E.conv32([x], w, b, 3, in_mode="up", bound=bound, res=res, res_mode="up")
    ref = _reference([x], w, b, "up", res=res, res_mode="up")
    assert torch.equal(em["out"], ref) and torch.equal(em["stored"], ref) and torch.equal(em36["out"], ref)
    assert (em["silu"] == 0).all()


@pytest.mark.parametrize("c", SMALL, ids=[c.name for c in SMALL])
def test_regrouping_stays_inside_the_shipped_bar(c):
    """the phase arithmetic against the 36-tap form's: the regrouped weight sums move the emulated output by a
    small part of the bound the 36-tap kernel is held to (test_gpu_conv32.elem_bound)"""
    t = G.inputs(c)
    em, em36 = GU.emulate_phase(c, t), G.emulate(c, t)
    ratio = float(((em["out"] - em36["out"]).abs() / G.elem_bound(c, em36)).max())
    print("%s: max |phase - 36-tap emulation| / elem_bound = %.3g" % (c.name, ratio))
    assert ratio < 0.1


@pytest.mark.parametrize("c", SMALL, ids=[c.name for c in SMALL])
def test_bugs_move_the_output_beyond_the_bar(c):
    """Discrimination, as test_conv32_emul_cpu.py: each bug moves the emulated output by >= 10x GU.elem_bound at
    some element.  The scale bug is the one the image's layout invites: the phase body has its own per-cout scales
    (over 64 phase taps) behind it, and the 36-tap image in front of it has others (over 36 taps) -- the bug scales
    and splits with one and un-scales in the epilogue with the other.  (A scale merely CHOSEN over 36 taps and used
    on both sides is a power of two on normal f16 halves: it changes nothing a bar could see, as the weight-scale
    note of test_conv32_emul_cpu.py says.)"""
    t = G.inputs(c)
    em = GU.emulate_phase(c, t)
    B = GU.elem_bound(c, em)
    for name, kw in BUGS.items():
        mu = GU.emulate_phase(c, t, pmut=UE.PMut(**kw))
        r = (mu["out"] - em["out"]).abs() / B
        ratio = float(torch.where(torch.isfinite(mu["out"]), r, torch.full_like(r, float("inf"))).max())
        print("%s / %s: %.3g" % (c.name, name, ratio))
        assert ratio >= 10.0, (name, ratio)
